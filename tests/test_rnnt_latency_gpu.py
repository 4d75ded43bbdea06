"""FastEmit and the delay penalty of rnnt_loss on the GPU against the float64 reference written from the contract
(tests/rnnt_latency_ref.py, itself checked against path enumeration and autograd in tests/test_rnnt_latency_ref.py).

Shapes: B = 3, T = 7, U = 4, ragged T_b = (7, 4, 1), U_b = (4, 2, 0) (a U_b = 0 utterance and a one-frame utterance);
V = 37 (unaligned head and tail, no full vector batch) and V = 4200 (one full unrolled batch plus a remainder in fp32).
Tolerances are those of tests/test_rnnt_gpu.py::check -- costs rtol 1e-5, atol 1e-5; gradient rtol 1e-4 and atol 1e-5
times the value range 1 + lambda (the label term is scaled by it) -- and that file's 2e-3 / 1.6e-2 for fp16 / bf16 logits
against the reference on the rounded logits."""
import functools

import numpy as np
import pytest
import torch

import rnnt_latency_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T, U = 3, 7, 4
LLENS = np.array([7, 4, 1], np.int32)
TLENS = np.array([4, 2, 0], np.int32)
VS = [37, 4200]
SETTINGS = [(0.01, 0.0), (0.5, 0.0), (0.0, 0.003), (0.0, 0.5), (0.5, 0.5)]
KEY_SKIP = 14                       # wr_tune_set: dead / faint rows are written without being read (default 1)


@functools.lru_cache(maxsize=None)
def case(V, seed=0, scale=1.5):
    rng = np.random.default_rng(7000 + V + seed)
    logits = (rng.normal(size=(B, T, U + 1, V)) * scale).astype(np.float32)
    targets = rng.integers(1, V, size=(B, U)).astype(np.int32)
    logits.setflags(write=False)
    targets.setflags(write=False)
    return logits, targets


@functools.lru_cache(maxsize=None)
def reference(V, lam, dp, dtype="float32"):
    """(costs, grad) of the shared case, computed once; for a 16-bit dtype on the logits rounded to it"""
    logits, targets = case(V)
    if dtype != "float32":
        logits = torch.tensor(logits).to(getattr(torch, dtype)).float().numpy()
    costs, grad, _ = ref.loss_f64(logits, targets, LLENS, TLENS, 0, lam, dp)
    return costs, grad


def run_hip(logits, targets, llens=LLENS, tlens=TLENS, blank=0, clamp=-1.0, reduction="none", grad_out=None, inplace=False,
            dtype=torch.float32, **kw):
    import wenet_celoss_amd as w
    x = torch.tensor(np.asarray(logits), device=DEV).to(dtype).requires_grad_(True)
    xin = x.clone() if inplace else x          # a non-leaf so that in-place gradient is legal
    y = torch.tensor(np.asarray(targets), dtype=torch.int32, device=DEV)
    ll = torch.tensor(llens, dtype=torch.int32, device=DEV)
    tl = torch.tensor(tlens, dtype=torch.int32, device=DEV)
    loss = w.rnnt_loss(xin, y, ll, tl, blank=blank, clamp=clamp, reduction=reduction, inplace_grad=inplace, **kw)
    if grad_out is None:
        loss.float().sum().backward()
    else:
        loss.backward(torch.tensor(grad_out, device=DEV, dtype=loss.dtype))
    return loss.detach().cpu(), x.grad.cpu()


def assert_padding_zero(grad):
    for b in range(B):
        assert not grad[b, LLENS[b]:].any() and not grad[b, :, TLENS[b] + 1:].any()


def kw(lam, dp):
    return dict(fastemit_lambda=lam, delay_penalty=dp)


@pytest.mark.parametrize("lam,dp", SETTINGS)
@pytest.mark.parametrize("V", VS)
def test_fp32_matches_the_reference(V, lam, dp):
    costs, grad = run_hip(*case(V), **kw(lam, dp))
    oc, og = reference(V, lam, dp)
    print("max |cost err|", np.abs(costs.numpy() - oc).max(), "max |grad err|", np.abs(grad.numpy() - og).max())
    np.testing.assert_allclose(costs.numpy(), oc, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(grad.numpy(), og, rtol=1e-4, atol=1e-5 * (1.0 + lam))
    assert_padding_zero(grad)
    # the options do something: the plain loss is further away than the tolerance
    pc, pg = reference(V, 0.0, 0.0)
    assert np.abs(og - pg).max() > 1e-3 * min(max(lam, dp), 1.0)
    assert (dp == 0.0) == bool(np.array_equal(oc, pc))


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
@pytest.mark.parametrize("lam,dp", SETTINGS)
@pytest.mark.parametrize("V", VS)
def test_half_precision_logits(V, lam, dp, dtype, tol):
    costs, grad = run_hip(*case(V), dtype=dtype, **kw(lam, dp))
    assert costs.dtype == dtype and grad.dtype == dtype
    oc, og = reference(V, lam, dp, str(dtype).split(".")[1])
    np.testing.assert_allclose(costs.float().numpy(), oc, rtol=tol)
    np.testing.assert_allclose(grad.float().numpy(), og, rtol=tol, atol=tol * 1e-1)
    assert_padding_zero(grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V", VS)
def test_costs_do_not_depend_on_lambda_and_defaults_are_the_plain_call(V, dtype):
    logits, targets = case(V)
    for dp in (0.0, 0.003, 0.5):
        c0, g0 = run_hip(logits, targets, dtype=dtype, **kw(0.0, dp))
        for lam in (0.01, 0.5):
            c1, g1 = run_hip(logits, targets, dtype=dtype, **kw(lam, dp))
            assert torch.equal(c0, c1), (dp, lam)               # bit-identical costs
            assert not torch.equal(g0, g1)
    plain_c, plain_g = run_hip(logits, targets, dtype=dtype)
    zero_c, zero_g = run_hip(logits, targets, dtype=dtype, **kw(0.0, 0.0))
    assert torch.equal(plain_c, zero_c) and torch.equal(plain_g.view(torch.uint8), zero_g.view(torch.uint8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("lam,dp", [(0.5, 0.0), (0.0, 0.5), (0.5, 0.5)])
@pytest.mark.parametrize("V", VS)
def test_inplace_gradient_is_bit_identical(V, lam, dp, dtype):
    """the label arc emit' comes from the workspace, never from the logits the gradient overwrites"""
    c0, g0 = run_hip(*case(V), dtype=dtype, **kw(lam, dp))
    c1, g1 = run_hip(*case(V), dtype=dtype, inplace=True, **kw(lam, dp))
    assert torch.equal(c0, c1) and torch.equal(g0.view(torch.uint8), g1.view(torch.uint8))


@pytest.mark.parametrize("V", VS)
def test_clamp_grad_costs_and_reductions(V):
    logits, targets = case(V)
    lam, dp = 0.5, 0.5
    oc, og = reference(V, lam, dp)
    clamp = 0.05
    _, ogc, _ = ref.loss_f64(logits, targets, LLENS, TLENS, 0, lam, dp, clamp=clamp)
    assert (np.abs(og) > clamp).any()
    _, grad = run_hip(logits, targets, clamp=clamp, **kw(lam, dp))
    np.testing.assert_allclose(grad.numpy(), ogc, rtol=1e-4, atol=1e-5 * (1.0 + lam))
    assert float(grad.abs().max()) <= np.float32(clamp)
    go = np.array([0.5, -2.0, 3.0], np.float32)
    _, grad = run_hip(logits, targets, grad_out=go, **kw(lam, dp))
    np.testing.assert_allclose(grad.numpy(), og * go[:, None, None, None], rtol=1e-4, atol=1e-5 * (1.0 + lam) * 3.0)
    for red, scale in (("mean", 1.0 / B), ("sum", 1.0)):
        loss, grad = run_hip(logits, targets, reduction=red, **kw(lam, dp))
        np.testing.assert_allclose(float(loss), oc.sum() * scale, rtol=1e-5)
        np.testing.assert_allclose(grad.numpy(), og * scale, rtol=1e-4, atol=1e-5 * (1.0 + lam))
    # the module form
    import wenet_celoss_amd as w
    x = torch.tensor(logits, device=DEV, requires_grad=True)
    loss = w.RNNTLoss(blank=0, reduction="sum", **kw(lam, dp))(
        x, torch.tensor(targets, device=DEV), torch.tensor(LLENS, device=DEV), torch.tensor(TLENS, device=DEV))
    loss.backward()
    np.testing.assert_allclose(float(loss), oc.sum(), rtol=1e-5)
    np.testing.assert_allclose(x.grad.cpu().numpy(), og, rtol=1e-4, atol=1e-5 * (1.0 + lam))


@pytest.mark.parametrize("lam,dp", [(0.5, 0.0), (0.5, 0.5)])
@pytest.mark.parametrize("V", VS)
def test_label_equal_to_blank_follows_the_case_chain(V, lam, dp):
    logits, targets = case(V)
    targets = targets.copy()
    targets[0, 2] = 0
    targets[1, 0] = 0
    oc, og, _ = ref.loss_f64(logits, targets, LLENS, TLENS, 0, lam, dp)
    costs, grad = run_hip(logits, targets, **kw(lam, dp))
    np.testing.assert_allclose(costs.numpy(), oc, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(grad.numpy(), og, rtol=1e-4, atol=1e-5 * (1.0 + lam))
    # and a blank that is not class 0
    blank = V - 1
    t2 = np.where(case(V)[1] == blank, 1, case(V)[1]).astype(np.int32)
    oc, og, _ = ref.loss_f64(logits, t2, LLENS, TLENS, blank, lam, dp)
    costs, grad = run_hip(logits, t2, blank=blank, **kw(lam, dp))
    np.testing.assert_allclose(costs.numpy(), oc, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(grad.numpy(), og, rtol=1e-4, atol=1e-5 * (1.0 + lam))


# ---------------------------------------------------------------------------------------------- dead / faint rows --
D_LLENS = np.array([10, 6], np.int32)
D_TLENS = np.array([4, 3], np.int32)
D_CASES = {37: (1000, 25.0), 4200: (1001, 18.0)}     # V -> (seed, scale): chosen on the CPU so that every class occurs


@functools.lru_cache(maxsize=None)
def dead_case(V):
    """Wide logits (tests/rnnt_dead_rows.py's kind: the lattice's off-path cells lose more than kDeadThr) at lambda = 0.5,
    delta = 0.5, with the reference's classification of every row."""
    seed, scale = D_CASES[V]
    rng = np.random.default_rng(seed)
    logits = (rng.normal(size=(2, 10, 5, V)) * scale).astype(np.float32)
    targets = rng.integers(1, V, size=(2, 4)).astype(np.int32)
    oc, og, lats = ref.loss_f64(logits, targets, D_LLENS, D_TLENS, 0, 0.5, 0.5)
    cls, need_b, need_l = ref.classify(lats, targets, D_LLENS, D_TLENS, 10, 5, 0, 0.5, 0.5)
    return logits, targets, oc, og, cls, need_l


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("V", VS)
def test_dead_row_skipping_on_and_off_is_bit_identical(V, dtype):
    from wenet_celoss_amd import _lib
    logits, targets, oc, og, cls, need_l = dead_case(V)
    assert (cls == ref.DEAD).any() and (cls == ref.LIVE).any() and ((cls == ref.FAINT) & need_l).any()
    lib = _lib.load()
    res = {}
    try:
        for skip in (1, 0):
            assert lib.wr_tune_set(KEY_SKIP, skip) == 0
            res[skip] = run_hip(logits, targets, D_LLENS, D_TLENS, dtype=dtype, **kw(0.5, 0.5))
    finally:
        lib.wr_tune_set(KEY_SKIP, 1)
    assert torch.equal(res[1][0], res[0][0])
    assert torch.equal(res[1][1].view(torch.uint8), res[0][1].view(torch.uint8))
    if dtype == torch.float32:
        np.testing.assert_allclose(res[1][0].numpy(), oc, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(res[1][1].numpy(), og, rtol=1e-4, atol=1e-5 * 1.5)
        # a dead row is all zeros; a faint row is zero except at its blank / label element
        g = res[1][1].numpy()
        assert not g[cls == ref.DEAD].any()
