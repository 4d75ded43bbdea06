"""The token-and-duration transducer loss on the GPU against the float64 reference written from the contract
(tests/rnnt_tdt_ref.py, itself checked against path enumeration and autograd in tests/test_rnnt_tdt_ref.py).

Shapes follow tests/test_rnnt_latency_gpu.py: B = 3, T = 7, U = 4, ragged T_b = (7, 4, 1), U_b = (4, 2, 0); V = 37
(unaligned head and tail, no full vector batch) and V = 4200 (one full unrolled batch plus a remainder in fp32); V + D is
never a multiple of 4, so row bases take every alignment.  Tolerances are those of tests/test_rnnt_gpu.py::check -- costs
(and alpha / beta, which are log-values like them) rtol 1e-5, atol 1e-5; gradient rtol 1e-4, atol 1e-5 -- and that file's
2e-3 / 1.6e-2 for fp16 / bf16 logits against the reference on the rounded logits.

An utterance without a path costs +inf on both sides; its gradient is not defined and is left out of the comparison.
Every case asserts on the reference's own values that at least one utterance is feasible."""
import functools

import numpy as np
import pytest
import torch

import rnnt_tdt_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
B, T, U = 3, 7, 4
LLENS = np.array([7, 4, 1], np.int32)
TLENS = np.array([4, 2, 0], np.int32)
VS = [37, 4200]
DURATIONS = [(0, 1, 2, 3, 4), (1,), (0, 2), (1, 4)]
SIGMAS = [0.0, 0.05]


@functools.lru_cache(maxsize=None)
def case(V, D, shape=(B, T, U), seed=0, scale=1.5):
    b, t, u = shape
    rng = np.random.default_rng(8100 + V + 10 * D + seed)
    logits = (rng.normal(size=(b, t, u + 1, V + D)) * scale).astype(np.float32)
    targets = rng.integers(1, V, size=(b, u)).astype(np.int32)
    logits.setflags(write=False)
    targets.setflags(write=False)
    return logits, targets


@functools.lru_cache(maxsize=None)
def reference(V, durs, sigma, dtype="float32"):
    """(costs, grad, alpha, beta) of the shared case, computed once; for a 16-bit dtype on the logits rounded to it"""
    logits, targets = case(V, len(durs))
    if dtype != "float32":
        logits = torch.tensor(logits).to(getattr(torch, dtype)).float().numpy()
    out = ref.tdt_ref(logits, targets, LLENS, TLENS, durs, 0, sigma)
    assert np.isfinite(out[0]).any(), "the case must hold a feasible utterance"
    return out


def run_hip(logits, targets, durs, llens=LLENS, tlens=TLENS, blank=0, sigma=0.0, reduction="none", grad_out=None,
            inplace=False, dtype=torch.float32):
    import wenet_celoss_amd as w
    x = torch.tensor(np.asarray(logits), device=DEV).to(dtype).requires_grad_(True)
    xin = x.clone() if inplace else x          # a non-leaf so that in-place gradient is legal
    y = torch.tensor(np.asarray(targets), dtype=torch.int32, device=DEV)
    ll = torch.tensor(llens, dtype=torch.int32, device=DEV)
    tl = torch.tensor(tlens, dtype=torch.int32, device=DEV)
    loss = w.rnnt_tdt_loss(xin, y, ll, tl, durs, blank=blank, sigma=sigma, reduction=reduction, inplace_grad=inplace)
    if grad_out is None:
        loss.float().sum().backward()
    else:
        loss.backward(torch.tensor(grad_out, device=DEV, dtype=loss.dtype))
    return loss.detach().cpu(), x.grad.cpu()


def run_lattice(logits, targets, durs, llens=LLENS, tlens=TLENS, sigma=0.0):
    import wenet_celoss_amd as w
    out = w.rnnt_tdt_lattice(torch.tensor(np.asarray(logits), device=DEV),
                             torch.tensor(np.asarray(targets), dtype=torch.int32, device=DEV),
                             torch.tensor(llens, dtype=torch.int32, device=DEV),
                             torch.tensor(tlens, dtype=torch.int32, device=DEV), durs, 0, sigma)
    return [o.cpu().numpy() for o in out]


def assert_padding_zero(grad, llens=LLENS, tlens=TLENS):
    for b in range(grad.shape[0]):
        assert not grad[b, llens[b]:].any() and not grad[b, :, tlens[b] + 1:].any()


def compare(costs, grad, oc, og, rtol_c, atol_c, rtol_g, atol_g):
    ok = np.isfinite(oc)
    assert ok.any()
    print("feasible", ok.tolist(), "max |cost err|", np.abs(costs[ok] - oc[ok]).max(), "max |grad err|",
          np.abs(grad[ok] - og[ok]).max())
    assert np.array_equal(np.isposinf(costs), ~ok)                # no path: +inf, on both sides
    np.testing.assert_allclose(costs[ok], oc[ok], rtol=rtol_c, atol=atol_c)
    np.testing.assert_allclose(grad[ok], og[ok], rtol=rtol_g, atol=atol_g)


@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("durs", DURATIONS)
@pytest.mark.parametrize("V", VS)
def test_fp32_matches_the_reference(V, durs, sigma):
    logits, targets = case(V, len(durs))
    assert (V + len(durs)) % 4 != 0
    costs, grad = run_hip(logits, targets, durs, sigma=sigma)
    oc, og, oa, ob = reference(V, durs, sigma)
    compare(costs.numpy(), grad.numpy(), oc, og, 1e-5, 1e-5, 1e-4, 1e-5)
    assert_padding_zero(grad)
    c2, alpha, beta = run_lattice(logits, targets, durs, sigma=sigma)
    assert np.array_equal(c2, costs.numpy())
    np.testing.assert_allclose(alpha, oa, rtol=1e-5, atol=1e-5)      # -inf where no path enters, 0 outside the lattice
    np.testing.assert_allclose(beta, ob, rtol=1e-5, atol=1e-5)
    if sigma > 0:                                                    # sigma does something
        ok = np.isfinite(oc)
        assert np.abs(oc[ok] - reference(V, durs, 0.0)[0][ok]).min() > 1e-2


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("durs", DURATIONS)
@pytest.mark.parametrize("V", VS)
def test_half_precision_logits(V, durs, sigma, dtype, tol):
    costs, grad = run_hip(*case(V, len(durs)), durs, sigma=sigma, dtype=dtype)
    assert costs.dtype == dtype and grad.dtype == dtype
    oc, og, _, _ = reference(V, durs, sigma, str(dtype).split(".")[1])
    compare(costs.float().numpy(), grad.float().numpy(), oc, og, tol, 0.0, tol, tol * 1e-1)
    assert_padding_zero(grad)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("V", VS)
def test_nan_in_padding_does_not_leak_and_inplace_is_bit_identical(V, dtype):
    durs = (0, 1, 2, 3, 4)
    logits, targets = case(V, len(durs))
    costs, grad = run_hip(logits, targets, durs, sigma=0.05, dtype=dtype)
    dirty = logits.copy()
    for b in range(B):
        dirty[b, LLENS[b]:] = np.nan
        dirty[b, :, TLENS[b] + 1:] = np.nan
    c1, g1 = run_hip(dirty, targets, durs, sigma=0.05, dtype=dtype)
    assert torch.equal(c1, costs) and torch.equal(g1, grad)
    assert_padding_zero(g1)
    c2, g2 = run_hip(logits, targets, durs, sigma=0.05, dtype=dtype, inplace=True)
    assert torch.equal(c2, costs) and torch.equal(g2, grad)
    c3, g3 = run_hip(logits, targets, durs, sigma=0.05, dtype=dtype)      # repeatability
    assert torch.equal(c3, costs) and torch.equal(g3, grad)


def test_reductions_and_grad_costs():
    V, durs = 37, (1, 4)
    logits, targets = case(V, len(durs))
    oc, og, _, _ = reference(V, durs, 0.05)
    assert np.isfinite(oc).all()
    for reduction, scale in (("mean", 1.0 / B), ("sum", 1.0)):
        loss, grad = run_hip(logits, targets, durs, sigma=0.05, reduction=reduction)
        np.testing.assert_allclose(loss.item(), oc.sum() * scale, rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(grad.numpy(), og * scale, rtol=1e-4, atol=1e-5)
    gout = np.array([0.5, -2.0, 3.0], np.float32)
    _, grad = run_hip(logits, targets, durs, sigma=0.05, grad_out=gout)
    # the absolute part of the bound scales with the largest |grad_costs| = 3, as the gradient does
    np.testing.assert_allclose(grad.numpy(), og * gout[:, None, None, None], rtol=1e-4, atol=3e-5)
    assert_padding_zero(grad)


def test_infeasible_utterance_and_unreachable_cells():
    # durations (0, 2): every move is two frames, so T_b = 5 has no path and the odd frames of the others are never entered
    V, durs = 37, (0, 2)
    llens, tlens = np.array([6, 4, 5], np.int32), np.array([4, 1, 2], np.int32)
    logits, targets = case(V, len(durs), shape=(3, 6, 4), seed=1)
    oc, og, oa, _ = ref.tdt_ref(logits, targets, llens, tlens, durs, 0, 0.0)
    assert np.isfinite(oc[:2]).all() and oc[2] == np.inf
    assert np.all(oa[0, 1, :5] == -np.inf) and np.all(og[0, 1] == 0)         # such a cell exists
    costs, grad = run_hip(logits, targets, durs, llens, tlens)
    compare(costs.numpy(), grad.numpy(), oc, og, 1e-5, 1e-5, 1e-4, 1e-5)
    assert costs[2] == np.inf
    assert torch.isfinite(grad[:2]).all()
    for b in range(2):
        assert not grad[b, 1:llens[b]:2].any()                               # exactly zero, never NaN
    assert_padding_zero(grad, llens, tlens)
    # the same batch without the infeasible utterance: the others do not change
    c2, g2 = run_hip(logits[:2], targets[:2], durs, llens[:2], tlens[:2])
    assert torch.equal(c2, costs[:2]) and torch.equal(g2, grad[:2])


def test_frameless_utterance_beside_live_ones_over_two_waves():
    """T_b = 0 between two live utterances at U1 = 65: its two workgroups leave through the sweep's early exit while the
    others run the two-wave barrier path.  The reference gives the frameless utterance cost 0 and no gradient."""
    V, durs = 17, (0, 1, 2)
    logits, targets = case(V, len(durs), shape=(3, 9, 64), seed=3)
    llens, tlens = np.array([9, 0, 5], np.int32), np.array([64, 7, 64], np.int32)
    oc, og, oa, ob = ref.tdt_ref(logits, targets, llens, tlens, durs, 0, 0.05)
    assert np.isfinite(oc).all() and oc[1] == 0
    costs, grad = run_hip(logits, targets, durs, llens, tlens, sigma=0.05)
    compare(costs.numpy(), grad.numpy(), oc, og, 1e-5, 1e-5, 1e-4, 1e-5)
    assert costs[1] == 0 and not grad[1].any()
    assert_padding_zero(grad, llens, tlens)
    _, alpha, beta = run_lattice(logits, targets, durs, llens, tlens, sigma=0.05)
    np.testing.assert_allclose(alpha, oa, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(beta, ob, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("shape,durs", [((1, 3, 70), (0, 1, 2)), ((1, 40, 2), (0, 1, 3, 8))])
def test_sweep_boundaries(shape, durs):
    """U + 1 = 71 columns: two waves in the sweep, so the LDS exchange across waves runs.  T = 40: longer than the prefetch
    depth and the rings."""
    V = 8
    b, t, u = shape
    logits, targets = case(V, len(durs), shape=shape, seed=2)
    llens, tlens = np.array([t], np.int32), np.array([u], np.int32)
    oc, og, oa, ob = ref.tdt_ref(logits, targets, llens, tlens, durs, 0, 0.05)
    assert np.isfinite(oc).all()
    costs, grad = run_hip(logits, targets, durs, llens, tlens, sigma=0.05)
    compare(costs.numpy(), grad.numpy(), oc, og, 1e-5, 1e-5, 1e-4, 1e-5)
    _, alpha, beta = run_lattice(logits, targets, durs, llens, tlens, sigma=0.05)
    np.testing.assert_allclose(alpha, oa, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(beta, ob, rtol=1e-5, atol=1e-5)
