"""Pruned RNN-T training on the GPU: prune ranges, the gather of the joiner's addends, the pruned loss and the model layer.

References (tests/rnnt_pruned_ref.py, checked on the CPU by test_rnnt_pruned_ref.py): `prune_ranges_ref` for the ranges
(exact: the float64 summation order is fixed), `torch.gather` / a float64 `index_add_` for the pruning, the float64 banded
lattice for the loss.  Tolerances are the project's bar for this lattice against float64 (test_rnnt_gpu.py check(): cost
rtol 1e-5 / atol 1e-5, gradient rtol 1e-4 / atol 1e-5); 16-bit logits as test_rnnt_gpu.py::test_half_precision_logits."""
import numpy as np
import pytest
import torch

import oracle
import rnnt_pruned_ref as ref
import test_rnnt_gpu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COST_TOL = dict(rtol=1e-5, atol=1e-5)
GRAD_TOL = dict(rtol=1e-4, atol=1e-5)
RAGGED_TABLE = [               # the (B, T, U, V) table of test_rnnt_gpu.py::test_parity_ragged, copied
    (1, 1, 0, 2),              # single cell
    (2, 5, 0, 7),              # no labels: blank-only path
    (3, 7, 3, 5),
    (4, 20, 9, 33),
    (3, 33, 17, 128),
    (2, 70, 64, 40),           # U1 = 65
    (2, 40, 150, 36),          # U1 = 151 (the BASELINE shape's width)
    (2, 12, 200, 20),
    (1, 9, 300, 12),
    (1, 6, 511, 8),
    (2, 9, 700, 12),
    (1, 5, 1023, 6),           # 1024 columns: the supported maximum
    (5, 130, 30, 64),
]


def boundary_of(t_lens, u_lens):
    bd = torch.zeros(len(t_lens), 4, dtype=torch.int64)
    bd[:, 2] = torch.as_tensor(np.asarray(u_lens))
    bd[:, 3] = torch.as_tensor(np.asarray(t_lens))
    return bd.to(DEV)


def ragged_lengths(rng, B, T, U):
    t_lens = np.concatenate([[T], rng.integers(1, T + 1, size=B - 1)]).astype(np.int64)
    u_lens = rng.integers(0, U + 1, size=B).astype(np.int64)
    u_lens[rng.integers(0, B)] = U
    return t_lens, u_lens


# ------------------------------------------------------------------------------------------------ 1. ranges --
@pytest.mark.parametrize("B,T,U,V", RAGGED_TABLE)
def test_ranges_equal_the_reference_on_every_frame(B, T, U, V):
    import wenet_celoss_amd as w
    rng = np.random.default_rng(B * 1000 + T * 10 + U + V)
    V = max(V, 2)
    lm = rng.normal(size=(B, U + 1, V)).astype(np.float32)
    am = rng.normal(size=(B, T, V)).astype(np.float32)
    symbols = rng.integers(1, V, size=(B, U)).astype(np.int64)
    t_lens, u_lens = ragged_lengths(rng, B, T, U)
    bd = boundary_of(t_lens, u_lens)
    _, (px, py) = w.rnnt_loss_simple(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV),
                                     torch.tensor(symbols, device=DEV), 0, boundary=bd, reduction="sum", return_grad=True)
    assert tuple(px.shape) == (B, U, T + 1) and tuple(py.shape) == (B, U + 1, T)
    pxh, pyh, bdh = px.cpu().numpy(), py.cpu().numpy(), bd.cpu().numpy()
    for s_range in (2, 5, U + 1, U + 7):
        if s_range < 2:
            with pytest.raises(ValueError):
                w.get_rnnt_prune_ranges(px, py, bd, s_range)
            continue
        got = w.get_rnnt_prune_ranges(px, py, bd, s_range)
        assert got.dtype == torch.int64 and tuple(got.shape) == (B, T, min(s_range, U + 1))
        want = ref.prune_ranges_ref(pxh, pyh, bdh, s_range)
        np.testing.assert_array_equal(got.cpu().numpy(), want)
        ref.check_range_properties(got.cpu().numpy(), bdh, U + 1)


def test_ranges_over_several_chunks_of_frames_and_without_boundary():
    """T = 2500 frames: three chunks of the per-utterance scan, the running minima carried across them."""
    import wenet_celoss_amd as w
    rng = np.random.default_rng(77)
    B, T, U = 3, 2500, 9
    px = torch.tensor(rng.random((B, U, T + 1)).astype(np.float32), device=DEV)
    py = torch.tensor(rng.random((B, U + 1, T)).astype(np.float32), device=DEV)
    bd = boundary_of([T, 1033, 2049], [U, 4, 1])
    for boundary, bdh in ((bd, bd.cpu().numpy()), (None, np.array([[0, 0, U, T]] * B))):
        for s_range in (2, 3, 5):
            got = w.get_rnnt_prune_ranges(px, py, boundary, s_range).cpu().numpy()
            np.testing.assert_array_equal(got, ref.prune_ranges_ref(px.cpu().numpy(), py.cpu().numpy(), bdh, s_range))
            ref.check_range_properties(got, bdh, U + 1)
    with pytest.raises(ValueError, match="begin"):
        w.get_rnnt_prune_ranges(px, py, torch.tensor([[0, 1, U, T]] * B, device=DEV), 3)


# ----------------------------------------------------------------------------------------------- 2. pruning --
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("B,T,U,R,C", [(3, 17, 8, 5, 64), (2, 9, 3, 2, 7), (2, 70, 30, 5, 512), (1, 5, 0, 1, 12)])
def test_pruning_forward_backward(dtype, B, T, U, R, C):
    import wenet_celoss_amd as w
    rng = np.random.default_rng(B + T + U + R + C)
    t_lens, u_lens = ragged_lengths(rng, B, T, U)
    ranges = torch.tensor(ref.random_band(rng, B, T, U + 1, R, t_lens, u_lens), device=DEV)
    am = torch.tensor(rng.normal(size=(B, T, C)).astype(np.float32), device=DEV).to(dtype).requires_grad_(True)
    lm = torch.tensor(rng.normal(size=(B, U + 1, C)).astype(np.float32), device=DEV).to(dtype).requires_grad_(True)
    am_p, lm_p = w.do_rnnt_pruning(am, lm, ranges)
    assert am_p.dtype == lm_p.dtype == dtype and tuple(am_p.shape) == tuple(lm_p.shape) == (B, T, R, C)
    assert torch.equal(am_p, am.detach()[:, :, None, :].expand(B, T, R, C))
    idx = ranges[..., None].expand(B, T, R, C)
    assert torch.equal(lm_p, torch.gather(lm.detach()[:, None].expand(B, T, U + 1, C), 2, idx))

    g_am = torch.tensor(rng.normal(size=(B, T, R, C)).astype(np.float32), device=DEV).to(dtype)
    g_lm = torch.tensor(rng.normal(size=(B, T, R, C)).astype(np.float32), device=DEV).to(dtype)
    grads = []
    for _ in range(2):
        am.grad = lm.grad = None
        a, l = w.do_rnnt_pruning(am, lm, ranges)
        torch.autograd.backward([a, l], [g_am, g_lm])
        grads.append((am.grad.clone(), lm.grad.clone()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])      # bit-identical run to run
    want_am = g_am.double().sum(2)
    want_lm = torch.zeros(B, U + 1, C, dtype=torch.float64, device=DEV)
    for b in range(B):
        want_lm[b].index_add_(0, ranges[b].reshape(-1), g_lm[b].double().reshape(-1, C))
    # error of an fp32 sum of n terms in any order: (n - 1) * 2^-24 * sum |terms|; plus one rounding to the output dtype
    out_ulp = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]
    abs_am = g_am.double().abs().sum(2)
    abs_lm = torch.zeros_like(want_lm)
    for b in range(B):
        abs_lm[b].index_add_(0, ranges[b].reshape(-1), g_lm[b].double().abs().reshape(-1, C))
    for got, want, mag, n in ((grads[0][0], want_am, abs_am, R), (grads[0][1], want_lm, abs_lm, T)):
        assert got.dtype == dtype
        bound = n * 2.0 ** -24 * mag + out_ulp * want.abs() + 1e-30
        err = (got.double() - want).abs()
        print(dtype, "scatter worst err / bound", float((err / bound).max()))
        assert bool((err <= bound).all())
    if U + 1 > R:                                               # a label row nothing points at gets an exact zero
        untouched = torch.ones(B, U + 1, dtype=torch.bool, device=DEV)
        for b in range(B):
            untouched[b, ranges[b].reshape(-1)] = False
        assert not grads[0][1][untouched].any()


def test_pruning_and_loss_reject_bad_ranges():
    import wenet_celoss_amd as w
    am, lm = torch.zeros(1, 4, 8, device=DEV), torch.zeros(1, 3, 8, device=DEV)
    good = torch.tensor([[[0, 1], [0, 1], [1, 2], [1, 2]]], device=DEV)
    w.do_rnnt_pruning(am, lm, good)
    logits, sy = torch.zeros(1, 4, 2, 5, device=DEV), torch.ones(1, 2, dtype=torch.int64, device=DEV)
    w.rnnt_loss_pruned(logits, sy, good, 0)
    for bad in (good + 2, good - 1, good * 2):
        with pytest.raises(ValueError, match="ranges"):
            w.do_rnnt_pruning(am, lm, bad)
        with pytest.raises(ValueError, match="ranges"):
            w.rnnt_loss_pruned(logits, sy, bad, 0)


# -------------------------------------------------------------------------------------------------- 3. loss --
def make_loss_case(rng, B, T, U, V, R, blank=0, scale=1.5, full=False):
    """Ragged lengths, a random valid band and logits on it.  Every utterance gets at least the max(U_b - R + 1, 0) + 1
    frames a band that starts at 0 and rises by at most one per frame needs to hold a complete path."""
    labels = [v for v in range(V) if v != blank]
    symbols = rng.choice(labels, size=(B, U)).astype(np.int64) if U > 0 else np.zeros((B, 0), np.int64)
    if full:
        t_lens, u_lens = np.full(B, T, np.int64), np.full(B, U, np.int64)
    else:
        t_lens, u_lens = ragged_lengths(rng, B, T, U)
    R = min(R, U + 1)
    t_lens = np.minimum(T, np.maximum(t_lens, np.maximum(u_lens - R + 1, 0) + 1))
    ranges = ref.random_band(rng, B, T, U + 1, R, t_lens, u_lens)
    logits = (rng.normal(size=(B, T, R, V)) * scale).astype(np.float32)
    return logits, ranges, symbols, t_lens, u_lens


def run_hip(logits, ranges, symbols, t_lens, u_lens, blank=0, reduction="none", grad_out=None, dtype=torch.float32):
    import wenet_celoss_amd as w
    x = torch.tensor(logits, device=DEV).to(dtype).requires_grad_(True)
    loss = w.rnnt_loss_pruned(x, torch.tensor(symbols, device=DEV), torch.tensor(ranges, device=DEV), blank,
                              boundary=boundary_of(t_lens, u_lens), reduction=reduction)
    assert loss.dtype == torch.float32
    if grad_out is None:
        loss.sum().backward()
    else:
        loss.backward(torch.tensor(grad_out, device=DEV, dtype=torch.float32))
    assert x.grad.dtype == dtype
    return loss.detach().cpu().numpy(), x.grad.float().cpu().numpy()


def check(logits, ranges, symbols, t_lens, u_lens, blank=0, all_feasible=True):
    costs, grad = run_hip(logits, ranges, symbols, t_lens, u_lens, blank=blank)
    want_c, want_g = ref.reference_batch(logits, ranges, symbols, blank, t_lens, u_lens)
    finite = np.isfinite(want_c)
    print("cost err", np.abs(costs - want_c)[finite].max(initial=0.0), "grad err", np.abs(grad - want_g)[finite].max(initial=0.0),
          "feasible", int(finite.sum()), "of", len(finite))
    assert finite.all() if all_feasible else finite.any()
    np.testing.assert_array_equal(np.isfinite(costs), finite)
    assert (costs[~finite] == np.inf).all()                   # a band without a complete path: +inf, a value
    np.testing.assert_allclose(costs[finite], want_c[finite], **COST_TOL)
    np.testing.assert_allclose(grad[finite], want_g[finite], **GRAD_TOL)
    for b in range(logits.shape[0]):                          # every element of a skipped row is zero
        assert not grad[b, t_lens[b]:].any()
        assert not grad[b][ranges[b] > u_lens[b]].any()
    return costs, grad


@pytest.mark.parametrize("V", [2, 31, 500, 1024, 5000])
def test_loss_parity_over_vocabularies(V):
    rng = np.random.default_rng(V)
    check(*make_loss_case(rng, 4, 23, 11, V, 5))


@pytest.mark.parametrize("B,T,U,R", [(3, 80, 70, 5), (2, 160, 150, 5), (2, 9, 5, 2), (3, 12, 3, 7), (2, 1, 0, 5),
                                     (5, 130, 30, 4)])
def test_loss_parity_ragged(B, T, U, R):
    rng = np.random.default_rng(B * 1000 + T * 10 + U + R)
    check(*make_loss_case(rng, B, T, U, 33, R))


def test_loss_parity_with_utterances_too_short_for_their_band():
    """U > T: an utterance with more labels than a unit-step band can climb in its frames has no complete path (+inf);
    the others in the batch are checked as usual."""
    rng = np.random.default_rng(50)
    logits, ranges, symbols, t_lens, u_lens = make_loss_case(rng, 4, 12, 30, 33, 5)
    t_lens[:], u_lens[:] = [12, 12, 5, 9], [30, 9, 12, 3]
    ranges = ref.random_band(rng, 4, 12, 31, 5, t_lens, u_lens)
    costs, _ = check(logits, ranges, symbols, t_lens, u_lens, all_feasible=False)
    assert list(np.isfinite(costs)) == [False, True, False, True]


def test_loss_against_the_differentiable_expression_blank_nonzero_and_label_equal_blank():
    rng = np.random.default_rng(41)
    blank = 12
    logits, ranges, symbols, t_lens, u_lens = make_loss_case(rng, 3, 9, 5, 13, 3, blank=blank, full=True)
    check(logits, ranges, symbols, t_lens, u_lens, blank=blank)
    symbols[0, 2] = blank                                     # a label equal to the blank (and, at b = 1, a repeated label)
    symbols[1, 4] = blank
    symbols[1, 3] = symbols[1, 2]
    for bl in (blank, 0):
        costs, grad = check(logits, ranges, symbols, t_lens, u_lens, blank=bl)
        x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
        want = ref.loss_pruned_torch_f64(x, ranges, symbols, bl, t_lens, u_lens)
        want.sum().backward()
        np.testing.assert_allclose(costs, want.detach().numpy(), **COST_TOL)
        np.testing.assert_allclose(grad, x.grad.numpy(), **GRAD_TOL)


def test_loss_single_frame_utterances():
    rng = np.random.default_rng(43)
    logits, ranges, symbols, _, _ = make_loss_case(rng, 3, 6, 4, 20, 5, full=True)
    t_lens, u_lens = np.array([1, 1, 6]), np.array([4, 0, 4])          # T_b = 1: the whole path sits in frame 0
    ranges = ref.random_band(rng, 3, 6, 5, 5, t_lens, u_lens)
    costs, _ = check(logits, ranges, symbols, t_lens, u_lens)
    assert np.isfinite(costs).all()


def test_reductions_and_grad_costs():
    rng = np.random.default_rng(44)
    case = make_loss_case(rng, 4, 11, 5, 24, 3)
    want_c, want_g = ref.reference_batch(case[0], case[1], case[2], 0, case[3], case[4])
    assert np.isfinite(want_c).all()
    for red, scale in (("mean", 1.0 / 4), ("sum", 1.0)):
        loss, grad = run_hip(*case, reduction=red)
        np.testing.assert_allclose(loss, want_c.sum() * scale, rtol=1e-5)
        np.testing.assert_allclose(grad, want_g * scale, **GRAD_TOL)
    go = np.array([0.5, -2.0, 0.0, 3.0], np.float32)
    _, grad = run_hip(*case, grad_out=go)
    np.testing.assert_allclose(grad, want_g * go[:, None, None, None], **GRAD_TOL)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
def test_logits_view_off_the_16_byte_grid_gives_the_same_result(dtype):
    """A contiguous view whose storage offset is no multiple of 16 bytes (one element into a buffer): the gradient tensor
    is freshly allocated, so logits and gradient would differ in their 16-byte phase.  Same bits as the aligned call."""
    import wenet_celoss_amd as w
    rng = np.random.default_rng(47)
    logits, ranges, symbols, t_lens, u_lens = make_loss_case(rng, 2, 9, 5, 37, 3)
    want_c, want_g = run_hip(logits, ranges, symbols, t_lens, u_lens, dtype=dtype)
    flat = torch.zeros(logits.size + 1, dtype=dtype, device=DEV)
    flat[1:] = torch.tensor(logits, device=DEV).to(dtype).reshape(-1)
    base = flat.requires_grad_(True)
    x = base[1:].view(logits.shape)
    assert x.is_contiguous() and x.data_ptr() % 16 != 0
    loss = w.rnnt_loss_pruned(x, torch.tensor(symbols, device=DEV), torch.tensor(ranges, device=DEV), 0,
                              boundary=boundary_of(t_lens, u_lens), reduction="none")
    loss.sum().backward()
    np.testing.assert_array_equal(loss.detach().cpu().numpy(), want_c)
    np.testing.assert_array_equal(base.grad[1:].view(logits.shape).float().cpu().numpy(), want_g)
    assert float(base.grad[0]) == 0.0


def test_nan_in_skipped_rows_does_not_leak():
    rng = np.random.default_rng(45)
    logits, ranges, symbols, t_lens, u_lens = make_loss_case(rng, 4, 14, 6, 40, 4)
    t_lens[1], u_lens[2] = 5, 1                               # make sure rows of both kinds are skipped
    ranges = ref.random_band(rng, 4, 14, 7, 4, t_lens, u_lens)
    clean_c, clean_g = run_hip(logits, ranges, symbols, t_lens, u_lens)
    dirty = logits.copy()
    skipped = np.zeros(dirty.shape[:3], bool)
    for b in range(4):
        skipped[b, t_lens[b]:] = True
        skipped[b][ranges[b] > u_lens[b]] = True
    assert skipped.any() and skipped[2, :t_lens[2]].any()
    dirty[skipped] = np.nan
    c, g = run_hip(dirty, ranges, symbols, t_lens, u_lens)
    np.testing.assert_array_equal(c, clean_c)
    np.testing.assert_array_equal(g, clean_g)
    assert not g[skipped].any()


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
@pytest.mark.parametrize("V", [64, 37])
def test_half_precision_logits(dtype, tol, V):
    """16-bit logits in, fp32 arithmetic inside, gradient in the input dtype: against the float64 lattice on the same
    rounded logits, at the output dtype's rounding (test_rnnt_gpu.py::test_half_precision_logits)."""
    rng = np.random.default_rng(21)
    logits, ranges, symbols, t_lens, u_lens = make_loss_case(rng, 3, 19, 7, V, 4)
    rounded = torch.tensor(logits).to(dtype).float().numpy()
    costs, grad = run_hip(rounded, ranges, symbols, t_lens, u_lens, dtype=dtype)
    want_c, want_g = ref.reference_batch(rounded, ranges, symbols, 0, t_lens, u_lens)
    assert np.isfinite(want_c).all()
    np.testing.assert_allclose(costs, want_c, rtol=tol)
    np.testing.assert_allclose(grad, want_g, rtol=tol, atol=tol * 1e-1)
    for b in range(3):
        assert not grad[b, t_lens[b]:].any() and not grad[b][ranges[b] > u_lens[b]].any()


def test_lattice_inside_the_band_matches_float64():
    """wr_rnnt_export_lattice after the pruned statistics: alpha / beta against the float64 recursion at the lattice bar of
    test_rnnt_gpu.py (rtol 1e-5, atol 1e-4) wherever a path inside the band reaches the cell, -inf elsewhere."""
    from wenet_celoss_amd.rnnt_pruned import rnnt_pruned_lattice
    rng = np.random.default_rng(46)
    B = 3
    logits, ranges, symbols, t_lens, u_lens = make_loss_case(rng, B, 90, 70, 20, 5)
    costs, alpha, beta = rnnt_pruned_lattice(torch.tensor(logits, device=DEV), torch.tensor(symbols, device=DEV),
                                             torch.tensor(ranges, device=DEV), 0, boundary_of(t_lens, u_lens))
    alpha, beta, costs = alpha.cpu().numpy(), beta.cpu().numpy(), costs.cpu().numpy()
    for b in range(B):
        T, U = int(t_lens[b]), int(u_lens[b])
        cost, a, be, _, _ = ref.lattice_pruned_f64(logits[b], ranges[b], symbols[b], 0, T, U)
        np.testing.assert_array_equal(np.isfinite(alpha[b, :T, :U + 1]), np.isfinite(a))
        np.testing.assert_array_equal(np.isfinite(beta[b, :T, :U + 1]), np.isfinite(be))
        fa, fb = np.isfinite(a), np.isfinite(be)
        np.testing.assert_allclose(alpha[b, :T, :U + 1][fa], a[fa], rtol=1e-5, atol=1e-4)
        np.testing.assert_allclose(beta[b, :T, :U + 1][fb], be[fb], rtol=1e-5, atol=1e-4)
        assert (alpha[b, :T, :U + 1][~fa] == -np.inf).all() and (beta[b, :T, :U + 1][~fb] == -np.inf).all()
        if np.isfinite(cost):
            assert abs(beta[b, 0, 0] + costs[b]) < 1e-6 * max(1.0, abs(costs[b]))


# ---------------------------------------------------------------------------- 4. identity with the full loss --
@pytest.mark.parametrize("B,T,U,V", [(3, 7, 3, 5), (4, 20, 9, 33), (2, 70, 64, 40), (3, 33, 17, 128)])
def test_whole_lattice_band_equals_the_full_loss(B, T, U, V):
    import wenet_celoss_amd as w
    rng = np.random.default_rng(B * 1000 + T * 10 + U + V)
    logits, targets, llens, tlens = test_rnnt_gpu.make_case(rng, B, T, U, V)
    ranges = ref.full_ranges(B, T, U + 1)
    costs, grad = run_hip(logits, ranges, targets.astype(np.int64), llens, tlens)
    full_c, full_g = test_rnnt_gpu.run_hip(logits, targets, llens, tlens)
    np.testing.assert_allclose(costs, full_c, **COST_TOL)
    np.testing.assert_allclose(grad, full_g, **GRAD_TOL)
    oc, og = oracle.rnnt_loss_f64(logits, targets, llens, tlens)
    np.testing.assert_allclose(costs, oc, **COST_TOL)
    np.testing.assert_allclose(grad, og, **GRAD_TOL)
    for b in range(B):
        assert not grad[b, llens[b]:].any() and not grad[b, :, tlens[b] + 1:].any()


# ------------------------------------------------------------------------------------------ 5. infeasible band --
def test_infeasible_band_costs_infinity_and_does_not_raise():
    rng = np.random.default_rng(47)
    logits, ranges, symbols, t_lens, u_lens = make_loss_case(rng, 3, 8, 6, 16, 2, full=True)
    ranges[1] = np.arange(2)                                  # b = 1 never leaves u in {0, 1}: U = 6 is out of reach
    costs, grad = run_hip(logits, ranges, symbols, t_lens, u_lens)
    want_c, want_g = ref.reference_batch(logits, ranges, symbols, 0, t_lens, u_lens)
    assert costs[1] == np.inf and want_c[1] == np.inf
    ok = [0, 2]                                               # the other utterances are untouched by it
    np.testing.assert_allclose(costs[ok], want_c[ok], **COST_TOL)
    np.testing.assert_allclose(grad[ok], want_g[ok], **GRAD_TOL)
    loss, _ = run_hip(logits, ranges, symbols, t_lens, u_lens, reduction="mean")
    assert loss == np.inf


# ---------------------------------------------------------------------------------------------------- 6. memory --
def test_step_memory_is_one_gradient_tensor_plus_workspaces():
    """B = 4, T = 400, U = 100, V = 2000, R = 5: the forward + backward step may allocate, above its inputs, at most twice
    the pruned logits' bytes plus the declared sizes of the two workspaces of pruned training (the RNN-T one, which this
    node uses, and the simple loss's) plus 16 MB.  What the node needs is one gradient tensor and the RNN-T workspace."""
    import wenet_celoss_amd as w
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    B, T, U, V, R = 4, 400, 100, 2000, 5
    rng = np.random.default_rng(48)
    t_lens, u_lens = np.array([400, 333, 250, 400]), np.array([100, 60, 100, 17])
    ranges = torch.tensor(ref.random_band(rng, B, T, U + 1, R, t_lens, u_lens), device=DEV)
    symbols = torch.randint(1, V, (B, U), device=DEV)
    bd = boundary_of(t_lens, u_lens)
    logits = torch.randn(B, T, R, V, device=DEV, requires_grad=True)
    warm = torch.randn(1, 8, R, V, device=DEV, requires_grad=True)           # load the library outside the measurement
    w.rnnt_loss_pruned(warm, symbols[:1], torch.arange(R, device=DEV).expand(1, 8, R), 0).backward()
    del warm
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss = w.rnnt_loss_pruned(logits, symbols, ranges, 0, boundary=bd, reduction="sum")
    loss.backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    logits_bytes = B * T * R * V * 4
    allowed = 2 * logits_bytes + lib.wr_rnnt_workspace_bytes(B, T, U + 1) + lib.wr_rnnt_simple_workspace_bytes(B, T, U + 1, V) \
        + 16 * 2 ** 20
    print(f"peak above inputs {peak / 2**20:.1f} MB, allowed {allowed / 2**20:.1f} MB, logits {logits_bytes / 2**20:.1f} MB")
    assert peak <= allowed
    assert torch.isfinite(loss) and torch.isfinite(logits.grad).all()


# ----------------------------------------------------------------------------------------------------- 7. model --
class TinyEncoder(torch.nn.Module):
    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)

    def forward(self, xs, xs_lens, decoding_chunk_size=0, num_decoding_left_chunks=-1):
        T = xs.size(1)
        mask = (torch.arange(T, device=xs.device)[None, :] < xs_lens[:, None].to(xs.device)).unsqueeze(1)
        return torch.tanh(self.proj(xs)), mask


def _model(**kw):
    import wenet_celoss_amd as w
    V, E, P = 23, 12, 10
    torch.manual_seed(3)
    return w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, 14, 2, dropout=0.0),
                        w.TransducerJoint(V, E, P, 16), ctc_weight=0.0, transducer_weight=1.0, hw_weight=0.0, **kw).to(DEV)


def _batch():
    g = torch.Generator().manual_seed(2)
    speech = torch.randn(3, 11, 8, generator=g).to(DEV)
    slen = torch.tensor([11, 7, 9], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9, 4, 1, 8], [4, 4, -1, -1, -1, -1, -1], [7, 1, 6, 2, -1, -1, -1]], device=DEV)
    tlen = torch.tensor([7, 2, 4], dtype=torch.int32, device=DEV)
    return speech, slen, text, tlen


def test_transducer_pruned_training_step():
    import wenet_celoss_amd as w
    m = _model(prune_range=5, simple_loss_weight=0.5)
    speech, slen, text, tlen = _batch()
    out = m(speech, slen, text, tlen)
    assert set(out.keys()) == {"loss", "loss_att", "loss_ctc", "loss_rnnt", "hw_loss", "loss_simple"}
    torch.testing.assert_close(out["loss"], out["loss_rnnt"] + 0.5 * out["loss_simple"])
    out["loss"].backward()
    for n, p in m.named_parameters():                              # the joiner's and both simple heads' included
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert not n.startswith(("joint.", "simple_")) or p.grad.abs().max() > 0, n
    assert {"joint.ffn_out.weight", "joint.enc_ffn.weight", "joint.pred_ffn.weight", "simple_am_proj.weight",
            "simple_lm_proj.weight"} <= {n for n, _ in m.named_parameters()}

    with torch.no_grad():                                          # loss_rnnt by hand from the same heads
        _, enc, _, enc_lens, _, pred, _ = m._loss_inputs(speech, slen, text, torch.IntTensor([0]), torch.IntTensor([0]))
        lm, am, symbols, boundary = m._simple_inputs(enc, enc_lens, pred, text, tlen)
        loss_simple, (px, py) = w.rnnt_loss_simple(lm, am, symbols, 0, boundary=boundary, reduction="mean", return_grad=True)
        ranges = w.get_rnnt_prune_ranges(px, py, boundary, 5)
        assert tuple(ranges.shape) == (3, 11, 5)
        logits = m.joint.forward_pruned(enc, pred, ranges)
        assert tuple(logits.shape) == (3, 11, 5, 23)
        by_hand = w.rnnt_loss_pruned(logits, symbols, ranges, 0, boundary=boundary, reduction="mean")
        # the band's logits are the full joiner's logits at the band's cells
        full = m.joint(enc, pred)
        picked = torch.gather(full, 2, ranges[..., None].expand(-1, -1, -1, 23))
        torch.testing.assert_close(logits, picked, rtol=1e-5, atol=1e-5)
    assert torch.equal(out["loss_rnnt"], by_hand) and torch.equal(out["loss_simple"], loss_simple)
    want_c, _ = ref.reference_batch(logits.cpu().numpy(), ranges.cpu().numpy(), symbols.cpu().numpy(), 0,
                                    enc_lens.cpu().numpy(), tlen.cpu().numpy())
    np.testing.assert_allclose(by_hand.item(), want_c.mean(), **COST_TOL)
    # the pruned loss drops paths: never below the full-lattice loss of the same joiner
    assert by_hand.item() >= _full_loss(m, speech, slen, text, tlen) - 1e-4


def _full_loss(m, speech, slen, text, tlen):
    with torch.no_grad():
        _, enc, _, enc_lens, _, pred, _ = m._loss_inputs(speech, slen, text, torch.IntTensor([0]), torch.IntTensor([0]))
        return m.compute_loss(enc, enc_lens, pred, text, tlen)[1].item()


def test_transducer_prune_range_zero_is_the_existing_step_and_misuse_raises():
    speech, slen, text, tlen = _batch()
    base = _model(simple_loss_weight=0.5)(speech, slen, text, tlen)
    zero = _model(simple_loss_weight=0.5, prune_range=0)(speech, slen, text, tlen)
    assert torch.equal(base["loss"], zero["loss"]) and torch.equal(base["loss_rnnt"], zero["loss_rnnt"])
    # the existing step by hand: the full-lattice loss block plus the weighted simple loss
    m = _model(simple_loss_weight=0.5)
    with torch.no_grad():
        _, enc, _, enc_lens, _, pred, _ = m._loss_inputs(speech, slen, text, torch.IntTensor([0]), torch.IntTensor([0]))
        want = 1.0 * m.compute_loss(enc, enc_lens, pred, text, tlen)[1] \
            + 0.5 * m.compute_simple_loss(enc, enc_lens, pred, text, tlen)
    assert torch.equal(base["loss"].detach(), want)
    plain = _model()(speech, slen, text, tlen)
    assert "loss_simple" not in plain and torch.equal(plain["loss"], plain["loss_rnnt"])
    with pytest.raises(ValueError, match="simple_loss_weight"):
        _model(prune_range=5)
    with pytest.raises(ValueError, match="prune_range"):
        _model(prune_range=1, simple_loss_weight=0.5)
