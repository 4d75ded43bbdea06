"""The modified lattice and the delay penalty of the k2 RNN-T losses on the GPU against float64.

References: tests/rnnt_lattice_ref.py (checked on the CPU by test_rnnt_lattice_ref.py against path enumeration): the
explicit-loop lattice for alpha / beta, the differentiable float64 torch expressions of the three losses for costs,
gradients and (through the gradient with respect to the arcs) the arc occupancies.  Tolerances are the project's bars for
these lattices against float64: cost rtol 1e-5 / atol 1e-5, gradient rtol 1e-4 / atol 1e-5, lattice rtol 1e-5 / atol 1e-4
where finite and -inf exactly where the reference has it.  Ragged lengths are drawn with T_b >= U_b unless a test says
otherwise.  The losses are called through `wenet_celoss_amd.k2`, the functions with k2's signatures (rnnt_type=,
delay_penalty=); the package-level functions of the same names keep theirs."""
import numpy as np
import pytest
import torch

import rnnt_lattice_ref as ref
import rnnt_pruned_ref as pref
import rnnt_simple_ref as sref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COST_TOL = dict(rtol=1e-5, atol=1e-5)
GRAD_TOL = dict(rtol=1e-4, atol=1e-5)
LAT_TOL = dict(rtol=1e-5, atol=1e-4)
RAGGED_TABLE = [               # the (B, T, U, V) table of test_rnnt_gpu.py::test_parity_ragged, copied
    (1, 1, 0, 2), (2, 5, 0, 7), (3, 7, 3, 5), (4, 20, 9, 33), (3, 33, 17, 128), (2, 70, 64, 40), (2, 40, 150, 36),
    (2, 12, 200, 20), (1, 9, 300, 12), (1, 6, 511, 8), (2, 9, 700, 12), (1, 5, 1023, 6), (5, 130, 30, 64),
]
MODES = [("modified", 0.0), ("modified", 0.02), ("regular", 0.02)]
SCALES = [(0.0, 0.0), (0.25, 0.0), (0.1, 0.1)]        # the simple loss, and the two smoothed settings


def boundary_of(t_lens, u_lens):
    bd = torch.zeros(len(t_lens), 4, dtype=torch.int64)
    bd[:, 2] = torch.as_tensor(np.asarray(u_lens))
    bd[:, 3] = torch.as_tensor(np.asarray(t_lens))
    return bd.to(DEV)


def make_case(rng, B, T, U, V, rnnt_type, scale=1.5, blank=0):
    """Ragged lengths (utterance 0 has all T frames, one utterance all U labels where they fit), then fixed up for the
    modified lattice: U_b <= T_b."""
    lm = (rng.normal(size=(B, U + 1, V)) * scale).astype(np.float32)
    am = (rng.normal(size=(B, T, V)) * scale).astype(np.float32)
    labels = [v for v in range(V) if v != blank]
    symbols = rng.choice(labels, size=(B, U)).astype(np.int64) if U > 0 else np.zeros((B, 0), np.int64)
    t_lens = np.concatenate([[T], rng.integers(1, T + 1, size=B - 1)]).astype(np.int64)
    u_lens = rng.integers(0, U + 1, size=B).astype(np.int64)
    u_lens[rng.integers(0, B)] = U
    if rnnt_type == "modified":                           # an utterance with more labels than frames draws U_b in [0, T_b]
        u_lens = np.where(u_lens > t_lens, rng.integers(0, t_lens + 1), u_lens)
    return lm, am, symbols, t_lens, u_lens


def loss_fn(ll, la):
    import wenet_celoss_amd as w
    if ll == 0.0 and la == 0.0:
        return w.k2.rnnt_loss_simple
    return lambda lm, am, sy, blank, **kw: w.k2.rnnt_loss_smoothed(lm, am, sy, blank, ll, la, **kw)


def run_hip(lm, am, symbols, t_lens, u_lens, ll, la, rnnt_type, dp, blank=0, grad_out=None, return_grad=False):
    l = torch.tensor(lm, device=DEV, requires_grad=True)
    a = torch.tensor(am, device=DEV, requires_grad=True)
    out = loss_fn(ll, la)(l, a, torch.tensor(symbols, device=DEV), blank, boundary=boundary_of(t_lens, u_lens),
                          reduction="none", return_grad=return_grad, rnnt_type=rnnt_type, delay_penalty=dp)
    costs = out[0] if return_grad else out
    g = torch.ones_like(costs) if grad_out is None else torch.tensor(grad_out, device=DEV, dtype=torch.float32)
    costs.backward(g)
    res = (costs.detach().cpu().numpy(), a.grad.cpu().numpy(), l.grad.cpu().numpy())
    return res + ((out[1][0].cpu().numpy(), out[1][1].cpu().numpy()),) if return_grad else res


def reference(lm, am, symbols, t_lens, u_lens, ll, la, rnnt_type, dp, blank=0, grad_out=None):
    """(costs, d_am, d_lm, occ_emit (B,T,U+1), occ_blank) in float64; the occupancies only with unit grad_costs."""
    arcs = []
    costs, (d_lm, d_am) = ref.costs_and_grads(
        lambda l, a: ref.simple_costs_torch(l, a, symbols, blank, t_lens, u_lens, ll, la, rnnt_type, dp, arcs=arcs),
        (lm, am), grad_out)
    oe, ob = ref.occupancies_from_arcs(arcs, lm.shape[0], am.shape[1], lm.shape[1])
    return costs, d_am, d_lm, oe, ob


def check(lm, am, symbols, t_lens, u_lens, ll, la, rnnt_type, dp, blank=0):
    costs, d_am, d_lm, (px, py) = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, rnnt_type, dp, blank, return_grad=True)
    want_c, want_am, want_lm, oe, ob = reference(lm, am, symbols, t_lens, u_lens, ll, la, rnnt_type, dp, blank)
    B, T, U = lm.shape[0], am.shape[1], lm.shape[1] - 1
    print("cost err", np.abs(costs - want_c).max(), "d_am err", np.abs(d_am - want_am).max(), "d_lm err",
          np.abs(d_lm - want_lm).max(), "py err", np.abs(py - ob.transpose(0, 2, 1)).max())
    assert np.isfinite(want_c).all()
    np.testing.assert_allclose(costs, want_c, **COST_TOL)
    np.testing.assert_allclose(d_am, want_am, **GRAD_TOL)
    np.testing.assert_allclose(d_lm, want_lm, **GRAD_TOL)
    # k2's layout: py_grad (B, U+1, T); px_grad (B, U, T) on the modified lattice, (B, U, T+1) with a zero last column else
    assert py.shape == (B, U + 1, T)
    np.testing.assert_allclose(py, ob.transpose(0, 2, 1), **GRAD_TOL)
    if rnnt_type == "modified":
        assert px.shape == (B, U, T)
        np.testing.assert_allclose(px, oe[:, :, :U].transpose(0, 2, 1), **GRAD_TOL)
    else:
        assert px.shape == (B, U, T + 1) and not px[:, :, T].any()
        np.testing.assert_allclose(px[:, :, :T], oe[:, :, :U].transpose(0, 2, 1), **GRAD_TOL)
    for b in range(B):                                    # padding is exactly zero (the unigram reaches padded lm rows)
        assert not d_am[b, t_lens[b]:].any()
        if la == 0.0:
            assert not d_lm[b, u_lens[b] + 1:].any()
    # without return_grad the gradient comes from the backward call: the same numbers
    c2, a2, l2 = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, rnnt_type, dp, blank)
    np.testing.assert_array_equal(c2, costs)
    np.testing.assert_allclose(a2, want_am, **GRAD_TOL)
    np.testing.assert_allclose(l2, want_lm, **GRAD_TOL)
    return costs


# --------------------------------------------------------------------------------- 1. lattice and cost, modified --
def lattice_of(lm, am, symbols, t_lens, u_lens, dp, blank=0):
    from wenet_celoss_amd.rnnt_simple import rnnt_simple_lattice
    costs, alpha, beta, flag = rnnt_simple_lattice(
        torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV), torch.tensor(symbols, device=DEV), blank,
        boundary_of(t_lens, u_lens), rnnt_type="modified", delay_penalty=dp)
    assert int(flag.item()) == 0
    return costs.cpu().numpy(), alpha.cpu().numpy(), beta.cpu().numpy()


def check_lattice(lm, am, symbols, t_lens, u_lens, dp):
    costs, alpha, beta = lattice_of(lm, am, symbols, t_lens, u_lens, dp)
    for b in range(lm.shape[0]):
        T, U = int(t_lens[b]), int(u_lens[b])
        skip, emit = sref.log_probs_f64(lm[b, :U + 1], am[b, :T], symbols[b], 0)
        emit = ref.penalised(emit, dp)
        cost, ra, rb, _, _ = ref.lattice_modified_f64(skip, emit)
        print("b", b, "T", T, "U", U, "cost", costs[b], cost)
        np.testing.assert_allclose(costs[b], cost, **COST_TOL)
        for got, want in ((alpha[b, :T, :U + 1], ra), (beta[b, :T, :U + 1], rb)):
            fin = np.isfinite(want)
            np.testing.assert_array_equal(got[~fin], want[~fin])          # -inf exactly where no path passes
            np.testing.assert_allclose(got[fin], want[fin], **LAT_TOL)
        assert not alpha[b, T:].any() and not alpha[b, :, U + 1:].any()   # zero outside the boundary
        assert not beta[b, T:].any() and not beta[b, :, U + 1:].any()
        if T == U:                                                        # the single path: a label on every frame
            np.testing.assert_allclose(costs[b], -sum(emit[t, t] for t in range(T)), **COST_TOL)


@pytest.mark.parametrize("T", [1, 7, 8, 9, 70])                 # around the prefetch depth of the sweep
@pytest.mark.parametrize("U1", [1, 2, 64, 65, 129])             # wave boundaries
def test_modified_lattice_and_cost(U1, T):
    """U + 1 label columns and T frames; utterance 0 is full length with U_0 = min(U, T) (T <= U: T_b = U_b, the single
    path), utterance 1 is ragged."""
    rng = np.random.default_rng(1000 * U1 + T)
    U, V = U1 - 1, 5
    lm = (rng.normal(size=(2, U1, V)) * 1.5).astype(np.float32)
    am = (rng.normal(size=(2, T, V)) * 1.5).astype(np.float32)
    symbols = rng.integers(1, V, size=(2, U)).astype(np.int64)
    t1 = int(rng.integers(1, T + 1))
    t_lens = np.array([T, t1])
    u_lens = np.array([min(U, T), int(rng.integers(0, min(U, t1) + 1))])
    check_lattice(lm, am, symbols, t_lens, u_lens, 0.0)
    check_lattice(lm, am, symbols, t_lens, u_lens, 0.05)


def test_modified_lattice_ragged_batch_over_several_waves():
    rng = np.random.default_rng(2)
    B, T, U, V = 5, 40, 140, 6
    lm = (rng.normal(size=(B, U + 1, V)) * 1.5).astype(np.float32)
    am = (rng.normal(size=(B, T, V)) * 1.5).astype(np.float32)
    symbols = rng.integers(1, V, size=(B, U)).astype(np.int64)
    t_lens = np.array([40, 33, 40, 9, 1])
    u_lens = np.array([40, 12, 0, 9, 1])          # T_b = U_b three times, U_b = 0 once
    check_lattice(lm, am, symbols, t_lens, u_lens, 0.0)
    check_lattice(lm, am, symbols, t_lens, u_lens, 0.01)


def test_modified_frameless_utterance_beside_live_ones_over_two_waves():
    """T_b = 0 between two live utterances at U1 = 65: its two workgroups leave through the sweep's early exit while the
    others run the two-wave barrier path.  Costs, gradients and occupancies against the float64 reference, which gives
    the frameless utterance cost 0."""
    rng = np.random.default_rng(65)
    B, T, U, V = 3, 9, 64, 17
    lm, am, symbols, _, _ = make_case(rng, B, T, U, V, "modified")
    t_lens, u_lens = np.array([T, 0, 5]), np.array([T, 0, 3])
    costs = check(lm, am, symbols, t_lens, u_lens, 0.0, 0.0, "modified", 0.0)
    assert costs[1] == 0


# -------------------------------------------------------------------------------- 2. simple and smoothed losses --
@pytest.mark.parametrize("rnnt_type,dp", MODES)
@pytest.mark.parametrize("ll,la", SCALES)
@pytest.mark.parametrize("B,T,U,V", RAGGED_TABLE)
def test_parity_ragged(B, T, U, V, ll, la, rnnt_type, dp):
    rng = np.random.default_rng(B * 1000 + T * 10 + U + V)
    check(*make_case(rng, B, T, U, V, rnnt_type), ll, la, rnnt_type, dp)


@pytest.mark.parametrize("rnnt_type,dp", MODES)
@pytest.mark.parametrize("ll,la", SCALES)
@pytest.mark.parametrize("V", [2, 31, 5000])
def test_parity_vocabularies(V, ll, la, rnnt_type, dp):
    rng = np.random.default_rng(V)
    check(*make_case(rng, 2, 37, 11, V, rnnt_type, scale=1.0), ll, la, rnnt_type, dp)


@pytest.mark.parametrize("ll,la", SCALES)
def test_modified_blank_nonzero_label_equal_blank_and_repeated_label(ll, la):
    """On the modified lattice a label equal to the blank has both its terms subtracted, for the simple loss too."""
    rng = np.random.default_rng(5)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 25, 11, 48, "modified", blank=47)
    symbols[:, 3] = 47
    symbols[:, 7] = symbols[:, 2]
    check(lm, am, symbols, t_lens, u_lens, ll, la, "modified", 0.01, blank=47)


@pytest.mark.parametrize("ll,la", SCALES)
@pytest.mark.parametrize("rnnt_type,dp", MODES)
def test_unequal_grad_costs(ll, la, rnnt_type, dp):
    rng = np.random.default_rng(6)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 19, 7, 23, rnnt_type)
    g = np.array([0.5, -2.0, 1.25])
    want = reference(lm, am, symbols, t_lens, u_lens, ll, la, rnnt_type, dp, grad_out=g)
    for return_grad in (False, True):
        got = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, rnnt_type, dp, grad_out=g, return_grad=return_grad)
        np.testing.assert_allclose(got[0], want[0], **COST_TOL)
        np.testing.assert_allclose(got[1], want[1], **GRAD_TOL)
        np.testing.assert_allclose(got[2], want[2], **GRAD_TOL)


def test_opposed_peaks_take_the_direct_path_on_the_modified_lattice():
    """The input of test_rnnt_simple_gpu.py::test_opposed_peaks_take_the_direct_path: the factored sum is exactly 0 in
    fp32, the flag goes up, and the direct kernels redo statistics and gradient -- from the modified lattice's
    occupancies."""
    from wenet_celoss_amd.rnnt_simple import rnnt_simple_lattice
    rng = np.random.default_rng(11)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 40, 8, 5000, "modified", scale=1.0)
    am[..., 3] += 120
    lm[..., 7] += 120
    flag = rnnt_simple_lattice(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV), torch.tensor(symbols, device=DEV),
                               0, boundary_of(t_lens, u_lens), rnnt_type="modified")[3]
    assert int(flag.item()) == 1
    check(lm, am, symbols, t_lens, u_lens, 0.0, 0.0, "modified", 0.0)
    check(lm, am, symbols, t_lens, u_lens, 0.25, 0.0, "modified", 0.01)


# ------------------------------------------------------------------------------------------------ 3. pruned loss --
def make_band_case(rng, B, T, U, V, R, rnnt_type, full=False):
    """Ragged lengths with U_b <= T_b, a random valid band (rnnt_pruned_ref.random_band) and logits on it."""
    symbols = rng.integers(1, V, size=(B, U)).astype(np.int64)
    if full:
        t_lens, u_lens = np.full(B, T, np.int64), np.full(B, U, np.int64)
    else:
        t_lens = np.concatenate([[T], rng.integers(1, T + 1, size=B - 1)]).astype(np.int64)
        u_lens = rng.integers(0, U + 1, size=B).astype(np.int64)
        u_lens[rng.integers(0, B)] = U
    R = min(R, U + 1)
    t_lens = np.minimum(T, np.maximum(t_lens, np.maximum(u_lens - R + 1, 0) + 1))
    if rnnt_type == "modified":
        u_lens = np.where(u_lens > t_lens, rng.integers(0, t_lens + 1), u_lens)
    ranges = pref.random_band(rng, B, T, U + 1, R, t_lens, u_lens)
    logits = (rng.normal(size=(B, T, R, V)) * 1.5).astype(np.float32)
    return logits, ranges, symbols, t_lens, u_lens


def run_pruned(logits, ranges, symbols, t_lens, u_lens, rnnt_type, dp, dtype=torch.float32, grad_out=None):
    import wenet_celoss_amd as w
    x = torch.tensor(logits, device=DEV).to(dtype).requires_grad_(True)
    costs = w.k2.rnnt_loss_pruned(x, torch.tensor(symbols, device=DEV), torch.tensor(ranges, device=DEV), 0,
                               boundary=boundary_of(t_lens, u_lens), reduction="none", rnnt_type=rnnt_type,
                               delay_penalty=dp)
    assert costs.dtype == torch.float32
    g = torch.ones_like(costs) if grad_out is None else torch.tensor(grad_out, device=DEV, dtype=torch.float32)
    costs.backward(g)
    assert x.grad.dtype == dtype
    return costs.detach().cpu().numpy(), x.grad.float().cpu().numpy()


def pruned_reference(logits, ranges, symbols, t_lens, u_lens, rnnt_type, dp, grad_out=None):
    costs, (grad,) = ref.costs_and_grads(
        lambda x: ref.pruned_costs_torch(x, ranges, symbols, 0, t_lens, u_lens, rnnt_type, dp), (logits,), grad_out)
    return costs, grad


def check_pruned(logits, ranges, symbols, t_lens, u_lens, rnnt_type, dp, dtype=torch.float32, tol=None):
    costs, grad = run_pruned(logits, ranges, symbols, t_lens, u_lens, rnnt_type, dp, dtype=dtype)
    want_c, want_g = pruned_reference(logits, ranges, symbols, t_lens, u_lens, rnnt_type, dp)
    print("cost err", np.abs(costs - want_c).max(), "grad err", np.abs(grad - want_g).max())
    assert np.isfinite(want_c).all()
    if tol is None:
        np.testing.assert_allclose(costs, want_c, **COST_TOL)
        np.testing.assert_allclose(grad, want_g, **GRAD_TOL)
    else:                                                     # 16-bit logits: the output dtype's rounding
        np.testing.assert_allclose(costs, want_c, rtol=tol)
        np.testing.assert_allclose(grad, want_g, rtol=tol, atol=tol * 1e-1)
    for b in range(logits.shape[0]):                          # every element of a skipped row is zero
        assert not grad[b, t_lens[b]:].any()
        assert not grad[b][ranges[b] > u_lens[b]].any()
    return costs, grad


BAND_SHAPES = [(3, 19, 7, 40, 1), (3, 19, 7, 40, 2), (4, 33, 17, 31, 5), (2, 70, 64, 20, 5), (2, 9, 0, 7, 1)]
# R = 1 is legal on the modified lattice only (a regular path needs two positions on the frame that emits a label)
BAND_CASES = [shape + mode for shape in BAND_SHAPES for mode in MODES
              if mode[0] == "modified" or shape[4] > 1 or shape[2] == 0]


@pytest.mark.parametrize("B,T,U,V,R,rnnt_type,dp", BAND_CASES)
def test_pruned_parity_on_random_bands(B, T, U, V, R, rnnt_type, dp):
    rng = np.random.default_rng(100 * T + 10 * U + R)
    check_pruned(*make_band_case(rng, B, T, U, V, R, rnnt_type), rnnt_type, dp)


@pytest.mark.parametrize("rnnt_type,dp", MODES)
def test_pruned_half_precision_logits(rnnt_type, dp):
    """fp16 logits in, fp32 arithmetic inside, gradient in fp16: against float64 on the same rounded logits at the
    output dtype's rounding (test_rnnt_pruned_gpu.py::test_half_precision_logits)."""
    rng = np.random.default_rng(21)
    logits, ranges, symbols, t_lens, u_lens = make_band_case(rng, 3, 19, 7, 64, 4, rnnt_type)
    rounded = torch.tensor(logits).to(torch.float16).float().numpy()
    check_pruned(rounded, ranges, symbols, t_lens, u_lens, rnnt_type, dp, dtype=torch.float16, tol=2e-3)


@pytest.mark.parametrize("dp", [0.0, 0.02])
def test_full_width_band_equals_the_unpruned_modified_loss(dp):
    import wenet_celoss_amd as w
    rng = np.random.default_rng(31)
    B, T, U, V = 3, 20, 9, 33
    lm, am, symbols, t_lens, u_lens = make_case(rng, B, T, U, V, "modified")
    logits = sref.materialised(lm, am)
    ranges = pref.full_ranges(B, T, U + 1)
    costs, grad = run_pruned(logits, ranges, symbols, t_lens, u_lens, "modified", dp)
    simple = w.k2.rnnt_loss_simple(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV), torch.tensor(symbols, device=DEV),
                                0, boundary=boundary_of(t_lens, u_lens), reduction="none", rnnt_type="modified",
                                delay_penalty=dp).cpu().numpy()
    np.testing.assert_allclose(costs, simple, **COST_TOL)
    want_c, want_am, want_lm, _, _ = reference(lm, am, symbols, t_lens, u_lens, 0.0, 0.0, "modified", dp)
    np.testing.assert_allclose(costs, want_c, **COST_TOL)
    np.testing.assert_allclose(grad.sum(2, dtype=np.float64), want_am, **GRAD_TOL)
    np.testing.assert_allclose(grad.sum(1, dtype=np.float64), want_lm, **GRAD_TOL)


def test_pruned_nan_in_skipped_rows_does_not_leak():
    rng = np.random.default_rng(45)
    logits, ranges, symbols, t_lens, u_lens = make_band_case(rng, 4, 14, 6, 40, 4, "modified")
    t_lens[1], u_lens[1], u_lens[2] = 5, 3, 1                 # make sure rows of both kinds are skipped
    ranges = pref.random_band(rng, 4, 14, 7, 4, t_lens, u_lens)
    clean_c, clean_g = run_pruned(logits, ranges, symbols, t_lens, u_lens, "modified", 0.02)
    dirty = logits.copy()
    skipped = np.zeros(dirty.shape[:3], bool)
    for b in range(4):
        skipped[b, t_lens[b]:] = True
        skipped[b][ranges[b] > u_lens[b]] = True
    assert skipped.any() and skipped[2, :t_lens[2]].any()
    dirty[skipped] = np.nan
    c, g = run_pruned(dirty, ranges, symbols, t_lens, u_lens, "modified", 0.02)
    assert np.isfinite(clean_c).all()
    np.testing.assert_array_equal(c, clean_c)
    np.testing.assert_array_equal(g, clean_g)
    assert not g[skipped].any()


# ----------------------------------------------------------------------------------------------- 4. prune ranges --
@pytest.mark.parametrize("B,T,U,V,R", [(3, 21, 8, 17, 1), (3, 21, 8, 17, 3), (2, 70, 40, 9, 5), (2, 1100, 6, 5, 2)])
def test_ranges_from_modified_occupancies_equal_the_reference_on_every_frame(B, T, U, V, R):
    import wenet_celoss_amd as w
    rng = np.random.default_rng(B + T + U + R)
    lm, am, symbols, t_lens, u_lens = make_case(rng, B, T, U, V, "modified")
    bd = boundary_of(t_lens, u_lens)
    _, (px, py) = w.k2.rnnt_loss_simple(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV),
                                     torch.tensor(symbols, device=DEV), 0, boundary=bd, return_grad=True,
                                     rnnt_type="modified", delay_penalty=0.01)
    assert px.shape == (B, U, T) and py.shape == (B, U + 1, T)
    ranges = w.k2.get_rnnt_prune_ranges(px, py, bd, R).cpu().numpy()
    want = ref.prune_ranges_ref(px.cpu().numpy(), py.cpu().numpy(), bd.cpu().numpy(), R)
    np.testing.assert_array_equal(ranges, want)
    pref.check_range_properties(ranges, bd.cpu().numpy(), U + 1)
    # the (B, U, T+1) form of the same occupancies gives the same band
    px1 = torch.cat([px, torch.zeros(B, U, 1, device=DEV)], 2)
    if R >= 2:
        assert torch.equal(w.k2.get_rnnt_prune_ranges(px1, py, bd, R).cpu(), torch.as_tensor(want))


# ------------------------------------------------------------------------------------- 5. one infeasible utterance --
@pytest.mark.parametrize("ll,la", [(0.0, 0.0), (0.25, 0.0)])
def test_one_infeasible_utterance_costs_infinity_and_leaves_the_others_alone(ll, la):
    """T_b < U_b has no path on the modified lattice: +inf for that utterance, a value, not an error.  With
    am_only_scale > 0 the unigram couples the utterances' gradients, so that setting is not part of this test."""
    rng = np.random.default_rng(51)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 12, 8, 19, "modified")
    t_lens[:], u_lens[:] = [12, 5, 9], [8, 7, 3]             # b = 1: five frames for seven labels
    g = np.array([1.0, 0.0, -0.5])
    costs, d_am, d_lm = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, "modified", 0.01, grad_out=g)
    want_c, want_am, want_lm, _, _ = reference(lm, am, symbols, t_lens, u_lens, ll, la, "modified", 0.01, grad_out=g)
    assert costs[1] == np.inf and want_c[1] == np.inf
    ok = [0, 2]
    np.testing.assert_allclose(costs[ok], want_c[ok], **COST_TOL)
    np.testing.assert_allclose(d_am[ok], want_am[ok], **GRAD_TOL)
    np.testing.assert_allclose(d_lm[ok], want_lm[ok], **GRAD_TOL)
    loss = loss_fn(ll, la)(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV), torch.tensor(symbols, device=DEV), 0,
                           boundary=boundary_of(t_lens, u_lens), rnnt_type="modified")
    assert loss.item() == np.inf


def test_one_infeasible_utterance_in_the_pruned_loss():
    rng = np.random.default_rng(52)
    logits, ranges, symbols, t_lens, u_lens = make_band_case(rng, 3, 12, 8, 19, 9, "modified", full=True)
    t_lens[:], u_lens[:] = [12, 5, 9], [8, 7, 3]
    g = np.array([1.0, 0.0, -0.5])
    costs, grad = run_pruned(logits, ranges, symbols, t_lens, u_lens, "modified", 0.01, grad_out=g)
    want_c, want_g = pruned_reference(logits, ranges, symbols, t_lens, u_lens, "modified", 0.01, grad_out=g)
    assert costs[1] == np.inf and want_c[1] == np.inf
    ok = [0, 2]
    np.testing.assert_allclose(costs[ok], want_c[ok], **COST_TOL)
    np.testing.assert_allclose(grad[ok], want_g[ok], **GRAD_TOL)


# ------------------------------------------------------------------------------------------------ 6. bit identity --
def test_explicit_defaults_are_the_existing_path_bit_for_bit():
    import wenet_celoss_amd as w
    rng = np.random.default_rng(61)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 33, 17, 128, "regular")
    bd = boundary_of(t_lens, u_lens)
    sy = torch.tensor(symbols, device=DEV)

    def run(fn, *args, **kw):
        leaves = [torch.tensor(x, device=DEV, requires_grad=True) for x in args]
        out = fn(*leaves, **kw)
        loss = out[0] if isinstance(out, tuple) else out
        loss.backward()
        extra = list(out[1]) if isinstance(out, tuple) else []
        return [loss.detach()] + [x.grad for x in leaves] + extra

    explicit = dict(rnnt_type="regular", delay_penalty=0.0)

    def pick(name, kw):                    # without the keywords: the package-level function; with them: the k2 form
        return getattr(w.k2 if kw else w, name)

    for rg in (False, True):
        for fn in (lambda l, a, **kw: pick("rnnt_loss_simple", kw)(l, a, sy, 0, boundary=bd, return_grad=rg, **kw),
                   lambda l, a, **kw: pick("rnnt_loss_smoothed", kw)(l, a, sy, 0, 0.25, 0.0, boundary=bd, return_grad=rg, **kw),
                   lambda l, a, **kw: pick("rnnt_loss_smoothed", kw)(l, a, sy, 0, 0.1, 0.1, boundary=bd, return_grad=rg, **kw)):
            for x, y in zip(run(fn, lm, am), run(fn, lm, am, **explicit)):
                assert torch.equal(x, y)
    logits, ranges, symbols, t_lens, u_lens = make_band_case(rng, 3, 19, 7, 40, 4, "regular")
    rgs, bd, sy = torch.tensor(ranges, device=DEV), boundary_of(t_lens, u_lens), torch.tensor(symbols, device=DEV)
    fn = lambda x, **kw: w.rnnt_loss_pruned(x, sy, rgs, 0, boundary=bd, **kw)     # noqa: E731
    for x, y in zip(run(fn, logits), run(fn, logits, **explicit)):
        assert torch.equal(x, y)


def test_modified_backward_is_bit_identical_run_to_run():
    rng = np.random.default_rng(62)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 4, 150, 40, 700, "modified")
    symbols[:, 10:20] = symbols[:, :10]                             # repeated labels: the chained scatter terms
    for ll, la in SCALES:
        first = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, "modified", 0.01)
        second = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, "modified", 0.01)
        for x, y in zip(first, second):
            assert np.array_equal(x, y)
    case = make_band_case(rng, 3, 60, 30, 200, 5, "modified")
    for x, y in zip(run_pruned(*case, "modified", 0.01), run_pruned(*case, "modified", 0.01)):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------- 7. model layer --
def test_transducer_trains_on_the_modified_lattice_with_a_delay_penalty():
    import wenet_celoss_amd as w
    from test_transducer_gpu import TinyEncoder
    V, E, P = 23, 12, 10
    kw = dict(rnnt_type="modified", delay_penalty=0.01)
    torch.manual_seed(3)
    m = w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, 14, 2, dropout=0.0),
                     w.TransducerJoint(V, E, P, 16), ctc_weight=0.0, transducer_weight=1.0, hw_weight=0.0,
                     prune_range=5, simple_loss_weight=0.5, lm_only_scale=0.25, **kw).to(DEV)
    g = torch.Generator().manual_seed(2)
    speech = torch.randn(3, 11, 8, generator=g).to(DEV)
    slen = torch.tensor([11, 7, 9], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9], [4, 4, -1, -1], [7, 1, 6, -1]], device=DEV)
    tlen = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    out = m(speech, slen, text, tlen)
    assert torch.isfinite(out["loss"])
    torch.testing.assert_close(out["loss"], out["loss_rnnt"] + 0.5 * out["loss_simple"])
    with torch.no_grad():                                   # loss_rnnt is the composition of the public functions
        _, enc, _, enc_lens, _, pred, _ = m._loss_inputs(speech, slen, text, torch.IntTensor([0]), torch.IntTensor([0]))
        lm, am, symbols, boundary = m._simple_inputs(enc, enc_lens, pred, text, tlen)
        simple, (px, py) = w.k2.rnnt_loss_smoothed(lm, am, symbols, 0, lm_only_scale=0.25, am_only_scale=0.0,
                                                boundary=boundary, return_grad=True, **kw)
        assert px.shape == (3, 4, enc.shape[1])
        ranges = w.k2.get_rnnt_prune_ranges(px, py, boundary, 5)
        logits = m.joint.forward_pruned(enc, pred, ranges)
        pruned = w.k2.rnnt_loss_pruned(logits, symbols, ranges, 0, boundary=boundary, **kw)
        regular = w.rnnt_loss_smoothed(lm, am, symbols, 0, lm_only_scale=0.25, am_only_scale=0.0, boundary=boundary)
    assert torch.equal(out["loss_simple"], simple)
    assert torch.equal(out["loss_rnnt"], pruned)
    assert abs(simple.item() - regular.item()) > 1e-3
    want = ref.simple_costs_torch(lm.cpu(), am.cpu(), symbols.cpu().numpy(), 0, enc_lens.cpu(), tlen.cpu(), 0.25, 0.0,
                                  "modified", 0.01).mean()
    np.testing.assert_allclose(simple.item(), want.item(), **COST_TOL)
    opt = torch.optim.SGD(m.parameters(), lr=1e-3)
    out["loss"].backward()
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    opt.step()
    assert torch.isfinite(m(speech, slen, text, tlen)["loss"])
