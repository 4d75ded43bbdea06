"""The smoothed additive-joiner loss (rnnt_loss_smoothed) on the GPU against the float64 references of
tests/rnnt_smoothed_ref.py, computed on the CPU.  Tolerances are the project's bar for this lattice against float64
(test_rnnt_simple_gpu.py): cost rtol 1e-5 / atol 1e-5, gradients and occupancies rtol 1e-4 / atol 1e-5."""
import numpy as np
import pytest
import torch

import rnnt_smoothed_ref as ref
from test_rnnt_simple_gpu import TinyEncoder, boundary_of, make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COST_TOL = dict(rtol=1e-5, atol=1e-5)
GRAD_TOL = dict(rtol=1e-4, atol=1e-5)
SCALES = [(0.25, 0.0), (0.0, 0.3), (0.1, 0.1), (0.5, 0.5)]


def run_hip(lm, am, symbols, t_lens, u_lens, ll, la, blank=0, reduction="none", grad_out=None, return_grad=False,
            fn=None):
    import wenet_celoss_amd as w
    l = torch.tensor(lm, device=DEV, requires_grad=True)
    a = torch.tensor(am, device=DEV, requires_grad=True)
    sy, bd = torch.tensor(symbols, device=DEV), boundary_of(t_lens, u_lens)
    if fn is None:
        out = w.rnnt_loss_smoothed(l, a, sy, blank, ll, la, boundary=bd, reduction=reduction, return_grad=return_grad)
    else:
        out = fn(l, a, sy, blank, boundary=bd, reduction=reduction, return_grad=return_grad)
    loss = out[0] if return_grad else out
    if grad_out is None:
        loss.sum().backward()
    else:
        loss.backward(torch.tensor(grad_out, device=DEV, dtype=torch.float32))
    res = (loss.detach().cpu().numpy(), a.grad.cpu().numpy(), l.grad.cpu().numpy())
    return res + ((out[1][0].cpu().numpy(), out[1][1].cpu().numpy()),) if return_grad else res


def reference(lm, am, symbols, t_lens, u_lens, ll, la, blank=0, grad_out=None):
    """(costs, d_am, d_lm) of sum_b grad_out[b] * cost_b (grad_out None = 1) in float64 from reference (a)."""
    tl = torch.tensor(lm, dtype=torch.float64, requires_grad=True)
    ta = torch.tensor(am, dtype=torch.float64, requires_grad=True)
    costs = ref.loss_torch_f64(tl, ta, symbols, blank, t_lens, u_lens, ll, la)
    g = torch.ones(len(t_lens), dtype=torch.float64) if grad_out is None else torch.tensor(grad_out, dtype=torch.float64)
    (costs * g).sum().backward()
    return costs.detach().numpy(), ta.grad.numpy(), tl.grad.numpy()


def occupancies(lm, am, symbols, t_lens, u_lens, ll, la, blank=0):
    """(px_grad (B,U,T+1), py_grad (B,U+1,T)) in float64 from reference (b)."""
    B, U1, _ = lm.shape
    T = am.shape[1]
    pbar = ref.pbar_f64(lm)
    px, py = np.zeros((B, U1 - 1, T + 1)), np.zeros((B, U1, T))
    lat = []
    for b in range(B):
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        out = ref.lattice_f64(lm[b], am[b], symbols[b], blank, Tb, Ub, pbar, ll, la)
        px[b, :Ub, :Tb] = out[3][:, :Ub].T
        py[b, :Ub + 1, :Tb] = out[4].T
        lat.append(out)
    return px, py, lat


def check(lm, am, symbols, t_lens, u_lens, ll, la, blank=0, expect_flag=None):
    oc, o_am, o_lm = reference(lm, am, symbols, t_lens, u_lens, ll, la, blank)
    plain = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, blank=blank)
    with_occ = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, blank=blank, return_grad=True)
    for costs, d_am, d_lm in (plain, with_occ[:3]):
        print("cost err", np.abs(costs - oc).max(), "d_am err", np.abs(d_am - o_am).max(), "d_lm err",
              np.abs(d_lm - o_lm).max())
        assert np.isfinite(costs).all() and np.isfinite(d_am).all() and np.isfinite(d_lm).all()
        np.testing.assert_allclose(costs, oc, **COST_TOL)
        np.testing.assert_allclose(d_am, o_am, **GRAD_TOL)
        np.testing.assert_allclose(d_lm, o_lm, **GRAD_TOL)
        for b in range(lm.shape[0]):
            assert not d_am[b, t_lens[b]:].any()
            if la == 0:
                assert not d_lm[b, u_lens[b] + 1:].any()
    px, py = with_occ[3]
    for b in range(lm.shape[0]):                          # every path takes T_b blank arcs and U_b emit arcs
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        assert abs(py[b].sum() - Tb) <= 1e-4 * Tb and abs(px[b].sum() - Ub) <= 1e-4 * max(Ub, 1)
        assert not px[b, Ub:].any() and not px[b, :, Tb:].any() and not py[b, Ub + 1:].any() and not py[b, :, Tb:].any()
    if expect_flag is not None:
        assert flag_of(lm, am, symbols, t_lens, u_lens, ll, la, blank) == expect_flag
    return with_occ


def flag_of(lm, am, symbols, t_lens, u_lens, ll, la, blank=0):
    from wenet_celoss_amd.rnnt_smoothed import rnnt_smoothed_lattice
    return int(rnnt_smoothed_lattice(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV),
                                     torch.tensor(symbols, device=DEV), blank, ll, la, boundary_of(t_lens, u_lens))[3].item())


# ---------------------------------------------------------------------------------------------- 1. parity --
# shapes that cross every tile edge: 64 x 64 lattice tile, 32-deep v slice, 64 x 128 gradient tile
@pytest.mark.parametrize("ll,la", SCALES)
@pytest.mark.parametrize("B,T,U,V", [(1, 1, 0, 2), (3, 7, 3, 5), (3, 33, 17, 128), (2, 70, 64, 40), (2, 40, 150, 36),
                                     (5, 130, 30, 64)])
def test_parity_ragged(B, T, U, V, ll, la):
    rng = np.random.default_rng(B * 1000 + T * 10 + U + V)
    check(*make_case(rng, B, T, U, V, scale=1.5), ll, la, expect_flag=0)


@pytest.mark.parametrize("ll,la", SCALES)
@pytest.mark.parametrize("V", [31, 129, 500])
def test_parity_vocabularies(V, ll, la):
    rng = np.random.default_rng(V)
    check(*make_case(rng, 2, 37, 11, V), ll, la)


@pytest.mark.parametrize("ll,la", SCALES)
def test_parity_blank_nonzero_label_equal_blank_and_repeated_label(ll, la):
    rng = np.random.default_rng(5)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 25, 11, 48, full=True, blank=47)
    t_lens[1], u_lens[2] = 19, 8
    symbols[:, 3] = 47                                    # a label equal to the blank, and a repeated label
    symbols[:, 7] = symbols[:, 2]
    check(lm, am, symbols, t_lens, u_lens, ll, la, blank=47)


def test_occupancies_agree_with_the_loop_reference():
    rng = np.random.default_rng(14)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 12, 5, 9)
    symbols[:, 4] = symbols[:, 1]
    for ll, la in SCALES:
        _, _, _, (px, py) = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, return_grad=True)
        want_px, want_py, _ = occupancies(lm, am, symbols, t_lens, u_lens, ll, la)
        assert px.shape == want_px.shape and py.shape == want_py.shape
        np.testing.assert_allclose(px, want_px, **GRAD_TOL)
        np.testing.assert_allclose(py, want_py, **GRAD_TOL)
        for b in range(3):
            Tb, Ub = int(t_lens[b]), int(u_lens[b])
            assert abs(py[b].sum() - Tb) <= 1e-4 * Tb and abs(px[b].sum() - Ub) <= 1e-4 * max(Ub, 1)


# --------------------------------------------------------------------------------------- 2. the unigram term --
def test_unigram_term_on_padded_rows_is_not_hidden_by_atol():
    """B = 1, U = 3, U_b = 1: rows 2 and 3 of lm are padded and receive only the unigram term, compared with an atol
    scaled to their own size."""
    rng = np.random.default_rng(21)
    lm, am, symbols, _, _ = make_case(rng, 1, 6, 3, 5, full=True)
    t_lens, u_lens = np.array([6]), np.array([1])
    _, o_am, o_lm = reference(lm, am, symbols, t_lens, u_lens, 0.0, 0.5)
    _, d_am, d_lm = run_hip(lm, am, symbols, t_lens, u_lens, 0.0, 0.5)
    big = np.abs(o_lm[0, 2:]).max()
    print("padded rows: largest reference magnitude", big, "largest error", np.abs(d_lm[0, 2:] - o_lm[0, 2:]).max())
    assert big > 0
    np.testing.assert_allclose(d_lm[0, 2:], o_lm[0, 2:], rtol=1e-4, atol=1e-5 * big)
    np.testing.assert_allclose(d_lm, o_lm, **GRAD_TOL)
    np.testing.assert_allclose(d_am, o_am, **GRAD_TOL)


# ---------------------------------------------------------------------------------------------- 3. identity --
def test_zero_scales_are_rnnt_loss_simple_bit_for_bit():
    import wenet_celoss_amd as w
    rng = np.random.default_rng(31)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 70, 20, 130)
    symbols[:, 9] = symbols[:, 2]
    gw = np.array([0.5, -2.0, 1.25], np.float32)
    for return_grad in (False, True):
        got = run_hip(lm, am, symbols, t_lens, u_lens, 0.0, 0.0, grad_out=gw, return_grad=return_grad)
        want = run_hip(lm, am, symbols, t_lens, u_lens, 0.0, 0.0, grad_out=gw, return_grad=return_grad,
                       fn=w.rnnt_loss_simple)
        for x, y in zip(got[:3], want[:3]):
            np.testing.assert_array_equal(x, y)
        if return_grad:
            np.testing.assert_array_equal(got[3][0], want[3][0])
            np.testing.assert_array_equal(got[3][1], want[3][1])


# --------------------------------------------------------------------------------- 4. cross-utterance gradient --
@pytest.mark.parametrize("ll,la", [(0.0, 0.3), (0.1, 0.1), (0.25, 0.0)])
def test_unequal_grad_costs_with_and_without_return_grad(ll, la):
    rng = np.random.default_rng(41)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 21, 8, 40)
    gw = np.array([0.5, -2.0, 1.25], np.float32)
    oc, o_am, o_lm = reference(lm, am, symbols, t_lens, u_lens, ll, la, grad_out=gw)
    for return_grad in (False, True):
        got = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, grad_out=gw, return_grad=return_grad)
        np.testing.assert_allclose(got[0], oc, **COST_TOL)
        np.testing.assert_allclose(got[1], o_am, **GRAD_TOL)
        np.testing.assert_allclose(got[2], o_lm, **GRAD_TOL)
    for reduction, scale in (("sum", 1.0), ("mean", 1.0 / 3)):
        oc1, o_am1, o_lm1 = reference(lm, am, symbols, t_lens, u_lens, ll, la, grad_out=np.full(3, scale))
        loss, d_am, d_lm = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, reduction=reduction)
        np.testing.assert_allclose(loss, oc1.sum() * scale, **COST_TOL)
        np.testing.assert_allclose(d_am, o_am1, **GRAD_TOL)
        np.testing.assert_allclose(d_lm, o_lm1, **GRAD_TOL)


# ------------------------------------------------------------------------------------------- 5. direct path --
def test_opposed_peaks_take_the_direct_path_under_smoothing():
    """The input of test_rnnt_simple_gpu.py::test_opposed_peaks_take_the_direct_path: the factored sum is exactly 0 in
    fp32, the flag is raised, and the interpolation sees the repaired denom."""
    rng = np.random.default_rng(11)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 40, 8, 5000)
    peak_am, peak_lm = am.copy(), lm.copy()
    peak_am[..., 3] += 120
    peak_lm[..., 7] += 120
    check(peak_lm, peak_am, symbols, t_lens, u_lens, 0.1, 0.1, expect_flag=1)


# ----------------------------------------------------------------------------------------------- 6. padding --
def test_padded_region_is_zero_and_nan_in_padded_am_does_not_leak():
    rng = np.random.default_rng(12)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 4, 70, 66, 37)
    t_lens[1], u_lens[1] = 33, 20
    dirty_am = am.copy()
    for b in range(4):
        dirty_am[b, t_lens[b]:] = np.nan
    for ll, la in ((0.25, 0.0), (0.1, 0.1)):
        clean = run_hip(lm, am, symbols, t_lens, u_lens, ll, la, return_grad=True)
        got = run_hip(lm, dirty_am, symbols, t_lens, u_lens, ll, la, return_grad=True)
        for x, y in zip(clean[:3] + clean[3], got[:3] + got[3]):
            np.testing.assert_array_equal(x, y)
        for b in range(4):
            assert not got[1][b, t_lens[b]:].any()
            if la == 0:
                assert not got[2][b, u_lens[b] + 1:].any()
    dirty_lm = lm.copy()                                  # am_only_scale == 0: padded lm rows are not read into anything
    for b in range(4):
        dirty_lm[b, u_lens[b] + 1:] = np.nan
    clean = run_hip(lm, am, symbols, t_lens, u_lens, 0.25, 0.0)
    got = run_hip(dirty_lm, dirty_am, symbols, t_lens, u_lens, 0.25, 0.0)
    for x, y in zip(clean, got):
        np.testing.assert_array_equal(x, y)


# ------------------------------------------------------------------------------------------- 7. determinism --
def test_backward_is_bit_identical_run_to_run():
    rng = np.random.default_rng(15)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 4, 150, 40, 700)
    symbols[:, 10:20] = symbols[:, :10]
    for ll, la in ((0.25, 0.0), (0.1, 0.1)):
        first = run_hip(lm, am, symbols, t_lens, u_lens, ll, la)
        second = run_hip(lm, am, symbols, t_lens, u_lens, ll, la)
        for x, y in zip(first, second):
            assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ 8. export --
def test_export_lattice_matches_the_loop_reference():
    from wenet_celoss_amd.rnnt_smoothed import rnnt_smoothed_lattice
    rng = np.random.default_rng(13)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 14, 6, 12)
    for ll, la in ((0.25, 0.0), (0.1, 0.1)):
        costs, alpha, beta, flag = rnnt_smoothed_lattice(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV),
                                                         torch.tensor(symbols, device=DEV), 0, ll, la,
                                                         boundary_of(t_lens, u_lens))
        alpha, beta, costs = alpha.cpu().numpy(), beta.cpu().numpy(), costs.cpu().numpy()
        assert int(flag.item()) == 0
        _, _, lat = occupancies(lm, am, symbols, t_lens, u_lens, ll, la)
        for b in range(3):
            T, U = int(t_lens[b]), int(u_lens[b])
            c, a, be, _, _ = lat[b]
            np.testing.assert_allclose(alpha[b, :T, :U + 1], a, rtol=1e-5, atol=1e-4)
            np.testing.assert_allclose(beta[b, :T, :U + 1], be, rtol=1e-5, atol=1e-4)
            np.testing.assert_allclose(costs[b], c, **COST_TOL)


# ------------------------------------------------------------------------------------------- 9. model layer --
def test_transducer_pruned_block_uses_the_smoothed_loss():
    import wenet_celoss_amd as w
    V, E, P = 23, 12, 10
    torch.manual_seed(3)
    m = w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, 14, 2, dropout=0.0),
                     w.TransducerJoint(V, E, P, 16), ctc_weight=0.0, transducer_weight=1.0, hw_weight=0.0,
                     prune_range=3, simple_loss_weight=0.5, lm_only_scale=0.25).to(DEV)
    g = torch.Generator().manual_seed(2)
    speech = torch.randn(3, 11, 8, generator=g).to(DEV)
    slen = torch.tensor([11, 7, 9], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9], [4, 4, -1, -1], [7, 1, 6, -1]], device=DEV)
    tlen = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    out = m(speech, slen, text, tlen)
    torch.testing.assert_close(out["loss"], out["loss_rnnt"] + 0.5 * out["loss_simple"])
    out["loss"].backward()
    with torch.no_grad():
        _, enc, _, enc_lens, _, pred, _ = m._loss_inputs(speech, slen, text, torch.IntTensor([0]), torch.IntTensor([0]))
        lm, am, symbols, boundary = m._simple_inputs(enc, enc_lens, pred, text, tlen)
        direct = w.rnnt_loss_smoothed(lm, am, symbols, 0, lm_only_scale=0.25, am_only_scale=0.0, boundary=boundary)
        plain = w.rnnt_loss_simple(lm, am, symbols, 0, boundary=boundary)
    assert torch.equal(out["loss_simple"], direct)
    assert abs(direct.item() - plain.item()) > 1e-3
    want = ref.loss_torch_f64(lm.cpu(), am.cpu(), symbols.cpu(), 0, enc_lens.cpu(), tlen.cpu(), 0.25, 0.0).mean()
    np.testing.assert_allclose(direct.item(), want.item(), **COST_TOL)
    for head in ("simple_am_proj", "simple_lm_proj"):
        for p in getattr(m, head).parameters():
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0


@pytest.mark.parametrize("rnnt_type,penalty", [("regular", 0.0), ("modified", 0.01)])
def test_both_scales_zero_stay_inside_the_simple_workspace(rnnt_type, penalty):
    """The raw smoothed calls with both scales 0, handed exactly `wr_rnnt_simple_workspace_bytes` of scratch, leave the
    bytes behind it alone and give the bits of `k2.rnnt_loss_simple`."""
    import wenet_celoss_amd as w
    from wenet_celoss_amd import _lib, rnnt_lattice
    B, T, U, V = 2, 9, 4, 33
    lm, am, symbols, _, _ = make_case(np.random.default_rng(41), B, T, U, V)
    t_lens, u_lens = np.array([9, 6]), np.array([3, 4])              # ragged; T_b >= U_b, so the modified lattice has paths
    lat = _lib.LATTICES[rnnt_type]
    l, a = torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV)
    sy = torch.tensor(symbols, device=DEV, dtype=torch.int32)
    ll = torch.tensor(t_lens, device=DEV, dtype=torch.int32)
    tl = torch.tensor(u_lens, device=DEV, dtype=torch.int32)

    n = _lib.load().wr_rnnt_simple_workspace_bytes(B, T, U + 1, V)
    assert 0 < n < _lib.load().wr_rnnt_smoothed_workspace_bytes(B, T, U + 1, V)
    buf = torch.full((n + 4096,), 0xA5, dtype=torch.uint8, device=DEV)
    sws = buf[:n]
    rws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U + 1, device=DEV)
    costs = torch.empty(B, dtype=torch.float32, device=DEV)
    d_am, d_lm = torch.empty_like(a), torch.empty_like(l)
    occ_emit = torch.empty(B, T, U + 1, dtype=torch.float32, device=DEV)
    occ_blank = torch.empty_like(occ_emit)
    _lib.call("wr_rnnt_smoothed_stats", a, l, sy, ll, tl, B, T, U + 1, V, 0, 0.0, 0.0, sws, n, rws, rws.numel(), device=DEV)
    _lib.call("wr_rnnt_lattice_sweeps", ll, tl, B, T, U + 1, lat, penalty, costs, rws, rws.numel(), device=DEV)
    _lib.call("wr_rnnt_smoothed_grad_lattice", a, l, sy, ll, tl, B, T, U + 1, V, 0, 0.0, 0.0, lat, None, d_am, d_lm, occ_emit,
              occ_blank, sws, n, rws, rws.numel(), device=DEV)
    assert bool((buf[n:] == 0xA5).all())

    l2, a2 = l.clone().requires_grad_(), a.clone().requires_grad_()
    want, (px_grad, py_grad) = w.k2.rnnt_loss_simple(l2, a2, torch.tensor(symbols, device=DEV), 0,
                                                     boundary=boundary_of(t_lens, u_lens), reduction="none",
                                                     return_grad=True, rnnt_type=rnnt_type, delay_penalty=penalty)
    want.sum().backward()
    assert torch.isfinite(want).all()
    assert torch.equal(costs, want.detach()) and torch.equal(d_am, a2.grad) and torch.equal(d_lm, l2.grad)
    px, py = rnnt_lattice.occupancies_to_k2(occ_emit, occ_blank, lat)
    assert torch.equal(px, px_grad) and torch.equal(py, py_grad)
