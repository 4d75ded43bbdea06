"""CPU-side checks of the smoothed additive-joiner loss: the float64 references of tests/rnnt_smoothed_ref.py against
each other, against path enumeration and against the gradient formula of include/wr_api.h; argument errors; symbols."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_simple_ref as sref
import rnnt_smoothed_ref as ref

SCALES = [(0.25, 0.0), (0.0, 0.3), (0.1, 0.1), (0.5, 0.5)]


def make_case(seed, B, T, U, V, blank=0):
    rng = np.random.default_rng(seed)
    lm = rng.normal(size=(B, U + 1, V)) * 1.5
    am = rng.normal(size=(B, T, V)) * 1.5
    symbols = rng.choice([v for v in range(V) if v != blank], size=(B, U)).astype(np.int64)
    t_lens = np.concatenate([[T], rng.integers(1, T + 1, size=B - 1)]).astype(np.int64)
    u_lens = np.concatenate([rng.integers(0, U + 1, size=B - 1), [U]]).astype(np.int64)
    return lm, am, symbols, t_lens, u_lens


def test_zero_scales_are_the_simple_loss():
    lm, am, symbols, t_lens, u_lens = make_case(1, 3, 6, 4, 7)
    tl, ta = torch.tensor(lm), torch.tensor(am)
    got = ref.loss_torch_f64(tl, ta, symbols, 0, t_lens, u_lens, 0.0, 0.0)
    want = sref.loss_torch_f64(tl, ta, symbols, 0, t_lens, u_lens)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-13, atol=1e-13)
    pbar = ref.pbar_f64(lm)
    for b in range(3):
        T, U = int(t_lens[b]), int(u_lens[b])
        for x, y in zip(ref.lattice_f64(lm[b], am[b], symbols[b], 0, T, U, pbar, 0.0, 0.0),
                        sref.lattice_f64(lm[b], am[b], symbols[b], 0, T, U)):
            np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("ll,la", SCALES)
def test_torch_costs_match_path_enumeration_and_the_loop_lattice(ll, la):
    B, T, U, V = 2, 3, 2, 4
    lm, am, symbols, _, _ = make_case(2, B, T, U, V, blank=1)
    symbols[1, 1] = symbols[1, 0]
    t_lens, u_lens = np.array([T, T]), np.array([U, U])
    costs = ref.loss_torch_f64(torch.tensor(lm), torch.tensor(am), symbols, 1, t_lens, u_lens, ll, la).numpy()
    pbar = ref.pbar_f64(lm)
    np.testing.assert_allclose(pbar.sum(), 1.0, rtol=1e-12)
    for b in range(B):
        skip, emit = ref.arcs_f64(lm[b], am[b], symbols[b], 1, T, U, pbar, ll, la)
        total, oe, ob = ref.enumerate_paths(skip, emit)
        np.testing.assert_allclose(costs[b], -np.log(total), rtol=1e-12)
        c, _, _, loe, lob = ref.lattice_from_arcs(skip, emit)
        np.testing.assert_allclose(c, costs[b], rtol=1e-12)
        np.testing.assert_allclose(loe, oe, rtol=1e-10, atol=1e-14)
        np.testing.assert_allclose(lob, ob, rtol=1e-10, atol=1e-14)


def test_ragged_batch_pbar_counts_padded_rows():
    """The unigram is over all B * (U+1) rows: changing a padded row of lm changes the cost when am_only_scale > 0."""
    lm, am, symbols, t_lens, u_lens = make_case(3, 2, 4, 3, 5)
    u_lens[:] = [1, 3]
    a = ref.loss_torch_f64(torch.tensor(lm), torch.tensor(am), symbols, 0, t_lens, u_lens, 0.1, 0.3).numpy()
    lm2 = lm.copy()
    lm2[0, 3, 2] += 2.0
    b = ref.loss_torch_f64(torch.tensor(lm2), torch.tensor(am), symbols, 0, t_lens, u_lens, 0.1, 0.3).numpy()
    assert np.abs(a - b).min() > 1e-6
    c = ref.loss_torch_f64(torch.tensor(lm2), torch.tensor(am), symbols, 0, t_lens, u_lens, 0.4, 0.0).numpy()
    d = ref.loss_torch_f64(torch.tensor(lm), torch.tensor(am), symbols, 0, t_lens, u_lens, 0.4, 0.0).numpy()
    np.testing.assert_array_equal(c, d)


def test_gradcheck_float64():
    lm, am, symbols, t_lens, u_lens = make_case(4, 2, 3, 2, 4)
    tl = torch.tensor(lm, requires_grad=True)
    ta = torch.tensor(am, requires_grad=True)
    w = torch.tensor([0.7, -1.3], dtype=torch.float64)
    for ll, la in ((0.25, 0.0), (0.1, 0.2)):
        assert torch.autograd.gradcheck(
            lambda l, a: (ref.loss_torch_f64(l, a, symbols, 0, t_lens, u_lens, ll, la) * w).sum(), (tl, ta),
            eps=1e-6, atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("ll,la", SCALES)
def test_gradient_formula_matches_autograd(ll, la):
    """B = 2 with unequal grad_costs, ragged (padded lm rows and am frames), a repeated label and a label equal to the
    blank: the formula of include/wr_api.h from the loop lattice's occupancies against autograd of the torch expression."""
    lm, am, symbols, t_lens, u_lens = make_case(5, 2, 5, 4, 6, blank=2)
    t_lens[:] = [5, 3]
    u_lens[:] = [2, 4]
    symbols[1, 2] = symbols[1, 0]
    symbols[1, 1] = 2
    g = np.array([0.5, -2.0])
    tl = torch.tensor(lm, requires_grad=True)
    ta = torch.tensor(am, requires_grad=True)
    (ref.loss_torch_f64(tl, ta, symbols, 2, t_lens, u_lens, ll, la) * torch.tensor(g)).sum().backward()
    d_am, d_lm = ref.gradient_formula(lm, am, symbols, 2, t_lens, u_lens, ll, la, g)
    np.testing.assert_allclose(d_am, ta.grad.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(d_lm, tl.grad.numpy(), rtol=1e-9, atol=1e-12)
    assert not d_am[1, 3:].any()
    assert bool(d_lm[0, 3:].any()) == (la != 0)


def test_argument_errors_raise_before_any_device():
    import wenet_celoss_amd as w
    lm, am = torch.zeros(2, 4, 6), torch.zeros(2, 5, 6)
    sy = torch.ones(2, 3, dtype=torch.int64)
    for ll, la in ((-0.1, 0.0), (0.0, -1e-3), (0.6, 0.5), (1.5, 0.0), (float("nan"), 0.0)):
        with pytest.raises(ValueError, match="scale"):
            w.rnnt_loss_smoothed(lm, am, sy, 0, lm_only_scale=ll, am_only_scale=la)
    with pytest.raises(ValueError, match="reduction"):
        w.rnnt_loss_smoothed(lm, am, sy, 0, reduction="avg")
    with pytest.raises(ValueError, match="termination_symbol"):
        w.rnnt_loss_smoothed(lm, am, sy, 6)
    with pytest.raises(ValueError, match="symbols"):
        w.rnnt_loss_smoothed(lm, am, sy[:, :2], 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.rnnt_loss_smoothed(lm, am, sy, 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.rnnt_loss_smoothed(lm, am, sy, 0, 0.0, 0.0)
    import inspect
    params = inspect.signature(w.rnnt_loss_smoothed).parameters
    assert list(params) == ["lm", "am", "symbols", "termination_symbol", "lm_only_scale", "am_only_scale", "boundary",
                            "reduction", "return_grad"]                       # k2's order and defaults
    assert params["lm_only_scale"].default == 0.1 and params["am_only_scale"].default == 0.1
    assert params["reduction"].default == "mean" and params["return_grad"].default is False


def test_transducer_scale_arguments():
    import test_rnnt_simple_host as h
    m = h._model(simple_loss_weight=0.5, lm_only_scale=0.25)
    assert (m.lm_only_scale, m.am_only_scale) == (0.25, 0.0)
    assert set(m.state_dict().keys()) == set(h._model(simple_loss_weight=0.5).state_dict().keys())
    for kw in (dict(lm_only_scale=-0.1), dict(lm_only_scale=0.7, am_only_scale=0.4)):
        with pytest.raises(ValueError, match="lm_only_scale"):
            h._model(simple_loss_weight=0.5, **kw)
    with pytest.raises(ValueError, match="simple_loss_weight"):
        h._model(lm_only_scale=0.25)


def test_symbols_present_and_bad_arguments_rejected_without_launch():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    for name in ("wr_rnnt_smoothed_workspace_bytes", "wr_rnnt_smoothed_stats", "wr_rnnt_smoothed_grad"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    null, one = ctypes.c_void_p(None), ctypes.c_void_p(256)

    def stats(p=one, B=2, T=4, U1=3, V=8, blank=0, ll=0.1, la=0.1, sws=1 << 30, rws=1 << 30):
        return lib.wr_rnnt_smoothed_stats(p, p, p, p, p, B, T, U1, V, blank, ll, la, p, sws, p, rws, null)

    def grad(p=one, B=2, T=4, U1=3, V=8, blank=0, ll=0.1, la=0.1, sws=1 << 30, rws=1 << 30):
        return lib.wr_rnnt_smoothed_grad(p, p, p, p, p, B, T, U1, V, blank, ll, la, null, p, p, null, null, p, sws, p, rws,
                                         null)
    for fn in (stats, grad):
        assert fn(p=null) == -1 and b"null" in lib.wr_last_error()
        assert fn(blank=8) == -1 and b"blank" in lib.wr_last_error()
        assert fn(U1=1100) == -2 and b"1024" in lib.wr_last_error()
        assert fn(ll=-0.5) == -1 and b"negative" in lib.wr_last_error()
        assert fn(ll=0.75, la=0.5) == -1 and b"exceeds 1" in lib.wr_last_error()
        assert fn(sws=16) == -3 and b"workspace" in lib.wr_last_error()
        assert fn(rws=16) == -3 and b"workspace" in lib.wr_last_error()
    # occupancies only: both occupancy outputs are needed
    assert lib.wr_rnnt_smoothed_grad(one, one, one, one, one, 2, 4, 3, 8, 0, 0.1, 0.1, null, null, null, null, null, one,
                                     1 << 30, one, 1 << 30, null) == -1
    assert lib.wr_rnnt_smoothed_workspace_bytes(0, 4, 3, 8) == 0
    small = lib.wr_rnnt_smoothed_workspace_bytes(2, 10, 5, 50)
    big = lib.wr_rnnt_smoothed_workspace_bytes(16, 1000, 151, 5000)
    assert lib.wr_rnnt_simple_workspace_bytes(2, 10, 5, 50) < small < big
    assert big < 16 * 1000 * 151 * 4 * 8                   # a few floats per cell plus a few rows of V: never logits-sized
