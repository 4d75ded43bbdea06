"""The float64 references of pruned RNN-T training check themselves (CPU): brute force over the band's paths equals the
lattice, autograd equals the occupancy gradient, a band that covers the whole lattice is the ordinary RNN-T loss (the C
oracle), and the provable properties of the prune ranges hold on random occupancies.  Ragged boundaries and utterances
with U_b + 1 < R are included.  Plus the argument checks of the new C entry points, which need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_pruned_ref as ref


def small_case(seed, B=3, T=6, U=4, V=7, R=3, blank=0, full=False):
    rng = np.random.default_rng(seed)
    labels = [v for v in range(V) if v != blank]
    symbols = rng.choice(labels, size=(B, U)).astype(np.int64)
    if full:
        t_lens, u_lens = np.full(B, T), np.full(B, U)
    else:
        t_lens = np.concatenate([[T], rng.integers(1, T + 1, size=B - 1)])
        u_lens = rng.integers(0, U + 1, size=B)
        u_lens[rng.integers(0, B)] = U
        u_lens[-1] = min(u_lens[-1], max(R - 2, 0))            # an utterance with U_b + 1 < R
    R = min(R, U + 1)
    ranges = ref.random_band(rng, B, T, U + 1, R, t_lens, u_lens)
    logits = rng.normal(size=(B, T, R, V)).astype(np.float32)
    return logits, ranges, symbols, t_lens, u_lens


@pytest.mark.parametrize("seed,T,U,R", [(0, 5, 3, 2), (1, 6, 4, 3), (2, 4, 4, 5), (3, 7, 2, 2), (4, 1, 2, 3), (5, 3, 5, 2)])
def test_brute_force_equals_lattice(seed, T, U, R):
    logits, ranges, symbols, t_lens, u_lens = small_case(seed, T=T, U=U, R=R)
    feasible = 0
    for b in range(logits.shape[0]):
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        total, oe, ob = ref.enumerate_paths_pruned(logits[b], ranges[b], symbols[b], 0, Tb, Ub)
        cost, _, _, occ_emit, occ_blank = ref.lattice_pruned_f64(logits[b], ranges[b], symbols[b], 0, Tb, Ub)
        if total == 0.0:
            assert cost == np.inf
            continue
        feasible += 1
        np.testing.assert_allclose(cost, -np.log(total), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(occ_emit, oe, rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(occ_blank, ob, rtol=1e-10, atol=1e-13)
    assert feasible or T == 1 or U > T


def test_band_really_prunes():
    """The banded cost is larger than the full-lattice cost of the same log-probabilities (paths are missing)."""
    logits, ranges, symbols, t_lens, u_lens = small_case(7, B=2, T=8, U=5, R=2, full=True)
    for b in range(2):
        total, _, _ = ref.enumerate_paths_pruned(logits[b], ranges[b], symbols[b], 0, 8, 5)
        assert 0.0 < total < 1.0
        n_cells = len({(t, int(u)) for t in range(8) for u in ranges[b, t]})
        assert n_cells == 16 < 8 * 6


@pytest.mark.parametrize("seed,blank,label_is_blank", [(10, 0, False), (11, 6, False), (12, 2, True)])
def test_autograd_equals_occupancy_gradient(seed, blank, label_is_blank):
    logits, ranges, symbols, t_lens, u_lens = small_case(seed, B=3, T=6, U=4, V=7, R=3, blank=blank)
    if label_is_blank:
        symbols[:, 1] = blank
    x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    costs = ref.loss_pruned_torch_f64(x, ranges, symbols, blank, t_lens, u_lens)
    want_c, want_g = ref.reference_batch(logits, ranges, symbols, blank, t_lens, u_lens)
    finite = np.isfinite(want_c)
    assert finite.any()
    np.testing.assert_array_equal(np.isfinite(costs.detach().numpy()), finite)
    np.testing.assert_allclose(costs.detach().numpy()[finite], want_c[finite], rtol=1e-12, atol=1e-12)
    costs[torch.tensor(finite)].sum().backward()
    for b in np.flatnonzero(finite):
        np.testing.assert_allclose(x.grad[b].numpy(), want_g[b], rtol=1e-9, atol=1e-12)
        assert not x.grad[b, int(t_lens[b]):].any()
        assert not want_g[b][ranges[b] > u_lens[b]].any()


def test_whole_lattice_band_is_the_rnnt_loss():
    import oracle
    rng = np.random.default_rng(20)
    B, T, U, V = 3, 7, 4, 9
    logits = rng.normal(size=(B, T, U + 1, V)).astype(np.float32)
    symbols = rng.integers(1, V, size=(B, U))
    t_lens, u_lens = np.array([7, 4, 6]), np.array([4, 2, 0])
    costs, grad = ref.reference_batch(logits, ref.full_ranges(B, T, U + 1), symbols, 0, t_lens, u_lens)
    oc, og = oracle.rnnt_loss_f64(logits, symbols.astype(np.int32), t_lens.astype(np.int32), u_lens.astype(np.int32))
    np.testing.assert_allclose(costs, oc, rtol=1e-12)
    np.testing.assert_allclose(grad, og, rtol=2.0 ** -23, atol=1e-12)      # the oracle returns its gradient in float32


def test_infeasible_band_costs_infinity():
    logits, _, symbols, _, _ = small_case(30, B=1, T=5, U=4, R=2, full=True)
    ranges = np.zeros((1, 5, 2), np.int64) + np.arange(2)          # the band never leaves u in {0, 1}: U = 4 is out of reach
    cost, _, _, oe, ob = ref.lattice_pruned_f64(logits[0], ranges[0], symbols[0], 0, 5, 4)
    assert cost == np.inf and not oe.any() and not ob.any()
    c = ref.loss_pruned_torch_f64(torch.tensor(logits), ranges, symbols, 0, [5], [4])
    assert c.item() == float("inf")


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("s_range", [2, 3, 5, 9])
def test_prune_range_properties_on_random_occupancies(seed, s_range):
    rng = np.random.default_rng(100 + seed)
    B, T, U = 4, int(rng.integers(1, 40)), int(rng.integers(0, 12))
    px = rng.random((B, U, T + 1)).astype(np.float32)
    py = rng.random((B, U + 1, T)).astype(np.float32)
    boundary = np.zeros((B, 4), np.int64)
    boundary[:, 2] = rng.integers(0, U + 1, size=B)
    boundary[:, 3] = rng.integers(0, T + 1, size=B)
    boundary[0, 2:] = (U, T)
    boundary[1, 2] = 0                                             # U_b + 1 < R
    ranges = ref.prune_ranges_ref(px, py, boundary, s_range)
    assert ranges.shape == (B, T, min(s_range, U + 1)) and ranges.dtype == np.int64
    ref.check_range_properties(ranges, boundary, U + 1)


def test_prune_ranges_follow_a_sharp_alignment():
    """Occupancies concentrated on one path: the band contains the path's cell at every frame before T_b - 1."""
    T, U, R = 12, 6, 3
    emit_frame = [1, 1, 4, 6, 6, 9]                                # label u+1 is emitted at this frame
    px, py = np.zeros((1, U, T + 1), np.float32), np.zeros((1, U + 1, T), np.float32)
    u = 0
    for t in range(T):
        while u < U and emit_frame[u] == t:
            px[0, u, t] = 1.0
            u += 1
        py[0, u, t] = 1.0
    ranges = ref.prune_ranges_ref(px, py, [[0, 0, U, T]], R)
    ref.check_range_properties(ranges, [[0, 0, U, T]], U + 1)
    u = 0
    for t in range(T - 1):
        while u < U and emit_frame[u] == t:
            u += 1
        assert ranges[0, t, 0] <= u <= ranges[0, t, -1], (t, u, ranges[0, t])


# ------------------------------------------------------------------------------------------------ C ABI, no GPU --
def test_new_entry_points_reject_bad_arguments_before_launch():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    one = ctypes.c_void_p(16)                                      # a non-null pointer that is never dereferenced
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    # prune ranges: (px, py, T_b, U_b, B, T, U1, R, ranges, stream)
    assert lib.wr_rnnt_prune_ranges(null, null, null, null, 2, 4, 3, 2, null, null) == EINVAL
    assert b"null" in lib.wr_last_error()
    assert lib.wr_rnnt_prune_ranges(one, one, one, one, 2, 0, 3, 2, one, null) == EINVAL
    assert lib.wr_rnnt_prune_ranges(one, one, one, one, 2, 4, 3, 4, one, null) == EINVAL
    assert b"R=4" in lib.wr_last_error()
    assert lib.wr_rnnt_prune_ranges(one, one, one, one, 2, 4, 3, 0, one, null) == EINVAL
    # gather / scatter: (.., ranges, dtype, B, T, U1, R, C, .., stream)
    assert lib.wr_rnnt_prune_gather(null, null, null, 0, 2, 4, 3, 2, 8, null, null, null) == EINVAL
    assert lib.wr_rnnt_prune_gather(one, one, one, 0, 2, 4, 3, 4, 8, one, one, null) == EINVAL
    assert lib.wr_rnnt_prune_gather(one, one, one, 7, 2, 4, 3, 2, 8, one, one, null) == EINVAL
    assert b"dtype" in lib.wr_last_error()
    assert lib.wr_rnnt_prune_gather(one, one, one, 0, 2, 4, 3, 2, 0, one, one, null) == EINVAL
    assert lib.wr_rnnt_prune_scatter(null, null, null, 0, 2, 4, 3, 2, 8, null, null, null) == EINVAL
    assert lib.wr_rnnt_prune_scatter(null, one, one, 0, 2, 4, 3, 2, 8, one, null, null) == EINVAL      # d_am without g_am
    assert lib.wr_rnnt_prune_scatter(one, one, one, 0, 2, 4, 3, 5, 8, one, one, null) == EINVAL
    # the loss: (logits, dtype, symbols, ranges, T_b, U_b, B, T, U1, R, V, blank, [grad_costs, grads,] ws, bytes, stream)
    assert lib.wr_rnnt_pruned_stats(null, 0, null, null, null, null, 2, 4, 3, 2, 8, 0, null, 0, null) == EINVAL
    assert b"null" in lib.wr_last_error()
    assert lib.wr_rnnt_pruned_stats(one, 0, one, one, one, one, 2, 4, 3, 2, 8, 9, one, 0, null) == EINVAL
    assert b"blank" in lib.wr_last_error()
    assert lib.wr_rnnt_pruned_stats(one, 0, one, one, one, one, 2, 4, 3, 4, 8, 0, one, 0, null) == EINVAL
    assert lib.wr_rnnt_pruned_stats(one, 0, one, one, one, one, 2, 4, 1100, 2, 8, 0, one, 0, null) == EUNSUPPORTED
    need = lib.wr_rnnt_workspace_bytes(2, 4, 3)
    assert lib.wr_rnnt_pruned_stats(one, 0, one, one, one, one, 2, 4, 3, 2, 8, 0, one, need - 1, null) == EWORKSPACE
    assert lib.wr_rnnt_pruned_grad(null, 0, null, null, null, null, 2, 4, 3, 2, 8, 0, null, null, null, 0, null) == EINVAL
    assert lib.wr_rnnt_pruned_grad(one, 0, one, one, one, one, 2, 4, 3, 2, 8, -1, null, one, one, need, null) == EINVAL
    assert lib.wr_rnnt_pruned_grad(one, 0, one, one, one, one, 2, 0, 3, 2, 8, 0, null, one, one, need, null) == EINVAL
    assert lib.wr_rnnt_pruned_grad(one, 0, one, one, one, one, 2, 4, 3, 2, 8, 0, null, one, one, need - 1, null) == EWORKSPACE
    off = ctypes.c_void_p(20)                                      # grads at another 16-byte phase than logits
    assert lib.wr_rnnt_pruned_grad(one, 0, one, one, one, one, 2, 4, 3, 2, 8, 0, null, off, one, need, null) == EINVAL
    assert b"16-byte" in lib.wr_last_error()


def test_python_argument_checks_need_no_device():
    import wenet_celoss_amd as w
    assert {"get_rnnt_prune_ranges", "do_rnnt_pruning", "rnnt_loss_pruned"} <= set(w.__all__)
    px, py = torch.zeros(1, 2, 5), torch.zeros(1, 3, 4)
    with pytest.raises(ValueError, match="s_range"):
        w.get_rnnt_prune_ranges(px, py, None, 1)
    with pytest.raises(ValueError, match="px_grad"):
        w.get_rnnt_prune_ranges(torch.zeros(1, 2, 4), py, None, 2)
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.get_rnnt_prune_ranges(px, py, None, 2)
    with pytest.raises(ValueError, match="do not agree"):
        w.do_rnnt_pruning(torch.zeros(1, 4, 8), torch.zeros(1, 3, 6), torch.zeros(1, 4, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.do_rnnt_pruning(torch.zeros(1, 4, 8), torch.zeros(1, 3, 8), torch.zeros(1, 4, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="reduction"):
        w.rnnt_loss_pruned(torch.zeros(1, 4, 2, 5), torch.zeros(1, 2, dtype=torch.int64),
                           torch.zeros(1, 4, 2, dtype=torch.int64), 0, reduction="avg")
    with pytest.raises(ValueError, match="termination_symbol"):
        w.rnnt_loss_pruned(torch.zeros(1, 4, 2, 5), torch.zeros(1, 2, dtype=torch.int64),
                           torch.zeros(1, 4, 2, dtype=torch.int64), 5)
    with pytest.raises(ValueError, match="R = 4"):
        w.rnnt_loss_pruned(torch.zeros(1, 4, 4, 5), torch.zeros(1, 2, dtype=torch.int64),
                           torch.zeros(1, 4, 4, dtype=torch.int64), 0)


def test_prune_range_needs_the_simple_heads():
    import wenet_celoss_amd as w

    class Enc(torch.nn.Module):
        def output_size(self):
            return 12

    def model(**kw):
        return w.Transducer(23, 0, Enc(), w.RNNPredictor(23, 10, 10, 0.0, 14, 2, dropout=0.0),
                            w.TransducerJoint(23, 12, 10, 16), ctc_weight=0.0, transducer_weight=1.0, **kw)
    with pytest.raises(ValueError, match="simple_loss_weight"):
        model(prune_range=5)
    with pytest.raises(ValueError, match="prune_range"):
        model(prune_range=1, simple_loss_weight=0.5)
    assert model(prune_range=5, simple_loss_weight=0.5).prune_range == 5
    assert model().prune_range == 0
    assert set(model(prune_range=5, simple_loss_weight=0.5).state_dict()) == set(model(simple_loss_weight=0.5).state_dict())
