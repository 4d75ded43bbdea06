"""The float64 references of the modified lattice and the delay penalty (tests/rnnt_lattice_ref.py) against brute-force
path enumeration, on the CPU: what the GPU tests trust is checked here first."""
import numpy as np
import pytest
import torch

import rnnt_lattice_ref as ref
import rnnt_pruned_ref
import rnnt_simple_ref

SHAPES = [(T, U) for T in range(1, 7) for U in range(0, T + 1)]


def arcs(rng, T, U, V=5, blank=0):
    lm = rng.normal(size=(U + 1, V)) * 1.5
    am = rng.normal(size=(T, V)) * 1.5
    symbols = rng.integers(1, V, size=U)
    skip, emit = rnnt_simple_ref.log_probs_f64(lm, am, symbols, blank)
    return lm, am, symbols, skip, emit


@pytest.mark.parametrize("dp", [0.0, 0.3])
@pytest.mark.parametrize("T,U", SHAPES)
def test_modified_lattice_equals_path_enumeration(T, U, dp):
    rng = np.random.default_rng(100 * T + U)
    _, _, _, skip, emit = arcs(rng, T, U)
    emit = ref.penalised(emit, dp)
    cost, alpha, beta, oe, ob = ref.lattice_modified_f64(skip, emit)
    total, want_oe, want_ob = ref.enumerate_paths_modified(skip, emit)
    np.testing.assert_allclose(cost, -np.log(total), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(oe, want_oe, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(ob, want_ob, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(cost, -beta[0, 0], rtol=1e-12, atol=1e-12)
    with np.errstate(invalid="ignore"):
        node = np.exp(alpha + beta + cost)                       # occ_blank + occ_emit = exp(alpha + beta - ll)
    np.testing.assert_allclose(oe + ob, np.nan_to_num(node), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose((oe + ob).sum(1), 1.0, rtol=1e-10)          # every frame carries exactly one arc
    if T == U:                                                   # the single path: every frame carries a label
        np.testing.assert_allclose(cost, -sum(emit[t, t] for t in range(T)), rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("T,U", [(1, 2), (3, 5), (4, 5)])
def test_modified_lattice_without_a_path_costs_infinity(T, U):
    _, _, _, skip, emit = arcs(np.random.default_rng(7), T, U)
    cost, _, _, oe, ob = ref.lattice_modified_f64(skip, emit)
    assert cost == np.inf and not oe.any() and not ob.any()
    assert ref.enumerate_paths_modified(skip, emit)[0] == 0.0
    assert float(ref.cost_torch(torch.tensor(skip), torch.tensor(emit), "modified")) == np.inf


def test_penalty_zero_reproduces_the_arcs_and_the_formula():
    _, _, _, skip, emit = arcs(np.random.default_rng(8), 5, 3)
    assert np.array_equal(ref.penalised(emit, 0.0), emit)
    np.testing.assert_array_equal(ref.penalty_f64(0.5, 5), [1.0, 0.5, 0.0, -0.5, -1.0])
    np.testing.assert_array_equal(ref.penalty_f64(0.25, 4), 0.25 * np.array([1.5, 0.5, -0.5, -1.5]))
    np.testing.assert_array_equal(ref.penalised(emit, 0.5), emit + ref.penalty_f64(0.5, 5)[:, None])


@pytest.mark.parametrize("T,U", [(1, 0), (1, 2), (3, 2), (4, 3), (5, 1)])
def test_regular_lattice_with_penalty_equals_path_enumeration(T, U):
    """rnnt_simple_ref.enumerate_paths builds its arcs from (lm, am); a penalty on every label arc of frame t is the same
    lattice with pen[t] added to am[t, label] only in the emit arcs -- enumerated here on the penalised arcs through
    rnnt_smoothed_ref.enumerate_paths, which takes arcs, after checking both enumerations agree without a penalty."""
    import rnnt_smoothed_ref
    rng = np.random.default_rng(10 * T + U)
    lm, am, symbols, skip, emit = arcs(rng, T, U)
    total0, oe0, ob0 = rnnt_simple_ref.enumerate_paths(lm, am, symbols, 0, T, U)
    total1, oe1, ob1 = rnnt_smoothed_ref.enumerate_paths(skip, emit)
    np.testing.assert_allclose(total1, total0, rtol=1e-12)
    np.testing.assert_allclose(oe1, oe0, rtol=1e-12, atol=1e-15)
    pe = ref.penalised(emit, 0.4)
    total, want_oe, want_ob = rnnt_smoothed_ref.enumerate_paths(skip, pe)
    cost, _, _, oe, ob = ref.lattice_regular_f64(skip, pe)
    np.testing.assert_allclose(cost, -np.log(total), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(oe, want_oe, rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(ob, want_ob, rtol=1e-10, atol=1e-14)
    got = ref.cost_torch(torch.tensor(skip), torch.tensor(pe), "regular")
    np.testing.assert_allclose(float(got), cost, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
@pytest.mark.parametrize("ll,la", [(0.0, 0.0), (0.25, 0.0), (0.1, 0.1)])
def test_torch_expression_matches_the_loop_lattice_and_its_occupancies(rnnt_type, ll, la):
    """cost_torch against the explicit-loop lattice, and its autograd gradient with respect to the arcs against the
    occupancies (d cost / d arc = -occupancy)."""
    import rnnt_smoothed_ref
    rng = np.random.default_rng(3)
    B, T, U, V = 2, 6, 3, 7
    lm = rng.normal(size=(B, U + 1, V))
    am = rng.normal(size=(B, T, V))
    symbols = rng.integers(1, V, size=(B, U))
    t_lens, u_lens = [6, 4], [3, 2]
    dp = 0.2
    costs = ref.simple_costs_torch(torch.tensor(lm), torch.tensor(am), symbols, 0, t_lens, u_lens, ll, la, rnnt_type, dp)
    pbar = rnnt_smoothed_ref.pbar_f64(lm)
    for b in range(B):
        skip, emit = rnnt_smoothed_ref.arcs_f64(lm[b], am[b], symbols[b], 0, t_lens[b], u_lens[b], pbar, ll, la)
        pe = ref.penalised(emit, dp)
        lat = ref.lattice_modified_f64 if rnnt_type == "modified" else ref.lattice_regular_f64
        cost, _, _, oe, ob = lat(skip, pe)
        np.testing.assert_allclose(float(costs[b]), cost, rtol=1e-11)
        sk, em = torch.tensor(skip, requires_grad=True), torch.tensor(pe, requires_grad=True)
        ref.cost_torch(sk, em, rnnt_type).backward()
        np.testing.assert_allclose(-sk.grad.numpy(), ob, rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(-em.grad.numpy()[:, :u_lens[b]], oe[:, :u_lens[b]], rtol=1e-9, atol=1e-13)


@pytest.mark.parametrize("rnnt_type", ["regular", "modified"])
def test_pruned_torch_expression_matches_the_loop_lattice(rnnt_type):
    rng = np.random.default_rng(4)
    B, T, U, V, R = 2, 7, 4, 6, 2
    t_lens, u_lens = np.array([7, 5]), np.array([4, 3])
    ranges = rnnt_pruned_ref.random_band(rng, B, T, U + 1, R, t_lens, u_lens)
    logits = rng.normal(size=(B, T, R, V))
    symbols = rng.integers(1, V, size=(B, U))
    costs = ref.pruned_costs_torch(torch.tensor(logits), ranges, symbols, 0, t_lens, u_lens, rnnt_type, 0.3)
    for b in range(B):
        skip, emit, _ = rnnt_pruned_ref.band_log_probs_f64(logits[b], ranges[b], symbols[b], 0, t_lens[b], u_lens[b])
        pe = ref.penalised(emit, 0.3)
        if rnnt_type == "modified":
            cost = ref.lattice_modified_f64(skip, pe)[0]
        else:
            with np.errstate(invalid="ignore"):
                cost = ref.lattice_regular_f64(skip, pe)[0]
        assert np.isfinite(cost)
        np.testing.assert_allclose(float(costs[b]), cost, rtol=1e-11)


def test_prune_ranges_ref_reads_no_column_past_the_last_frame():
    rng = np.random.default_rng(5)
    B, T, U = 2, 9, 5
    py = rng.random((B, U + 1, T)).astype(np.float32)
    px_t = rng.random((B, U, T)).astype(np.float32)
    px_t1 = np.concatenate([px_t, np.full((B, U, 1), 99.0, np.float32)], 2)
    boundary = np.array([[0, 0, 5, 9], [0, 0, 3, 6]])
    for R in (2, 3):
        a = ref.prune_ranges_ref(px_t, py, boundary, R)
        np.testing.assert_array_equal(a, ref.prune_ranges_ref(px_t1, py, boundary, R))
        rnnt_pruned_ref.check_range_properties(a, boundary, U + 1)
    one = ref.prune_ranges_ref(px_t, py, boundary, 1)
    assert one.shape == (B, T, 1)
    rnnt_pruned_ref.check_range_properties(one, boundary, U + 1)
    with pytest.raises(AssertionError):
        ref.prune_ranges_ref(px_t1, py, boundary, 1)
