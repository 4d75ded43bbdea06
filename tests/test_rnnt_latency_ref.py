"""The float64 reference of FastEmit and the delay penalty (tests/rnnt_latency_ref.py) against independent truth on tiny
lattices (T <= 4, U <= 3, V = 5): path enumeration and float64 autograd.  CPU only."""
import os

import numpy as np
import pytest
import torch

import rnnt_latency_ref as ref
import rnnt_lattice_ref
import rnnt_smoothed_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
V, BLANK = 5, 0
SHAPES = [(1, 0), (1, 2), (2, 1), (3, 3), (4, 2), (4, 3)]
SETTINGS = [(0.0, 0.0), (0.01, 0.0), (0.5, 0.0), (0.0, 0.003), (0.0, 0.5), (0.5, 0.5)]


def case(T, U, seed=0):
    rng = np.random.default_rng(100 * T + 10 * U + seed)
    logits = rng.normal(size=(1, T, U + 1, V)) * 1.5
    targets = rng.integers(1, V, size=(1, max(U, 1)))[:, :U]
    return logits, targets


def torch_arcs(x, targets, T, U, dp):
    """(skip, emit') as differentiable float64 torch expressions of the logits x (T, U+1, V)."""
    lp = torch.log_softmax(x, -1)
    skip = lp[:, :, BLANK]
    emit = lp.new_full((T, U + 1), rnnt_lattice_ref.NEG_BIG)
    if U:
        idx = torch.as_tensor(np.asarray(targets[:U], np.int64))[None, :, None].expand(T, U, 1)
        em = lp[:, :U].gather(-1, idx)[..., 0]
        if dp > 0:
            em = em + torch.as_tensor(rnnt_lattice_ref.penalty_f64(dp, T))[:, None]
        emit = torch.cat([em, emit[:, U:]], 1)
    return skip, emit


@pytest.mark.parametrize("T,U", SHAPES)
@pytest.mark.parametrize("dp", [0.0, 0.003, 0.5])
def test_cost_and_label_occupancy_equal_path_enumeration(T, U, dp):
    logits, targets = case(T, U)
    costs, _, lats = ref.loss_f64(logits, targets, [T], [U], BLANK, 0.0, dp)
    skip, emit, _ = ref.arcs_f64(logits[0], targets[0], T, U, BLANK)
    emit_p = rnnt_lattice_ref.penalised(emit, dp)
    total, oe, ob = rnnt_smoothed_ref.enumerate_paths(skip, emit_p)
    assert abs(costs[0] + np.log(total)) < 1e-12
    np.testing.assert_allclose(lats[0]["occ_emit"][:, :U], oe[:, :U], rtol=0, atol=1e-12)
    np.testing.assert_allclose(lats[0]["occ_blank"], ob, rtol=0, atol=1e-12)
    if dp > 0 and U:        # the penalty is inside the cost: it differs from the cost without one
        plain, _, _ = ref.loss_f64(logits, targets, [T], [U], BLANK)
        assert T == 1 or abs(plain[0] - costs[0]) > 1e-6


@pytest.mark.parametrize("T,U", SHAPES)
@pytest.mark.parametrize("dp", [0.0, 0.003, 0.5])
def test_gradient_without_fastemit_is_the_derivative_of_the_cost(T, U, dp):
    logits, targets = case(T, U, seed=1)
    _, grad, _ = ref.loss_f64(logits, targets, [T], [U], BLANK, 0.0, dp)
    x = torch.tensor(logits[0], dtype=torch.float64, requires_grad=True)
    skip, emit = torch_arcs(x, targets[0], T, U, dp)
    rnnt_lattice_ref.cost_torch(skip, emit, "regular").backward()
    np.testing.assert_allclose(grad[0], x.grad.numpy(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("T,U", SHAPES)
@pytest.mark.parametrize("lam,dp", [s for s in SETTINGS if s[0] > 0])
def test_fastemit_gradient_is_the_derivative_of_the_surrogate(T, U, lam, dp):
    """-sum occ_blank.detach() blank - (1 + lambda) sum occ_emit.detach() emit', through the log-softmax"""
    logits, targets = case(T, U, seed=2)
    costs, grad, lats = ref.loss_f64(logits, targets, [T], [U], BLANK, lam, dp)
    x = torch.tensor(logits[0], dtype=torch.float64, requires_grad=True)
    skip, emit = torch_arcs(x, targets[0], T, U, dp)
    ob = torch.as_tensor(lats[0]["occ_blank"])
    oe = torch.as_tensor(lats[0]["occ_emit"])
    sur = -(ob * skip).sum()
    if U:
        sur = sur - (1.0 + lam) * (oe[:, :U] * emit[:, :U]).sum()
    sur.backward()
    np.testing.assert_allclose(grad[0], x.grad.numpy(), rtol=0, atol=1e-12)
    # the costs do not depend on lambda
    base, _, _ = ref.loss_f64(logits, targets, [T], [U], BLANK, 0.0, dp)
    assert costs[0] == base[0]


@pytest.mark.parametrize("T,U", SHAPES)
@pytest.mark.parametrize("lam,dp", SETTINGS)
def test_every_valid_row_sums_to_zero(T, U, lam, dp):
    logits, targets = case(T, U, seed=3)
    _, grad, _ = ref.loss_f64(logits, targets, [T], [U], BLANK, lam, dp)
    assert np.abs(grad[0].sum(-1)).max() < 1e-12


def test_padding_is_zero_and_ragged_batch_matches_single_utterances():
    rng = np.random.default_rng(7)
    logits = rng.normal(size=(3, 4, 4, V))
    targets = rng.integers(1, V, size=(3, 3))
    llens, tlens = [4, 2, 1], [3, 1, 0]
    costs, grad, _ = ref.loss_f64(logits, targets, llens, tlens, BLANK, 0.5, 0.5, grad_costs=[1.0, -2.0, 0.5])
    for b in range(3):
        T, U = llens[b], tlens[b]
        assert not grad[b, T:].any() and not grad[b, :, U + 1:].any()
        c1, g1, _ = ref.loss_f64(logits[b:b + 1, :T, :U + 1], targets[b:b + 1, :U], [T], [U], BLANK, 0.5, 0.5)
        assert costs[b] == c1[0]
        np.testing.assert_allclose(grad[b, :T, :U + 1], g1[0] * [1.0, -2.0, 0.5][b], rtol=0, atol=1e-15)


def test_label_equal_to_blank_drops_the_label_and_fastemit_terms():
    """at a cell with a blank term the blank element gets the blank term only, and lambda does not enter the row"""
    logits, _ = case(3, 2, seed=4)
    targets = np.array([[BLANK, 3]])
    _, g0, lats = ref.loss_f64(logits, targets, [3], [2], BLANK, 0.0, 0.0)
    _, g1, _ = ref.loss_f64(logits, targets, [3], [2], BLANK, 0.5, 0.0)
    np.testing.assert_array_equal(g0[0, :2, 0], g1[0, :2, 0])             # rows (t < T-1, u = 0): no FastEmit term
    assert np.abs(g0[0, 2, 0] - g1[0, 2, 0]).max() > 1e-6                 # row (T-1, 0) has no blank term: the label term is kept
    sm = np.exp(ref.arcs_f64(logits[0], targets[0], 3, 2, BLANK)[2])
    lat = lats[0]
    want = sm[0, 0] * np.exp(lat["alpha"][0, 0] + lat["beta"][0, 0] + lat["cost"])
    want[BLANK] -= lat["occ_blank"][0, 0]
    np.testing.assert_allclose(g0[0, 0, 0], want, rtol=0, atol=1e-15)


def test_defaults_reproduce_the_known_answer():
    kat = np.load(os.path.join(GOLDEN, "rnnt_kat.npz"))
    costs, grad, _ = ref.loss_f64(kat["logits"], kat["targets"], [2], [2], BLANK)
    assert abs(costs[0] - float(kat["cost"])) < 5e-8
    np.testing.assert_allclose(grad, kat["grad"], rtol=0, atol=2e-7)


def test_classification_restates_the_plain_one_at_the_defaults_and_moves_with_the_options():
    """at (0, 0) the three bounds are rnnt_faint_rows.classify's; lambda raises the main and label bounds (be_eff >= beta,
    log1p(lambda) > 0) and an early frame's positive penalty raises the label bound"""
    import rnnt_faint_rows
    rng = np.random.default_rng(11)
    B, T, U = 2, 6, 3
    logits = rng.normal(size=(B, T, U + 1, V)) * 30.0
    targets = rng.integers(1, V, size=(B, U))
    llens, tlens = [6, 4], [3, 2]
    _, _, lats = ref.loss_f64(logits, targets, llens, tlens, BLANK)
    alpha = np.full((B, T, U + 1), -np.inf)
    beta = np.full((B, T, U + 1), -np.inf)
    for b, lat in enumerate(lats):
        alpha[b, :llens[b], :tlens[b] + 1] = lat["alpha"]
        beta[b, :llens[b], :tlens[b] + 1] = lat["beta"]
    want, nb, nl = rnnt_faint_rows.classify(alpha, beta, [l["cost"] for l in lats], targets, llens, tlens, BLANK)
    got, gb, gl = ref.classify(lats, targets, llens, tlens, T, U + 1, BLANK)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(gb, nb)
    np.testing.assert_array_equal(gl, nl)
    assert {ref.LIVE, ref.DEAD} <= set(np.unique(got))
    # monotone in lambda: no row becomes "more dead"
    _, _, lats5 = ref.loss_f64(logits, targets, llens, tlens, BLANK, 0.5, 0.0)
    got5, _, _ = ref.classify(lats5, targets, llens, tlens, T, U + 1, BLANK, 0.5, 0.0)
    order = {ref.PADDED: -1, ref.DEAD: 0, ref.FAINT: 1, ref.LIVE: 2}
    rank = np.vectorize(order.get)
    assert (rank(got5) >= rank(got)).all()
