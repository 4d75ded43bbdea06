"""The float64 TDT reference (tests/rnnt_tdt_ref.py) against brute-force path enumeration, torch autograd of a float64
expression and the modified-lattice reference.  CPU only."""
import numpy as np
import pytest
import torch

import rnnt_lattice_ref
import rnnt_tdt_ref as ref

V = 4
DURATION_SETS = [(0, 1), (0, 1, 2), (0, 1, 2, 3, 4), (1, 2), (0, 2), (2,), (0, 3), (1, 4)]

# (T, U, durations, labels, blank, sigma)
CASES = [(4, 2, (0, 1), (1, 2), 0, 0.0),
         (5, 3, (0, 1, 2), (3, 1, 2), 0, 0.05),
         (6, 2, (0, 1, 2, 3, 4), (2, 2), 0, 0.0),
         (5, 2, (1, 2), (1, 3), 0, 0.1),
         (4, 2, (0, 2), (2, 1), 0, 0.0),
         (6, 1, (2,), (3,), 0, 0.02),
         (6, 3, (0, 3), (1, 2, 3), 0, 0.0),
         (5, 1, (1, 4), (2,), 0, 0.05),
         (5, 2, (0, 1, 2), (1, 1), 1, 0.0),          # a label equal to the blank
         (4, 3, (0, 1), (2, 0, 2), 2, 0.03),         # blank in the middle of the vocabulary
         (4, 0, (0, 1, 2), (), 0, 0.0),              # U_b = 0
         (1, 2, (0, 1), (1, 2), 0, 0.0),             # T_b = 1: both labels with d = 0, then one blank
         (1, 0, (1, 2), (), 0, 0.0)]


def _logits(T, U, D, seed):
    return np.random.default_rng(seed).normal(size=(T, U + 1, V + D)) * 1.5


def test_duration_sets_are_all_covered():
    assert {c[2] for c in CASES} >= set(DURATION_SETS)


@pytest.mark.parametrize("case", range(len(CASES)))
def test_reference_equals_path_enumeration_and_autograd(case):
    T, U, durs, labels, blank, sigma = CASES[case]
    x = _logits(T, U, len(durs), 100 + case)
    cost, grad, alpha, beta = ref.tdt_utt_f64(x, labels, T, U, durs, blank, sigma)
    brute = ref.enumerate_paths(x, labels, T, U, durs, blank, sigma)
    assert np.isfinite(cost) and np.isfinite(brute)
    np.testing.assert_allclose(-cost, brute, rtol=0, atol=1e-12)
    np.testing.assert_allclose(alpha[0, 0], 0.0)
    np.testing.assert_allclose(beta[0, 0], -cost, rtol=0, atol=1e-12)
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ct = ref.cost_torch(xt, labels, T, U, durs, blank, sigma)
    ct.backward()
    np.testing.assert_allclose(ct.item(), cost, rtol=0, atol=1e-12)
    np.testing.assert_allclose(grad, xt.grad.numpy(), rtol=0, atol=2e-14)


def test_infeasible_lattice_costs_inf_from_both():
    T, U, durs = 3, 1, (2,)
    x = _logits(T, U, 1, 7)
    cost, grad, _, _ = ref.tdt_utt_f64(x, (1,), T, U, durs, 0, 0.0)
    assert cost == np.inf and np.isnan(grad).all()
    assert ref.enumerate_paths(x, (1,), T, U, durs, 0, 0.0) == -np.inf
    assert ref.cost_torch(torch.tensor(x), (1,), T, U, durs, 0, 0.0).item() > -ref.NEG_BIG / 2


@pytest.mark.parametrize("T,U", [(5, 2), (3, 3), (4, 0), (1, 1)])
def test_duration_one_is_the_modified_lattice(T, U):
    rng = np.random.default_rng(T * 10 + U)
    x = rng.normal(size=(T, U + 1, V + 1))
    labels = rng.integers(1, V, size=U)
    cost, _, alpha, beta = ref.tdt_utt_f64(x, labels, T, U, (1,), 0, 0.0)
    tok, _ = ref.arcs_f64(x, V, 0.0)
    skip = tok[..., 0]
    emit = np.zeros((T, U + 1))
    for u in range(U):
        emit[:, u] = tok[:, u, labels[u]]
    # the one difference: TDT's terminal is entered by a blank, so a label arc out of the last frame does not exist
    emit[T - 1, :] = -np.inf
    mcost, malpha, mbeta, _, _ = rnnt_lattice_ref.lattice_modified_f64(skip, emit)
    if T <= U:
        assert cost == np.inf and mcost == np.inf
        return
    np.testing.assert_allclose(cost, mcost, rtol=0, atol=1e-12)
    np.testing.assert_allclose(alpha, malpha, rtol=0, atol=1e-12)
    np.testing.assert_allclose(beta, mbeta, rtol=0, atol=1e-12)


def test_unreachable_valid_cell_has_exactly_zero_gradient():
    # durations (0, 2), T = 4: blanks move two frames, so frames 1 and 3 are never entered
    T, U, durs = 4, 2, (0, 2)
    x = _logits(T, U, 2, 11)
    cost, grad, alpha, beta = ref.tdt_utt_f64(x, (1, 2), T, U, durs, 0, 0.0)
    assert np.isfinite(cost)
    assert np.all(alpha[1] == -np.inf) and np.all(alpha[3] == -np.inf)
    assert np.all(grad[1] == 0.0) and np.all(grad[3] == 0.0)
    assert np.abs(grad[0]).max() > 0 and np.isfinite(grad).all()
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    ref.cost_torch(xt, (1, 2), T, U, durs, 0, 0.0).backward()
    np.testing.assert_allclose(grad, xt.grad.numpy(), rtol=0, atol=2e-14)


def test_batch_wrapper_pads_with_zeros():
    rng = np.random.default_rng(3)
    B, T, U, durs = 3, 5, 2, (0, 1, 2)
    x = rng.normal(size=(B, T, U + 1, V + 3))
    targets = rng.integers(1, V, size=(B, U))
    llens, tlens = [5, 3, 1], [2, 1, 0]
    costs, grad, alpha, beta = ref.tdt_ref(x, targets, llens, tlens, durs, 0, 0.05)
    assert np.isfinite(costs).all()
    for b in range(B):
        c, g, a, be = ref.tdt_utt_f64(x[b], targets[b], llens[b], tlens[b], durs, 0, 0.05)
        assert c == costs[b]
        assert np.array_equal(g, grad[b, :llens[b], :tlens[b] + 1])
        assert np.all(grad[b, llens[b]:] == 0) and np.all(grad[b, :, tlens[b] + 1:] == 0)
        assert np.all(alpha[b, llens[b]:] == 0) and np.all(beta[b, :, tlens[b] + 1:] == 0)
