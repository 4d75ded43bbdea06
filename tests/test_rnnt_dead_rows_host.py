"""CPU checks of the dead-cell test of the RNN-T gradient pass (tests/rnnt_dead_rows.py restates it): on small random
lattices every cell it marks dead has a float64 oracle gradient below 2^-150 in every entry, i.e. exactly zero once
rounded to fp32.  Sharp logits make dead cells common at these sizes."""
import numpy as np
import pytest

import oracle
from rnnt_dead_rows import dead_mask, dead_share, lattice_f64


def _case(rng, B, T, U, V, scale, blank):
    logits = (rng.normal(size=(B, T, U + 1, V)) * scale).astype(np.float32)
    targets = rng.integers(0, V, size=(B, U)).astype(np.int32)
    targets[targets == blank] = (blank + 1) % V
    llens = np.concatenate([[T], rng.integers(1, T + 1, size=B - 1)]).astype(np.int32)
    tlens = np.concatenate([[U], rng.integers(0, U + 1, size=B - 1)]).astype(np.int32)
    return logits, targets, llens, tlens


@pytest.mark.parametrize("seed,B,T,U,V,scale,blank", [
    (0, 3, 40, 12, 24, 10.0, 0),
    (1, 2, 60, 8, 17, 8.0, 16),       # blank = V - 1
    (2, 3, 30, 15, 9, 10.0, 3),
    (3, 2, 60, 15, 33, 12.0, 0),
])
def test_dead_cells_have_zero_oracle_gradient(seed, B, T, U, V, scale, blank):
    rng = np.random.default_rng(seed)
    logits, targets, llens, tlens = _case(rng, B, T, U, V, scale, blank)
    if seed == 2:
        targets[0, ::3] = blank                           # label == blank: the label term merges into the blank term
    denom, alpha, beta, cost = lattice_f64(logits, targets, llens, tlens, blank)
    oc, og = oracle.rnnt_loss_f64(logits, targets, llens, tlens, blank=blank)
    np.testing.assert_allclose(cost, oc, rtol=1e-9, atol=1e-9)      # the restated lattice is the oracle's
    dead = dead_mask(alpha, beta, cost, targets, llens, tlens, blank, denom=denom)
    share = dead_share(dead, llens, tlens)
    assert share > 0.05, share                           # the cases exercise the test
    assert np.all(np.abs(og[dead].astype(np.float64)) < 2.0 ** -150)   # (in float32 2^-150 itself rounds to 0)
    # and it is not vacuous: the live cells carry the gradient
    assert np.abs(og[~dead]).max() > 1e-3


def test_predicate_edges():
    """NaN and the thresholds: a NaN bound keeps a cell live, a bound at the threshold is live, and the final cell's
    blank bound is alpha + cost."""
    B, T, U1 = 1, 2, 2
    targets = np.array([[5]], np.int32)
    llens, tlens = [2], [1]
    cost = np.array([0.0])
    alpha = np.full((B, T, U1), -200.0)
    beta = np.full((B, T, U1), -200.0)
    assert dead_mask(alpha, beta, cost, targets, llens, tlens).all()
    a2 = alpha.copy(); a2[0, 1, 1] = np.nan
    assert not dead_mask(a2, beta, cost, targets, llens, tlens)[0, 1, 1]
    a3 = alpha.copy(); a3[0, 1, 1] = 90.0                # final cell: alpha + beta = -110 exactly -> live
    assert not dead_mask(a3, beta, cost, targets, llens, tlens)[0, 1, 1]
    a4 = alpha.copy(); a4[0, 1, 1] = -50.0; b4 = beta.copy(); b4[0, 1, 1] = -100.0
    m = dead_mask(a4, b4, cost, targets, llens, tlens)   # alpha + beta = -150 but the blank bound alpha + cost = -50
    assert not m[0, 1, 1]
    b5 = beta.copy(); b5[0, 0, 1] = 150.0                # label bound of (0, 0) = alpha + cost + beta(0, 1) = -50
    m = dead_mask(alpha, b5, cost, targets, llens, tlens)
    assert not m[0, 0, 0] and m[0, 1, 0]
    d = np.full((B, T, U1), 1.0); d[0, 0, 0] = np.inf; d[0, 1, 0] = np.nan; d[0, 0, 1] = 65536.0
    m = dead_mask(alpha, beta, cost, targets, llens, tlens, denom=d)
    assert not m[0, 0, 0] and not m[0, 1, 0] and not m[0, 0, 1] and m[0, 1, 1]
