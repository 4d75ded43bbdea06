"""CPU checks of the three-way row classification of the RNN-T gradient pass (tests/rnnt_faint_rows.py restates it) on
small sharp lattices against the float64 oracle: every element of a row the rule calls dead, and every element of a
faint row other than its blank / label, is below 2^-126 in magnitude, the least non-zero value the gradient pass's
exponential returns (the cut-off is the helper's constant, not something taken from the kernel under test)."""
import numpy as np
import pytest

import oracle
from rnnt_dead_rows import dead_mask, lattice_f64
from rnnt_faint_rows import CUTOFF, DEAD, DEAD_THR, FAINT, LIVE, LOG2E, MARGIN_LOG2, PADDED, X0, classify, share, \
    thr_from_cutoff


def _case(rng, B, T, U, V, scale, blank):
    logits = (rng.normal(size=(B, T, U + 1, V)) * scale).astype(np.float32)
    targets = rng.integers(0, V, size=(B, U)).astype(np.int32)
    targets[targets == blank] = (blank + 1) % V
    llens = np.concatenate([[T], rng.integers(1, T + 1, size=B - 1)]).astype(np.int32)
    tlens = np.concatenate([[U], rng.integers(0, U + 1, size=B - 1)]).astype(np.int32)
    return logits, targets, llens, tlens


def test_constants():
    assert X0 == float(np.nextafter(np.float32(-126.0), np.float32(-np.inf)))
    assert CUTOFF == 2.0 ** -126
    assert DEAD_THR == thr_from_cutoff(X0) == -93.3
    assert DEAD_THR * LOG2E <= X0 - MARGIN_LOG2


@pytest.mark.parametrize("seed,B,T,U,V,scale,blank", [
    (0, 3, 40, 12, 24, 10.0, 0),
    (1, 2, 60, 8, 17, 8.0, 16),       # blank = V - 1
    (2, 3, 30, 15, 9, 10.0, 3),
    (3, 2, 60, 15, 33, 12.0, 0),
])
def test_dead_and_faint_rows_against_the_oracle_gradient(seed, B, T, U, V, scale, blank):
    rng = np.random.default_rng(seed)
    logits, targets, llens, tlens = _case(rng, B, T, U, V, scale, blank)
    if seed == 2:
        targets[0, ::3] = blank                           # label == blank: the label term merges into the blank term
    denom, alpha, beta, cost = lattice_f64(logits, targets, llens, tlens, blank)
    oc, og = oracle.rnnt_loss_f64(logits, targets, llens, tlens, blank=blank)
    np.testing.assert_allclose(cost, oc, rtol=1e-9, atol=1e-9)      # the restated lattice is the oracle's
    cls, need_b, need_l = classify(alpha, beta, cost, targets, llens, tlens, blank, denom=denom)
    assert share(cls, FAINT, llens, tlens) > 0.005 and share(cls, DEAD, llens, tlens) > 0.05   # the cases exercise it
    og = np.abs(np.asarray(og, np.float64))
    assert np.all(og[cls == DEAD] < CUTOFF)
    # a faint row: everything but the element(s) it reads
    small = og < CUTOFF
    small[..., blank] |= need_b
    lab = np.zeros(cls.shape, np.int64)
    lab[:, :, :U] = targets[:, None, :]
    got = np.take_along_axis(small, lab[..., None], axis=-1)[..., 0]
    np.put_along_axis(small, lab[..., None], (got | need_l)[..., None], axis=-1)
    assert np.all(small[cls == FAINT])
    # not vacuous: every faint row has an element it reads, and the live rows carry the gradient
    assert np.all((need_b | need_l)[cls == FAINT]) and not (need_b | need_l)[cls != FAINT].any()
    assert og[cls == LIVE].max() > 1e-3
    assert not og[cls == PADDED].any()
    # the rule before this one (all three bounds below -110) marks a subset of the new dead rows
    old = dead_mask(alpha, beta, cost, targets, llens, tlens, blank, denom=denom)
    assert np.all(cls[old] == DEAD)


def test_classification_edges():
    """NaN and the thresholds: a NaN in the main bound keeps a row live, a NaN in a side bound keeps that element read,
    a bound at the threshold is not below it, and the final cell's blank bound is alpha + cost."""
    B, T, U1 = 1, 2, 2
    targets = np.array([[5]], np.int32)
    llens, tlens = [2], [1]
    cost = np.array([0.0])
    alpha = np.full((B, T, U1), -200.0)
    beta = np.full((B, T, U1), -200.0)
    cls, nb, nl = classify(alpha, beta, cost, targets, llens, tlens)
    assert (cls == DEAD).all() and not nb.any() and not nl.any()
    a2 = alpha.copy(); a2[0, 1, 1] = np.nan
    assert classify(a2, beta, cost, targets, llens, tlens)[0][0, 1, 1] == LIVE
    a3 = alpha.copy(); a3[0, 1, 1] = 200.0 + DEAD_THR    # final cell: alpha + beta = DEAD_THR exactly -> live
    assert classify(a3, beta, cost, targets, llens, tlens)[0][0, 1, 1] == LIVE
    a4 = alpha.copy(); a4[0, 1, 1] = -50.0; b4 = beta.copy(); b4[0, 1, 1] = -100.0
    cls, nb, nl = classify(a4, b4, cost, targets, llens, tlens)   # main -150, the blank bound alpha + cost = -50: faint
    assert cls[0, 1, 1] == FAINT and nb[0, 1, 1] and not nl[0, 1, 1]
    b5 = beta.copy(); b5[0, 0, 1] = 150.0                # label bound of (0, 0) = alpha + cost + beta(0, 1) = -50
    cls, nb, nl = classify(alpha, b5, cost, targets, llens, tlens)
    assert cls[0, 0, 0] == FAINT and nl[0, 0, 0] and not nb[0, 0, 0] and cls[0, 1, 0] == DEAD
    b6 = beta.copy(); b6[0, 1, 0] = np.nan               # blank bound of (0, 0) is NaN: read the blank, main still dead
    cls, nb, nl = classify(alpha, b6, cost, targets, llens, tlens)
    assert cls[0, 0, 0] == FAINT and nb[0, 0, 0]
    d = np.full((B, T, U1), 1.0); d[0, 0, 0] = np.inf; d[0, 1, 0] = np.nan; d[0, 0, 1] = 65536.0
    cls, _, _ = classify(alpha, beta, cost, targets, llens, tlens, denom=d)
    assert cls[0, 0, 0] == LIVE and cls[0, 1, 0] == LIVE and cls[0, 0, 1] == LIVE and cls[0, 1, 1] == DEAD
