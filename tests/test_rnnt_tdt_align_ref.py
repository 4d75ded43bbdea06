"""The float64 TDT alignment reference (tests/rnnt_tdt_align_ref.py) against what it cannot share a mistake with:
brute-force enumeration of every path, the regular-lattice reference on the lattice that durations = (1,) is equivalent
to, and the TDT loss reference (the best path is one of the paths the loss sums).  CPU only."""
import numpy as np
import pytest

import rnnt_align_ref
import rnnt_tdt_align_ref as aref
import rnnt_tdt_ref

V = 6
DURATIONS = [(0, 1, 2, 3, 4), (1,), (1, 2, 4), (0, 8), (2,), tuple(range(9))]
SHAPES = [(1, 0), (3, 0), (5, 2), (7, 3), (9, 1)]


def case(T, U, D, seed=0):
    rng = np.random.default_rng(4200 + 100 * T + 10 * U + D + seed)
    logits = (rng.normal(size=(T, U + 1, V + D)) * 2.0).astype(np.float32)
    labels = rng.integers(1, V, size=U)
    return logits, labels


@pytest.mark.parametrize("T,U", SHAPES)
@pytest.mark.parametrize("durs", DURATIONS)
def test_reference_against_every_path(durs, T, U):
    logits, labels = case(T, U, len(durs))
    tb, tl, dur = aref.arcs(logits, labels, T, U, durs)
    a = aref.viterbi(tb, tl, dur, T, U, durs)
    best, paths = aref.brute_force(tb, tl, dur, T, U, durs)
    assert a.score == best                                     # the same sums in the same order: exactly
    if not paths:
        assert a.score == -np.inf and aref.is_no_path(a.frames, a.durations, a.jumps)
        assert not aref.is_valid_path(a.frames, a.durations, a.jumps, T, U, durs)
        return
    path = aref.rebuild_path(a.frames, a.durations, a.jumps, T, U, durs)
    assert path in paths
    assert aref.path_score(tb, tl, dur, durs, path) == best
    assert a.margin >= 0 and (a.ties > 0) == (a.margin == 0) and a.clear > 0


def test_infeasible_and_feasible_lengths_exist_among_the_cases():
    feasible = {(durs, T, U): aref.align_utt(*case(T, U, len(durs)), T, U, durs).score > -np.inf
                for durs in DURATIONS for T, U in SHAPES}
    assert not feasible[((2,), 3, 0)] and not feasible[((0, 8), 5, 2)]
    assert feasible[((2,), 7, 3)] is False and feasible[((1,), 7, 3)] and feasible[((0, 8), 9, 1)] is False
    assert sum(feasible.values()) >= 18


@pytest.mark.parametrize("T,U", [(3, 0), (5, 2), (7, 3), (9, 1)])
def test_duration_one_is_the_modified_lattice(T, U):
    """durations = (1,): every arc consumes a frame.  Cell (t, u) of it is cell (t - u, u) of a regular lattice of T - U
    frames whose blank / emit log-probabilities are the TDT cell's -- the cells this leaves out cannot reach the
    terminal -- and both references send a tie to the blank."""
    logits, labels = case(T, U, 1, seed=3)
    tb, tl, dur = aref.arcs(logits, labels, T, U, (1,))
    assert not dur.any()                                        # a one-column softmax
    a = aref.viterbi(tb, tl, dur, T, U, (1,))
    Tr = T - U
    blank_lp = np.array([[tb[t + u, u] for u in range(U + 1)] for t in range(Tr)])
    emit_lp = np.array([[tl[t + u, u] for u in range(U)] for t in range(Tr)]).reshape(Tr, U)
    score, frames, _ = rnnt_align_ref.viterbi(blank_lp, emit_lp, Tr, U)
    np.testing.assert_allclose(a.score, score, rtol=1e-12)
    assert np.array_equal(a.frames, np.asarray(frames) + np.arange(U))
    assert np.all(a.durations == 1)


@pytest.mark.parametrize("durs", [(0, 1, 2, 3, 4), (1, 2, 4), tuple(range(9))])
def test_score_is_at_most_the_log_likelihood(durs):
    T, U = 7, 3
    logits, labels = case(T, U, len(durs), seed=5)
    for sigma in (0.0, 0.05):
        a = aref.align_utt(logits, labels, T, U, durs, 0, sigma)
        cost = rnnt_tdt_ref.tdt_utt_f64(logits, labels, T, U, durs, 0, sigma)[0]
        assert np.isfinite(cost) and a.score <= -cost + 1e-6 and a.score > -cost - 20.0


def test_tie_rule_and_diagnostics():
    """Every cell holds the same row and the labels are one token: paths that differ only in where the d = 0 and d = 2
    label arcs stand tie exactly.  Blank beats label, the smaller d wins."""
    durs, T, U = (0, 1, 2, 3), 9, 4
    row = np.zeros(12 + 4, np.float32)
    row[:12] = np.linspace(-1.0, 1.0, 12)
    row[12:] = (0.0, 0.5, 0.0, -1.0)
    logits = np.broadcast_to(row, (T, U + 1, 16))
    a = aref.align_utt(logits, np.full(U, 3), T, U, durs)
    assert a.ties >= 1 and a.margin == 0 and a.clear > 1e-3
    tb, tl, dur = aref.arcs(logits, np.full(U, 3), T, U, durs)
    best, paths = aref.brute_force(tb, tl, dur, T, U, durs)
    assert a.score == best and len(paths) > 1
    assert aref.rebuild_path(a.frames, a.durations, a.jumps, T, U, durs) in paths
