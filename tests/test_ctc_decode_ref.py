"""The float64 CTC decode references of tests/ctc_decode_ref.py, on the CPU: what the GPU tests trust is checked here
first -- against oracle.decode_oracle at blank 0, against the fixtures the reference's own modules produced
(tests/golden/ctc_decode_*.npz, ctc_prefix_kat.npz, ctc_align_*.npz), and for equivariance under a relabelling of the
vocabulary that moves the blank."""
import glob
import math
import os

import numpy as np
import pytest

import ctc_decode_ref as ref
from conftest import GOLDEN
from oracle import decode_oracle as do

DECODE = sorted(glob.glob(os.path.join(GOLDEN, "ctc_decode_*.npz")))
ALIGN = sorted(glob.glob(os.path.join(GOLDEN, "ctc_align_*.npz")))


@pytest.mark.parametrize("seed,T,V,beam", [(0, 12, 7, 3), (1, 25, 18, 16), (2, 30, 40, 5), (3, 9, 2, 2), (4, 20, 16, 16),
                                           (5, 1, 5, 1)])
def test_prefix_search_equals_oracle_at_blank_0(seed, T, V, beam):
    lp = do.log_softmax(ref.peaky_logits(seed, T, V, 0))
    want = do.ctc_prefix_beam_search(lp, T, beam)
    got, st = ref.prefix_beam_search_logp(lp.astype(np.float64), T, beam, 0)
    assert got == want                                  # same arithmetic on the same values: bit for bit
    assert 1 <= st.max_ncur <= beam and st.max_slots <= 2 * beam * beam


def test_prefix_search_float64_softmax_keeps_the_oracle_hypotheses():
    x = ref.peaky_logits(7, 30, 19, 0)
    want = do.ctc_prefix_beam_search(do.log_softmax(x), 30, 6)
    got, st = ref.prefix_beam_search(x, 30, 6, 0)
    assert st.min_gap > 1e-4                            # far above the fp32 log-softmax's rounding
    assert [p for p, _ in got] == [p for p, _ in want]
    np.testing.assert_allclose([s for _, s in got], [s for _, s in want], rtol=1e-6)


def test_prefix_search_statistics_on_a_hand_case():
    """Two frames, V = 3, beam 2, blank 0.  Frame 0 keeps symbols {1, 0}: prefixes (1,), ().  Frame 1 keeps {1, 0}
    again: symbol 1 on (1,) is a same-symbol pair (2 slots), so 2 * 2 + 1 = 5 slots; (1,) is reached from (1,) and
    from (): one merge."""
    x = np.log(np.array([[0.3, 0.6, 0.1], [0.3, 0.6, 0.1]], np.float32))
    got, st = ref.prefix_beam_search(x, 2, 2, 0)
    assert st.max_ncur == 2 and st.max_slots == 5 and st.pairs == 1 and st.merges == 1 and st.ties == 0
    # (1,): 0.6*0.3 (1,blank) + 0.6*0.6 (1,1) + 0.3*0.6 (blank,1) = 0.72; (): 0.09; (1,1): needs a blank between -> 0
    assert got[0][0] == (1,) and math.exp(got[0][1]) == pytest.approx(0.72, rel=1e-6)
    assert got[1][0] == () and math.exp(got[1][1]) == pytest.approx(0.09, rel=1e-6)
    # gaps: the top-k cut log .3 - log .1 and the final list's log .72 - log .09; the prune cut's loser (1, 1) is -inf
    assert st.min_gap == pytest.approx(math.log(3.0), rel=1e-6)


def test_uniform_rows_are_ties_not_gaps():
    got, st = ref.prefix_beam_search(np.zeros((1, 3), np.float32), 1, 3, 0)
    assert st.ties == 2 and st.min_gap == float("inf")
    assert [p for p, _ in got] == [(), (1,), (2,)]      # equal scores: the visiting (= index) order
    assert all(s == math.log(1 / 3) for _, s in got)
    got, st = ref.prefix_beam_search(np.zeros((2, 3), np.float32), 2, 3, 0)
    # 1/9 for (), (2, 1), (1, 2); 3/9 for (1,), (2,): the prune cut falls between () and (2, 1), a tie
    assert [p for p, _ in got] == [(1,), (2,), ()] and st.ties >= 2 and st.min_gap == pytest.approx(math.log(3))


@pytest.mark.parametrize("path", DECODE)
def test_reproduces_decode_fixture(path):
    d = np.load(path)
    logits, lens, beam = d["logits"], d["lens"], int(d["beam"])
    hyps, scores = ref.greedy_search(logits, lens, 0, -1)
    for b, h in enumerate(hyps):
        assert h == list(d["greedy"][b][: d["greedy_lens"][b]])
    np.testing.assert_allclose(scores, d["greedy_scores"], rtol=1e-5, atol=1e-6)
    for b in range(logits.shape[0]):
        nb, _ = ref.prefix_beam_search(logits[b], int(lens[b]), beam, 0)
        assert len(nb) == int(d["nbest_n"][b])
        for k, (pref, sc) in enumerate(nb):
            assert list(pref) == list(d["nbest"][b, k][: d["nbest_lens"][b, k]]), (b, k)
            assert sc == pytest.approx(d["nbest_scores"][b, k], rel=1e-5)


def test_reproduces_known_answer():
    d = np.load(os.path.join(GOLDEN, "ctc_prefix_kat.npz"))
    nb, _ = ref.prefix_beam_search(np.log(d["probs"]).astype(np.float32), 3, int(d["beam"]), 0)
    for k, (pref, sc) in enumerate(nb):
        assert list(pref) == list(d["nbest"][k][: d["nbest_lens"][k]])
        assert math.exp(sc) == pytest.approx(float(d["likelihood"][k]), rel=1e-4)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_greedy_equals_oracle_at_blank_0(seed):
    rng = np.random.default_rng(seed)
    B, T, V = 4, 23, 11
    x = (rng.normal(size=(B, T, V)) * 2).astype(np.float32)
    x[:, :, 0] += 2
    lens = np.array([T, 0, 7, T + 3])
    wh, ws = do.ctc_greedy_search(x, lens, V - 1)
    gh, gs = ref.greedy_search(x, lens, 0, V - 1)
    assert gh == wh
    np.testing.assert_allclose(gs, ws, rtol=1e-5, atol=1e-6)


def _swap(V, b):
    perm = np.arange(V)
    perm[0], perm[b] = b, 0
    return perm


@pytest.mark.parametrize("b", [5, 16])
@pytest.mark.parametrize("beam", [4, 16])
def test_prefix_search_is_equivariant_under_moving_the_blank(b, beam):
    T, V = 28, 17
    x = ref.peaky_logits(11, T, V, 0)
    perm = _swap(V, b)
    base, st0 = ref.prefix_beam_search(x, T, beam, 0)
    moved, st1 = ref.prefix_beam_search(x[:, perm], T, beam, b)
    assert st0.min_gap > 1e-6 and st0.ties == 0         # no decision hangs on the summation order of the softmax
    assert [tuple(int(perm[v]) for v in p) for p, _ in moved] == [p for p, _ in base]
    np.testing.assert_allclose([s for _, s in moved], [s for _, s in base], rtol=1e-12)
    assert (st1.max_ncur, st1.max_slots, st1.pairs, st1.merges) == (st0.max_ncur, st0.max_slots, st0.pairs, st0.merges)


@pytest.mark.parametrize("b", [3, 10])
def test_greedy_is_equivariant_under_moving_the_blank(b):
    rng = np.random.default_rng(b)
    B, T, V = 3, 31, 11
    x = (rng.normal(size=(B, T, V)) * 2).astype(np.float32)
    x[:, :, 0] += 2
    lens = np.array([T, 12, 0])
    perm = _swap(V, b)
    eos = 7                                             # a label the swap leaves alone
    bh, bs = ref.greedy_search(x, lens, 0, eos)
    mh, ms = ref.greedy_search(x[:, :, perm], lens, b, eos)
    assert [[int(perm[v]) for v in h] for h in mh] == bh
    np.testing.assert_allclose(ms, bs, rtol=1e-12)
    assert any(0 in h for h in mh)                      # label 0 is an ordinary token once the blank has moved


@pytest.mark.parametrize("path", ALIGN)
def test_forced_align_reproduces_fixture(path):
    d = np.load(path)
    assert ref.forced_align(d["ctc_probs"], d["y"]) == list(d["alignment"])


@pytest.mark.parametrize("blank_id", [0, 3, 8])
def test_forced_align_equals_oracle_and_reports_ties(blank_id):
    rng = np.random.default_rng(blank_id)
    T, V = 26, 9
    lp = (np.round(rng.normal(size=(T, V)) * 8) / 8 - 3).astype(np.float32)       # multiples of 1/8: exact sums, ties
    y = [1, 1, blank_id, 4, 5, 5, 2]
    ali, ties = ref.forced_align(lp, y, blank_id, return_ties=True)
    assert ali == do.forced_align(lp, y, blank_id)
    assert all(len(k) == 2 and k[0] < k[1] for k in ties)
    assert ref.forced_align(lp, [], blank_id) == [blank_id] * T


@pytest.mark.parametrize("T,S", [(1, 1), (1, 3), (4, 6), (9, 6), (40, 8), (60, 5)])
def test_forced_align_equals_oracle_in_every_length_regime(T, S):
    """One frame, fewer frames than labels, fewer than 2S+1, and T >> 2S+1 (where the s-1 = -1 wrap is taken)."""
    V = 7
    for seed in range(4):
        rng = np.random.default_rng(100 * T + 10 * S + seed)
        lp = do.log_softmax((rng.normal(size=(T, V)) * 2).astype(np.float32))
        if seed % 2:
            lp = (np.round(lp * 4) / 4).astype(np.float32)
        y = rng.integers(0, V, size=S)
        for blank_id in (0, 2, V - 1):
            assert ref.forced_align(lp, y, blank_id) == do.forced_align(lp, y, blank_id), (seed, blank_id)
