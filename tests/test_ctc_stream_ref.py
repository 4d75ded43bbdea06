"""The float64 reference of the streaming CTC prefix beam search (tests/ctc_stream_ref.py) on the CPU: the reference
test's known answers for all three outputs (runtime/core/test/ctc_prefix_beam_search_test.cc:30-73), equality with the
whole-utterance reference of tests/ctc_decode_ref.py, chunk invariance, the times invariant, and that every input the
GPU file uses keeps its decisions apart."""
import json
import math
import os

import numpy as np
import pytest

import ctc_decode_ref as cref
import ctc_stream_ref as sref
from conftest import GOLDEN

MIN_GAP = 1e-3
RANGE_CASES = [(1, 30, 17, 0), (2, 31, 18, 0), (9, 33, 19, 4), (12, 35, 20, 4), (13, 37, 19, 6), (16, 40, 20, 0)]
# (beam, T, V, seed, blank) of every other peaky_logits input of tests/test_ctc_stream_gpu.py
OTHER_CASES = [(16, 23, 20, 5, 0), (16, 1, 20, 0, 0), (16, 32, 19, 3, 5), (3, 32, 19, 0, 18), (1, 12, 2, 0, 0),
               (2, 12, 2, 0, 0), (2, 12, 2, 0, 1), (16, 30, 16, 0, 0), (3, 40, 20, 0, 0)]


def kat():
    d = np.load(os.path.join(GOLDEN, "ctc_prefix_kat.npz"))
    with open(os.path.join(GOLDEN, "ctc_prefix_times_kat.json")) as f:
        k = json.load(f)
    assert k["beam"] == int(d["beam"])
    assert k["nbest"] == [list(map(int, d["nbest"][i][: d["nbest_lens"][i]])) for i in range(3)]
    np.testing.assert_allclose(k["likelihood"], d["likelihood"], rtol=1e-6)
    return np.log(d["probs"].astype(np.float64)), k


@pytest.mark.parametrize("chunks", [None, [1, 2], [2, 1], [1, 1, 1]])
def test_known_answers_of_the_reference_test(chunks):
    lp, k = kat()
    nb, _ = sref.search_logp(lp, 3, k["beam"], chunks=chunks)
    assert [list(t) for t, _, _, _ in nb] == k["nbest"]
    assert [list(tm) for _, _, _, tm in nb] == k["times"]
    for (_, s, v, _), like, vit in zip(nb, k["likelihood"], k["viterbi_likelihood"]):
        assert math.exp(s) == pytest.approx(like, rel=1e-6)
        assert math.exp(v) == pytest.approx(vit, rel=1e-6)


@pytest.mark.parametrize("beam,T,V,seed", RANGE_CASES)
def test_hypotheses_and_scores_equal_the_whole_utterance_reference(beam, T, V, seed):
    x = cref.peaky_logits(seed, T, V, 0)
    lp = cref.log_softmax_f64(x)
    nb, st = sref.search_logp(lp, T, beam)
    want, st0 = cref.prefix_beam_search_logp(lp, T, beam)
    assert [(t, s) for t, s, _, _ in nb] == want               # value for value
    assert (st.max_ncur, st.max_slots, st.pairs, st.merges) == (st0.max_ncur, st0.max_slots, st0.pairs, st0.merges)
    assert st.min_gap <= st0.min_gap                            # the Viterbi decisions only add to the list


@pytest.mark.parametrize("beam,T,V,seed", RANGE_CASES)
def test_chunk_invariance_and_times_invariant(beam, T, V, seed):
    x = cref.peaky_logits(seed, T, V, 0)
    whole, _ = sref.search(x, T, beam)
    sref.check_times(whole, T)
    for chunks in ([1] * T, [7, 16, T - 23], [T - 1, 0, 1]):
        assert sref.search(x, T, beam, chunks=chunks)[0] == whole


def test_partial_results_satisfy_the_times_invariant():
    x = cref.peaky_logits(0, 40, 20, 0)
    s = sref.Stream(16)
    lp = cref.log_softmax_f64(x)
    for t in range(40):
        s.consume(lp[t:t + 1])
        assert s.a_next == t + 1
        sref.check_times(s.nbest(), t + 1)


def test_every_gpu_input_keeps_its_decisions_apart():
    for beam, T, V, seed in RANGE_CASES:
        _, st = sref.search(cref.peaky_logits(seed, T, V, 0), T, beam)
        assert st.min_gap >= MIN_GAP and st.ties == 0, (beam, T, V, seed, st)
        if beam >= 9:
            assert 4 <= st.kept <= 13 and st.merges > 0 and st.pairs > 0, st
    for beam, T, V, seed, blank in OTHER_CASES:
        _, st = sref.search(cref.peaky_logits(seed, T, V, blank), T, beam, blank)
        assert st.min_gap >= MIN_GAP and st.ties == 0, (beam, T, V, seed, blank, st)

