"""The context graph builder and the float64 reference of the biased CTC prefix beam search (tests/ctc_context_ref.py):
the three-state example table, the builder's refusals, purity on random inputs, the known answers, UpdateOutputs.
No GPU is needed and none is used."""
import json
import math
import os

import numpy as np
import pytest

import ctc_context_ref as xref
import ctc_decode_ref as cref
import ctc_stream_ref as sref
from conftest import GOLDEN


def _graph(*a, **k):
    from wenet_celoss_amd.context_graph import ContextGraph
    return ContextGraph(*a, **k)


def test_builder_three_state_table():
    """[1,2], [1,2,3], [4] at score 1: state 0: 1->1, 4->0; state 1: 2->2, escape -1; state 2: final, 3->0, escape 0."""
    g = _graph([[1, 2], [1, 2, 3], [4]], 1.0)
    assert g.n_states == 3 and g.n_arcs == 4
    assert g.arc_begin.tolist() == [0, 2, 3, 4] and g.arc_begin.dtype == np.int32
    assert g.arc_token.tolist() == [1, 4, 2, 3] and g.arc_next.tolist() == [1, 0, 2, 0]
    assert g.arc_score.tolist() == [1.0] * 4 and g.arc_score.dtype == np.float32
    assert g.escape.tolist() == [0.0, -1.0, 0.0] and g.escape.dtype == np.float32
    assert not np.signbit(g.escape[[0, 2]]).any()                 # +0.0 at the root and at final states
    assert g.final.tolist() == [1, 0, 1]
    # next(): an arc, a start boundary from the root, an end boundary into a final state or back to the root
    assert g.next(0, 1) == (1, 1.0, True, False)
    assert g.next(1, 2) == (2, 1.0, False, True)
    assert g.next(2, 3) == (0, 1.0, False, True)
    assert g.next(0, 4) == (0, 1.0, True, True)
    # no arc: back to the root with the escape; the breaking token is not retried from the root
    assert g.next(1, 1) == (0, -1.0, False, False)
    assert g.next(2, 1) == (0, 0.0, False, False)                 # the nested phrase is committed: its bonus stays
    assert g.next(0, 7) == (0, 0.0, False, False)
    # the same phrases again and in another order of duplicates: de-duplicated, insertion order of the first occurrences
    h = _graph([[1, 2], [1, 2], [1, 2, 3], [4], [1, 2, 3]], 1.0)
    assert all(np.array_equal(getattr(g, n), getattr(h, n)) for n in ("arc_begin", "arc_token", "arc_next", "escape", "final"))


def test_builder_escape_values_and_order():
    g = _graph([[5, 6, 7, 8], [5, 6], [5, 9], [3]], 0.3)
    s = np.float32(0.3)
    # states in insertion order: 1 = (5), 2 = (5,6) final, 3 = (5,6,7); [5,6,7,8], [5,9] and [3] end on arcs to the root
    assert g.n_states == 4
    assert g.final.tolist() == [1, 0, 1, 0]
    assert g.escape.tolist() == [0.0, float(-s), 0.0, float(np.float32(0.0) - s)]
    assert g.arc_begin.tolist() == [0, 2, 4, 5, 6]
    assert g.arc_token.tolist() == [3, 5, 6, 9, 7, 8] and g.arc_next.tolist() == [0, 1, 2, 0, 3, 0]
    assert all((np.diff(g.arc_token[a:b]) > 0).all() for a, b in zip(g.arc_begin[:-1], g.arc_begin[1:]))
    # a long unnested phrase: the escape is minus the running float32 sum
    g = _graph([[1, 2, 3, 4]], 0.1)
    acc, want = np.float32(0.0), [0.0]
    for _ in range(3):
        acc = np.float32(acc - np.float32(0.1))
        want.append(float(acc))
    assert g.escape.tolist() == want
    # reachability: every state but the root is some arc's target
    assert set(range(1, g.n_states)) <= set(g.arc_next.tolist())


def test_builder_empty_graph():
    g = _graph([])
    assert (g.n_states, g.n_arcs) == (1, 0)
    assert g.arc_begin.tolist() == [0, 0] and g.escape.tolist() == [0.0] and g.final.tolist() == [1]
    assert g.arc_token.size == g.arc_next.size == g.arc_score.size == 0
    assert g.next(0, 3) == (0, 0.0, False, False)


@pytest.mark.parametrize("args, text", [
    (([[1], []],), "empty phrase"), (([[1, -1]],), "token -1"), (([[1, 0]],), "token 0"),
    (([[1, 4]], 3.0, 4), "token 4"), (([[1]], float("nan")), "not finite"), (([[1]], float("inf")), "not finite"),
    (([[1]], 1e39), "not finite"), (([[i + 1] for i in range(5001)],), "5001 phrases"),
    (([list(range(1, 102))],), "101 tokens")])
def test_builder_refusals(args, text):
    with pytest.raises(ValueError, match=text):
        _graph(*args)


def test_builder_limits_pass():
    assert _graph([[i + 1] for i in range(5000)]).n_arcs == 5000
    assert _graph([list(range(1, 101))]).n_states == 100
    assert _graph([[0, 1]], blank=2).n_arcs == 2                  # 0 is a token when the blank is elsewhere


@pytest.mark.parametrize("beam,T,V,seed,blank", [(4, 25, 9, 0, 0), (8, 30, 12, 1, 0), (16, 30, 20, 2, 0), (6, 25, 9, 3, 4)])
def test_purity_on_random_inputs(beam, T, V, seed, blank):
    """Every contributor to a key yields the same (ctx_state, ctx_score, tags): the reference asserts it per
    contribution; here random phrase sets over a small vocabulary make keys with many contributors."""
    rng = np.random.default_rng(100 + seed)
    labels = [v for v in range(V) if v != blank]
    phrases = [[int(labels[i]) for i in rng.integers(len(labels), size=int(rng.integers(1, 5)))] for _ in range(30)]
    x = cref.peaky_logits(seed, T, V, blank)
    nb, st = xref.search(x, T, beam, _graph(phrases, 1.5, blank), blank)
    print(st)
    assert st.purity > 0 and st.merges > 0 and st.ends > 0 and st.starts > 0
    xref.check_tags(nb)
    sref.check_times([h[:4] for h in nb], T)
    for h in nb:
        assert h[1] == h[4] + h[5]
    # chunking the reference changes nothing
    assert xref.search(x, T, beam, _graph(phrases, 1.5, blank), blank, chunks=[7, 1, T - 8])[0] == nb


@pytest.fixture(scope="module")
def kat():
    with open(os.path.join(GOLDEN, "ctc_context_kat.json")) as f:
        k = json.load(f)
    probs = np.load(os.path.join(GOLDEN, k["probs_file"]))["probs"]
    return k, np.log(probs.astype(np.float64))


def test_known_answers(kat):
    """The reference test's probabilities {0.25,0.40,0.35},{0.40,0.35,0.25},{0.10,0.50,0.40}, beam 3, blank 0, phrase [1,2].

    By hand, the first line of each row (frames f1, f2, f3; a path is one symbol per frame):
      score 0: [2,1] is reached by the paths 2,1,1 (.35*.35*.5 = .06125), 2,2,1 (.35*.25*.5 = .04375), 2,0,1
        (.35*.40*.5 = .07), 0,2,1 (.25*.25*.5 = .03125) and 2,1,0 (.35*.35*.1 = .01225): 0.2185, the unbiased 1-best.
      score 0.25: [1,2] is reached by 1,1,2 (.4*.35*.4 = .056), 1,2,2 (.4*.25*.4 = .04), 1,0,2 (.4*.4*.4 = .064), 0,1,2
        (.25*.35*.4 = .035) and 1,2,0 (.4*.25*.1 = .01): 0.2050 -- all of them, since the bonus keeps [1] and [1,2] in
        the beam (unbiased, the beam holds only 0.1550 of it).  Two arcs at 0.25: ctx 0.5; tags (1, 2): the phrase starts
        at token 0 and ends at token 1.  Total ln 0.205 + 0.5 = -1.0847.  Finalising leaves it alone (its state is the
        root) and takes 0.25 back from [1] and [2,1], which sit inside a match.
      score 3.0: [1,2,1] is the one path 1,2,1 (.4*.25*.5 = .05); three arcs (1, 2 back to the root, 1 again): ctx 9,
        tags (1, 2, 1), total ln 0.05 + 9 = 6.0043.  Finalising takes the third arc's 3 back: ctx 6, total 3.0043, below
        [1,2] at ln 0.205 + 6 = 4.4153 -- the 1-best changes."""
    k, lp = kat
    for row in k["rows"]:
        g = _graph(k["phrases"], row["context_score"], k["blank"])
        nb, st = xref.search_logp(lp, 3, k["beam"], g, k["blank"], finalize=row["finalize"])
        print(row["context_score"], row["finalize"], nb, st)
        assert [list(h[0]) for h in nb] == row["nbest"]
        assert [list(h[6]) for h in nb] == row["tags"]
        assert [h[5] for h in nb] == row["context"]
        assert list(st.states) == row["states"]
        for h, like in zip(nb, row["ctc_likelihood"]):
            assert math.exp(h[4]) == pytest.approx(like, rel=1e-6)       # the fixture's probabilities are float32
            assert h[1] == h[4] + h[5]
        assert st.ties == 0 and st.min_gap > 1e-2
    rows = {(r["context_score"], r["finalize"]): r for r in k["rows"]}
    assert rows[(3.0, True)]["nbest"][0] != rows[(3.0, False)]["nbest"][0]            # finalising changes the 1-best
    assert math.log(0.205) + 6.0 == pytest.approx(4.4153, abs=5e-5) and math.log(0.05) + 6.0 == pytest.approx(3.0043, abs=5e-5)


def test_unbiased_rows_equal_the_stream_reference(kat):
    """Score 0 (the graph is walked, so its tags are set, but no bonus moves anything) and the empty graph (tags all 0):
    hypotheses, scores, Viterbi scores and times equal ctc_stream_ref value for value, in one chunk and in chunks."""
    k, lp = kat
    plain, _ = sref.search_logp(lp, 3, k["beam"], k["blank"])
    for g in (_graph(k["phrases"], 0.0), _graph([])):
        for chunks in (None, [1, 2], [1, 1, 1]):
            for fin in (False, True):
                nb, _ = xref.search_logp(lp, 3, k["beam"], g, k["blank"], chunks=chunks, finalize=fin)
                assert [h[:4] for h in nb] == plain
                assert all(h[5] == 0.0 and h[4] == h[1] for h in nb)
    u = k["unbiased_empty_graph"]
    nb, _ = xref.search_logp(lp, 3, k["beam"], _graph([]), k["blank"])
    assert [list(h[0]) for h in nb] == u["nbest"] and [list(h[6]) for h in nb] == u["tags"]
    for h, like in zip(nb, u["ctc_likelihood"]):
        assert math.exp(h[4]) == pytest.approx(like, rel=1e-6)       # the fixture's probabilities are float32
    # and on a longer random input
    x = cref.peaky_logits(0, 40, 20, 0)
    plain, pst = sref.search(x, 40, 16)
    nb, st = xref.search(x, 40, 16, _graph([]))
    assert [h[:4] for h in nb] == plain and st.starts == st.ends == st.saved == st.taken_back == 0


def test_finalize_does_not_change_the_stream(kat):
    k, lp = kat
    s = xref.ContextStream(k["beam"], _graph(k["phrases"], 3.0))
    s.consume(lp[:2])
    a = s.nbest()
    assert s.nbest(finalize=True) != a and s.nbest() == a
    s.consume(lp[2:])
    assert s.nbest(finalize=True) == xref.search_logp(lp, 3, k["beam"], _graph(k["phrases"], 3.0))[0]


def test_outputs_with_nested_and_abandoned_matches():
    """UpdateOutputs: nested phrases [1,2] / [1,2,3] commit at 2 and end again at 3; [4] starts and ends on one token;
    a match abandoned after its first token keeps the start tag (as in the reference) and never gets an end tag."""
    import wenet_celoss_amd as w
    g = _graph([[1, 2], [1, 2, 3], [4], [5, 6]], 1.0)
    S, E = 100, 101

    def walk(tokens):
        state, tags, score = 0, [], 0.0
        for t in tokens:
            state, sc, a, b = g.next(state, t)
            score += sc
            tags.append(int(a) | int(b) << 1)
        return (tuple(tokens), 0.0, 0.0, (), 0.0, score, tuple(tags))

    result = [walk([1, 2, 3, 7]), walk([1, 2, 7]), walk([4, 4]), walk([5, 7, 5, 6]), walk([1, 1, 2])]
    assert [h[6] for h in result] == [(1, 2, 2, 0), (1, 2, 0), (3, 3), (1, 0, 1, 2), (1, 0, 0)]
    assert [h[5] for h in result] == [3.0, 2.0, 2.0, 2.0, 0.0]                # [5,7]: +1 -1; [1,1,2]: +1 -1, 1 not retried
    want = [[S, 1, 2, E, 3, E, 7], [S, 1, 2, E, 7], [S, 4, E, S, 4, E], [S, 5, 7, S, 5, 6, E], [S, 1, 1, 2]]
    assert xref.outputs(result, S, E) == want
    assert w.CtcContextPrefixBeamStream.outputs(result, S, E) == want

