"""The biased CTC prefix beam search on the GPU (include/wr_api.h, "Context-graph biasing in the CTC prefix beam search").

Bars, those of tests/test_ctc_stream_gpu.py: tokens, times, tags and context states exact; context_score == the
reference's (a sum of float32 values taken in float64, in position order); ctc_score and Viterbi score at rel = 1e-5;
score == ctc_score + context_score exactly.  Every test first asserts on the float64 reference of
tests/ctc_context_ref.py that the smallest decision gap -- the comparisons of totals in every frame's prune and in the
finalising sort included -- is at least MIN_GAP = 1e-3 with no exact tie (the device's fp32 log-softmax differs from
float64 by at most ~1e-5 per frame, 4e-4 over the 40 frames used here); the seeds were picked on the CPU so that it
holds.  Equalities between two device runs are bit for bit: tuples of ints and Python floats compared with ==."""
import json
import math
import os

import numpy as np
import pytest
import torch

import ctc_context_ref as xref
import ctc_decode_ref as cref
import ctc_stream_ref as sref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_GAP = 1e-3
PAD = 7.0           # value of the frames of a chunk past a stream's lens: never consumed


def _graph(*a, **k):
    from wenet_celoss_amd import ContextGraph
    return ContextGraph(*a, **k)


def _reference(x, T, beam, graph, blank=0, finalize=True):
    nb, st = xref.search(x, T, beam, graph, blank, finalize=finalize)
    print(f"reference: T={T} V={x.shape[1]} beam={beam} blank={blank} finalize={finalize}: {st}")
    assert st.min_gap >= MIN_GAP and st.ties == 0, st
    sref.check_times([h[:4] for h in nb], T)
    xref.check_tags(nb)
    return nb, st


def _same(got, want, states=None, want_states=None):
    assert [(h[0], h[3], h[6]) for h in got] == [(h[0], h[3], h[6]) for h in want]
    for g, r in zip(got, want):
        print(f"ctc {g[4]!r} reference {r[4]!r}; context {g[5]!r} reference {r[5]!r}; viterbi {g[2]!r} reference {r[2]!r}")
        assert g[5] == r[5]
        assert g[4] == pytest.approx(r[4], rel=1e-5) and g[2] == pytest.approx(r[2], rel=1e-5)
        assert g[1] == g[4] + g[5]
    if want_states is not None:
        assert list(states) == list(want_states)


def _feed(stream, xs, plan, finalize=()):
    """tests/test_ctc_stream_gpu.py's _feed for the biased stream; `finalize` holds the indices of the plan's chunks that
    are fed with finalize=True."""
    pos = [0] * len(xs)
    out = None
    for i, lens in enumerate(plan):
        width = max(max(lens), 1)
        chunk = np.full((len(xs), width, xs[0].shape[1]), PAD, np.float32)
        for b, n in enumerate(lens):
            chunk[b, :n] = xs[b][pos[b]:pos[b] + n]
            pos[b] += n
        out = stream.search(torch.tensor(chunk, device=DEV), torch.tensor(lens), finalize=i in finalize)
        assert stream.frames == pos
    return out


def _whole(x, T, beam, graph, blank=0, finalize=True):
    import wenet_celoss_amd as w
    s = w.CtcContextPrefixBeamStream(1, beam, T, graph, blank=blank)
    out = s.search(torch.tensor(x[None, :T], device=DEV), torch.tensor([T]), finalize=finalize)[0]
    return out, s.context_states[0]


def _chunked(x, widths, beam, graph, blank=0, finalize=True, also=()):
    import wenet_celoss_amd as w
    s = w.CtcContextPrefixBeamStream(1, beam, sum(max(n, 1) for n in widths), graph, blank=blank)
    fin = set(also) | ({len(widths) - 1} if finalize else set())
    return _feed(s, [x], [(n,) for n in widths], finalize=fin)[0]


# ---- 1. known answers ----
@pytest.mark.parametrize("widths", [[3], [1, 2], [2, 1], [1, 1, 1]])
def test_known_answers(widths):
    """tests/golden/ctc_context_kat.json (derived in tests/test_ctc_context_ref.py::test_known_answers): every row at
    every chunking."""
    with open(os.path.join(GOLDEN, "ctc_context_kat.json")) as f:
        k = json.load(f)
    x = np.log(np.load(os.path.join(GOLDEN, k["probs_file"]))["probs"]).astype(np.float32)
    for row in k["rows"]:
        g = _graph(k["phrases"], row["context_score"], k["blank"])
        want, st = _reference(x, 3, k["beam"], g, finalize=row["finalize"])
        nb = _chunked(x, widths, k["beam"], g, finalize=row["finalize"])
        _same(nb, want)
        assert [list(h[0]) for h in nb] == row["nbest"] and [list(h[6]) for h in nb] == row["tags"]
        assert [h[5] for h in nb] == row["context"]
        for h, like in zip(nb, row["ctc_likelihood"]):
            assert math.exp(h[4]) == pytest.approx(like, rel=1e-5)


# ---- 2. a graph that never acts moves nothing ----
ABSENT = (7, 11)        # pushed to the bottom of every frame: never among the top 16 of 20


@pytest.fixture(scope="module")
def idle_case():
    x = cref.peaky_logits(IDLE_SEED, 40, 20, 0)
    x[:, ABSENT] -= 30.0
    return x


IDLE_SEED = 81


@pytest.mark.parametrize("phrases", [[], [[7, 11], [11, 3], [7]]], ids=["empty", "never_occurring"])
def test_idle_graph_is_bit_identical_to_the_plain_stream(idle_case, phrases):
    import wenet_celoss_amd as w
    x, beam, T = idle_case, 16, 40
    assert all(set(np.argsort(-row, kind="stable")[:beam].tolist()).isdisjoint(ABSENT) for row in x)
    g = _graph(phrases, 3.0)
    want, st = _reference(x, T, beam, g)
    assert st.starts == st.ends == st.saved == st.taken_back == 0
    xt, ln = torch.tensor(x[None], device=DEV), torch.tensor([T])
    plain = w.CtcPrefixBeamStream(1, beam, T).search(xt, ln)[0]
    for fin in (False, True):
        got, states = _whole(x, T, beam, g, finalize=fin)
        assert [h[:4] for h in got] == plain                      # hyps / scores / Viterbi / times, bit for bit
        assert all(h[4] == h[1] and h[5] == 0.0 and set(h[6]) <= {0} for h in got) and set(states) == {0}
    _same(got, want)


# ---- 3. range ----
RANGE = [(1, 30, 17, 10, 3.0), (2, 31, 18, 0, 3.0), (9, 33, 19, 4, 3.0), (16, 40, 20, 365, 3.0)]


def _range_case(beam, T, V, seed, score):
    x = cref.peaky_logits(seed, T, V, 0)
    unb, _ = sref.search(x, T, max(beam, 2), 0)
    g = _graph(xref.phrases_from(unb[1][0]), score)
    return x, g


def test_range_inputs_exercise_the_biasing():
    """On the reference alone, before the device is touched: over the cases of RANGE the biased 1-best differs from the
    unbiased one, end boundaries are set, finalisation takes a bonus back, and (beam > 1) an entry survives a prune only
    because of its bonus."""
    diff = ends = back = 0
    for beam, T, V, seed, score in RANGE:
        x, g = _range_case(beam, T, V, seed, score)
        want, st = _reference(x, T, beam, g)
        unb, _ = sref.search(x, T, beam, 0)
        diff += want[0][0] != unb[0][0]
        ends += st.ends
        back += st.taken_back
        assert st.max_ncur == beam
        if beam > 1:
            assert st.saved > 0
    assert diff >= 1 and ends >= 1 and back >= 1


@pytest.mark.parametrize("beam,T,V,seed,score", RANGE)
def test_range_whole_against_reference(beam, T, V, seed, score):
    x, g = _range_case(beam, T, V, seed, score)
    assert len(g.phrases) >= 3 and g.final[1:].sum() >= 1          # 2- and 3-token pieces and the nested pair
    want, st = _reference(x, T, beam, g)
    assert st.max_ncur == beam and st.ends >= 1
    if beam > 1:
        assert st.saved >= 1                                       # an entry survived a prune only because of its bonus
    got, states = _whole(x, T, beam, g)
    _same(got, want, states, st.states)
    want_nf, st_nf = _reference(x, T, beam, g, finalize=False)
    got_nf, states_nf = _whole(x, T, beam, g, finalize=False)
    _same(got_nf, want_nf, states_nf, st_nf.states)


# ---- 4. chunk invariance ----
@pytest.fixture(scope="module")
def case16():
    beam, T, V, seed, score = RANGE[-1]
    x, g = _range_case(beam, T, V, seed, score)
    out = {}
    for fin in (False, True):
        want, _ = _reference(x, T, beam, g, finalize=fin)
        out[fin], _ = _whole(x, T, beam, g, finalize=fin)
        _same(out[fin], want)
    assert [h[0] for h in out[True]] != [h[0] for h in out[False]]            # finalising reorders this list
    return x, g, out


@pytest.mark.parametrize("fin", [False, True], ids=["plain", "finalize"])
@pytest.mark.parametrize("widths", [[1] * 40, [7, 16, 16, 1], [16, 0, 24]], ids=["40x1", "7+16+16+1", "16+0+24"])
def test_chunking_is_bit_identical(case16, widths, fin):
    x, g, whole = case16
    assert _chunked(x, widths, 16, g, finalize=fin) == whole[fin]


def test_finalize_in_the_middle_changes_nothing_afterwards(case16):
    import wenet_celoss_amd as w
    x, g, whole = case16
    assert _chunked(x, [7, 16, 16, 1], 16, g, finalize=True, also=(0, 1)) == whole[True]
    assert _chunked(x, [7, 16, 16, 1], 16, g, finalize=False, also=(1, 2)) == whole[False]
    # finalize(): a zero-length chunk with the flag, also at full capacity, and the stream goes on after it
    s = w.CtcContextPrefixBeamStream(1, 16, 40, g)
    _feed(s, [x], [(24,)])
    mid = s.finalize()[0]
    _same(mid, _reference(x, 24, 16, g)[0])
    assert s.frames == [24]
    assert s.search(torch.tensor(x[None, 24:], device=DEV), torch.tensor([16]))[0] == whole[False]
    assert s.finalize()[0] == whole[True] and s.frames == [40]


# ---- 5. stream independence ----
def test_three_streams_ragged_equal_each_alone():
    import wenet_celoss_amd as w
    beam, V = STREAMS_BEAM, 20
    xs = [cref.peaky_logits(sd, n, V, 0) for sd, n in STREAMS]
    unb, _ = sref.search(xs[0], len(xs[0]), beam, 0)
    g = _graph(xref.phrases_from(unb[1][0]), 2.0)
    plan = [(8, 8, 0), (8, 7, 1), (8, 0, 0), (8, 8, 0), (8, 0, 0)]
    assert [sum(p[b] for p in plan) for b in range(3)] == [len(x) for x in xs] == [40, 23, 1]
    wants = [_reference(x, len(x), beam, g) for x in xs]
    assert wants[0][1].ends >= 1 and wants[0][1].saved >= 1
    s = w.CtcContextPrefixBeamStream(3, beam, 40, g)
    got = _feed(s, xs, plan, finalize={4})
    for b, x in enumerate(xs):
        _same(got[b], wants[b][0], s.context_states[b], wants[b][1].states)
        assert got[b] == _whole(x, len(x), beam, g)[0], b


STREAMS_BEAM = 4
STREAMS = [(0, 40), (2, 23), (1, 1)]


# ---- 6. edge graphs ----
EDGES = {
    # name: (beam, T, V, seed, blank, phrases -- "one": the best hypothesis's second token; "repeat": a token it doubles;
    #        "cut": phrases_from the second-best hypothesis --, score)
    "one_token": (4, 30, 12, 1, 0, "one", 2.0),
    "repeated_token": (4, 30, 6, 2, 0, "repeat", 2.0),
    "blank5": (4, 30, 12, 0, 5, "cut", 2.0),
    "blank_last": (3, 30, 12, 1, 11, "cut", 2.0),
    "V2_beam1": (1, 12, 2, 0, 0, [[1]], 2.0),
    "V2_beam2": (2, 12, 2, 0, 0, [[1, 1]], 2.0),
    "V2_blank1": (2, 12, 2, 0, 1, [[0], [0, 0]], 2.0),
}


def _edge_case(name):
    beam, T, V, seed, blank, how, score = EDGES[name]
    x = cref.peaky_logits(seed, T, V, blank)
    unb, _ = sref.search(x, T, max(beam, 2), blank)
    best = list(unb[0][0])
    if how == "one":
        phrases = [[best[1]]]
    elif how == "repeat":
        # [t, t]: needs a hypothesis with the token doubled, which only the blank-separated case *s-s -> *ss builds
        t = next(a for a, b in zip(best[:-1], best[1:]) if a == b)
        phrases = [[t, t]]
    elif how == "cut":
        phrases = xref.phrases_from(unb[1][0])
    else:
        phrases = how
    return x, T, beam, blank, _graph(phrases, score, blank)


@pytest.mark.parametrize("name", list(EDGES))
def test_edge_graphs(name):
    x, T, beam, blank, g = _edge_case(name)
    want, st = _reference(x, T, beam, g, blank)
    assert st.starts >= 1 and st.ends >= 1
    if name == "repeated_token":
        t = g.phrases[0][0]
        assert st.pairs > 0 and any(a == b == t and (ga, gb) == (1, 2) for h in want
                                    for a, b, ga, gb in zip(h[0][:-1], h[0][1:], h[6][:-1], h[6][1:]))
    got, states = _whole(x, T, beam, g, blank)
    _same(got, want, states, st.states)
    assert _chunked(x, [5, 1, T - 6], beam, g, blank) == got


# ---- 7. state and capacity ----
def test_state_reuse_after_reset_with_another_graph():
    import wenet_celoss_amd as w
    from wenet_celoss_amd import _lib
    beam, T, V, seed, score = RANGE[2]
    x, g = _range_case(beam, T, V, seed, score)
    want, st = _reference(x, T, beam, g)
    lib = _lib.load()
    assert lib.wr_ctc_context_stream_state_bytes(1, beam, T) > lib.wr_ctc_stream_state_bytes(1, beam, T)
    state = torch.empty(lib.wr_ctc_context_stream_state_bytes(1, beam, T), dtype=torch.uint8, device=DEV)
    other = _graph([[3, 4, 5], [6]], 1.0)
    _feed(w.CtcContextPrefixBeamStream(1, beam, T, other, state=state), [x], [(16,), (T - 16,)])
    reused = _feed(w.CtcContextPrefixBeamStream(1, beam, T, g, state=state), [x], [(16,), (T - 16,)], finalize={1})[0]
    _same(reused, want)
    assert reused == _whole(x, T, beam, g)[0]
    s = w.CtcContextPrefixBeamStream(1, beam, T, g, state=state)
    _feed(s, [x], [(9,)])
    s.reset()
    assert s.frames == [0]
    assert _feed(s, [x], [(T,)], finalize={0})[0] == reused


def test_capacity():
    import wenet_celoss_amd as w
    beam, T, V, seed, score = RANGE[2]
    x, g = _range_case(beam, T, V, seed, score)
    x = x[:8]
    whole, _ = _whole(x, 8, beam, g)
    s = w.CtcContextPrefixBeamStream(1, beam, 8, g)
    _feed(s, [x], [(5,)])
    with pytest.raises(RuntimeError, match=r"5 frames done \+ a chunk of 4 exceeds max_frames=8"):
        s.search(torch.zeros(1, 4, V, device=DEV), torch.tensor([4]))
    assert s.frames == [5]
    out = s.search(torch.tensor(x[None, 5:], device=DEV), torch.tensor([3]), finalize=True)[0]
    assert out == whole and s.frames == [8]                       # the refused call left the stream as it was
    assert s.finalize()[0] == whole                               # at full capacity a zero-length chunk still passes
    from wenet_celoss_amd import _lib
    ws = _lib.workspace("wr_ctc_stream_workspace_bytes", 1, 4, beam, device=DEV)
    with pytest.raises(RuntimeError, match=r"frames_done=5 \+ T=4 exceeds Lcap=8"):
        t = torch.zeros(1, 4, V, device=DEV)
        i = torch.zeros(1, beam, 8, dtype=torch.int32, device=DEV)
        d = torch.zeros(1, beam, dtype=torch.float64, device=DEV)
        _lib.call("wr_ctc_prefix_beam_search_context_chunk", t, i, 1, 4, V, beam, 0, 0, 5, 8, s._state, s._state.numel(),
                  *g.to(DEV), g.n_states, g.n_arcs, 0, i, i, d, d, i, i, i, d, d, i, i, ws, ws.numel(), device=DEV)


# ---- 8. model methods ----
def test_transducer_methods():
    """The three Transducer methods on the tiny encoder of tests/test_ctc_stream_gpu.py: the one-shot call against the
    reference on the device's own logits, the streaming pair over 4-frame chunks against the one-shot call."""
    import wenet_celoss_amd as w
    from test_ctc_stream_gpu import TinyEncoder
    V, E, P, beam = 23, 12, 10, 4
    torch.manual_seed(1)
    m = w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, 14, 2, dropout=0.0), w.TransducerJoint(V, E, P, 16),
                     ctc=w.CTC(V, E), ctc_weight=0.3, transducer_weight=0.7, hw_weight=0.0)
    with torch.no_grad():
        m.ctc.ctc_lo.weight.mul_(12.0)                           # peaky posteriors: decisions well apart
    m = m.to(DEV).eval()
    gen = torch.Generator().manual_seed(5)
    speech = torch.randn(2, 20, 8, generator=gen).to(DEV)
    slen = torch.tensor([20, 13], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        enc, _ = m.encoder(speech, slen)
        logits = m.ctc.ctc_lo(enc).cpu().numpy()
        unb, _ = sref.search(logits[0], 20, beam, 0)
        g = _graph(xref.phrases_from(unb[1][0]), 2.0)
        refs = [_reference(logits[b], int(slen[b]), beam, g) for b in range(2)]
        assert refs[0][1].ends >= 1
        got = m.ctc_context_prefix_beam_search(speech, slen, beam, g)
        for b in range(2):
            _same(got[b], refs[b][0])
        with pytest.raises(RuntimeError, match="reset_ctc_context_stream"):
            m.forward_ctc_context_prefix_beam_search(enc[:, :4], slen.clamp(0, 4))
        m.reset_ctc_context_stream(2, beam, 20, g)
        for t0 in range(0, 20, 4):
            part = m.forward_ctc_context_prefix_beam_search(enc[:, t0:t0 + 4], (slen - t0).clamp(0, 4), finalize=t0 == 16)
        assert m._ctc_context_stream.frames == [20, 13]
        for b in range(2):
            _same(part[b], refs[b][0])
            assert [(h[0], h[3], h[5], h[6]) for h in part[b]] == [(h[0], h[3], h[5], h[6]) for h in got[b]]
