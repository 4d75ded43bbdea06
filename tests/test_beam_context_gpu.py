"""Context-graph biasing in the streaming transducer prefix beam search on the device (wr_prefix_beam_search_context_chunk,
DeviceDecoder.prefix_beam_context_chunk, TransducerContextPrefixBeamStream, the Transducer methods): against the unbiased
chunk call bit for bit for an empty and an all-zero graph, under chunking bit for bit, and against the float64 rule of
tests/beam_context_ref.py over copies of the same modules.

The cases come from tests/test_beam_context_ref.py (those of tests/test_tdt_beam_ref.py: E = P = 16, J = 32, five ragged
utterances of at most 40 frames), which has shown on the CPU what the bonus does in each and that at least four of the five
utterances have an extended reference margin above 1e-4.  Two configurations: a plain joiner cut to its V token columns
(the plain search needs the CTC posterior, so this one always mixes it in) and a token-and-duration joiner with durations
0..4, with and without the CTC mixture.  Against the reference an utterance is compared where its margin exceeds 1e-4:
tokens, order, n_hyps, times, tags and graph states equal, the bonus equal, trans_score and vscore at rtol 1e-5 (the bar of
tests/test_beam_stream_gpu.py for the same arithmetic), score == trans_score + context_score exactly."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import beam_context_ref as ref
import test_beam_context_ref as cref
import test_tdt_beam_ref as cases
from test_beam_context_ref import BONUS, CTX_SPEC, CTX_SPECS
from test_beam_stream_gpu import DEV, EVEN_7, EVEN_16, MIXED, ONES, TMAX, final_chunk, settled
from test_tdt_beam_ref import LENS, MARGIN, MIN_QUALIFY, SPEC
from wenet_celoss_amd.context_graph import ContextGraph

pytestmark = pytest.mark.gpu

IDS = [s.name for s in CTX_SPECS]


def device_durations(spec):
    """None for the plain configuration: the durations-(1,) case runs as a plain model on the joiner cut to V columns."""
    return None if spec.durations == (1,) else spec.durations


@functools.lru_cache(maxsize=None)
def joiner(spec):
    c = cases.make_case(spec)
    if device_durations(spec) is not None:
        return c.joint
    import wenet_celoss_amd as w
    plain = w.TransducerJoint(c.V, cases.E, cases.P, cases.J).eval()
    plain.load_state_dict({k: (v[:c.V] if k.startswith("ffn_out.") else v) for k, v in c.joint.state_dict().items()})
    return plain


def decoder(spec, B=len(LENS), T=TMAX, max_frames=TMAX, biased=True):
    from wenet_celoss_amd.decoder import DeviceDecoder
    c = cases.make_case(spec)
    dec = DeviceDecoder(copy.deepcopy(c.pred).to(DEV), copy.deepcopy(joiner(spec)).to(DEV), B * spec.beam, B, T, 0, spec.beam)
    (dec.attach_beam_context_stream if biased else dec.attach_beam_stream)(B, spec.beam, max_frames)
    return dec


def feed(dec, spec, graph, pos, width, lens, reset, final, finalize=False, rows=slice(None)):
    """frames pos .. pos + width of the utterances `rows` of the case, as one chunk; graph None: the unbiased chunk call"""
    c = cases.make_case(spec)
    take = [max(0, min(width, n - pos)) for n in lens]
    ctc = c.ctc_logp[rows, pos:pos + width].to(DEV) if c.ctc_logp is not None else None
    kw = dict(ctc_logp=ctc, ctc_weight=c.weights[0], transducer_weight=c.weights[1], durations=device_durations(spec),
              reset=reset, final=final)
    enc, ln = c.enc[rows, pos:pos + width].to(DEV), torch.tensor(take, dtype=torch.int32)
    if graph is None:
        return dec.prefix_beam_chunk(enc, ln, spec.beam, spec.blank, **kw)
    return dec.prefix_beam_context_chunk(enc, ln, spec.beam, spec.blank, graph, finalize=finalize, **kw)


def stream(dec, spec, graph, widths, rows=slice(None), every=None, final="own", finalize="final"):
    """The utterances `rows` through dec in chunks of `widths`, reset with the first; final "own": every stream with the
    chunk that holds its last frame, "last": all with the last chunk; finalize "final": bit 2 goes with the final flag and
    with every later call (bit 2 is about a call's export alone, and a finished stream is left as it is), "never" /
    "always": with no / every chunk -> the n-best after the last chunk; `every` receives every chunk's."""
    lens, pos, out = cases.make_case(spec).lens[rows], 0, None
    for i, w in enumerate(widths):
        fin = [i == len(widths) - 1] * len(lens) if final == "last" else [final_chunk(widths, n) == i for n in lens]
        done = fin if final == "last" else [final_chunk(widths, n) <= i for n in lens]
        fz = done if finalize == "final" else [finalize == "always"] * len(lens)
        out = feed(dec, spec, graph, pos, w, lens, i == 0, fin, fz, rows)
        pos += w
        if every is not None:
            every.append(out)
    return out


@functools.lru_cache(maxsize=None)
def one_chunk(spec, finalize="final"):
    """(the handle, the n-best of one reset-and-final call over the whole utterances), computed once and shared"""
    dec = decoder(spec)
    return dec, stream(dec, spec, cref.graph_for(spec), (TMAX,), finalize=finalize)


def host_finalise(rows, graph):
    """bit 2 on the host, from a stream's export that is not finalised: the same float64 adds, a stable sort"""
    out = []
    for h, s, v, tm, ts, cx, tg, st in rows:
        cx2 = cx + float(graph.escape[st]) if st != 0 else cx
        out.append((h, ts + cx2, v, tm, ts, cx2, tg, st))
    return sorted(out, key=lambda r: -r[1])


def check(got, want, what=""):
    """Device n-best against the float64 exports: every utterance whose margin is clear, and enough of them."""
    print(what, "margins", [float(r.margin) for r in want])
    qualify = 0
    for b, (g, r) in enumerate(zip(got, want)):
        rows = r.exports[-1]
        print(" utt", b, "device", [(x[0], round(x[1], 5), x[5], x[6], x[7]) for x in g][:2], "reference",
              [(list(x[0]), round(x[1], 5), x[5], list(x[6]), x[7]) for x in rows][:2])
        for h, s, v, tm, ts, cx, tg, st in g:
            assert s == ts + cx and len(tg) == len(tm) == len(h) - 1, (what, b)
        if r.margin <= MARGIN:
            continue
        qualify += 1
        assert [x[0] for x in g] == [list(x[0]) for x in rows], (what, b, r.margin)
        assert [x[3] for x in g] == [list(x[3]) for x in rows], (what, b, r.margin)
        assert [x[6] for x in g] == [list(x[6]) for x in rows], (what, b, r.margin)
        assert [x[7] for x in g] == [x[7] for x in rows], (what, b, r.margin)
        assert [x[5] for x in g] == [x[5] for x in rows], (what, b, r.margin)
        np.testing.assert_allclose([x[4] for x in g], [x[4] for x in rows], rtol=1e-5, err_msg=f"{what} utt {b}")
        np.testing.assert_allclose([x[2] for x in g], [x[2] for x in rows], rtol=1e-5, err_msg=f"{what} utt {b}")
    assert qualify >= MIN_QUALIFY, (what, [r.margin for r in want])


# ------------------------------------------------------------------------------------------- graph equivalences --
@pytest.mark.parametrize("spec", CTX_SPECS, ids=IDS)
def test_the_empty_and_the_all_zero_graph_equal_the_unbiased_chunk_call_bit_for_bit(spec):
    dec = decoder(spec)
    empty = ContextGraph([], BONUS, blank=spec.blank)
    zero = ContextGraph(cref.graph_for(spec).phrases, 0.0, blank=spec.blank)
    got = {}
    for name, g in (("empty", empty), ("zero", zero)):
        every = []
        stream(dec, spec, g, MIXED, every=every, final="last")
        got[name] = every
    dec.attach_beam_stream(len(LENS), spec.beam, TMAX)       # the same handle, the unbiased form
    plain = []
    stream(dec, spec, None, MIXED, every=plain, final="last")
    for name, every in got.items():
        for chunk, want in zip(every, plain):
            assert [[x[:4] for x in u] for u in chunk] == want, name    # hyps, scores, vscores, times, n_hyps: exactly
            for u in chunk:
                for h, s, v, tm, ts, cx, tg, st in u:
                    assert ts == s and cx == 0.0 and len(tg) == len(h) - 1
    assert all(t == 0 and x[7] == 0 for chunk in got["empty"] for u in chunk for x in u for t in x[6])
    assert any(t != 0 for u in got["zero"][-1] for x in u for t in x[6])
    assert any(len(x[0]) > 1 for u in plain[-1] for x in u)


# --------------------------------------------------------------------------------------- against the float64 rule --
@pytest.mark.parametrize("spec", CTX_SPECS, ids=IDS)
def test_the_biased_search_is_the_float64_rule(spec):
    want = cref.reference(spec)
    assert cref.context_conditions(spec, want) == []
    check(one_chunk(spec)[1], want, spec.name + " finalised")
    check(one_chunk(spec, "never")[1], cref.reference(spec, None, False), spec.name + " not finalised")
    assert one_chunk(spec)[1] != one_chunk(spec, "never")[1]


# --------------------------------------------------------------------------------- chunking invariance on the device --
@pytest.mark.parametrize("spec", CTX_SPECS, ids=IDS)
def test_every_chunking_equals_the_one_chunk_call_with_and_without_bit_2(spec):
    c = cases.make_case(spec)
    dur = device_durations(spec)
    ways = [w for w in (EVEN_16, EVEN_7, MIXED, ONES) if dur is None or w[-1] >= max(dur)]
    assert len(ways) >= (4 if dur is None else 2)
    for finalize in ("final", "never"):
        dec, whole = one_chunk(spec, finalize)
        for widths in ways:
            got = stream(dec, spec, cref.graph_for(spec), widths, finalize=finalize)
            compared = [b for b, n in enumerate(c.lens) if settled(widths, n, dur)]
            assert len(compared) >= 3 and 0 in compared, (widths, compared)
            for b in compared:
                assert got[b] == whole[b], (finalize, widths, b)


@pytest.mark.parametrize("spec", CTX_SPECS, ids=IDS)
def test_bit_2_in_the_middle_of_a_stream_changes_nothing_later_and_is_the_host_side_finalisation(spec):
    g = cref.graph_for(spec)
    dec = one_chunk(spec)[0]
    live, done = [], []
    stream(dec, spec, g, EVEN_16, every=live, final="last", finalize="never")
    stream(dec, spec, g, EVEN_16, every=done, final="last", finalize="always")
    changed = 0
    for a, b in zip(live, done):
        for ua, ub in zip(a, b):
            assert ub == host_finalise(ua, g)
            changed += ua != ub
    assert changed > 0                                       # a partial match did give its bonus back somewhere


def test_bit_2_alone_in_a_call_of_no_frames_exports_finalised_and_leaves_the_stream_as_it_was():
    spec = CTX_SPEC["beam8-ctc"]
    g = cref.graph_for(spec)
    c = cases.make_case(spec)
    dec = decoder(spec, max_frames=TMAX + 24)                # a call of no frames still counts its width on the host
    want = stream(dec, spec, g, EVEN_16, final="last")
    out = None
    for i, (p, w) in enumerate([(0, 16), (16, 16), (32, 8)]):
        out = feed(dec, spec, g, p, w, c.lens, i == 0, i == 2, i == 2)
        if i == 1:
            live = feed(dec, spec, g, 32, 8, [0] * len(LENS), False, False, False)     # nothing at all: untouched
            assert live == out
            alone = feed(dec, spec, g, 32, 8, [0] * len(LENS), False, False, True)     # bit 2 only
            assert alone == [host_finalise(u, g) for u in live] and alone != live
            assert feed(dec, spec, g, 32, 8, [0] * len(LENS), False, False, False) == live
    assert out == want


# ------------------------------------------------------------------------------------------- per-stream behaviour --
def test_a_per_stream_reset_and_a_per_stream_bit_2():
    spec = CTX_SPEC["beam8-ctc"]
    g = cref.graph_for(spec)
    c = cases.make_case(spec)
    dec = one_chunk(spec)[0]
    yes = stream(dec, spec, g, EVEN_16, final="last", finalize="final")
    no = stream(dec, spec, g, EVEN_16, final="last", finalize="never")
    # bit 2 for streams 0 and 2 only, in the last call
    out, pos = None, 0
    for i, w in enumerate(EVEN_16):
        out = feed(dec, spec, g, pos, w, c.lens, i == 0, i == 2, [i == 2, False, i == 2, False, False])
        pos += w
    assert [out[b] == (yes if b in (0, 2) else no)[b] for b in range(len(LENS))] == [True] * len(LENS)
    assert yes[0] != no[0] or yes[2] != no[2]
    # stream 2 is reset alone with the second chunk and takes utterance 0's first 24 frames; the others run on
    new_len, pos, out = 24, 0, None
    for i, w in enumerate(EVEN_16):
        enc, ctc = c.enc[:, pos:pos + w].clone(), c.ctc_logp[:, pos:pos + w].clone()
        take = [max(0, min(w, n - pos)) for n in c.lens]
        if i >= 1:
            npos = pos - EVEN_16[0]
            enc[2, :min(w, TMAX - npos)] = c.enc[0, npos:npos + w]
            ctc[2, :min(w, TMAX - npos)] = c.ctc_logp[0, npos:npos + w]
            take[2] = max(0, min(w, new_len - npos))
        out = dec.prefix_beam_context_chunk(enc.to(DEV), torch.tensor(take, dtype=torch.int32), spec.beam, spec.blank, g,
                                            ctc_logp=ctc.to(DEV), ctc_weight=c.weights[0], transducer_weight=c.weights[1],
                                            durations=spec.durations, reset=[i == 0, i == 0, i <= 1, i == 0, i == 0],
                                            final=i == 2, finalize=i == 2)
        pos += w
    for b in (0, 1, 3, 4):
        assert out[b] == yes[b], b
    fresh = decoder(spec)
    lone = None
    for i, (p, w) in enumerate([(0, 16), (16, 8)]):
        enc, ctc = torch.zeros(len(LENS), w, cases.E), torch.zeros(len(LENS), w, c.V)
        enc[2], ctc[2] = c.enc[0, p:p + w], c.ctc_logp[0, p:p + w]
        lone = fresh.prefix_beam_context_chunk(enc.to(DEV), torch.tensor([0, 0, w, 0, 0], dtype=torch.int32), spec.beam,
                                               spec.blank, g, ctc_logp=ctc.to(DEV), ctc_weight=c.weights[0],
                                               transducer_weight=c.weights[1], durations=spec.durations, reset=i == 0,
                                               final=i == 1, finalize=i == 1)
    assert out[2] == lone[2] and out[2] != yes[2]
    assert all(u == [([spec.blank], 0.0, 0.0, [], 0.0, 0.0, [], 0)] for b, u in enumerate(lone) if b != 2)


# ------------------------------------------------------------------------------------------------- other modes --
def test_graphs_on_and_off_give_identical_outputs():
    for name in ("beam8-ctc", "dur1-ctc"):
        spec = CTX_SPEC[name]
        g = cref.graph_for(spec)
        dec = decoder(spec)
        dec.set_graph(True)
        on = stream(dec, spec, g, MIXED)
        dec.set_graph(False)
        off = stream(dec, spec, g, MIXED)
        dec.set_graph(True)
        assert on == off == stream(dec, spec, g, MIXED), name
        assert any(x[5] != 0.0 for u in on for x in u)


def test_a_batch_equals_single_streams():
    spec = CTX_SPEC["beam8-ctc"]
    g, want = cref.graph_for(spec), cref.reference(spec)
    batch = one_chunk(spec)[1]
    dec = decoder(spec, B=1)
    for b, r in enumerate(want):
        single = stream(dec, spec, g, (TMAX,), rows=slice(b, b + 1))[0]
        if r.margin > MARGIN:
            assert [(x[0], x[3], x[5], x[6], x[7]) for x in single] == [(x[0], x[3], x[5], x[6], x[7]) for x in batch[b]], b
            np.testing.assert_allclose([x[4] for x in single], [x[4] for x in batch[b]], rtol=1e-6)
            np.testing.assert_allclose([x[2] for x in single], [x[2] for x in batch[b]], rtol=1e-6)


@functools.lru_cache(maxsize=None)
def small_graph(spec, kind):
    """`one`: a one-token phrase, `twice`: the phrase [t, t] -- t the most frequent token of the unbiased reference's lists"""
    import collections
    import test_beam_stream_ref as sref
    count = collections.Counter(t for r in sref.reference(spec) for e in r.beam for t in e[0][1:])
    t = count.most_common(1)[0][0]
    return ContextGraph([[t]] if kind == "one" else [[t, t]], BONUS, blank=spec.blank)


@pytest.mark.parametrize("kind", ["one", "twice"])
def test_a_one_token_phrase_and_a_repeated_token_phrase(kind):
    spec = CTX_SPEC["beam3"]
    g = small_graph(spec, kind)
    c = cases.make_case(spec)
    want = ref.decode(c.pred, c.joint, c.enc, c.lens, c.V, spec.durations, spec.beam, g, spec.blank, None, *c.weights)
    got = stream(decoder(spec), spec, g, (TMAX,))
    check(got, want, f"beam3 {kind}")
    assert any(t for u in got for x in u for t in x[6])


def test_beam_1():
    spec = SPEC["beam1"]
    c = cases.make_case(spec)
    g = small_graph(spec, "one")
    want = ref.decode(c.pred, c.joint, c.enc, c.lens, c.V, spec.durations, 1, g, spec.blank, None, *c.weights)
    got = stream(decoder(spec), spec, g, (TMAX,))
    check(got, want, "beam1")
    assert all(len(u) == 1 and u[0][1] == u[0][2] + u[0][5] for u in got)       # one hypothesis: the Viterbi score is the score


def test_a_stream_may_be_filled_to_max_frames_and_no_further():
    spec = CTX_SPEC["beam3"]
    g = cref.graph_for(spec)
    c = cases.make_case(spec)
    dec = decoder(spec, max_frames=TMAX)
    want = one_chunk(spec)[1]
    assert stream(dec, spec, g, EVEN_16)[0] == want[0]       # 40 of 40 frames; Lcap = 41 slots per hypothesis
    feed(dec, spec, g, 0, 16, c.lens, True, False)
    feed(dec, spec, g, 16, 16, c.lens, False, False)
    with pytest.raises(RuntimeError, match=r"32 frames since its reset \+ a chunk of 16 exceed max_frames=40"):
        feed(dec, spec, g, 24, 16, c.lens, False, False)
    assert feed(dec, spec, g, 32, 8, c.lens, False, True, True)[0] == want[0]


# ------------------------------------------------------------------------------------------------ invalidation --
def test_a_plain_chunk_call_or_another_search_in_between_ends_the_biased_streams():
    spec = CTX_SPEC["beam3"]
    g = cref.graph_for(spec)
    c = cases.make_case(spec)
    dec = decoder(spec)
    feed(dec, spec, g, 0, 16, c.lens, True, False)
    dec.prefix_beam_tdt(c.enc.to(DEV), torch.tensor(c.lens, dtype=torch.int32), spec.durations, spec.beam, spec.blank)
    with pytest.raises(RuntimeError, match=r"prefix_beam_search_context_chunk: stream 0 continues, but another search or "
                                           r"wr_predictor_step on the handle has overwritten the streams"):
        feed(dec, spec, g, 16, 16, c.lens, False, False)
    want = stream(dec, spec, g, EVEN_16)
    # a plain chunk call needs the plain block, and attaching it ends the biased streams
    feed(dec, spec, g, 0, 16, c.lens, True, False)
    with pytest.raises(RuntimeError, match="attach_beam_stream"):
        feed(dec, spec, None, 16, 16, c.lens, False, False)
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    B, beam, cap = len(LENS), spec.beam, TMAX + 1
    i32, f64 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float64, device=DEV)
    bufs = [torch.empty(B, beam, cap, **i32), torch.empty(B, beam, cap, **i32), torch.empty(B, beam, **i32),
            torch.empty(B, beam, **f64), torch.empty(B, beam, **f64), torch.empty(B, **i32)]
    enc, ln = c.enc[:, :16].contiguous().to(DEV), torch.full((B,), 16, **i32)
    rc = lib.wr_prefix_beam_search_chunk(dec._h, enc.data_ptr(), ln.data_ptr(), None, B, 16, beam, 0.0, 1.0, spec.blank,
                                         (ctypes.c_int32 * 5)(*spec.durations), 5, None, *[t.data_ptr() for t in bufs], None)
    assert rc == -1 and b"no stream state is attached (wr_decoder_attach_beam_stream comes first)" in lib.wr_last_error()
    dec.attach_beam_stream(B, beam, TMAX)
    feed(dec, spec, None, 0, 16, c.lens, True, False)
    with pytest.raises(RuntimeError, match="attach_beam_context_stream"):
        feed(dec, spec, g, 16, 16, c.lens, False, False)
    dec.attach_beam_context_stream(B, beam, TMAX)
    with pytest.raises(RuntimeError, match="stream 0 continues without ever having been reset"):
        feed(dec, spec, g, 16, 16, c.lens, False, False)
    assert stream(dec, spec, g, EVEN_16) == want


# ---------------------------------------------------------------- refusals that need a handle, before any HIP call --
def test_the_handle_checks_refuse_in_the_stated_order_with_a_message_naming_the_cause():
    from wenet_celoss_amd import _lib
    from wenet_celoss_amd.decoder import DeviceDecoder
    lib = _lib.load()
    spec = SPEC["beam3"]
    c = cases.make_case(spec)
    B, T, beam, cap = 2, 8, 3, 20
    dec = DeviceDecoder(copy.deepcopy(c.pred).to(DEV), copy.deepcopy(c.joint).to(DEV), B * 4, B, T, 0, 4)
    i32, f64 = dict(dtype=torch.int32, device=DEV), dict(dtype=torch.float64, device=DEV)
    enc = torch.zeros(B, T, cases.E, device=DEV)
    lens = torch.full((B,), T, **i32)
    hyps, tm, tg = (torch.empty(B, beam, cap + 1, **i32) for _ in range(3))
    hl, cs, nh = torch.empty(B, beam, **i32), torch.empty(B, beam, **i32), torch.empty(B, **i32)
    sc, vs, ts, cx = (torch.empty(B, beam, **f64) for _ in range(4))
    g = ContextGraph([[1, 2], [3]], BONUS)
    table = [t.data_ptr() for t in g.to(DEV)]

    def call(B_=B, T_=T, beam_=beam, cw=0.0, tw=1.0, blank=0, d=(0, 1, 2, 3, 4), flags=(1, 1), S=g.n_states, A=g.n_arcs,
             tab=table):
        arr = (ctypes.c_int32 * len(d))(*d) if d else None
        fl = (ctypes.c_int32 * len(flags))(*flags) if flags is not None else None
        rc = lib.wr_prefix_beam_search_context_chunk(dec._h, enc.data_ptr(), lens.data_ptr(), None, B_, T_, beam_, cw, tw, blank,
                                                     arr, len(d), fl, hyps.data_ptr(), tm.data_ptr(), hl.data_ptr(),
                                                     sc.data_ptr(), vs.data_ptr(), nh.data_ptr(), *tab, S, A, ts.data_ptr(),
                                                     cx.data_ptr(), tg.data_ptr(), cs.data_ptr(), None)
        return rc, lib.wr_last_error()

    def refused(text, code=-1, **kw):
        rc, err = call(**kw)
        assert rc == code and err.startswith(b"prefix_beam_search_context_chunk: ") and text in err, (kw, rc, err)

    refused(b"no stream state is attached (wr_decoder_attach_beam_context_stream comes first)")
    plain_need = lib.wr_decoder_beam_stream_workspace_bytes(dec._h, B, beam, cap)
    pws = torch.empty(plain_need, dtype=torch.uint8, device=DEV)
    assert lib.wr_decoder_attach_beam_stream(dec._h, B, beam, cap, pws.data_ptr(), plain_need) == 0
    refused(b"no stream state is attached")                  # the plain form's block is not the biased form's
    att = lib.wr_decoder_attach_beam_context_stream
    assert att(dec._h, B, 5, cap, None, 0) == -1 and b"decoder_attach_beam_context_stream: beam=5" in lib.wr_last_error()
    assert att(dec._h, B + 1, beam, cap, None, 0) == -1 and b"max_streams=3" in lib.wr_last_error()
    assert att(dec._h, B, beam, 0, None, 0) == -1 and b"max_frames=0" in lib.wr_last_error()
    assert att(dec._h, B, beam, cap, None, 0) == -1 and b"null workspace" in lib.wr_last_error()
    need = lib.wr_decoder_beam_context_stream_workspace_bytes(dec._h, B, beam, cap)
    assert need >= plain_need + 2 * B * beam * (cap + 1) * 4 + B * beam * 12
    assert lib.wr_decoder_beam_context_stream_workspace_bytes(dec._h, B, 17, cap) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert att(dec._h, B, beam, cap, ws.data_ptr(), need - 1) == -3
    assert att(dec._h, B, beam, cap, ws.data_ptr(), need) == 0
    # everything the plain chunk call refuses, in its order, before the table is looked at (S = 0 rides along)
    refused(b"B=1, beam=3 differ from the attached 2 streams of beam 3", B_=1, S=0)
    refused(b"T=9 exceeds", T_=T + 1, S=0)
    refused(b"no CTC posterior", cw=0.3, tw=0.7, S=0)
    refused(b"may not be null", d=(), S=0)
    refused(b"blank 300 out of range [0,300)", blank=c.V, S=0)
    refused(b"flags[1]=8 has bits beyond reset (1), final (2) and finalised export (4)", flags=(1, 8), S=0)
    refused(b"stream 1 continues without ever having been reset", flags=(1, 4), S=0)
    # then the table: sizes, null pointers, limits
    refused(b"S=0 states and A=3 arcs (S >= 1, A >= 0)", S=0)
    refused(b"S=2 states and A=-1 arcs", A=-1, tab=[None] * 6)
    for k in range(6):
        refused(b"null context-graph table pointer", tab=table[:k] + [None] + table[k + 1:], S=70000)
    refused(b"exceeds 65536 states / 1048576 arcs", code=-2, S=65537)
    refused(b"exceeds 65536 states / 1048576 arcs", code=-2, A=1048577)
    assert call(flags=(5, 1))[0] == 0                        # both reset, stream 0 exported finalised: 8 of 20 frames
    assert call(flags=(4, 0))[0] == 0                        # 16
    refused(b"stream 0: 16 frames since its reset + a chunk of 8 exceed max_frames=20", flags=(4, 4))
    refused(b"durations or blank changed in the middle of a stream", flags=(1, 0), d=(0, 1, 2, 3, 5), T_=4)
    assert call(flags=(7, 0), T_=4)[0] == 0                  # stream 0 reset, final and finalised; stream 1 at 20
    refused(b"stream 0 is fed after its final call", flags=(2, 0), T_=1)
    assert call(flags=(4, 1), T_=1)[0] == 0                  # bit 2 for a finished stream: exported finalised, left as it is
    # the unbiased call keeps refusing bit 2, and cannot continue a biased stream
    rc = lib.wr_prefix_beam_search_chunk(dec._h, enc.data_ptr(), lens.data_ptr(), None, B, T, beam, 0.0, 1.0, 0,
                                         (ctypes.c_int32 * 5)(0, 1, 2, 3, 4), 5, (ctypes.c_int32 * 2)(1, 1), hyps.data_ptr(),
                                         tm.data_ptr(), hl.data_ptr(), sc.data_ptr(), vs.data_ptr(), nh.data_ptr(), None)
    assert rc == -1 and b"prefix_beam_search_chunk: no stream state is attached" in lib.wr_last_error()
    assert lib.wr_decoder_attach_beam_stream(dec._h, B, beam, cap, pws.data_ptr(), plain_need) == 0
    rc = lib.wr_prefix_beam_search_chunk(dec._h, enc.data_ptr(), lens.data_ptr(), None, B, T, beam, 0.0, 1.0, 0,
                                         (ctypes.c_int32 * 5)(0, 1, 2, 3, 4), 5, (ctypes.c_int32 * 2)(1, 4), hyps.data_ptr(),
                                         tm.data_ptr(), hl.data_ptr(), sc.data_ptr(), vs.data_ptr(), nh.data_ptr(), None)
    assert rc == -1 and b"flags[1]=4 has bits beyond reset (1) and final (2)" in lib.wr_last_error()


# ------------------------------------------------------------------------------------- the Transducer methods --
from test_beam_stream_gpu import model  # noqa: E402  (the small plain / token-and-duration models of the stream tests)


@pytest.mark.parametrize("tdt", [False, True], ids=["plain", "tdt"])
def test_transducer_methods_agree(tdt):
    import wenet_celoss_amd as w
    m = model(tdt)
    lens = [26, 15, 20]
    speech = torch.randn(3, 26, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    slen = torch.tensor(lens, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        plain = m.beam_search_times(speech, slen, beam_size=4)
        phrases = [p for u in plain for h in u[1:3] if h[0] for p in ref.phrases_from(h[0])]
        assert phrases
        g = w.ContextGraph(phrases, BONUS, blank=m.blank)
        whole = m.beam_search_context(speech, slen, 4, g)
        assert [[x[:4] for x in u] for u in m.beam_search_context(speech, slen, 4, w.ContextGraph([], BONUS, blank=m.blank))] == plain
        enc, mask = m.encoder(speech, slen)
        m.reset_beam_context_stream(3, 4, 32, 8, g)
        out = None
        for p in range(0, 26, 8):
            wd = min(8, 26 - p)
            take = torch.tensor([max(0, min(wd, n - p)) for n in lens], dtype=torch.int32)
            out = m.forward_context_prefix_beam_search(enc[:, p:p + wd], take, final=[p < n <= p + wd for n in lens])
    print("biased", whole, "plain", plain)
    assert [[(x[0][1:],) + x[1:] for x in u] for u in out] == whole
    assert any(x[5] != 0.0 for u in whole for x in u) and all(x[1] == x[4] + x[5] for u in whole for x in u)
    tagged = w.TransducerContextPrefixBeamStream.outputs(out[0], 100, 101)
    assert [[t for t in o if t < 100] for o in tagged] == [x[0][1:] for x in out[0]]
    with pytest.raises(RuntimeError, match="is fed after its final chunk"):
        m.forward_context_prefix_beam_search(enc[:, :8], torch.tensor([8, 8, 8]), final=False)
    # an unbiased stream on the model's handle between two chunks ends the biased streams
    m.reset_beam_context_stream(3, 4, 32, 8, g)
    m.forward_context_prefix_beam_search(enc[:, :8], torch.tensor([8, 8, 8]))
    m.reset_beam_stream(3, beam_size=4, max_frames=32, chunk_frames=8)
    m.forward_prefix_beam_search(enc[:, :8], torch.tensor([8, 8, 8]))
    with pytest.raises(RuntimeError, match="ever having been reset|overwritten the streams|rebuilt"):
        m.forward_context_prefix_beam_search(enc[:, 8:16], torch.tensor([8, 8, 8]))
