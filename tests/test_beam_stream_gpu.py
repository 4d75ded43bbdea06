"""Streaming transducer prefix beam search on the device (wr_prefix_beam_search_chunk, DeviceDecoder.prefix_beam_chunk,
TransducerPrefixBeamStream, the Transducer methods): against the whole-utterance searches bit for bit, under chunking bit
for bit, and against the float64 rule of tests/beam_stream_ref.py over copies of the same modules.

The cases come from tests/test_beam_stream_ref.py (those of tests/test_tdt_beam_ref.py: E = P = 16, J = 32, five ragged
utterances of at most 40 frames), which has shown on the CPU that at least four of the five utterances of every case have
an extended reference margin above 1e-4.  Against the reference an utterance is compared where its margin exceeds 1e-4:
hypotheses, order, n_hyps and times equal, scores and Viterbi scores at rtol 1e-5 (the tolerance tests/test_tdt_beam_gpu.py
uses for scores of the same arithmetic)."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_beam_stream_ref as sref
import test_tdt_beam_ref as cases
from test_beam_stream_ref import SHORT_FINAL, STREAM_SPEC, STREAM_SPECS, cut
from test_tdt_beam_ref import DUR1_SPECS, LENS, MARGIN, MIN_QUALIFY, SPEC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TMAX = max(LENS)
EVEN_16, EVEN_7, MIXED, ONES = (16, 16, 8), (7, 7, 7, 7, 7, 5), (5, 16, 3, 16), (1,) * 40


def decoder(pred, joint, beam, B=len(LENS), T=TMAX, max_frames=TMAX, max_hyp=0):
    from wenet_celoss_amd.decoder import DeviceDecoder
    dec = DeviceDecoder(copy.deepcopy(pred).to(DEV), copy.deepcopy(joint).to(DEV), B * beam, B, T, max_hyp, beam)
    dec.attach_beam_stream(B, beam, max_frames)
    return dec


def feed(dec, c, pos, width, lens, durations, reset, final, rows=slice(None), with_ctc=True):
    """frames pos .. pos + width of the utterances `rows` of case c, as one chunk"""
    take = [max(0, min(width, n - pos)) for n in lens]
    ctc = c.ctc_logp[rows, pos:pos + width].to(DEV) if (with_ctc and c.ctc_logp is not None) else None
    weights = c.weights if ctc is not None else (0.0, 1.0)
    return dec.prefix_beam_chunk(c.enc[rows, pos:pos + width].to(DEV), torch.tensor(take, dtype=torch.int32), c.spec.beam,
                                 c.spec.blank, ctc_logp=ctc, ctc_weight=weights[0], transducer_weight=weights[1],
                                 durations=durations, reset=reset, final=final)


def final_chunk(widths, n):
    """the chunk that holds the last of an utterance's n frames"""
    return next(i for i in range(len(widths)) if sum(widths[:i + 1]) >= n)


def settled(widths, n, durations):
    """Whether chunking an utterance of n frames this way, final with the chunk that holds its last frame, provably changes
    nothing: the plain search always; a token-and-duration search if that chunk holds max(durations) frames of it, or is its
    first -- then no arc made before the end was known reaches beyond it."""
    i = final_chunk(widths, n)
    return durations is None or i == 0 or n - sum(widths[:i]) >= max(durations)


def stream(dec, c, widths, durations="spec", rows=slice(None), every=None, final="own"):
    """The utterances `rows` of case c through dec in chunks of `widths`, reset with the first; final "own": every stream
    with the chunk that holds its last frame, after which it gets no frames and no flag; "last": all with the last chunk
    (a call of no frames for the utterances that ended earlier) -> the n-best after the last chunk; `every`: a list that
    receives the n-best after every chunk."""
    durations = c.spec.durations if durations == "spec" else durations
    lens, pos, out = c.lens[rows], 0, None
    for i, w in enumerate(widths):
        fin = i == len(widths) - 1 if final == "last" else [final_chunk(widths, n) == i for n in lens]
        out = feed(dec, c, pos, w, lens, durations, i == 0, fin, rows)
        pos += w
        if every is not None:
            every.append(out)
    return out


@functools.lru_cache(maxsize=None)
def one_chunk(spec):
    """(the handle, the n-best of one reset-and-final call over the whole utterances), computed once and shared"""
    c = cases.make_case(spec)
    dec = decoder(c.pred, c.joint, spec.beam)
    return dec, stream(dec, c, (TMAX,))


def check(got, want, what=""):
    """Device n-best against the float64 beams: every utterance whose margin is clear, and enough of them."""
    print(what, "margins", [r.margin for r in want])
    for b, (g, r) in enumerate(zip(got, want)):
        print(" utt", b, "device", [(h, round(s, 5), round(v, 5), tm) for h, s, v, tm in g][:2], "reference",
              [(list(h), round(s, 5), round(v, 5), list(tm)) for h, _, s, v, tm in r.beam][:2])
    qualify = 0
    for b, (g, r) in enumerate(zip(got, want)):
        if r.margin <= MARGIN:
            continue
        qualify += 1
        assert [h for h, _, _, _ in g] == [list(h) for h, _, _, _, _ in r.beam], (what, b, r.margin)
        assert [tm for _, _, _, tm in g] == [list(tm) for _, _, _, _, tm in r.beam], (what, b, r.margin)
        np.testing.assert_allclose([s for _, s, _, _ in g], [s for _, _, s, _, _ in r.beam], rtol=1e-5, err_msg=f"{what} utt {b}")
        np.testing.assert_allclose([v for _, _, v, _ in g], [v for _, _, _, v, _ in r.beam], rtol=1e-5, err_msg=f"{what} utt {b}")
    assert qualify >= MIN_QUALIFY, (what, [r.margin for r in want])


# ------------------------------------------------------------------- equality with the whole-utterance searches --
@pytest.mark.parametrize("spec", STREAM_SPECS, ids=[s.name for s in STREAM_SPECS])
def test_one_reset_and_final_call_equals_the_whole_utterance_search(spec):
    c = cases.make_case(spec)
    dec, got = one_chunk(spec)
    ctc = c.ctc_logp.to(DEV) if c.ctc_logp is not None else None
    want = dec.prefix_beam_tdt(c.enc.to(DEV), torch.tensor(c.lens, dtype=torch.int32), spec.durations, spec.beam, spec.blank,
                               ctc_logp=ctc, ctc_weight=c.weights[0], transducer_weight=c.weights[1])
    assert [[(h, s) for h, s, _, _ in u] for u in got] == want           # hypotheses, order, n_hyps, scores: exactly
    for u in got:
        for h, s, v, tm in u:
            assert h[0] == spec.blank and len(tm) == len(h) - 1 and tm == sorted(tm) and v <= s
    assert any(tm for u in got for _, _, _, tm in u)
    # the handle's lanes were taken by the whole-utterance search: the streams have to start again
    with pytest.raises(RuntimeError, match="has overwritten the streams"):
        feed(dec, c, 0, 8, c.lens, spec.durations, False, False)


@pytest.mark.parametrize("spec", [s for s in DUR1_SPECS if s.name in STREAM_SPEC], ids=lambda s: s.name)
def test_the_plain_form_equals_the_plain_prefix_beam_search(spec):
    """durations None on the joiner cut to its V token columns, as test_durations_1_equals_the_plain_prefix_beam_search cuts
    it: one call equals wr_prefix_beam_search exactly, and every chunking equals that call in all outputs."""
    import wenet_celoss_amd as w
    c = cases.make_case(spec)
    plain_joint = w.TransducerJoint(c.V, cases.E, cases.P, cases.J).eval()
    plain_joint.load_state_dict({k: (v[:c.V] if k.startswith("ffn_out.") else v) for k, v in c.joint.state_dict().items()})
    dec = decoder(c.pred, plain_joint, spec.beam)
    got = stream(dec, c, (TMAX,), durations=None)
    want = dec.prefix_beam(c.enc.to(DEV), torch.tensor(c.lens, dtype=torch.int32), c.ctc_logp.to(DEV), spec.beam, *c.weights,
                           spec.blank)
    assert [[(h, s) for h, s, _, _ in u] for u in got] == want
    for widths in (EVEN_16, EVEN_7, MIXED) + ((ONES,) if spec.name == "dur1-ctc" else ()):
        assert stream(dec, c, widths, durations=None) == got, widths
    check(got, sref.reference(spec), spec.name + " plain")


# --------------------------------------------------------------------------------- chunking invariance on the device --
@pytest.mark.parametrize("spec", STREAM_SPECS, ids=[s.name for s in STREAM_SPECS])
def test_every_chunking_equals_the_one_chunk_call(spec):
    """Widths 16 (the 16-step replay boundary), 7 and (5, 16, 3, 16); every stream is final with the chunk that holds its
    last frame, and the shorter utterances get chunks of no frames after that.  A stream is compared wherever its final chunk
    holds max(durations) of its frames (or is its first): all six outputs, exactly."""
    c = cases.make_case(spec)
    dec, whole = one_chunk(spec)
    ways = [w for w in (EVEN_16, EVEN_7, MIXED) if w[-1] >= max(spec.durations)]
    assert len(ways) >= 2
    for widths in ways:
        every = []
        got = stream(dec, c, widths, every=every)
        compared = [b for b, n in enumerate(c.lens) if settled(widths, n, spec.durations)]
        assert len(compared) >= 3 and 0 in compared, (widths, compared)
        for b in compared:
            assert got[b] == whole[b], (widths, b)
        assert all(1 <= len(u) <= spec.beam for u in got)
        # the n-best after a chunk that is not the last: n frames in, nothing emitted beyond them
        done = widths[0]
        for u, n in zip(every[0], c.lens):
            assert 1 <= len(u) <= spec.beam and all(t < min(done, n) for _, _, _, tm in u for t in tm)


# --------------------------------------------------------------------------------------- against the float64 rule --
@pytest.mark.parametrize("spec", STREAM_SPECS, ids=[s.name for s in STREAM_SPECS])
def test_scores_viterbi_scores_and_times_are_those_of_the_float64_rule(spec):
    want = sref.reference(spec)
    assert sref.stream_conditions(want) == []
    check(one_chunk(spec)[1], want, spec.name)


def test_a_short_final_chunk_and_a_zero_frame_final_call_follow_the_rule():
    """durations (0, 8) with a final chunk of 3 frames: arcs made before the end was known stand beyond it until the final
    call clamps, fuses and re-sorts; the utterances that ended earlier get a final call of no frames."""
    spec = STREAM_SPEC["beam3-08-ctc-blank2"]
    c, want = cases.make_case(spec), sref.reference(spec, SHORT_FINAL)
    assert sref.stream_conditions(want) == []
    assert [cut(SHORT_FINAL, n)[-1] for n in c.lens] == [3, 0, 0, 0, 0]
    dec = decoder(c.pred, c.joint, spec.beam)
    check(stream(dec, c, SHORT_FINAL, final="last"), want, "short final chunk")


def test_beam_1_times_are_the_frames_of_the_greedy_search():
    spec = SPEC["beam1"]
    c = cases.make_case(spec)
    dec = decoder(c.pred, c.joint, 1, max_hyp=TMAX)
    got = stream(dec, c, EVEN_16)
    toks, frames = dec.greedy_tdt(c.enc.to(DEV), torch.tensor(c.lens, dtype=torch.int32), spec.durations, n_steps=4,
                                  blank=spec.blank, return_frames=True)
    print("beam", got, "greedy", toks, frames)
    assert [u[0][0][1:] for u in got] == toks and [u[0][3] for u in got] == frames
    assert any(toks)
    assert all(u[0][1] == u[0][2] for u in got)            # one hypothesis, nothing fused: the Viterbi score is the score


# ---------------------------------------------------------------------------------------------- per-stream reset --
def test_resetting_one_stream_leaves_the_others_alone():
    """Stream 2 is reset alone after the first chunk and takes 24 frames of another utterance; it gives what a fresh handle
    gives for them, the other streams what their uninterrupted run gives."""
    spec = STREAM_SPEC["beam8-ctc"]
    c = cases.make_case(spec)
    dec = one_chunk(spec)[0]
    whole = stream(dec, c, EVEN_16, final="last")           # the uninterrupted run with the same chunks and flags
    new_len = 24
    widths = EVEN_16
    out, pos = None, 0
    for i, w in enumerate(widths):
        enc = c.enc[:, pos:pos + w].clone()
        ctc = c.ctc_logp[:, pos:pos + w].clone()
        take = [max(0, min(w, n - pos)) for n in c.lens]
        if i >= 1:                                          # stream 2: utterance 0's frames from the start
            npos = pos - widths[0]
            enc[2, :min(w, TMAX - npos)] = c.enc[0, npos:npos + w]
            ctc[2, :min(w, TMAX - npos)] = c.ctc_logp[0, npos:npos + w]
            take[2] = max(0, min(w, new_len - npos))
        out = dec.prefix_beam_chunk(enc.to(DEV), torch.tensor(take, dtype=torch.int32), spec.beam, spec.blank,
                                    ctc_logp=ctc.to(DEV), ctc_weight=c.weights[0], transducer_weight=c.weights[1],
                                    durations=spec.durations, reset=[i == 0, i == 0, i <= 1, i == 0, i == 0],
                                    final=i == len(widths) - 1)
        pos += w
    for b in (0, 1, 3, 4):
        assert out[b] == whole[b], b
    # a fresh handle with the new utterance in stream 2 (the same lanes) and nothing in the other streams
    fresh = decoder(c.pred, c.joint, spec.beam)
    lone = None
    for i, (p, w) in enumerate([(0, 16), (16, 8)]):
        enc, ctc = torch.zeros(len(LENS), w, cases.E), torch.zeros(len(LENS), w, c.V)
        enc[2], ctc[2] = c.enc[0, p:p + w], c.ctc_logp[0, p:p + w]
        lone = fresh.prefix_beam_chunk(enc.to(DEV), torch.tensor([0, 0, w, 0, 0], dtype=torch.int32), spec.beam, spec.blank,
                                       ctc_logp=ctc.to(DEV), ctc_weight=c.weights[0], transducer_weight=c.weights[1],
                                       durations=spec.durations, reset=i == 0, final=i == 1)
    print("stream 2", out[2][:2], "fresh", lone[2][:2])
    assert out[2] == lone[2] and out[2] != whole[2]
    assert max(t for _, _, _, tm in out[2] for t in tm) < new_len
    assert all(u == [([spec.blank], 0.0, 0.0, [])] for b, u in enumerate(lone) if b != 2)      # a stream that got no frame


# ------------------------------------------------------------------------------------ invariances, invalidation --
def test_graphs_on_and_off_give_identical_outputs():
    for name, durations in (("beam8-ctc", "spec"), ("dur1-ctc", "spec")):
        c = cases.make_case(STREAM_SPEC[name])
        dec = decoder(c.pred, c.joint, c.spec.beam)
        dec.set_graph(True)
        on = stream(dec, c, MIXED, durations)
        dec.set_graph(False)
        off = stream(dec, c, MIXED, durations)
        dec.set_graph(True)
        assert on == off == stream(dec, c, MIXED, durations), name
    # and the plain kernels, whose frames are replayed from a graph only on request
    import wenet_celoss_amd as w
    plain_joint = w.TransducerJoint(c.V, cases.E, cases.P, cases.J).eval()
    plain_joint.load_state_dict({k: (v[:c.V] if k.startswith("ffn_out.") else v) for k, v in c.joint.state_dict().items()})
    dec = decoder(c.pred, plain_joint, c.spec.beam)
    off = stream(dec, c, MIXED, None)
    dec.set_graph(True)
    assert stream(dec, c, MIXED, None) == off


def test_a_batch_equals_single_streams():
    spec = STREAM_SPEC["beam8-ctc"]
    c, want = cases.make_case(spec), sref.reference(spec)
    batch = one_chunk(spec)[1]
    dec = decoder(c.pred, c.joint, spec.beam, B=1)
    for b, r in enumerate(want):
        single = stream(dec, c, (TMAX,), rows=slice(b, b + 1))[0]
        if r.margin > MARGIN:
            assert [(h, tm) for h, _, _, tm in single] == [(h, tm) for h, _, _, tm in batch[b]], b
            np.testing.assert_allclose([s for _, s, _, _ in single], [s for _, s, _, _ in batch[b]], rtol=1e-6)
            np.testing.assert_allclose([v for _, _, v, _ in single], [v for _, _, v, _ in batch[b]], rtol=1e-6)


def test_another_search_between_two_chunks_ends_the_streams():
    spec = STREAM_SPEC["embedding"]
    c = cases.make_case(spec)
    dec = decoder(c.pred, c.joint, spec.beam)
    feed(dec, c, 0, 16, c.lens, spec.durations, True, False)
    dec.prefix_beam_tdt(c.enc.to(DEV), torch.tensor(c.lens, dtype=torch.int32), spec.durations, spec.beam, spec.blank)
    with pytest.raises(RuntimeError, match=r"stream 0 continues, but another search or wr_predictor_step on the handle has "
                                           r"overwritten the streams"):
        feed(dec, c, 16, 16, c.lens, spec.durations, False, False)
    # a partial reset is not enough, a reset of every stream is
    with pytest.raises(RuntimeError, match="stream 1 continues"):
        feed(dec, c, 0, 16, c.lens, spec.durations, [True, False, True, True, True], False)
    assert stream(dec, c, EVEN_16) == stream(decoder(c.pred, c.joint, spec.beam), c, EVEN_16)


# ---------------------------------------------------------------- refusals that need a handle, before any HIP call --
def test_the_handle_checks_refuse_with_a_message_naming_the_cause():
    from wenet_celoss_amd import _lib
    from wenet_celoss_amd.decoder import DeviceDecoder
    lib = _lib.load()
    spec = SPEC["beam3"]
    c = cases.make_case(spec)
    B, T, beam, cap = 2, 8, 3, 20
    dec = DeviceDecoder(copy.deepcopy(c.pred).to(DEV), copy.deepcopy(c.joint).to(DEV), B * 4, B, T, 0, 4)
    enc = torch.zeros(B, T, cases.E, device=DEV)
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    hyps = torch.empty(B, beam, cap + 1, dtype=torch.int32, device=DEV)
    tm = torch.empty_like(hyps)
    hl = torch.empty(B, beam, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, beam, dtype=torch.float64, device=DEV)
    vs = torch.empty_like(sc)
    nh = torch.empty(B, dtype=torch.int32, device=DEV)

    def call(B_=B, T_=T, beam_=beam, cw=0.0, tw=1.0, blank=0, d=(0, 1, 2, 3, 4), flags=(1, 1)):
        arr = (ctypes.c_int32 * len(d))(*d) if d else None
        fl = (ctypes.c_int32 * len(flags))(*flags) if flags is not None else None
        rc = lib.wr_prefix_beam_search_chunk(dec._h, enc.data_ptr(), lens.data_ptr(), None, B_, T_, beam_, cw, tw, blank, arr,
                                             len(d), fl, hyps.data_ptr(), tm.data_ptr(), hl.data_ptr(), sc.data_ptr(),
                                             vs.data_ptr(), nh.data_ptr(), None)
        return rc, lib.wr_last_error()

    def refused(text, **kw):
        rc, err = call(**kw)
        assert rc == -1 and err.startswith(b"prefix_beam_search_chunk: ") and text in err, (kw, rc, err)

    refused(b"no stream state is attached")
    assert lib.wr_decoder_attach_beam_stream(dec._h, B, 5, cap, None, 0) == -1 and b"beam=5" in lib.wr_last_error()
    assert lib.wr_decoder_attach_beam_stream(dec._h, B + 1, beam, cap, None, 0) == -1 and b"max_streams=3" in lib.wr_last_error()
    assert lib.wr_decoder_attach_beam_stream(dec._h, B, beam, 0, None, 0) == -1 and b"max_frames=0" in lib.wr_last_error()
    assert lib.wr_decoder_attach_beam_stream(dec._h, B, beam, cap, None, 0) == -1 and b"null workspace" in lib.wr_last_error()
    need = lib.wr_decoder_beam_stream_workspace_bytes(dec._h, B, beam, cap)
    assert need >= 2 * 2 * B * beam * (cap + 1) * 4 and lib.wr_decoder_beam_stream_workspace_bytes(dec._h, B, 17, cap) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    assert lib.wr_decoder_attach_beam_stream(dec._h, B, beam, cap, ws.data_ptr(), need - 1) == -3
    assert lib.wr_decoder_attach_beam_stream(dec._h, B, beam, cap, ws.data_ptr(), need) == 0
    refused(b"B=1, beam=3 differ from the attached 2 streams of beam 3", B_=1)
    refused(b"B=2, beam=2 differ from the attached 2 streams of beam 3", beam_=2)
    refused(b"T=9 exceeds", T_=T + 1)
    refused(b"blank 300 out of range [0,300)", blank=c.V)
    refused(b"no CTC posterior", cw=0.3, tw=0.7)
    refused(b"may not be null", d=())                       # the plain search needs the posterior
    refused(b"flags[1]=4 has bits beyond", flags=(1, 4))
    refused(b"stream 0 continues without ever having been reset", flags=None)
    refused(b"stream 1 continues without ever having been reset", flags=(1, 0))
    assert call()[0] == 0                                   # both reset: 8 of 20 frames
    assert call(flags=None)[0] == 0                         # 16
    refused(b"stream 0: 16 frames since its reset + a chunk of 8 exceed max_frames=20", flags=None)
    refused(b"durations or blank changed in the middle of a stream", flags=(1, 0), d=(0, 1, 2, 3, 5), T_=4)
    refused(b"durations or blank changed in the middle of a stream", flags=(1, 0), blank=1, T_=4)
    assert call(flags=(3, 0), T_=4)[0] == 0                 # stream 0 reset and final; stream 1 at 20
    refused(b"stream 0 is fed after its final call", flags=(2, 0), T_=1)
    refused(b"stream 1: 20 frames since its reset + a chunk of 1 exceed", flags=(0, 0), T_=1)
    assert call(flags=(0, 1), T_=1)[0] == 0                 # a finished stream without a flag is left as it is
    # any other search or wr_predictor_step on the handle ends the streams
    assert lib.wr_prefix_beam_search_tdt(dec._h, enc.data_ptr(), lens.data_ptr(), None, B, T, beam, 0.0, 1.0, 0,
                                         (ctypes.c_int32 * 5)(0, 1, 2, 3, 4), 5, hyps.data_ptr(), hl.data_ptr(), sc.data_ptr(),
                                         nh.data_ptr(), None) == 0
    refused(b"has overwritten the streams", flags=(0, 0), T_=1)
    assert call(d=(0, 1, 2, 3, 5))[0] == 0                        # and a reset of every stream may change the durations


# ------------------------------------------------------------------------------------- the Transducer methods --
from test_tdt_beam_gpu import TinyAttnDecoder, TinyEncoder  # noqa: E402  (the stand-in encoder of the TDT beam tests)


@functools.lru_cache(maxsize=None)
def model(tdt):
    import wenet_celoss_amd as w
    V, E, P, J, H = 23, 12, 10, 16, 14
    torch.manual_seed(21)
    extra = dict(tdt_durations=(0, 1, 2), tdt_sigma=0.05) if tdt else {}
    m = w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, H, 2, dropout=0.0),
                     w.TransducerJoint(V + (3 if tdt else 0), E, P, J), ctc=w.CTC(V, E), ctc_weight=0.3, transducer_weight=0.7,
                     hw_weight=0.0, **extra)
    m.decoder = TinyAttnDecoder(V, E)
    with torch.no_grad():
        m.joint.ffn_out.weight *= 5
        m.joint.ffn_out.bias[0] += 1.5
        m.ctc.ctc_lo.weight *= 5
        m.ctc.ctc_lo.bias[0] += 1.0
    return m.to(DEV).eval()


@pytest.mark.parametrize("tdt", [False, True], ids=["plain", "tdt"])
def test_transducer_methods_agree(tdt):
    m = model(tdt)
    lens = [26, 15, 20]
    speech = torch.randn(3, 26, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    slen = torch.tensor(lens, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        whole = m.beam_search_times(speech, slen, beam_size=4)
        enc, mask = m.encoder(speech, slen)
        m.reset_beam_stream(3, beam_size=4, max_frames=32, chunk_frames=8)
        out = None
        for p in range(0, 26, 8):
            w = min(8, 26 - p)
            take = torch.tensor([max(0, min(w, n - p)) for n in lens], dtype=torch.int32)
            out = m.forward_prefix_beam_search(enc[:, p:p + w], take, final=[p < n <= p + w for n in lens])
        best = (m.tdt_beam_search if tdt else m.beam_search)(speech[:1], slen[:1], beam_size=4)
        alone = m.beam_search_times(speech[:1], slen[:1], beam_size=4)
    print("n-best", whole, "best", best)
    assert [[(h[1:], s, v, tm) for h, s, v, tm in u] for u in out] == whole
    assert len(whole) == 3 and all(1 <= len(u) <= 4 for u in whole) and any(tm for u in whole for _, _, _, tm in u)
    assert (alone[0][0][0], alone[0][0][1]) == best
    with pytest.raises(RuntimeError, match="is fed after its final chunk"):
        m.forward_prefix_beam_search(enc[:, :8], torch.tensor([8, 8, 8]), final=False)
    # a whole-utterance search on the model's handle between two chunks ends the streams
    m.reset_beam_stream(3, beam_size=4, max_frames=32, chunk_frames=8)
    m.forward_prefix_beam_search(enc[:, :8], torch.tensor([8, 8, 8]))
    if tdt:
        m.tdt_beam_search(speech[:1], slen[:1], beam_size=4)
    else:                                                  # (beam_search keeps a handle of its own)
        m.greedy_search_batch(speech, slen)
    with pytest.raises(RuntimeError, match="overwritten the streams|rebuilt"):
        m.forward_prefix_beam_search(enc[:, 8:16], torch.tensor([8, 8, 8]))
