"""Host-side checks of context-graph biasing in the streaming transducer prefix beam search: what
wr_prefix_beam_search_context_chunk and the attach calls refuse before any HIP call (by return code and wr_last_error
text, in the stated order), that the header, the exports and the signatures agree, the size queries, the Python record of
the streams with the errors the wrappers raise on their own, and outputs().  No GPU is needed and none is used.  (The
refusals that need a decoder handle -- the attached form, the flag bits, the streams' record, the table's sizes, pointers and
limits -- are in tests/test_beam_context_gpu.py: a handle cannot be built without a device.)"""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT
from test_beam_stream_host import NULL, PTR, _model, durs

POINTERS = ["enc", "lens", "hyps", "times", "hl", "scores", "vscores", "nh", "trans", "ctx", "tags", "states"]
TABLE = ["arc_begin", "arc_token", "arc_next", "arc_score", "escape", "final"]


@pytest.fixture(scope="module")
def lib():
    from wenet_celoss_amd import _lib
    return _lib.load()


def chunk(lib, h=PTR, ctc=NULL, d=(0, 1, 2), D=None, durations=None, flags=NULL, S=1, A=0, **ptrs):
    p = {name: ptrs.get(name, PTR) for name in POINTERS + TABLE}
    arr = durs(*d) if durations is None else durations
    return lib.wr_prefix_beam_search_context_chunk(h, p["enc"], p["lens"], ctc, 2, 8, 4, 0.0, 1.0, 0, arr, len(d) if D is None else D,
                                                   flags, p["hyps"], p["times"], p["hl"], p["scores"], p["vscores"], p["nh"],
                                                   *[p[n] for n in TABLE], S, A, p["trans"], p["ctx"], p["tags"], p["states"], NULL)


@pytest.mark.parametrize("kw, text", [
    (dict(D=10, d=tuple(range(9))), b"D=10 durations (1 to 9 are supported)"),
    (dict(d=(0, 9)), b"durations[1]=9 lies outside [0, 8]"),
    (dict(d=(0, 2, 1)), b"durations must be strictly increasing (durations[2]=1 after 2)"),
    (dict(d=(0,)), b"at least one duration must be 1 or more (no arc would consume a frame)"),
    (dict(durations=NULL, D=3), b"durations is null"),
] + [(dict({name: NULL}), b"null pointer argument") for name in POINTERS] + [
    (dict(h=NULL), b"null handle"),
    (dict(h=NULL, durations=NULL, D=0), b"null handle"),                          # a plain model: no durations, D = 0
    # the table is looked at last, after everything that needs the handle: without one, a bad table is not what is named
    (dict(h=NULL, S=0), b"null handle"),
    (dict(h=NULL, arc_begin=NULL), b"null handle"),
    (dict(h=NULL, S=1 << 20), b"null handle"),
])
def test_the_entry_point_refuses_before_any_hip_call(lib, kw, text):
    assert chunk(lib, **kw) == -1
    err = lib.wr_last_error()
    assert err.startswith(b"prefix_beam_search_context_chunk: ") and text in err, err


def test_the_checks_run_in_the_documented_order(lib):
    # durations before the pointers -- the four new outputs count with them --, the pointers before the handle; a null
    # posterior and null flags are no refusals
    assert chunk(lib, h=NULL, tags=NULL, d=(2, 1)) == -1 and b"strictly increasing" in lib.wr_last_error()
    for name in ("trans", "ctx", "tags", "states"):
        assert chunk(lib, h=NULL, **{name: NULL}) == -1 and b"null pointer argument" in lib.wr_last_error()
    assert chunk(lib, h=NULL, ctc=NULL, flags=NULL) == -1 and b"null handle" in lib.wr_last_error()


def test_the_size_queries_and_the_attach_call(lib):
    plain, biased = lib.wr_decoder_beam_stream_workspace_bytes, lib.wr_decoder_beam_context_stream_workspace_bytes
    assert biased(NULL, 2, 4, 100) == 0
    assert biased(PTR, 0, 4, 100) == 0 and biased(PTR, 2, 17, 100) == 0 and biased(PTR, 2, 4, 0) == 0
    shapes = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 4, 100), (2, 4, 101), (3, 4, 100), (2, 5, 100), (16, 8, 1500), (16, 16, 4096)]
    for n, beam, frames in shapes:
        p, b = plain(PTR, n, beam, frames), biased(PTR, n, beam, frames)
        nb, cap = n * beam, frames + 1
        # the plain block's contents, then a bonus and a state per entry and the double-buffered tags
        assert p > 0 and p + 2 * nb * cap * 4 + nb * 12 <= b < p + 2 * nb * cap * 4 + nb * 12 + 4 * 256, (n, beam, frames)
    # monotone in every argument
    for (n, beam, frames) in shapes[3:4]:
        base = biased(PTR, n, beam, frames)
        assert biased(PTR, n + 1, beam, frames) > base and biased(PTR, n, beam + 1, frames) > base
        assert biased(PTR, n, beam, frames + 64) > base
        assert biased(PTR, n, beam, frames - 64) < base
    assert lib.wr_decoder_attach_beam_context_stream(NULL, 2, 4, 100, PTR, 1 << 40) == -1
    assert lib.wr_last_error() == b"decoder_attach_beam_context_stream: null handle"
    # the plain query and attach are as they were
    assert 2 * 2 * 2 * 4 * 101 * 4 <= plain(PTR, 2, 4, 100) < 2 * 2 * 2 * 4 * 101 * 4 + 16 * 256
    assert lib.wr_decoder_attach_beam_stream(NULL, 2, 4, 100, PTR, 1 << 40) == -1
    assert lib.wr_last_error() == b"decoder_attach_beam_stream: null handle"


def test_header_exports_and_signatures_agree(lib):
    from wenet_celoss_amd import _lib
    text = open(os.path.join(ROOT, "include", "wr_api.h")).read()
    assert "Context-graph biasing in the streaming transducer prefix beam search" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("wr_decoder_beam_context_stream_workspace_bytes", 4), ("wr_decoder_attach_beam_context_stream", 6),
                         ("wr_prefix_beam_search_context_chunk", 32), ("wr_prefix_beam_search_chunk", 20)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["wr_decoder_beam_context_stream_workspace_bytes"][0] is ctypes.c_size_t
    # S and A are the two ints between the table pointers and the new outputs
    sig = _lib.SIGNATURES["wr_prefix_beam_search_context_chunk"][1]
    assert sig[:19] == _lib.SIGNATURES["wr_prefix_beam_search_chunk"][1][:19]
    assert sig[19:] == [ctypes.c_void_p] * 6 + [ctypes.c_int] * 2 + [ctypes.c_void_p] * 5
    assert lib.wr_api_version() == _lib.API_VERSION == 3 == int(re.search(r"#define\s+WR_API_VERSION\s+(\d+)", text).group(1))
    flat = text.replace("\n * ", " ")
    for phrase in ("the bonus never enters the fp32 cast", "total = fused_score + ctx_score", "flag bits beyond 7 instead of beyond 3",
                   "S > 65536 or A > 1048576", "Bit 2 is independent of bit 1"):
        assert phrase in flat, phrase


def test_python_surface():
    import wenet_celoss_amd as w
    from wenet_celoss_amd.decoder import DeviceDecoder
    from wenet_celoss_amd.search.prefix_beam_search import TransducerContextPrefixBeamStream, TransducerPrefixBeamStream
    assert "TransducerContextPrefixBeamStream" in w.__all__
    assert w.TransducerContextPrefixBeamStream is TransducerContextPrefixBeamStream
    assert issubclass(TransducerContextPrefixBeamStream, TransducerPrefixBeamStream)
    assert list(inspect.signature(DeviceDecoder.attach_beam_context_stream).parameters) == ["self", "n_streams", "beam", "max_frames"]
    sig = inspect.signature(DeviceDecoder.prefix_beam_context_chunk)
    assert list(sig.parameters) == ["self", "encoder_chunk", "chunk_lens", "beam_size", "blank", "graph", "ctc_logp", "ctc_weight",
                                    "transducer_weight", "durations", "reset", "final", "finalize"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[6:]] == [None, 0.0, 1.0, None, False, False, False]
    sig = inspect.signature(TransducerContextPrefixBeamStream.__init__)
    assert list(sig.parameters)[:7] == ["self", "model", "n_streams", "beam_size", "max_frames", "chunk_frames", "context_graph"]
    assert list(inspect.signature(TransducerContextPrefixBeamStream.search).parameters) == [
        "self", "encoder_out_chunk", "lens", "final", "finalize"]
    assert inspect.signature(TransducerContextPrefixBeamStream.search).parameters["finalize"].default is None
    assert list(inspect.signature(TransducerContextPrefixBeamStream.reset).parameters) == ["self", "streams"]
    assert list(inspect.signature(w.Transducer.reset_beam_context_stream).parameters)[:6] == [
        "self", "n_streams", "beam_size", "max_frames", "chunk_frames", "context_graph"]
    assert list(inspect.signature(w.Transducer.forward_context_prefix_beam_search).parameters) == [
        "self", "encoder_out_chunk", "encoder_out_lens", "final", "finalize"]
    assert list(inspect.signature(w.Transducer.beam_search_context).parameters)[:5] == [
        "self", "speech", "speech_lengths", "beam_size", "context_graph"]
    # the unbiased stream's surface is as it was
    assert list(inspect.signature(TransducerPrefixBeamStream.search).parameters) == ["self", "encoder_out_chunk", "lens", "final"]


def test_the_graph_is_checked_against_the_model_at_construction():
    import wenet_celoss_amd as w
    g = w.ContextGraph([[1, 2], [22]], 3.0)
    s = w.TransducerContextPrefixBeamStream(_model(), 2, 4, 32, 8, g)
    assert s.context_graph is g and (s.ctc_weight, s.transducer_weight, s.durations) == (0.3, 0.7, None)
    s = w.TransducerContextPrefixBeamStream(_model(26, tdt_durations=(0, 1, 2)), 2, 4, 32, 8, g)
    assert (s.ctc_weight, s.transducer_weight, s.durations, s._with_ctc) == (0.0, 1.0, (0, 1, 2), False)
    with pytest.raises(ValueError, match="must be a ContextGraph"):
        w.TransducerContextPrefixBeamStream(_model(), 2, 4, 32, 8, None)
    with pytest.raises(ValueError, match="built for blank 5, the model's is 0"):
        w.TransducerContextPrefixBeamStream(_model(), 2, 4, 32, 8, w.ContextGraph([[1]], 3.0, blank=5))
    # the token vocabulary of a token-and-duration model is vocab_size, not the joiner's width
    for m in (_model(), _model(26, tdt_durations=(0, 1, 2))):
        with pytest.raises(ValueError, match=r"phrase token 23 lies outside the token vocabulary \[0, 23\)"):
            w.TransducerContextPrefixBeamStream(m, 2, 4, 32, 8, w.ContextGraph([[1, 23]], 3.0))
    w.TransducerContextPrefixBeamStream(_model(), 2, 4, 32, 8, w.ContextGraph([], 3.0))          # an empty graph is legal
    with pytest.raises(RuntimeError, match="TransducerPrefixBeamStream"):
        w.TransducerContextPrefixBeamStream(_model(), 2, 17, 32, 8, g)


def test_the_python_record_of_the_streams():
    import wenet_celoss_amd as w
    m = _model(26, tdt_durations=(0, 1, 2))
    g = w.ContextGraph([[1, 2]], 3.0)
    lens = torch.tensor([4, 4], dtype=torch.int32)
    s = w.TransducerContextPrefixBeamStream(m, 2, 4, 16, 8, g)
    assert s.frames == [0, 0]
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.search(torch.zeros(2, 4, 12), lens)
    with pytest.raises(RuntimeError, match=r"finalize has 3 entries for 2 streams"):
        s.search(torch.zeros(2, 4, 12), lens, finalize=[True, False, True])
    with pytest.raises(RuntimeError, match=r"chunk has 3 streams, the stream set has 2"):
        s.search(torch.zeros(3, 4, 12), torch.tensor([4, 4, 4]))
    with pytest.raises(RuntimeError, match=r"a chunk of 9 frames exceeds chunk_frames=8"):
        s.search(torch.zeros(2, 9, 12), lens)
    s._phase, s.frames = [1, 2], [12, 8]                     # stream 0 after three chunks of four, stream 1 finished
    with pytest.raises(RuntimeError, match=r"stream 0: 12 frames done \+ a chunk of 5 exceeds max_frames=16"):
        s.search(torch.zeros(2, 5, 12), torch.tensor([5, 0]))
    with pytest.raises(RuntimeError, match=r"stream 1 is fed after its final chunk \(reset it first\)"):
        s.search(torch.zeros(2, 4, 12), lens)
    with pytest.raises(RuntimeError, match="no CPU path"):   # finalising a finished stream is no error
        s.search(torch.zeros(2, 4, 12), torch.tensor([4, 0]), finalize=[False, True])
    with pytest.raises(RuntimeError, match="no CPU path"):   # and by default a finished stream stays finalised
        s.search(torch.zeros(2, 4, 12), torch.tensor([4, 0]))
    assert s._finalize == [False, True]
    with pytest.raises(RuntimeError, match=r"final has 3 entries for 2 streams"):
        s.search(torch.zeros(2, 4, 12), lens, final=[True, False, True])
    s.reset([1])
    assert (s._phase, s.frames) == ([1, 0], [12, 0])
    # finalize defaults to final
    s.reset()
    for final, finalize, want in ((True, None, [True, True]), ([True, False], None, [True, False]), (True, False, [False, False]),
                                  (False, [False, True], [False, True])):
        with pytest.raises(RuntimeError, match="no CPU path"):
            s.search(torch.zeros(2, 4, 12), lens, final=final, finalize=finalize)
        assert s._finalize == want
    # the Transducer methods pass the same errors on
    with pytest.raises(RuntimeError, match="call reset_beam_context_stream"):
        m.forward_context_prefix_beam_search(torch.zeros(2, 4, 12), lens)
    m.reset_beam_context_stream(2, 4, 16, 8, g)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.forward_context_prefix_beam_search(torch.zeros(2, 4, 12), lens)
    with pytest.raises(ValueError, match="must be a ContextGraph"):
        m.reset_beam_context_stream(2, 4, 16, 8, [[1, 2]])


def test_outputs_interleaves_the_tags():
    import wenet_celoss_amd as w
    import beam_context_ref as ref
    # (tokens incl. the seed blank, score, vscore, times, trans_score, context_score, tags, context_state)
    result = [([0, 7, 8, 9], 1.0, 0.5, [0, 2, 5], -2.0, 3.0, [1, 2, 0], 0),
              ([0, 4], 0.0, 0.0, [1], 0.0, 0.0, [3], 0),
              ([0], 0.0, 0.0, [], 0.0, 0.0, [], 0)]
    want = [[100, 7, 8, 101, 9], [100, 4, 101], []]
    assert w.TransducerContextPrefixBeamStream.outputs(result, 100, 101) == want
    assert ref.outputs([(tuple(r[0]),) + tuple(r[1:]) for r in result], 100, 101) == want
