"""Host-side checks of the streaming transducer prefix beam search: what wr_prefix_beam_search_chunk and the attach calls
refuse before any HIP call (by return code and wr_last_error text), that the header, the exports and the signatures agree,
and the errors the Python wrappers raise on their own record of the streams.  No GPU is needed and none is used.  (The
refusals that need a decoder handle -- no attached state, B / beam, a stream continued without a reset or after another
search, fed after its final call, max_frames, a change of durations or blank -- are in tests/test_beam_stream_gpu.py: a
handle cannot be built without a device.  TransducerPrefixBeamStream keeps the same record on the host and is checked here.)"""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

NULL = ctypes.c_void_p(None)
PTR = ctypes.c_void_p(0x1000)        # a non-null placeholder: every call here is refused before anything reads it
POINTERS = ["enc", "lens", "hyps", "times", "hl", "scores", "vscores", "nh"]


@pytest.fixture(scope="module")
def lib():
    from wenet_celoss_amd import _lib
    return _lib.load()


def durs(*d):
    return (ctypes.c_int32 * max(len(d), 1))(*d)


def chunk(lib, h=PTR, ctc=NULL, d=(0, 1, 2), D=None, durations=None, flags=NULL, **ptrs):
    p = {name: ptrs.get(name, PTR) for name in POINTERS}
    arr = durs(*d) if durations is None else durations
    return lib.wr_prefix_beam_search_chunk(h, p["enc"], p["lens"], ctc, 2, 8, 4, 0.0, 1.0, 0, arr, len(d) if D is None else D,
                                           flags, p["hyps"], p["times"], p["hl"], p["scores"], p["vscores"], p["nh"], NULL)


@pytest.mark.parametrize("kw, text", [
    (dict(D=10, d=tuple(range(9))), b"D=10 durations (1 to 9 are supported)"),
    (dict(D=-1), b"D=-1 durations (1 to 9 are supported)"),
    (dict(d=(0, 9)), b"durations[1]=9 lies outside [0, 8]"),
    (dict(d=(0, 2, 1)), b"durations must be strictly increasing (durations[2]=1 after 2)"),
    (dict(d=(0,)), b"at least one duration must be 1 or more (no arc would consume a frame)"),
    (dict(durations=NULL, D=3), b"durations is null"),
    (dict(durations=durs(1), D=0), b"D=0 durations (1 to 9 are supported)"),      # durations without a count
] + [(dict({name: NULL}), b"null pointer argument") for name in POINTERS] + [
    (dict(h=NULL), b"null handle"),
    (dict(h=NULL, durations=NULL, D=0), b"null handle"),                          # a plain model: no durations, D = 0
])
def test_the_entry_point_refuses_before_any_hip_call(lib, kw, text):
    assert chunk(lib, **kw) == -1
    err = lib.wr_last_error()
    assert err.startswith(b"prefix_beam_search_chunk: ") and text in err, err


def test_the_checks_run_in_the_documented_order(lib):
    # durations before the pointers, the pointers before the handle; a null posterior and null flags are no refusals
    assert chunk(lib, h=NULL, hyps=NULL, d=(2, 1)) == -1 and b"strictly increasing" in lib.wr_last_error()
    assert chunk(lib, h=NULL, hyps=NULL) == -1 and b"null pointer argument" in lib.wr_last_error()
    assert chunk(lib, h=NULL, ctc=NULL, flags=NULL) == -1 and b"null handle" in lib.wr_last_error()


def test_the_attach_calls_refuse_a_null_handle(lib):
    assert lib.wr_decoder_beam_stream_workspace_bytes(NULL, 2, 4, 100) == 0
    assert lib.wr_decoder_beam_stream_workspace_bytes(PTR, 0, 4, 100) == 0
    assert lib.wr_decoder_beam_stream_workspace_bytes(PTR, 2, 17, 100) == 0
    assert lib.wr_decoder_beam_stream_workspace_bytes(PTR, 2, 4, 0) == 0
    # hypotheses and times, double-buffered, Lcap = max_frames + 1 slots each (the handle is not read for the size)
    need = lib.wr_decoder_beam_stream_workspace_bytes(PTR, 2, 4, 100)
    assert 2 * 2 * 2 * 4 * 101 * 4 <= need < 2 * 2 * 2 * 4 * 101 * 4 + 16 * 256
    assert lib.wr_decoder_attach_beam_stream(NULL, 2, 4, 100, PTR, 1 << 40) == -1
    assert lib.wr_last_error() == b"decoder_attach_beam_stream: null handle"


def test_header_exports_and_signatures_agree(lib):
    from wenet_celoss_amd import _lib
    text = open(os.path.join(ROOT, "include", "wr_api.h")).read()
    assert "Streaming transducer prefix beam search" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in (("wr_decoder_beam_stream_workspace_bytes", 4), ("wr_decoder_attach_beam_stream", 6),
                         ("wr_prefix_beam_search_chunk", 20)):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        proto = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code, flags=re.S).group(1)
        assert len(proto.split(",")) == n_args == len(_lib.SIGNATURES[name][1]), name
    assert _lib.SIGNATURES["wr_decoder_beam_stream_workspace_bytes"][0] is ctypes.c_size_t
    # the new entry points only add to the ABI: nothing existing changed its signature or layout
    assert lib.wr_api_version() == _lib.API_VERSION == int(re.search(r"#define\s+WR_API_VERSION\s+(\d+)", text).group(1))
    # the contract states the one case in which chunking may change a token-and-duration result
    assert "at least max(durations) frames" in text.replace("\n * ", " ")


def test_python_surface():
    import wenet_celoss_amd as w
    from wenet_celoss_amd.decoder import DeviceDecoder
    from wenet_celoss_amd.search.prefix_beam_search import TransducerPrefixBeamStream
    assert "TransducerPrefixBeamStream" in w.__all__ and w.TransducerPrefixBeamStream is TransducerPrefixBeamStream
    assert list(inspect.signature(DeviceDecoder.attach_beam_stream).parameters) == ["self", "n_streams", "beam", "max_frames"]
    sig = inspect.signature(DeviceDecoder.prefix_beam_chunk)
    assert list(sig.parameters) == ["self", "encoder_chunk", "chunk_lens", "beam_size", "blank", "ctc_logp", "ctc_weight",
                                    "transducer_weight", "durations", "reset", "final"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[4:]] == [0, None, 0.0, 1.0, None, False, False]
    sig = inspect.signature(TransducerPrefixBeamStream.__init__)
    assert list(sig.parameters) == ["self", "model", "n_streams", "beam_size", "max_frames", "chunk_frames", "ctc_weight",
                                    "transducer_weight"]
    assert list(inspect.signature(TransducerPrefixBeamStream.reset).parameters) == ["self", "streams"]
    assert list(inspect.signature(TransducerPrefixBeamStream.search).parameters) == ["self", "encoder_out_chunk", "lens", "final"]
    assert list(inspect.signature(w.Transducer.forward_prefix_beam_search).parameters) == [
        "self", "encoder_out_chunk", "encoder_out_lens", "final"]
    assert list(inspect.signature(w.Transducer.beam_search_times).parameters)[:6] == [
        "self", "speech", "speech_lengths", "beam_size", "ctc_weight", "transducer_weight"]
    assert list(inspect.signature(w.Transducer.reset_beam_stream).parameters)[:4] == ["self", "n_streams", "beam_size", "max_frames"]
    # existing methods are untouched, the refusals of a TDT model included
    assert list(inspect.signature(w.Transducer.forward_greedy_search).parameters) == [
        "self", "encoder_out", "encoder_out_lens", "n_steps", "reference_new_cache"]


class _Enc(torch.nn.Module):
    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)

    def output_size(self):
        return self.proj.out_features


def _model(joint_outputs=23, **kw):
    import wenet_celoss_amd as w
    torch.manual_seed(0)
    return w.Transducer(23, 0, _Enc(8, 12), w.RNNPredictor(23, 10, 10, 0.0, 14, 2, dropout=0.0),
                        w.TransducerJoint(joint_outputs, 12, 10, 16), ctc=w.CTC(23, 12), ctc_weight=0.3, transducer_weight=0.7,
                        **kw)


def test_the_weights_default_to_those_of_the_whole_utterance_searches():
    import wenet_celoss_amd as w
    s = w.TransducerPrefixBeamStream(_model(), 2, 4, 32, 8)
    assert (s.ctc_weight, s.transducer_weight, s.durations, s._with_ctc) == (0.3, 0.7, None, True)
    s = w.TransducerPrefixBeamStream(_model(26, tdt_durations=(0, 1, 2)), 2, 4, 32, 8)
    assert (s.ctc_weight, s.transducer_weight, s.durations, s._with_ctc) == (0.0, 1.0, (0, 1, 2), False)
    s = w.TransducerPrefixBeamStream(_model(26, tdt_durations=(0, 1, 2)), 2, 4, 32, 8, 0.3, 0.7)
    assert s._with_ctc


def test_python_errors():
    import wenet_celoss_amd as w
    m = _model(26, tdt_durations=(0, 1, 2))
    lens = torch.tensor([4, 4], dtype=torch.int32)
    for bad in [dict(n_streams=0), dict(beam_size=0), dict(beam_size=17), dict(max_frames=0), dict(chunk_frames=0)]:
        with pytest.raises(RuntimeError, match="TransducerPrefixBeamStream"):
            w.TransducerPrefixBeamStream(m, **{**dict(n_streams=2, beam_size=4, max_frames=16, chunk_frames=8), **bad})
    s = w.TransducerPrefixBeamStream(m, 2, 4, 16, 8)
    assert s.frames == [0, 0]
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.search(torch.zeros(2, 4, 12), lens)
    with pytest.raises(RuntimeError, match=r"chunk has 3 streams, the stream set has 2"):
        s.search(torch.zeros(3, 4, 12), torch.tensor([4, 4, 4]))
    with pytest.raises(RuntimeError, match=r"a chunk of 9 frames exceeds chunk_frames=8"):
        s.search(torch.zeros(2, 9, 12), lens)
    with pytest.raises(RuntimeError, match=r"final has 3 entries for 2 streams"):
        s.search(torch.zeros(2, 4, 12), lens, final=[True, False, True])
    with pytest.raises(RuntimeError, match=r"lens has 3 elements for 2 streams"):
        s.search(torch.zeros(2, 4, 12), torch.tensor([4, 4, 4]))
    s._phase, s.frames = [1, 2], [12, 8]                     # stream 0 after three chunks of four, stream 1 finished
    with pytest.raises(RuntimeError, match=r"stream 0: 12 frames done \+ a chunk of 5 exceeds max_frames=16"):
        s.search(torch.zeros(2, 5, 12), torch.tensor([5, 0]))
    with pytest.raises(RuntimeError, match=r"stream 1 is fed after its final chunk \(reset it first\)"):
        s.search(torch.zeros(2, 4, 12), lens)
    with pytest.raises(RuntimeError, match=r"stream 1 is fed after its final chunk"):
        s.search(torch.zeros(2, 4, 12), torch.tensor([4, 0]), final=True)
    with pytest.raises(RuntimeError, match="no CPU path"):   # a finished stream that gets nothing is no error
        s.search(torch.zeros(2, 4, 12), torch.tensor([4, 0]))
    s.reset([1])
    assert (s._phase, s.frames) == ([1, 0], [12, 0])
    s.reset()
    assert (s._phase, s.frames) == ([0, 0], [0, 0])
    # the Transducer methods build the stream set on demand and pass the same errors on
    with pytest.raises(RuntimeError, match="no CPU path"):
        m.forward_prefix_beam_search(torch.zeros(2, 4, 12), lens)
    assert m._beam_stream.n_streams == 2 and m._beam_stream.chunk_frames == 64
    with pytest.raises(RuntimeError, match=r"chunk has 3 streams, the stream set has 2"):
        m.forward_prefix_beam_search(torch.zeros(3, 4, 12), torch.tensor([4, 4, 4]))
    # the existing streaming search still refuses a TDT model
    with pytest.raises(NotImplementedError, match="TDT"):
        m.forward_greedy_search(torch.zeros(1, 4, 12), torch.tensor([4]))
