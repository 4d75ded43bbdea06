"""Host-side checks of the streaming CTC prefix beam search: what wr_ctc_prefix_beam_search_chunk refuses before any HIP
call and in which order (by return code and wr_last_error text), the size queries, the Python errors and the new
signatures.  No GPU is needed and none is used."""
import ctypes
import inspect

import pytest
import torch

NULL = ctypes.c_void_p(None)
PTR = ctypes.c_void_p(0x1000)        # a non-null placeholder: every call here is refused before anything reads it
BIG = 1 << 40
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
POINTERS = ["logits", "lens", "state", "hyps", "hyp_lens", "scores", "viterbi", "times", "n_hyps", "n_frames", "workspace"]


@pytest.fixture(scope="module")
def lib():
    from wenet_celoss_amd import _lib
    return _lib.load()


def chunk(lib, B=2, T=4, V=8, beam=3, blank=0, reset=0, frames_done=0, Lcap=16, state_bytes=BIG, workspace_bytes=BIG, **ptrs):
    p = {name: ptrs.get(name, PTR) for name in POINTERS}
    return lib.wr_ctc_prefix_beam_search_chunk(p["logits"], p["lens"], B, T, V, beam, blank, reset, frames_done, Lcap,
                                               p["state"], state_bytes, p["hyps"], p["hyp_lens"], p["scores"], p["viterbi"],
                                               p["times"], p["n_hyps"], p["n_frames"], p["workspace"], workspace_bytes, NULL)


REFUSALS = [
    (dict(B=0), EINVAL, b"ctc decode: B, T must be positive and V > 1 (got 0,4,8)"),
    (dict(T=0), EINVAL, b"ctc decode: B, T must be positive and V > 1 (got 2,0,8)"),
    (dict(V=1, beam=1), EINVAL, b"ctc decode: B, T must be positive and V > 1 (got 2,4,1)"),
    (dict(blank=8), EINVAL, b"ctc decode: blank 8 out of range"),
    (dict(blank=-1), EINVAL, b"ctc decode: blank -1 out of range"),
    (dict(V=16321), EUNSUPPORTED, b"ctc decode: V=16321 exceeds 16320"),
] + [(dict({name: NULL}), EINVAL, b"ctc_prefix_beam_search_chunk: null pointer argument") for name in POINTERS] + [
    (dict(beam=0), EUNSUPPORTED, b"ctc_prefix_beam_search_chunk: beam=0 (1..16, at most V)"),
    (dict(beam=17, V=20), EUNSUPPORTED, b"ctc_prefix_beam_search_chunk: beam=17 (1..16, at most V)"),
    (dict(beam=9), EUNSUPPORTED, b"ctc_prefix_beam_search_chunk: beam=9 (1..16, at most V)"),
    (dict(Lcap=0), EINVAL, b"ctc_prefix_beam_search_chunk: Lcap=0 must be 1 or more"),
    (dict(frames_done=-1), EINVAL, b"ctc_prefix_beam_search_chunk: frames_done=-1 is negative"),
    (dict(reset=1, frames_done=4), EINVAL,
     b"ctc_prefix_beam_search_chunk: reset with frames_done=4 (a fresh stream has consumed nothing)"),
    (dict(frames_done=13), EUNSUPPORTED, b"ctc_prefix_beam_search_chunk: frames_done=13 + T=4 exceeds Lcap=16"),
    (dict(T=17), EUNSUPPORTED, b"ctc_prefix_beam_search_chunk: frames_done=0 + T=17 exceeds Lcap=16"),
    (dict(frames_done=2147483647), EUNSUPPORTED,
     b"ctc_prefix_beam_search_chunk: frames_done=2147483647 + T=4 exceeds Lcap=16"),
]


@pytest.mark.parametrize("kw, rc, text", REFUSALS)
def test_the_entry_point_refuses_before_any_hip_call(lib, kw, rc, text):
    assert chunk(lib, **kw) == rc
    assert lib.wr_last_error() == text


def test_sizes_below_the_queries_are_refused(lib):
    need_s = lib.wr_ctc_stream_state_bytes(2, 3, 16)
    need_w = lib.wr_ctc_stream_workspace_bytes(2, 4, 3)
    assert chunk(lib, state_bytes=need_s - 1) == EWORKSPACE
    assert lib.wr_last_error() == b"ctc_prefix_beam_search_chunk: state block too small"
    assert chunk(lib, state_bytes=need_s, workspace_bytes=need_w - 1) == EWORKSPACE
    assert lib.wr_last_error() == b"ctc_prefix_beam_search_chunk: workspace too small"
    assert chunk(lib, state_bytes=0, workspace_bytes=0) == EWORKSPACE and b"state block" in lib.wr_last_error()


def test_the_checks_run_in_the_documented_order(lib):
    """shape, pointers, beam, Lcap, frames_done, reset with frames_done, capacity, state size, workspace size"""
    bad = dict(blank=9, logits=NULL, beam=0, Lcap=0, frames_done=-1, reset=1, state_bytes=0, workspace_bytes=0)
    steps = [("blank", dict(blank=0), b"blank 9 out of range"), ("logits", dict(logits=PTR), b"null pointer"),
             ("beam", dict(beam=3), b"beam=0"), ("Lcap", dict(Lcap=16), b"Lcap=0"),
             ("frames_done", dict(frames_done=14), b"frames_done=-1 is negative"),
             ("reset", dict(reset=0), b"reset with frames_done=14"), ("capacity", dict(frames_done=12), b"exceeds Lcap=16"),
             ("state", dict(state_bytes=BIG), b"state block too small"), ("workspace", None, b"workspace too small")]
    for name, fix, text in steps:
        assert chunk(lib, **bad) < 0
        assert text in lib.wr_last_error(), (name, lib.wr_last_error())
        if fix:
            bad.update(fix)


def test_size_queries_are_positive_and_non_decreasing(lib):
    state, ws = lib.wr_ctc_stream_state_bytes, lib.wr_ctc_stream_workspace_bytes
    for q in (state, ws):
        assert q(1, 1, 1) > 0
        for base in [(1, 1, 1), (3, 5, 7), (32, 16, 16)]:
            for i in range(3):
                prev = 0
                for step in range(6):
                    args = list(base)
                    args[i] += step
                    if q is state and args[1] > 16:
                        break
                    assert q(*args) >= prev > -1
                    prev = q(*args)
                assert prev > 0
        assert q(0, 4, 4) == q(4, 0, 4) == q(4, 4, 0) == 0
    assert state(2, 17, 8) == 0                                  # beyond the beam limit there is nothing to size
    # three int32 lists of beam * Lcap, double-buffered, and the scalars of the entries, per stream
    assert state(4, 16, 1000) >= 4 * (3 * 2 * 16 * 1000 * 4 + 16 * 48)
    assert state(4, 16, 1000) < 4 * (3 * 2 * 16 * 1000 * 4 + 16 * 48) + 4 * 1024
    assert ws(32, 16, 10) >= 32 * 16 * 10 * 8


def test_api_version_and_bindings(lib):
    from wenet_celoss_amd import _lib
    assert lib.wr_api_version() == _lib.API_VERSION                # the new entry points only add to the ABI
    for name in ("wr_ctc_stream_state_bytes", "wr_ctc_stream_workspace_bytes", "wr_ctc_prefix_beam_search_chunk"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["wr_ctc_prefix_beam_search_chunk"][1]) == 22


def test_python_surface():
    import wenet_celoss_amd as w
    from wenet_celoss_amd import ctc
    assert {"CtcPrefixBeamStream", "ctc_prefix_beam_search_times"} <= set(w.__all__)
    assert w.CtcPrefixBeamStream is ctc.CtcPrefixBeamStream and w.ctc_prefix_beam_search_times is ctc.ctc_prefix_beam_search_times
    sig = inspect.signature(w.CtcPrefixBeamStream.__init__)
    assert list(sig.parameters)[:5] == ["self", "n_streams", "beam_size", "max_frames", "blank"]
    assert sig.parameters["blank"].default == 0
    assert list(inspect.signature(w.CtcPrefixBeamStream.search).parameters) == ["self", "logits_chunk", "lens"]
    assert list(inspect.signature(w.CtcPrefixBeamStream.reset).parameters) == ["self"]
    sig = inspect.signature(w.ctc_prefix_beam_search_times)
    assert list(sig.parameters) == ["logits", "lens", "beam_size", "blank"] and sig.parameters["blank"].default == 0
    sig = inspect.signature(w.Transducer.ctc_prefix_beam_search_times)
    assert list(sig.parameters) == ["self", "speech", "speech_lengths", "beam_size", "decoding_chunk_size",
                                    "num_decoding_left_chunks", "simulate_streaming"]
    assert list(sig.parameters) == list(inspect.signature(w.Transducer.ctc_prefix_beam_search).parameters)
    assert [sig.parameters[n].default for n in list(sig.parameters)[4:]] == [-1, -1, False]
    sig = inspect.signature(w.Transducer.reset_ctc_stream)
    assert list(sig.parameters) == ["self", "n_streams", "beam_size", "max_frames"]
    assert (sig.parameters["n_streams"].default, sig.parameters["beam_size"].default) == (1, 10)
    assert list(inspect.signature(w.Transducer.forward_ctc_prefix_beam_search).parameters) == [
        "self", "encoder_out_chunk", "encoder_out_lens"]
    # the existing searches keep their signatures
    assert list(inspect.signature(w.ctc_prefix_beam_search).parameters) == ["logits", "lens", "beam_size", "blank"]


def test_python_errors():
    import wenet_celoss_amd as w
    lens = torch.tensor([4, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.ctc_prefix_beam_search_times(torch.zeros(2, 4, 8), lens, 3)
    s = w.CtcPrefixBeamStream(2, 3, 16)
    assert s.frames == [0, 0]
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.search(torch.zeros(2, 4, 8), lens)
    with pytest.raises(RuntimeError, match=r"chunk has 3 streams, the stream set has 2"):
        s.search(torch.zeros(3, 4, 8), torch.tensor([4, 4, 4]))
    with pytest.raises(RuntimeError, match=r"0 frames done \+ a chunk of 17 exceeds max_frames=16"):
        s.search(torch.zeros(2, 17, 8), lens)
    s._vocab, s._frames_done = 8, 12                              # as after three chunks of four frames
    with pytest.raises(RuntimeError, match=r"vocabulary changed from 8 to 9"):
        s.search(torch.zeros(2, 4, 9), lens)
    with pytest.raises(RuntimeError, match=r"12 frames done \+ a chunk of 5 exceeds max_frames=16"):
        s.search(torch.zeros(2, 5, 8), lens)
    s.reset()
    assert s._frames_done == 0 and s.frames == [0, 0]
    for bad in [dict(n_streams=0), dict(beam_size=0), dict(beam_size=17), dict(max_frames=0)]:
        with pytest.raises(RuntimeError, match="CtcPrefixBeamStream"):
            w.CtcPrefixBeamStream(**{**dict(n_streams=1, beam_size=4, max_frames=8), **bad})
