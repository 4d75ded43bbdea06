"""Host-side checks of the biased CTC prefix beam search: what wr_ctc_prefix_beam_search_context_chunk refuses before any
HIP call and in which order (by return code and wr_last_error text), the size query, the Python errors, the new
signatures, and that the existing stream class and functions keep theirs.  No GPU is needed and none is used."""
import ctypes
import inspect

import pytest
import torch

NULL = ctypes.c_void_p(None)
PTR = ctypes.c_void_p(0x1000)        # a non-null placeholder: every call here is refused before anything reads it
BIG = 1 << 40
EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
TABLE = ["arc_begin", "arc_token", "arc_next", "arc_score", "escape", "final"]
OUT = ["hyps", "hyp_lens", "scores", "viterbi", "times", "n_hyps", "n_frames", "ctc_scores", "context_scores", "tags",
       "context_states"]
POINTERS = ["logits", "lens", "state"] + OUT + ["workspace"]
NAME = b"ctc_prefix_beam_search_context_chunk: "


@pytest.fixture(scope="module")
def lib():
    from wenet_celoss_amd import _lib
    return _lib.load()


def chunk(lib, B=2, T=4, V=8, beam=3, blank=0, reset=0, frames_done=0, Lcap=16, state_bytes=BIG, workspace_bytes=BIG, S=3, A=4,
          finalize=0, **ptrs):
    p = {name: ptrs.get(name, PTR) for name in POINTERS + TABLE}
    return lib.wr_ctc_prefix_beam_search_context_chunk(
        p["logits"], p["lens"], B, T, V, beam, blank, reset, frames_done, Lcap, p["state"], state_bytes,
        *[p[n] for n in TABLE], S, A, finalize, *[p[n] for n in OUT], p["workspace"], workspace_bytes, NULL)


REFUSALS = [
    (dict(B=0), EINVAL, b"ctc decode: B, T must be positive and V > 1 (got 0,4,8)"),
    (dict(T=0), EINVAL, b"ctc decode: B, T must be positive and V > 1 (got 2,0,8)"),
    (dict(V=1, beam=1), EINVAL, b"ctc decode: B, T must be positive and V > 1 (got 2,4,1)"),
    (dict(blank=8), EINVAL, b"ctc decode: blank 8 out of range"),
    (dict(blank=-1), EINVAL, b"ctc decode: blank -1 out of range"),
    (dict(V=16321), EUNSUPPORTED, b"ctc decode: V=16321 exceeds 16320"),
] + [(dict({name: NULL}), EINVAL, NAME + b"null pointer argument") for name in POINTERS] + [
    (dict(beam=0), EUNSUPPORTED, NAME + b"beam=0 (1..16, at most V)"),
    (dict(beam=17, V=20), EUNSUPPORTED, NAME + b"beam=17 (1..16, at most V)"),
    (dict(beam=9), EUNSUPPORTED, NAME + b"beam=9 (1..16, at most V)"),
    (dict(Lcap=0), EINVAL, NAME + b"Lcap=0 must be 1 or more"),
    (dict(frames_done=-1), EINVAL, NAME + b"frames_done=-1 is negative"),
    (dict(reset=1, frames_done=4), EINVAL, NAME + b"reset with frames_done=4 (a fresh stream has consumed nothing)"),
    (dict(frames_done=13), EUNSUPPORTED, NAME + b"frames_done=13 + T=4 exceeds Lcap=16"),
    (dict(T=17), EUNSUPPORTED, NAME + b"frames_done=0 + T=17 exceeds Lcap=16"),
    (dict(frames_done=2147483647), EUNSUPPORTED, NAME + b"frames_done=2147483647 + T=4 exceeds Lcap=16"),
    (dict(S=0), EINVAL, NAME + b"context graph with S=0 states, A=4 arcs"),
    (dict(A=-1), EINVAL, NAME + b"context graph with S=3 states, A=-1 arcs"),
] + [(dict({name: NULL}), EINVAL, NAME + b"null context graph pointer") for name in TABLE] + [
    (dict(S=65537), EUNSUPPORTED, NAME + b"context graph with S=65537 states, A=4 arcs exceeds 65536, 1048576"),
    (dict(A=1048577), EUNSUPPORTED, NAME + b"context graph with S=3 states, A=1048577 arcs exceeds 65536, 1048576"),
]


@pytest.mark.parametrize("kw, rc, text", REFUSALS)
def test_the_entry_point_refuses_before_any_hip_call(lib, kw, rc, text):
    assert chunk(lib, **kw) == rc
    assert lib.wr_last_error() == text


def test_sizes_below_the_queries_are_refused(lib):
    need_s = lib.wr_ctc_context_stream_state_bytes(2, 3, 16)
    need_w = lib.wr_ctc_stream_workspace_bytes(2, 4, 3)
    assert chunk(lib, state_bytes=need_s - 1, S=0) == EWORKSPACE
    assert lib.wr_last_error() == NAME + b"state block too small"
    assert chunk(lib, state_bytes=lib.wr_ctc_stream_state_bytes(2, 3, 16), S=0) == EWORKSPACE    # the plain block is too small
    assert chunk(lib, state_bytes=need_s, workspace_bytes=need_w - 1, S=0) == EWORKSPACE
    assert lib.wr_last_error() == NAME + b"workspace too small"
    assert chunk(lib, state_bytes=need_s, workspace_bytes=need_w, S=0) == EINVAL                 # and then the table


def test_the_checks_run_in_the_documented_order(lib):
    """everything of the plain chunk call in its order, then S / A, the table's pointers, the table's size limits"""
    bad = dict(blank=9, logits=NULL, beam=0, Lcap=0, frames_done=-1, reset=1, state_bytes=0, workspace_bytes=0, S=0, A=1 << 30,
               escape=NULL, tags=NULL)
    steps = [("blank", dict(blank=0), b"blank 9 out of range"), ("logits", dict(logits=PTR), b"null pointer argument"),
             ("tags", dict(tags=PTR), b"null pointer argument"),
             ("beam", dict(beam=3), b"beam=0"), ("Lcap", dict(Lcap=16), b"Lcap=0"),
             ("frames_done", dict(frames_done=14), b"frames_done=-1 is negative"),
             ("reset", dict(reset=0), b"reset with frames_done=14"), ("capacity", dict(frames_done=12), b"exceeds Lcap=16"),
             ("state", dict(state_bytes=BIG), b"state block too small"), ("workspace", dict(workspace_bytes=BIG), b"workspace too small"),
             ("S", dict(S=70000), b"with S=0 states"), ("escape", dict(escape=PTR), b"null context graph pointer"),
             ("limits", None, b"exceeds 65536, 1048576")]
    for name, fix, text in steps:
        assert chunk(lib, **bad) < 0
        assert text in lib.wr_last_error(), (name, lib.wr_last_error())
        if fix:
            bad.update(fix)


def test_size_query(lib):
    ctx, plain = lib.wr_ctc_context_stream_state_bytes, lib.wr_ctc_stream_state_bytes
    assert ctx(0, 4, 4) == ctx(4, 0, 4) == ctx(4, 4, 0) == ctx(-1, 4, 4) == 0
    assert ctx(2, 17, 8) == 0 and ctx(2, 16, 8) > 0
    for args in [(1, 1, 1), (3, 5, 7), (32, 16, 16), (4, 16, 1000)]:
        assert ctx(*args) > plain(*args) > 0
    # four int32 lists of beam * Lcap, double-buffered, and the scalars of the entries (48 + 12 bytes), per stream
    assert ctx(4, 16, 1000) >= 4 * (4 * 2 * 16 * 1000 * 4 + 16 * 60)
    assert ctx(4, 16, 1000) < 4 * (4 * 2 * 16 * 1000 * 4 + 16 * 60) + 4 * 1024
    # the plain query did not move: three lists and 48 bytes per entry
    assert 4 * (3 * 2 * 16 * 1000 * 4 + 16 * 48) <= plain(4, 16, 1000) < 4 * (3 * 2 * 16 * 1000 * 4 + 16 * 48) + 4 * 1024


def test_api_version_and_bindings(lib):
    from wenet_celoss_amd import _lib
    assert lib.wr_api_version() == _lib.API_VERSION == 3              # the new entry points only add to the ABI
    for name in ("wr_ctc_context_stream_state_bytes", "wr_ctc_prefix_beam_search_context_chunk"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["wr_ctc_prefix_beam_search_context_chunk"][1]) == 22 + 8 + 1 + 4
    assert len(_lib.SIGNATURES["wr_ctc_prefix_beam_search_chunk"][1]) == 22


def test_python_surface():
    import wenet_celoss_amd as w
    from wenet_celoss_amd import context_graph, ctc
    assert {"ContextGraph", "CtcContextPrefixBeamStream", "ctc_context_prefix_beam_search"} <= set(w.__all__)
    assert w.ContextGraph is context_graph.ContextGraph and w.CtcContextPrefixBeamStream is ctc.CtcContextPrefixBeamStream
    assert w.ctc_context_prefix_beam_search is ctc.ctc_context_prefix_beam_search
    sig = inspect.signature(w.ContextGraph.__init__)
    assert list(sig.parameters) == ["self", "phrases", "context_score", "blank"]
    assert (sig.parameters["context_score"].default, sig.parameters["blank"].default) == (3.0, 0)
    sig = inspect.signature(w.CtcContextPrefixBeamStream.__init__)
    assert list(sig.parameters) == ["self", "n_streams", "beam_size", "max_frames", "context_graph", "blank", "state"]
    assert (sig.parameters["blank"].default, sig.parameters["state"].default) == (0, None)
    sig = inspect.signature(w.CtcContextPrefixBeamStream.search)
    assert list(sig.parameters) == ["self", "logits_chunk", "lens", "finalize"] and sig.parameters["finalize"].default is False
    assert list(inspect.signature(w.CtcContextPrefixBeamStream.reset).parameters) == ["self"]
    assert list(inspect.signature(w.CtcContextPrefixBeamStream.finalize).parameters) == ["self"]
    assert list(inspect.signature(w.CtcContextPrefixBeamStream.outputs).parameters) == ["result", "start_tag_id", "end_tag_id"]
    sig = inspect.signature(w.ctc_context_prefix_beam_search)
    assert list(sig.parameters) == ["logits", "lens", "beam_size", "context_graph", "blank"] and sig.parameters["blank"].default == 0
    sig = inspect.signature(w.Transducer.reset_ctc_context_stream)
    assert list(sig.parameters) == ["self", "n_streams", "beam_size", "max_frames", "context_graph"]
    sig = inspect.signature(w.Transducer.forward_ctc_context_prefix_beam_search)
    assert list(sig.parameters) == ["self", "encoder_out_chunk", "encoder_out_lens", "finalize"]
    assert sig.parameters["finalize"].default is False
    sig = inspect.signature(w.Transducer.ctc_context_prefix_beam_search)
    assert list(sig.parameters)[:5] == ["self", "speech", "speech_lengths", "beam_size", "context_graph"]


def test_existing_signatures_are_unchanged():
    import wenet_celoss_amd as w
    sig = inspect.signature(w.CtcPrefixBeamStream.__init__)
    assert list(sig.parameters) == ["self", "n_streams", "beam_size", "max_frames", "blank", "state"]
    assert (sig.parameters["blank"].default, sig.parameters["state"].default) == (0, None)
    assert list(inspect.signature(w.CtcPrefixBeamStream.search).parameters) == ["self", "logits_chunk", "lens"]
    assert list(inspect.signature(w.CtcPrefixBeamStream.reset).parameters) == ["self"]
    for fn in (w.ctc_prefix_beam_search_times, w.ctc_prefix_beam_search):
        sig = inspect.signature(fn)
        assert list(sig.parameters) == ["logits", "lens", "beam_size", "blank"] and sig.parameters["blank"].default == 0
    sig = inspect.signature(w.Transducer.ctc_prefix_beam_search_times)
    assert list(sig.parameters) == ["self", "speech", "speech_lengths", "beam_size", "decoding_chunk_size",
                                    "num_decoding_left_chunks", "simulate_streaming"]
    sig = inspect.signature(w.Transducer.reset_ctc_stream)
    assert list(sig.parameters) == ["self", "n_streams", "beam_size", "max_frames"]
    assert [sig.parameters[n].default for n in ("n_streams", "beam_size", "max_frames")] == [1, 10, 4096]
    assert list(inspect.signature(w.Transducer.forward_ctc_prefix_beam_search).parameters) == [
        "self", "encoder_out_chunk", "encoder_out_lens"]


def test_python_errors():
    import wenet_celoss_amd as w
    g = w.ContextGraph([[1, 2]], 1.0)
    lens = torch.tensor([4, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.ctc_context_prefix_beam_search(torch.zeros(2, 4, 8), lens, 3, g)
    s = w.CtcContextPrefixBeamStream(2, 3, 16, g)
    assert s.frames == [0, 0]
    with pytest.raises(RuntimeError, match="no CPU path"):
        s.search(torch.zeros(2, 4, 8), lens)
    with pytest.raises(RuntimeError, match=r"chunk has 3 streams, the stream set has 2"):
        s.search(torch.zeros(3, 4, 8), torch.tensor([4, 4, 4]))
    with pytest.raises(RuntimeError, match=r"0 frames done \+ a chunk of 17 exceeds max_frames=16"):
        s.search(torch.zeros(2, 17, 8), lens)
    with pytest.raises(RuntimeError, match=r"finalize\(\) before the first search"):
        s.finalize()
    s._vocab, s._frames_done = 8, 12                              # as after three chunks of four frames
    with pytest.raises(RuntimeError, match=r"vocabulary changed from 8 to 9"):
        s.search(torch.zeros(2, 4, 9), lens)
    with pytest.raises(RuntimeError, match=r"12 frames done \+ a chunk of 5 exceeds max_frames=16"):
        s.search(torch.zeros(2, 5, 8), lens)
    s.reset()
    assert s._frames_done == 0 and s.frames == [0, 0]
    for bad in [dict(n_streams=0), dict(beam_size=0), dict(beam_size=17), dict(max_frames=0)]:
        with pytest.raises(RuntimeError, match="CtcContextPrefixBeamStream"):
            w.CtcContextPrefixBeamStream(**{**dict(n_streams=1, beam_size=4, max_frames=8, context_graph=g), **bad})
    with pytest.raises(RuntimeError, match="must be a ContextGraph"):
        w.CtcContextPrefixBeamStream(1, 4, 8, [[1, 2]])
    with pytest.raises(RuntimeError, match="built for blank 0, the search uses 3"):
        w.CtcContextPrefixBeamStream(1, 4, 8, g, blank=3)
