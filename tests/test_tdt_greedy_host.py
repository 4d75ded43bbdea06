"""Host-side checks of the TDT greedy search: what wr_greedy_search_tdt refuses before any HIP call, the durations
contract it shares with the loss, and the Python surface.  No GPU is needed and none is used."""
import ctypes
import inspect

import pytest
import torch


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
                        w.TransducerJoint(joint_outputs, 12, 10, 16), ctc_weight=0.0, transducer_weight=1.0, **kw)


@pytest.fixture(scope="module")
def lib():
    from wenet_celoss_amd import _lib
    return _lib.load()


NULL = ctypes.c_void_p(None)
PTR = ctypes.c_void_p(0x1000)        # a non-null placeholder: every call here is refused before anything reads it


def durs(*d):
    return (ctypes.c_int32 * max(len(d), 1))(*d)


def search(lib, h=PTR, enc=PTR, lens=PTR, n_steps=4, d=(0, 1, 2), D=None, durations=None, hyps=PTR, hl=PTR, frames=NULL):
    arr = durs(*d) if durations is None else durations
    return lib.wr_greedy_search_tdt(h, enc, lens, 2, 8, n_steps, 0, arr, len(d) if D is None else D, hyps, hl, frames, NULL)


@pytest.mark.parametrize("kw, text", [
    (dict(D=0), b"D=0 durations (1 to 9 are supported)"),
    (dict(d=tuple(range(9)), D=10), b"D=10 durations (1 to 9 are supported)"),
    (dict(d=(0, 9)), b"durations[1]=9 lies outside [0, 8]"),
    (dict(d=(0, 2, 1)), b"durations must be strictly increasing (durations[2]=1 after 2)"),
    (dict(d=(1, 1)), b"durations must be strictly increasing (durations[1]=1 after 1)"),
    (dict(d=(0,)), b"at least one duration must be 1 or more"),
    (dict(durations=NULL), b"durations is null"),
    (dict(n_steps=0), b"n_steps=0 must be 1 or more"),
    (dict(hyps=NULL), b"null pointer argument"),
    (dict(hl=NULL), b"null pointer argument"),
    (dict(enc=NULL), b"null pointer argument"),
    (dict(lens=NULL), b"null pointer argument"),
    (dict(h=NULL), b"null handle"),
])
def test_the_entry_point_refuses_before_any_hip_call(lib, kw, text):
    assert search(lib, **kw) == -1
    err = lib.wr_last_error()
    assert err.startswith(b"greedy_search_tdt: ") and text in err, err


def test_the_checks_run_in_the_documented_order(lib):
    # durations before n_steps, n_steps before the pointers, the pointers before the handle
    assert search(lib, h=NULL, hyps=NULL, n_steps=0, d=(2, 1)) == -1 and b"strictly increasing" in lib.wr_last_error()
    assert search(lib, h=NULL, hyps=NULL, n_steps=0) == -1 and b"n_steps" in lib.wr_last_error()
    assert search(lib, h=NULL, hyps=NULL) == -1 and b"null pointer argument" in lib.wr_last_error()
    assert search(lib, h=NULL) == -1 and b"null handle" in lib.wr_last_error()


def test_the_loss_gives_the_same_duration_rejections_as_before(lib):
    big = 1 << 40

    def fwd(d=(0, 1, 2), D=None):
        return lib.wr_rnnt_tdt_loss_fwd(NULL, 0, NULL, NULL, NULL, 2, 4, 3, 8, 0, durs(*d), len(d) if D is None else D, 0.0,
                                        NULL, NULL, big, NULL)

    want = [(dict(D=0), b"rnnt_tdt_loss_fwd: D=0 durations (1 to 9 are supported)"),
            (dict(d=tuple(range(9)), D=10), b"rnnt_tdt_loss_fwd: D=10 durations (1 to 9 are supported)"),
            (dict(d=(0, 9)), b"rnnt_tdt_loss_fwd: durations[1]=9 lies outside [0, 8]"),
            (dict(d=(-1, 1)), b"rnnt_tdt_loss_fwd: durations[0]=-1 lies outside [0, 8]"),
            (dict(d=(0, 2, 1)), b"rnnt_tdt_loss_fwd: durations must be strictly increasing (durations[2]=1 after 2)"),
            (dict(d=(0,)), b"rnnt_tdt_loss_fwd: at least one duration must be 1 or more (no arc would consume a frame)")]
    for kw, text in want:
        assert fwd(**kw) == -1
        assert lib.wr_last_error() == text
    assert lib.wr_rnnt_tdt_loss_fwd(NULL, 0, NULL, NULL, NULL, 2, 4, 3, 8, 0, NULL, 3, 0.0, NULL, NULL, big, NULL) == -1
    assert lib.wr_last_error() == b"rnnt_tdt_loss_fwd: durations is null"


def test_python_surface():
    import wenet_celoss_amd as w
    from wenet_celoss_amd.decoder import DeviceDecoder
    from wenet_celoss_amd.search.greedy_search import tdt_greedy_search
    assert "tdt_greedy_search" in w.__all__ and w.tdt_greedy_search is tdt_greedy_search
    assert list(inspect.signature(DeviceDecoder.greedy_tdt).parameters) == [
        "self", "encoder_out", "encoder_out_lens", "durations", "n_steps", "blank", "return_frames"]
    assert list(inspect.signature(tdt_greedy_search).parameters) == [
        "model", "encoder_out", "encoder_out_lens", "n_steps", "return_frames"]
    sig = inspect.signature(w.Transducer.tdt_greedy_search_batch)
    assert list(sig.parameters) == ["self", "speech", "speech_lengths", "decoding_chunk_size", "num_decoding_left_chunks",
                                    "n_steps", "return_frames"]
    assert sig.parameters["n_steps"].default == 64 and sig.parameters["return_frames"].default is False


def test_the_refusal_names_the_new_method_and_a_plain_model_refuses_it():
    m = _model(26, tdt_durations=(0, 1, 2))
    with pytest.raises(NotImplementedError, match="TDT") as e:
        m._refuse_tdt("greedy_search_batch")
    assert "tdt_greedy_search_batch" in str(e.value) and "greedy_search_batch" in str(e.value)
    with pytest.raises(ValueError, match="tdt_durations"):
        _model().tdt_greedy_search_batch(torch.zeros(1, 5, 8), torch.tensor([5], dtype=torch.int32))
