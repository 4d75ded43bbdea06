"""Host-side checks of the TDT prefix beam search: what wr_prefix_beam_search_tdt refuses before any HIP call and in
which order, the durations contract it shares with the loss, the Python surface and its ValueErrors, and that the plain
beam methods still refuse a TDT model.  No GPU is needed and none is used.  (The refusals that need a decoder handle --
beam, capacities, vocabulary, blank, embedding rows, weights without a posterior -- are in tests/test_tdt_beam_gpu.py: a
handle cannot be built without a device.)"""
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


def search(lib, h=PTR, enc=PTR, lens=PTR, ctc=NULL, beam=4, d=(0, 1, 2), D=None, durations=None, hyps=PTR, hl=PTR,
           scores=PTR, nh=PTR):
    arr = durs(*d) if durations is None else durations
    return lib.wr_prefix_beam_search_tdt(h, enc, lens, ctc, 2, 8, beam, 0.0, 1.0, 0, arr, len(d) if D is None else D, hyps,
                                         hl, scores, nh, NULL)


@pytest.mark.parametrize("kw, text", [
    (dict(D=0), b"D=0 durations (1 to 9 are supported)"),
    (dict(d=tuple(range(9)), D=10), b"D=10 durations (1 to 9 are supported)"),
    (dict(d=(0, 9)), b"durations[1]=9 lies outside [0, 8]"),
    (dict(d=(-1, 1)), b"durations[0]=-1 lies outside [0, 8]"),
    (dict(d=(0, 2, 1)), b"durations must be strictly increasing (durations[2]=1 after 2)"),
    (dict(d=(1, 1)), b"durations must be strictly increasing (durations[1]=1 after 1)"),
    (dict(d=(0,)), b"at least one duration must be 1 or more (no arc would consume a frame)"),
    (dict(durations=NULL), b"durations is null"),
    (dict(enc=NULL), b"null pointer argument"),
    (dict(lens=NULL), b"null pointer argument"),
    (dict(hyps=NULL), b"null pointer argument"),
    (dict(hl=NULL), b"null pointer argument"),
    (dict(scores=NULL), b"null pointer argument"),
    (dict(nh=NULL), b"null pointer argument"),
    (dict(h=NULL), b"null handle"),
])
def test_the_entry_point_refuses_before_any_hip_call(lib, kw, text):
    assert search(lib, **kw) == -1
    err = lib.wr_last_error()
    assert err.startswith(b"prefix_beam_search_tdt: ") and text in err, err


def test_the_checks_run_in_the_documented_order(lib):
    # durations before the pointers, the pointers before the handle; a null CTC posterior is no null-pointer refusal
    assert search(lib, h=NULL, hyps=NULL, d=(2, 1)) == -1 and b"strictly increasing" in lib.wr_last_error()
    assert search(lib, h=NULL, hyps=NULL) == -1 and b"null pointer argument" in lib.wr_last_error()
    assert search(lib, h=NULL, ctc=NULL) == -1 and b"null handle" in lib.wr_last_error()
    assert search(lib, h=NULL, ctc=PTR, beam=0) == -1 and b"null handle" in lib.wr_last_error()


def test_the_loss_gives_the_same_duration_rejections_as_before(lib):
    big = 1 << 40

    def fwd(d=(0, 1, 2), D=None):
        return lib.wr_rnnt_tdt_loss_fwd(NULL, 0, NULL, NULL, NULL, 2, 4, 3, 8, 0, durs(*d), len(d) if D is None else D, 0.0,
                                        NULL, NULL, big, NULL)

    want = [(dict(D=0), b"rnnt_tdt_loss_fwd: D=0 durations (1 to 9 are supported)"),
            (dict(d=(0, 9)), b"rnnt_tdt_loss_fwd: durations[1]=9 lies outside [0, 8]"),
            (dict(d=(0, 2, 1)), b"rnnt_tdt_loss_fwd: durations must be strictly increasing (durations[2]=1 after 2)"),
            (dict(d=(0,)), b"rnnt_tdt_loss_fwd: at least one duration must be 1 or more (no arc would consume a frame)")]
    for kw, text in want:
        assert fwd(**kw) == -1
        assert lib.wr_last_error() == text
    # and the greedy search its own
    assert lib.wr_greedy_search_tdt(PTR, PTR, PTR, 2, 8, 4, 0, durs(0, 9), 2, PTR, PTR, NULL, NULL) == -1
    assert lib.wr_last_error() == b"greedy_search_tdt: durations[1]=9 lies outside [0, 8]"


def test_the_counters_accessor_refuses_null_pointers(lib):
    out = (ctypes.c_int32 * 3)()
    assert lib.wr_decoder_last_counters(NULL, out) == -1 and b"decoder_last_counters: null pointer" in lib.wr_last_error()
    assert lib.wr_decoder_last_counters(PTR, NULL) == -1


def test_api_version_is_unchanged(lib):
    from wenet_celoss_amd import _lib
    assert lib.wr_api_version() == _lib.API_VERSION == 3
    assert "wr_prefix_beam_search_tdt" in _lib.SIGNATURES


def test_python_surface():
    import wenet_celoss_amd as w
    from wenet_celoss_amd.decoder import DeviceDecoder
    from wenet_celoss_amd.search.prefix_beam_search import tdt_prefix_beam_search
    assert "tdt_prefix_beam_search" in w.__all__ and w.tdt_prefix_beam_search is tdt_prefix_beam_search
    sig = inspect.signature(DeviceDecoder.prefix_beam_tdt)
    assert list(sig.parameters) == ["self", "encoder_out", "encoder_out_lens", "durations", "beam_size", "blank", "ctc_logp",
                                    "ctc_weight", "transducer_weight"]
    assert (sig.parameters["ctc_logp"].default, sig.parameters["ctc_weight"].default,
            sig.parameters["transducer_weight"].default) == (None, 0.0, 1.0)
    assert list(inspect.signature(tdt_prefix_beam_search).parameters) == [
        "model", "encoder_out", "encoder_out_lens", "beam_size", "ctc_weight", "transducer_weight"]
    sig = inspect.signature(w.Transducer.tdt_beam_search)
    assert list(sig.parameters) == ["self", "speech", "speech_lengths", "decoding_chunk_size", "beam_size",
                                    "num_decoding_left_chunks", "simulate_streaming", "ctc_weight", "transducer_weight",
                                    "_ignored"]
    plain = inspect.signature(w.Transducer.beam_search)
    assert list(plain.parameters) == list(sig.parameters)
    assert (sig.parameters["beam_size"].default, sig.parameters["ctc_weight"].default,
            sig.parameters["transducer_weight"].default) == (5, 0.0, 1.0)
    assert (plain.parameters["ctc_weight"].default, plain.parameters["transducer_weight"].default) == (0.3, 0.7)
    assert "skips" in w.Transducer.tdt_beam_search.__doc__          # why the defaults differ
    sig = inspect.signature(w.Transducer.tdt_beam_search_batch)
    assert (sig.parameters["ctc_weight"].default, sig.parameters["transducer_weight"].default) == (0.0, 1.0)
    rescoring = list(inspect.signature(w.Transducer.transducer_attention_rescoring).parameters)
    rescoring.remove("beam_search_type")
    assert list(inspect.signature(w.Transducer.tdt_attention_rescoring).parameters) == rescoring
    assert list(inspect.signature(w.Transducer._cal_tdt_score).parameters) == list(
        inspect.signature(w.Transducer._cal_transducer_score).parameters)


def test_a_plain_model_refuses_the_tdt_methods():
    m = _model()
    speech, lens = torch.zeros(1, 5, 8), torch.tensor([5], dtype=torch.int32)
    with pytest.raises(ValueError, match=r"tdt_beam_search: the model has no tdt_durations \(use beam_search\)"):
        m.tdt_beam_search(speech, lens)
    with pytest.raises(ValueError, match=r"tdt_beam_search_batch: the model has no tdt_durations"):
        m.tdt_beam_search_batch(speech, lens)
    with pytest.raises(ValueError, match=r"tdt_attention_rescoring: the model has no tdt_durations \(use "
                                         r"transducer_attention_rescoring\)"):
        m.tdt_attention_rescoring(speech, lens, 4)


def test_the_plain_beam_methods_still_refuse_a_tdt_model():
    m = _model(26, tdt_durations=(0, 1, 2))
    speech, lens = torch.zeros(1, 5, 8), torch.tensor([5], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="TDT"):
        m.beam_search(speech, lens)
    with pytest.raises(NotImplementedError, match="TDT"):
        m.transducer_attention_rescoring(speech, lens, 4, beam_search_type="transducer")
    with pytest.raises(NotImplementedError, match="reads every joiner column as a token"):
        m._refuse_tdt("beam_search")
