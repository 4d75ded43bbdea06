"""Host-side checks of the token-and-duration transducer (TDT) loss: argument validation in Python and in the library,
the ABI, and the Transducer options.  No GPU is needed and none is used: every library call here is rejected before the
first HIP call."""
import ctypes
import inspect
import pickle
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = ["wr_rnnt_tdt_workspace_bytes", "wr_rnnt_tdt_loss_fwd", "wr_rnnt_tdt_loss_bwd", "wr_rnnt_tdt_export_lattice"]


def _cpu_call(durations=(0, 1, 2), blank=0, sigma=0.0, V=6):
    import wenet_celoss_amd as w
    D = len(durations) if hasattr(durations, "__len__") else 1
    logits = torch.zeros(1, 2, 2, V + D)
    return w.rnnt_tdt_loss(logits, torch.ones(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
                           torch.tensor([1], dtype=torch.int32), durations, blank=blank, sigma=sigma)


@pytest.mark.parametrize("bad", [dict(durations=()), dict(durations=tuple(range(9)) + (9,)), dict(durations=(0, 9)),
                                 dict(durations=(-1, 1)), dict(durations=(1, 1)), dict(durations=(2, 1)),
                                 dict(durations=(0,)), dict(durations=(0.0, 1.0)), dict(durations=(True, 2)),
                                 dict(durations=3), dict(sigma=-0.1), dict(sigma=float("inf")), dict(sigma=float("nan")),
                                 dict(sigma="x"), dict(blank=6), dict(blank=-1), dict(blank=7), dict(blank=1.0)])
def test_bad_values_raise_value_error_before_the_device_check(bad):
    with pytest.raises(ValueError):
        _cpu_call(**bad)


@pytest.mark.parametrize("good", [dict(), dict(durations=(1,)), dict(durations=[0, 2]), dict(durations=tuple(range(9))),
                                  dict(durations=(8,)), dict(sigma=0.05), dict(blank=5)])
def test_good_values_reach_the_device_check(good):
    with pytest.raises(RuntimeError, match="no CPU path"):
        _cpu_call(**good)


def test_module_and_exports():
    import wenet_celoss_amd as w
    assert {"rnnt_tdt_loss", "TDTLoss", "rnnt_tdt_lattice"} <= set(w.__all__)
    mod = w.TDTLoss((0, 1, 2), blank=0, sigma=0.05, reduction="sum")
    assert mod.durations == (0, 1, 2) and mod.sigma == 0.05
    with pytest.raises(ValueError):
        w.TDTLoss((0,))
    with pytest.raises(ValueError):
        w.rnnt_tdt_loss(torch.zeros(1, 2, 2, 8), None, None, None, (0, 1), reduction="average")
    with pytest.raises(RuntimeError, match="no CPU path"):
        mod(torch.zeros(1, 2, 2, 9), torch.ones(1, 1, dtype=torch.int32), torch.tensor([2], dtype=torch.int32),
            torch.tensor([1], dtype=torch.int32))


def test_symbols_are_declared_exported_and_bound():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    text = open(ROOT + "/include/wr_api.h").read()
    assert "Token-and-duration transducer" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", text), s
        assert hasattr(lib, s) and s in _lib.SIGNATURES
    assert _lib.API_VERSION == 3 and lib.wr_api_version() == 3


def test_library_rejects_bad_arguments_without_launch():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    big = 1 << 40

    def durs(*d):
        return (ctypes.c_int32 * max(len(d), 1))(*d)

    def fwd(B=2, T=4, U1=3, V=8, blank=0, d=(0, 1, 2), D=None, sigma=0.0, wsb=big, dtype=0):
        return lib.wr_rnnt_tdt_loss_fwd(null, dtype, null, null, null, B, T, U1, V, blank, durs(*d),
                                        len(d) if D is None else D, sigma, null, null, wsb, null)

    def bwd(B=2, T=4, U1=3, V=8, blank=0, d=(0, 1, 2), D=None, sigma=0.0, wsb=big, dtype=0):
        return lib.wr_rnnt_tdt_loss_bwd(null, dtype, null, null, null, B, T, U1, V, blank, durs(*d),
                                        len(d) if D is None else D, sigma, null, null, null, wsb, null)

    for fn in (fwd, bwd):
        assert fn(D=0) == -1 and b"durations" in lib.wr_last_error()
        assert fn(d=tuple(range(9)), D=10) == -1 and b"durations" in lib.wr_last_error()
        assert fn(d=(0, 2, 1)) == -1 and b"strictly increasing" in lib.wr_last_error()
        assert fn(d=(1, 1)) == -1 and b"strictly increasing" in lib.wr_last_error()
        assert fn(d=(-1, 1)) == -1 and b"outside [0, 8]" in lib.wr_last_error()
        assert fn(d=(0, 9)) == -1 and b"outside [0, 8]" in lib.wr_last_error()
        assert fn(d=(0,)) == -1 and b"at least one duration" in lib.wr_last_error()
        assert fn(sigma=-1.0) == -1 and b"sigma" in lib.wr_last_error()
        assert fn(sigma=float("nan")) == -1 and b"sigma" in lib.wr_last_error()
        assert fn(blank=8) == -1 and b"blank" in lib.wr_last_error()
        assert fn(blank=-1) == -1 and b"blank" in lib.wr_last_error()
        assert fn(U1=1100) == -2 and b"1024" in lib.wr_last_error()
        assert fn(B=4000, T=4000, U1=1000) == -2 and b"2^31" in lib.wr_last_error()
        assert fn(B=0) == -1
        assert fn(dtype=7) == -1 and b"dtype" in lib.wr_last_error()
        assert fn(wsb=16) == -3 and b"workspace" in lib.wr_last_error()
        assert fn() == -1 and b"null" in lib.wr_last_error()
    # a null durations array
    assert lib.wr_rnnt_tdt_loss_fwd(null, 0, null, null, null, 2, 4, 3, 8, 0, null, 3, 0.0, null, null, big, null) == -1
    assert b"durations is null" in lib.wr_last_error()

    def export(B=2, T=4, U1=3, D=3, wsb=big):
        return lib.wr_rnnt_tdt_export_lattice(null, wsb, null, null, B, T, U1, D, null, null, null)

    assert export(D=0) == -1 and export(D=10) == -1
    assert export(U1=1100) == -2 and b"1024" in lib.wr_last_error()
    assert export(wsb=16) == -3 and b"workspace" in lib.wr_last_error()
    assert export() == -1 and b"null" in lib.wr_last_error()

    size = lib.wr_rnnt_tdt_workspace_bytes
    assert size(0, 4, 3, 3) == 0 and size(2, 4, 3, 0) == 0 and size(2, 4, 3, 10) == 0
    small, big_ws = size(2, 10, 5, 5), size(16, 1000, 151, 5)
    assert 0 < small < big_ws
    assert size(2, 10, 5, 1) < small                             # the duration arrays scale with D
    assert big_ws * 100 < 16 * 1000 * 151 * 5005 * 4             # far below the logits tensor


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


def test_transducer_options():
    import wenet_celoss_amd as w
    assert list(inspect.signature(w.Transducer.__init__).parameters)[-3:] == ["tdt_durations", "tdt_sigma",
                                                                               "simple_loss_weight"]
    m = _model(26, tdt_durations=[0, 1, 2], tdt_sigma=0.05)
    assert m.tdt_durations == (0, 1, 2) and m.tdt_sigma == 0.05 and m._is_tdt() and not m._can_fuse_loss()
    assert m.vocab_size == 23
    with pytest.raises(ValueError, match="26"):
        _model(23, tdt_durations=(0, 1, 2))                      # the joiner lacks the duration outputs
    with pytest.raises(ValueError):
        _model(26, tdt_durations=(0,))
    with pytest.raises(ValueError):
        _model(26, tdt_durations=(0, 1, 2), tdt_sigma=-1.0)
    with pytest.raises(ValueError, match="tdt_durations must be set"):
        _model(23, tdt_sigma=0.05)
    for extra in (dict(fastemit_lambda=0.01), dict(rnnt_delay_penalty=0.01), dict(context_bias=torch.nn.Identity()),
                  dict(prune_range=3, simple_loss_weight=0.5)):
        with pytest.raises(ValueError, match="cannot be combined"):
            _model(26, tdt_durations=(0, 1, 2), **extra)
    # a simple loss beside TDT keeps vocab_size
    m2 = _model(26, tdt_durations=(0, 1, 2), simple_loss_weight=0.5)
    assert m2.simple_am_proj.out_features == 23 and m2.simple_lm_proj.out_features == 23


def test_tdt_model_refuses_the_decoders_that_read_vocab_size_columns():
    m = _model(26, tdt_durations=(0, 1, 2))
    speech, lens = torch.zeros(1, 5, 8), torch.tensor([5], dtype=torch.int32)
    with pytest.raises(NotImplementedError, match="TDT"):
        m.beam_search(speech, lens)
    with pytest.raises(NotImplementedError, match="TDT"):
        m.transducer_attention_rescoring(speech, lens, 2, beam_search_type="transducer")
    with pytest.raises(NotImplementedError, match="TDT"):
        m.greedy_search_batch(speech, lens)
    with pytest.raises(NotImplementedError, match="TDT"):
        m.forward_greedy_search(torch.zeros(1, 4, 12), torch.tensor([4]))


def test_default_model_is_unchanged_and_pickles():
    m = _model()
    assert m.tdt_durations is None and m.tdt_sigma == 0.0 and not m._is_tdt()
    assert set(m.state_dict().keys()) == set(_model(tdt_durations=None).state_dict().keys())
    m2 = pickle.loads(pickle.dumps(m))
    assert not m2._is_tdt() and set(m2.state_dict().keys()) == set(m.state_dict().keys())
    del m2.__dict__["tdt_durations"], m2.__dict__["tdt_sigma"]       # a model pickled before the options existed
    assert not m2._is_tdt()
    m2._refuse_tdt("beam_search")
    t = pickle.loads(pickle.dumps(_model(26, tdt_durations=(0, 1, 2), tdt_sigma=0.05)))
    assert t.tdt_durations == (0, 1, 2) and t.tdt_sigma == 0.05
