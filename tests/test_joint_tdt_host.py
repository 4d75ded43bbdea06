"""Host-side checks of the memory-bounded joiner + TDT loss: the three entry points' ABI and refusals, and the Python
function's argument validation.  No GPU is needed and none is used: every library call here is rejected before the first
HIP call."""
import ctypes
import re

import pytest
import torch

from conftest import ROOT

SYMBOLS = {
    "wr_joint_tdt_stats": 22,      # number of parameters in include/wr_api.h
    "wr_rnnt_tdt_sweeps": 11,
    "wr_joint_tdt_grad": 27,
}


def test_symbols_are_declared_exported_and_bound():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    text = open(ROOT + "/include/wr_api.h").read()
    assert "Joiner + TDT loss without a logits tensor" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s, nargs in SYMBOLS.items():
        m = re.search(r"\bint\s+" + s + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
        assert m, s
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == nargs, (s, params)
        assert hasattr(lib, s) and s in _lib.SIGNATURES
        res, argtypes = _lib.SIGNATURES[s]
        assert res is ctypes.c_int and len(argtypes) == nargs
        for p, a in zip(params, argtypes):              # every header parameter against its ctypes binding
            want = (ctypes.c_void_p if "*" in p else ctypes.c_double if p.startswith("double ") else
                    ctypes.c_size_t if p.startswith("size_t ") else ctypes.c_longlong if p.startswith("long long ") else
                    ctypes.c_int)
            assert a is want, (s, p, a)
    assert "joint_rnnt_tdt_loss" in __import__("wenet_celoss_amd").__all__


def test_library_rejects_bad_arguments_without_launch():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    p = ctypes.c_void_p(64)                # a non-null placeholder: no call below gets as far as reading it
    big = 1 << 40

    def durs(*d):
        return (ctypes.c_int32 * max(len(d), 1))(*d)

    def stats(B=2, T=4, U1=3, J=16, W=11, blank=0, d=(0, 1, 2), D=None, sigma=0.0, ptr=p, wsb=big, twsb=big, dptr=True):
        return lib.wr_joint_tdt_stats(ptr, ptr, ptr, ptr, ptr, ptr, ptr, B, T, U1, J, W, 0, blank, durs(*d) if dptr else null,
                                      len(d) if D is None else D, sigma, ptr, wsb, ptr, twsb, null)

    def grad(B=2, T=4, U1=3, J=16, W=11, blank=0, d=(0, 1, 2), D=None, sigma=0.0, ptr=p, wsb=big, twsb=big, dptr=True,
             cb=0, ce=24, gout=p):
        return lib.wr_joint_tdt_grad(ptr, ptr, ptr, ptr, ptr, ptr, ptr, B, T, U1, J, W, 0, blank, durs(*d) if dptr else null,
                                     len(d) if D is None else D, sigma, null, ptr, twsb, cb, ce, gout, ptr, wsb, 0, null)

    def sweeps(B=2, T=4, U1=3, d=(0, 1, 2), D=None, ptr=p, wsb=big, dptr=True):
        return lib.wr_rnnt_tdt_sweeps(ptr, ptr, B, T, U1, durs(*d) if dptr else null, len(d) if D is None else D, ptr, ptr,
                                      wsb, null)

    def err():
        return lib.wr_last_error()

    for fn, name in ((stats, b"joint_tdt_stats"), (grad, b"joint_tdt_grad"), (sweeps, b"rnnt_tdt_sweeps")):
        # the durations contract: the codes and texts of wr_rnnt_tdt_loss_fwd under this entry point's name
        assert fn(D=0) == -1 and b"durations" in err() and err().startswith(name)
        assert fn(d=tuple(range(9)), D=10) == -1 and b"durations" in err() and err().startswith(name)
        assert fn(d=(0, 2, 1)) == -1 and b"strictly increasing" in err() and err().startswith(name)
        assert fn(d=(1, 1)) == -1 and b"strictly increasing" in err()
        assert fn(d=(-1, 1)) == -1 and b"outside [0, 8]" in err() and err().startswith(name)
        assert fn(d=(0, 9)) == -1 and b"outside [0, 8]" in err()
        assert fn(d=(0,)) == -1 and b"at least one duration" in err() and err().startswith(name)
        assert fn(dptr=False) == -1 and b"durations is null" in err() and err().startswith(name)
        assert fn(B=0) == -1 and err().startswith(name)
        assert fn(ptr=null) == -1 and b"null" in err() and err().startswith(name)
        assert fn(U1=1100) == -2 and b"1024" in err() and err().startswith(name)
        assert fn(B=4000, T=4000, U1=1000) == -2 and b"2^31" in err() and err().startswith(name)
    for fn, name in ((stats, b"joint_tdt_stats"), (grad, b"joint_tdt_grad")):
        assert fn(W=4) == -1 and b"token columns" in err() and err().startswith(name)          # V = W - D = 1
        assert fn(W=3) == -1 and b"token columns" in err()                                     # V = 0
        assert fn(blank=8) == -1 and b"blank" in err() and err().startswith(name)              # V = 8
        assert fn(blank=-1) == -1 and b"blank" in err()
        assert fn(sigma=-1.0) == -1 and b"sigma" in err() and err().startswith(name)
        assert fn(sigma=float("nan")) == -1 and b"sigma" in err()
        assert fn(sigma=float("inf")) == -1 and b"sigma" in err()
        assert fn(twsb=16) == -3 and b"TDT workspace" in err() and err().startswith(name)
        assert fn(wsb=16) == -3 and b"workspace" in err() and err().startswith(name)
        assert fn(J=516) == -2 and b"join_dim" in err()
        # only the default forward kernel carries the TDT epilogues
        assert lib.wr_tune_set(5, 1) == 0
        try:
            assert fn() == -2 and b"wr_tune_set(5, 1)" in err() and err().startswith(name)
        finally:
            assert lib.wr_tune_set(5, 0) == 0
    assert sweeps(wsb=16) == -3 and b"workspace" in err() and err().startswith(b"rnnt_tdt_sweeps")
    # the cell range of the gradient: inside [0, B * T * U1] = [0, 24], not reversed
    assert grad(cb=-1) == -1 and b"cell range" in err() and err().startswith(b"joint_tdt_grad")
    assert grad(ce=25) == -1 and b"cell range" in err()
    assert grad(cb=8, ce=4) == -1 and b"cell range" in err()
    assert grad(gout=null) == -1 and b"null" in err()

    size = lib.wr_rnnt_tdt_workspace_bytes
    assert size(0, 4, 3, 3) == 0 and size(2, 4, 3, 0) == 0 and size(2, 4, 3, 10) == 0     # a bad shape: 0, as before
    assert size(2, 0, 3, 3) == 0 and size(2, 4, 0, 3) == 0
    assert size(2, 10, 5, 5) > 0


def _cpu_call(**kw):
    import wenet_celoss_amd as w
    args = dict(durations=(0, 1, 2), logits_budget=1 << 20)
    args.update(kw)
    durations = args.pop("durations")
    ep, pp = torch.zeros(1, 3, 8), torch.zeros(1, 2, 8)
    return w.joint_rnnt_tdt_loss(ep, pp, torch.zeros(10, 8), torch.zeros(10), torch.ones(1, 1, dtype=torch.int32),
                                 torch.tensor([3], dtype=torch.int32), torch.tensor([1], dtype=torch.int32), durations, **args)


def test_python_refusals_need_no_device():
    import wenet_celoss_amd as w
    with pytest.raises(ValueError, match="bf16x3"):
        _cpu_call(precision="bf16x3")
    with pytest.raises(ValueError, match="autocast"):
        _cpu_call(precision="autocast")
    # a budget below one frame row, stating U1 * W * 4 = 2 * 10 * 4 = 80
    with pytest.raises(ValueError, match=r"2 \* 10 \* 4 = 80"):
        _cpu_call(logits_budget=79)
    for bad in ((), (0,), (2, 1), (1, 1), (0, 9), (-1, 1), (0.0, 1.0), 3):
        with pytest.raises(ValueError, match="joint_rnnt_tdt_loss: .*duration"):
            _cpu_call(durations=bad)
    with pytest.raises(ValueError, match="sigma"):
        _cpu_call(sigma=-0.5)
    with pytest.raises(ValueError, match="blank"):
        _cpu_call(blank=7)                               # V = 10 - 3 = 7
    with pytest.raises(ValueError, match="reduction"):
        _cpu_call(reduction="average")
    with pytest.raises(ValueError, match="token columns"):
        _cpu_call(durations=tuple(range(9)))             # V = 1
    with pytest.raises(TypeError, match="logits_budget"):        # the budget is required
        w.joint_rnnt_tdt_loss(torch.zeros(1, 3, 8), torch.zeros(1, 2, 8), torch.zeros(10, 8), torch.zeros(10), None, None,
                              None, (0, 1, 2))
    with pytest.raises(RuntimeError, match="no CPU path"):
        _cpu_call()


def test_transducer_routing_predicates():
    """The bounded TDT node serves the fused fp32 joiner only; _can_fuse_loss stays False for a TDT model."""
    from test_rnnt_tdt_host import _model
    import wenet_celoss_amd as w
    m = _model(26, tdt_durations=(0, 1, 2))
    assert m._is_tdt() and not m._can_fuse_loss() and m._can_bound_tdt_loss()
    m.fused_loss = False
    assert not m._can_bound_tdt_loss()
    m.fused_loss = True
    m.joint = w.TransducerJoint(26, 12, 10, 16, precision="bf16x3")
    assert not m._can_bound_tdt_loss()
    plain = _model()
    assert plain._can_fuse_loss() and not plain._can_bound_tdt_loss()
