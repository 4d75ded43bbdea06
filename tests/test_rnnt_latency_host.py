"""FastEmit and the delay penalty of the full-lattice loss, the parts that need no GPU: argument checks in Python (raised
before the "no CPU path" error), the new symbols, and the library's own rejections before any launch."""
import ctypes
import inspect
import pickle

import pytest
import torch

import wenet_celoss_amd as w
from wenet_celoss_amd import _lib

BAD = [-0.1, float("nan"), float("inf"), float("-inf"), "x", None]
NEW = ["wr_rnnt_loss_fwd_lattice", "wr_rnnt_loss_fwd_from_lse_lattice", "wr_rnnt_loss_bwd_lattice",
       "wr_joint_rnnt_grad_lattice"]


def loss_args(B=2, T=3, U=2, V=5):
    return (torch.zeros(B, T, U + 1, V), torch.ones(B, U, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32),
            torch.full((B,), U, dtype=torch.int32))


def fused_args(B=2, T=3, U=2, V=5, J=8):
    return (torch.zeros(B, T, J), torch.zeros(B, U + 1, J), torch.zeros(V, J), torch.zeros(V),
            torch.ones(B, U, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32),
            torch.full((B,), U, dtype=torch.int32))


@pytest.mark.parametrize("key", ["fastemit_lambda", "delay_penalty"])
@pytest.mark.parametrize("bad", BAD)
def test_bad_values_raise_value_error_before_the_device_check(key, bad):
    with pytest.raises(ValueError, match=key):
        w.rnnt_loss(*loss_args(), blank=0, **{key: bad})
    with pytest.raises(ValueError, match=key):
        w.joint_rnnt_loss(*fused_args(), **{key: bad})
    with pytest.raises(ValueError, match=key):
        w.joint_rnnt_loss(*fused_args(), logits_budget=1 << 20, **{key: bad})
    with pytest.raises(ValueError, match=key):
        w.RNNTLoss(**{key: bad})


def test_good_values_reach_the_device_check():
    for kw in ({}, {"fastemit_lambda": 0.01}, {"delay_penalty": 0.003}, {"fastemit_lambda": 0.5, "delay_penalty": 0.5}):
        with pytest.raises(RuntimeError, match="no CPU path"):
            w.rnnt_loss(*loss_args(), blank=0, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            w.joint_rnnt_loss(*fused_args(), **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            w.joint_rnnt_loss(*fused_args(), logits_budget=1 << 20, **kw)
        with pytest.raises(RuntimeError, match="no CPU path"):
            w.RNNTLoss(blank=0, **kw)(*loss_args())


def test_keywords_are_keyword_only_and_default_to_zero():
    for fn in (w.rnnt_loss, w.joint_rnnt_loss):
        p = inspect.signature(fn).parameters
        for key in ("fastemit_lambda", "delay_penalty"):
            assert p[key].kind is inspect.Parameter.KEYWORD_ONLY and p[key].default == 0.0
    p = inspect.signature(w.Transducer.__init__).parameters
    assert p["fastemit_lambda"].default == 0.0 and p["rnnt_delay_penalty"].default == 0.0
    assert "FastEmit" in w.rnnt_loss.__doc__ and "bit-identical" in w.rnnt_loss.__doc__


class _Enc(torch.nn.Module):
    def output_size(self):
        return 8


def _model(**kw):
    joint = w.TransducerJoint(5, 8, 8, 8)
    return w.Transducer(5, 0, _Enc(), torch.nn.Identity(), joint, **kw)


@pytest.mark.parametrize("key", ["fastemit_lambda", "rnnt_delay_penalty"])
@pytest.mark.parametrize("bad", BAD)
def test_transducer_rejects_bad_values(key, bad):
    with pytest.raises(ValueError):
        _model(**{key: bad})


def test_transducer_passes_the_options_to_the_full_lattice_term_only():
    m = _model(fastemit_lambda=0.01, rnnt_delay_penalty=0.003)
    assert m._latency_kwargs() == {"fastemit_lambda": 0.01, "delay_penalty": 0.003}
    assert m._lattice_kwargs() == {}                       # the k2 losses' own keywords are untouched
    assert _model()._latency_kwargs() == {}
    # the k2 keyword keeps its meaning and its refusal without a simple loss
    with pytest.raises(ValueError, match="simple_loss_weight"):
        _model(delay_penalty=0.1)
    # a model pickled before the options existed loads with both at 0
    old = _model()
    del old.fastemit_lambda, old.rnnt_delay_penalty
    again = pickle.loads(pickle.dumps(old))
    assert not hasattr(again, "fastemit_lambda") and again._latency_kwargs() == {}
    loss = w.RNNTLoss()
    del loss.fastemit_lambda, loss.delay_penalty
    with pytest.raises(RuntimeError, match="no CPU path"):
        loss(*loss_args())


def test_transducer_compute_loss_hands_the_options_to_every_route(monkeypatch):
    """plain, AMP-bucketed and fused / bounded routes of compute_loss"""
    from wenet_celoss_amd import transducer as tr
    seen = []

    def fake_rnnt(logits, *a, **kw):
        seen.append(("rnnt_loss", kw))
        costs = torch.zeros(logits.shape[0])
        return costs if kw.get("reduction") == "none" else costs.mean()

    def fake_fused(*a, **kw):
        seen.append(("joint_rnnt_loss", kw))
        return torch.zeros(())

    monkeypatch.setattr(tr, "rnnt_loss", fake_rnnt)
    monkeypatch.setattr(tr, "joint_rnnt_loss", fake_fused)
    m = _model(fastemit_lambda=0.25, rnnt_delay_penalty=0.5)
    monkeypatch.setattr(type(m.joint), "forward", lambda self, e, p, *a: torch.zeros(e.shape[0], e.shape[1], p.shape[1], 5))
    enc, pred = torch.zeros(2, 4, 8), torch.zeros(2, 3, 8)
    text, tl, el = torch.ones(2, 2, dtype=torch.long), torch.tensor([2, 1]), torch.tensor([4, 3])
    monkeypatch.setattr(type(m), "_can_fuse_loss", lambda self: True)
    m.compute_loss(enc, el, pred, text, tl)
    m.logits_budget = 1 << 20
    m.compute_loss(enc, el, pred, text, tl)
    monkeypatch.setattr(type(m), "_can_fuse_loss", lambda self: False)
    m.logits_budget = None
    m.fused_loss = False
    m.compute_loss(enc, el, pred, text, tl)                 # plain two-op route
    m.fused_loss = True
    monkeypatch.setattr(tr, "plan_buckets", lambda *a, **k: [[0], [1]])
    m.compute_loss(enc, el, pred, text, tl)                 # AMP route: label-length groups, rnnt_loss per group
    assert [n for n, _ in seen] == ["joint_rnnt_loss", "joint_rnnt_loss", "rnnt_loss", "rnnt_loss", "rnnt_loss"]
    for _, kw in seen:
        assert kw["fastemit_lambda"] == 0.25 and kw["delay_penalty"] == 0.5
    assert seen[1][1]["logits_budget"] == 1 << 20
    # the defaults hand nothing new over
    seen.clear()
    m0 = _model()
    m0.fused_loss = False
    m0.compute_loss(enc, el, pred, text, tl)
    assert "fastemit_lambda" not in seen[0][1] and "delay_penalty" not in seen[0][1]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_new_symbols_exist_and_are_bound(lib):
    for name in NEW:
        assert hasattr(lib, name) and name in _lib.SIGNATURES


NULL = None
PTR = ctypes.c_void_p(0x100000)          # never dereferenced: every call below is rejected before a launch


def fwd(lib, lat=0, dp=0.0, B=2):
    return lib.wr_rnnt_loss_fwd_lattice(PTR, 0, PTR, PTR, PTR, B, 4, 3, 8, 0, lat, dp, PTR, PTR, 0, NULL)


def fwd_lse(lib, lat=0, dp=0.0, B=2):
    return lib.wr_rnnt_loss_fwd_from_lse_lattice(PTR, PTR, PTR, PTR, B, 4, 3, 8, 0, lat, dp, PTR, PTR, 0, NULL)


def bwd(lib, lat=0, dp=0.0, lam=0.0, B=2):
    return lib.wr_rnnt_loss_bwd_lattice(PTR, 0, PTR, PTR, PTR, B, 4, 3, 8, 0, -1.0, lat, dp, lam, PTR, PTR, PTR, 0, NULL)


def jgrad(lib, lat=0, dp=0.0, lam=0.0, B=2):
    return lib.wr_joint_rnnt_grad_lattice(PTR, PTR, PTR, PTR, PTR, PTR, PTR, B, 4, 3, 8, 8, 0, 0, -1.0, 3, lat, dp, lam, PTR,
                                          PTR, 0, 0, 1, PTR, PTR, 0, 0, NULL)


WR_EINVAL, WR_EUNSUPPORTED, WR_EWORKSPACE = -1, -2, -3


@pytest.mark.parametrize("call", [fwd, fwd_lse, bwd, jgrad])
def test_library_rejects_bad_values_before_any_launch(lib, call):
    name = call.__name__
    for dp in (-0.5, float("nan"), float("inf")):
        assert call(lib, dp=dp) == WR_EINVAL
        assert b"delay_penalty" in lib.wr_last_error()
    if call in (bwd, jgrad):
        for lam in (-0.01, float("nan"), float("inf")):
            assert call(lib, lam=lam) == WR_EINVAL, name
            assert b"fastemit_lambda" in lib.wr_last_error()
    assert call(lib, lat=1) == WR_EUNSUPPORTED                     # the modified lattice: accepted as a code, not built
    assert b"regular lattice" in lib.wr_last_error()
    assert call(lib, lat=1, dp=0.5) == WR_EUNSUPPORTED
    assert call(lib, lat=2) == WR_EINVAL and b"lattice type" in lib.wr_last_error()
    assert call(lib, lat=-1) == WR_EINVAL
    # good values get as far as the plain entry point's own checks (here: the workspace size), under the new name
    for kw in ({}, {"dp": 0.5}):
        assert call(lib, **kw) == WR_EWORKSPACE
        assert lib.wr_last_error().decode().startswith(call_name(call))
    assert call(lib, B=0) == WR_EINVAL


def call_name(call):
    return {"fwd": "rnnt_loss_fwd_lattice", "fwd_lse": "rnnt_loss_fwd_from_lse_lattice", "bwd": "rnnt_loss_bwd_lattice",
            "jgrad": "joint_rnnt_grad_lattice"}[call.__name__]


def test_a_penalty_needs_the_prepare_kernels_position_count(lib):
    # B * (T + U1 - 1) * U1 >= 2^31 with B * T * U1 < 2^31: only the call with a penalty refuses it, before pass 1
    args = (PTR, 0, PTR, PTR, PTR, 1025, 1 << 10, 1024, 8, 0, 0)
    assert lib.wr_rnnt_loss_fwd_lattice(*args, 0.5, PTR, PTR, 0, NULL) == WR_EUNSUPPORTED
    assert b"positions" in lib.wr_last_error()
    assert lib.wr_rnnt_loss_fwd_lattice(*args, 0.0, PTR, PTR, 0, NULL) == WR_EWORKSPACE
