"""CPU checks of the float16 joiner mode and of the autocast-following precision: how "f16" / "autocast" resolve, which
calls refuse them, when the fused joiner + loss node is taken, and that a build exports the new entry points (no
compute calls here -- this runs without a GPU)."""
import ctypes
import re

import pytest
import torch


def test_effective_precision_table():
    """(precision, autocast enabled, autocast dtype) -> the mode the call runs in: all 2 x 3 combinations of the new
    names, and the existing names unchanged by autocast."""
    from wenet_celoss_amd.joint import effective_precision as eff
    assert eff("f16", False, None) == "f16"
    assert eff("f16", True, torch.bfloat16) == "f16"
    assert eff("f16", True, torch.float16) == "f16"
    assert eff("autocast", False, None) == "fp32"
    assert eff("autocast", False, torch.float16) == "fp32"      # autocast off: the dtype setting does not matter
    assert eff("autocast", True, torch.bfloat16) == "bf16"
    assert eff("autocast", True, torch.float16) == "f16"
    for p in ("fp32", "bf16x3", "bf16"):
        for on, dt in ((False, None), (True, torch.bfloat16), (True, torch.float16)):
            assert eff(p, on, dt) == p


def test_new_names_accepted(monkeypatch):
    from wenet_celoss_amd import joint as jm
    monkeypatch.delenv("WR_JOINT_PRECISION", raising=False)
    assert jm._resolve_precision(None) == "fp32"                 # the default stays exact fp32
    assert jm._resolve_precision("f16") == "f16"
    assert jm._resolve_precision("autocast") == "autocast"
    monkeypatch.setenv("WR_JOINT_PRECISION", "autocast")
    assert jm._resolve_precision(None) == "autocast"
    assert jm._call_precision(None) == "fp32"                     # no autocast active here
    monkeypatch.setenv("WR_JOINT_PRECISION", "f16")
    assert jm._call_precision(None) == "f16"
    with pytest.raises(ValueError, match="precision"):
        jm._resolve_precision("fp16")


def _cuda_autocast_state(monkeypatch, enabled, dtype):
    """What torch.is_autocast_enabled / get_autocast_dtype report inside `torch.autocast("cuda", dtype)` -- the state the
    resolution reads -- without a device."""
    real_on, real_dt = torch.is_autocast_enabled, torch.get_autocast_dtype

    def on(*a):
        return enabled if a == ("cuda",) else real_on(*a)

    def dt(device_type):
        return dtype if device_type == "cuda" else real_dt(device_type)
    monkeypatch.setattr(torch, "is_autocast_enabled", on)
    monkeypatch.setattr(torch, "get_autocast_dtype", dt)


def _ragged_inputs(B=2, T=5, U=3, J=8, V=11):
    ep = torch.zeros(B, T, J)
    pp = torch.zeros(B, U + 1, J)
    w = torch.zeros(V, J)
    b = torch.zeros(V)
    y = torch.ones(B, U, dtype=torch.int32)
    ll = torch.tensor([T, T - 1], dtype=torch.int32)
    tl = torch.tensor([U, U - 1], dtype=torch.int32)
    return ep, pp, w, b, y, ll, tl


@pytest.mark.parametrize("precision,autocast_dtype", [("bf16", None), ("f16", None), ("f16", torch.float16),
                                                      ("autocast", torch.float16), ("autocast", torch.bfloat16)])
def test_joint_rnnt_loss_refuses_16bit_modes(monkeypatch, precision, autocast_dtype):
    """joint_rnnt_loss keeps fp32 logits inside the node: "f16", and "autocast" under autocast, get the message "bf16"
    gets -- before anything touches a device."""
    import wenet_celoss_amd as w
    if autocast_dtype is not None:
        _cuda_autocast_state(monkeypatch, True, autocast_dtype)
    ep, pp, W, b, y, ll, tl = _ragged_inputs()
    with pytest.raises(ValueError, match="AMP single-term mode keeps 16-bit logits"):
        w.joint_rnnt_loss(ep, pp, W, b, y, ll, tl, precision=precision)


def test_joint_rnnt_loss_takes_autocast_outside_autocast():
    """"autocast" outside autocast is "fp32": accepted, and the call gets as far as the device check."""
    import wenet_celoss_amd as w
    ep, pp, W, b, y, ll, tl = _ragged_inputs()
    with pytest.raises(RuntimeError) as e:
        w.joint_rnnt_loss(ep, pp, W, b, y, ll, tl, precision="autocast", buckets=1)
    assert "16-bit logits" not in str(e.value)


def _transducer(precision):
    import wenet_celoss_amd as w
    V, E = 11, 8
    m = w.Transducer.__new__(w.Transducer)
    torch.nn.Module.__init__(m)
    m.joint = w.TransducerJoint(V, E, E, E, precision=precision)
    m.fused_loss = True
    return m


@pytest.mark.parametrize("precision,autocast_dtype,fuse", [
    ("fp32", None, True), ("bf16", None, False), ("f16", None, False), ("f16", torch.float16, False),
    ("autocast", None, True), ("autocast", torch.float16, False), ("autocast", torch.bfloat16, False),
    ("fp32", torch.float16, True)])
def test_can_fuse_loss(monkeypatch, precision, autocast_dtype, fuse):
    """Transducer._can_fuse_loss: "autocast" fuses only while autocast is off at that call; "f16" never fuses."""
    if autocast_dtype is not None:
        _cuda_autocast_state(monkeypatch, True, autocast_dtype)
    assert _transducer(precision)._can_fuse_loss() is fuse


def test_can_fuse_loss_follows_the_environment(monkeypatch):
    monkeypatch.setenv("WR_JOINT_PRECISION", "autocast")
    m = _transducer(None)
    assert m._can_fuse_loss()
    _cuda_autocast_state(monkeypatch, True, torch.float16)
    assert not m._can_fuse_loss()


NEW_SYMBOLS = ("wr_joint_fwd_f16", "wr_joint_bwd_dz_f16", "wr_joint_bwd_dw_f16")


def test_new_symbols_declared_bound_and_exported():
    """A fresh build exports the f16 entry points; the header declares them; _lib binds them; the API version is still 3
    (no existing signature changed)."""
    import os
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    text = open(os.path.join(_lib._INCLUDE, "wr_api.h")).read()
    assert int(re.search(r"#define\s+WR_API_VERSION\s+(\d+)", text).group(1)) == 3 == _lib.API_VERSION
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", text), s
        assert s in _lib.SIGNATURES, s
        assert hasattr(lib, s), s


def test_new_entry_points_reject_bad_arguments_without_launch():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    rc = lib.wr_joint_fwd_f16(null, null, null, null, null, null, 1, 2, 3, 8, 16, 0, null, 0, null, 0, null)
    assert rc == -1 and b"null" in lib.wr_last_error()
    rc = lib.wr_joint_fwd_f16(null, null, null, null, null, null, 1, 2, 3, 6, 16, 0, null, 0, null, 0, null)
    assert rc == -2 and b"join_dim" in lib.wr_last_error()
    rc = lib.wr_joint_bwd_dz_f16(null, 2, null, null, null, null, null, 1, 2, 3, 8, 64, 0, null, null, null, 0, null)
    assert rc == -1 and b"WR_F16" in lib.wr_last_error()          # a bf16 gradient is not an f16-kernel input
    rc = lib.wr_joint_bwd_dz_f16(null, 1, null, null, null, null, null, 1, 2, 3, 8, 60, 0, null, null, null, 0, null)
    assert rc == -2 and b"multiple of 8" in lib.wr_last_error()   # f16 gradient rows: 16-byte aligned
    rc = lib.wr_joint_bwd_dw_f16(null, 2, null, null, null, 1, 2, 3, 8, 64, null, null, null, 0, null)
    assert rc == -1 and b"WR_F16" in lib.wr_last_error()
    rc = lib.wr_joint_bwd_dw_f16(null, 0, null, null, null, 1, 2, 3, 8, 66, null, null, null, 0, null)
    assert rc == -2
