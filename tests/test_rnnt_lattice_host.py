"""CPU-side checks of ``rnnt_type=`` / ``delay_penalty=`` on the k2 losses (the k2-signature functions of
`wenet_celoss_amd.k2`; the package-level `rnnt_loss_simple`, `rnnt_loss_smoothed` and `get_rnnt_prune_ranges` keep the
signatures their own tests pin): bad values are refused before the device check, the px_grad shape rules of get_rnnt_prune_ranges, the Transducer's use of the two arguments, and the new entry
points' argument validation (no launch)."""
import ctypes

import numpy as np
import pytest
import torch


def _inputs(B=2, T=5, U=3, V=7):
    g = torch.Generator().manual_seed(0)
    lm, am = torch.randn(B, U + 1, V, generator=g), torch.randn(B, T, V, generator=g)
    symbols = torch.randint(1, V, (B, U), generator=g)
    return lm, am, symbols


def _losses():
    import wenet_celoss_amd as w
    from wenet_celoss_amd.rnnt_pruned import rnnt_pruned_lattice
    from wenet_celoss_amd.rnnt_simple import rnnt_simple_lattice
    from wenet_celoss_amd.rnnt_smoothed import rnnt_smoothed_lattice
    lm, am, symbols = _inputs()
    logits = torch.randn(2, 5, 2, 7)
    ranges = torch.zeros(2, 5, 2, dtype=torch.int64) + torch.arange(2)
    return [
        lambda **kw: w.k2.rnnt_loss_simple(lm, am, symbols, 0, **kw),
        lambda **kw: w.k2.rnnt_loss_smoothed(lm, am, symbols, 0, 0.25, 0.0, **kw),
        lambda **kw: w.rnnt_loss_pruned(logits, symbols, ranges, 0, **kw),
        lambda **kw: rnnt_simple_lattice(lm, am, symbols, 0, **kw),
        lambda **kw: rnnt_smoothed_lattice(lm, am, symbols, 0, **kw),
        lambda **kw: rnnt_pruned_lattice(logits, symbols, ranges, 0, **kw),
    ]


@pytest.mark.parametrize("i", range(6))
def test_bad_lattice_arguments_are_refused_before_the_device_check(i):
    fn = _losses()[i]
    with pytest.raises(NotImplementedError, match="constrained"):
        fn(rnnt_type="constrained")
    for bad in ("Modified", "", "simple", None, 1):
        with pytest.raises(ValueError, match="rnnt_type"):
            fn(rnnt_type=bad)
    for bad in (-0.01, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(ValueError, match="delay_penalty"):
            fn(delay_penalty=bad)
        with pytest.raises(ValueError, match="delay_penalty"):
            fn(rnnt_type="modified", delay_penalty=bad)
    # good values get as far as the device check: these are CPU tensors
    for kw in (dict(rnnt_type="modified"), dict(delay_penalty=0.003), dict(rnnt_type="regular", delay_penalty=0.0)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            fn(**kw)


def test_the_keywords_are_keyword_only_and_the_positional_signatures_are_k2s():
    import inspect
    import wenet_celoss_amd as w
    want = {
        "rnnt_loss_simple": ["lm", "am", "symbols", "termination_symbol", "boundary", "reduction", "return_grad"],
        "rnnt_loss_smoothed": ["lm", "am", "symbols", "termination_symbol", "lm_only_scale", "am_only_scale", "boundary",
                               "reduction", "return_grad"],
        "rnnt_loss_pruned": ["logits", "symbols", "ranges", "termination_symbol", "boundary", "reduction"],
    }
    for name, positional in want.items():
        ps = inspect.signature(getattr(w.k2, name)).parameters
        assert [n for n, p in ps.items() if p.kind == p.POSITIONAL_OR_KEYWORD] == positional
        assert ps["rnnt_type"].kind == ps["delay_penalty"].kind == inspect.Parameter.KEYWORD_ONLY
        assert ps["rnnt_type"].default == "regular" and ps["delay_penalty"].default == 0.0
        # the package-level function has the same positional parameters, with the same defaults
        top = inspect.signature(getattr(w, name)).parameters
        assert [(n, top[n].default) for n in positional] == [(n, ps[n].default) for n in positional]
    assert w.k2.rnnt_loss_pruned is w.rnnt_loss_pruned and w.k2.do_rnnt_pruning is w.do_rnnt_pruning
    assert list(inspect.signature(w.k2.get_rnnt_prune_ranges).parameters) == ["px_grad", "py_grad", "boundary", "s_range"]


def test_prune_ranges_px_grad_shape_rules():
    import wenet_celoss_amd as w
    B, U, T = 2, 4, 6
    py = torch.rand(B, U + 1, T)
    px_t, px_t1 = torch.rand(B, U, T), torch.rand(B, U, T + 1)
    for px in (torch.rand(B, U, T + 2), torch.rand(B, U, T - 1), torch.rand(B, U + 1, T), torch.rand(B + 1, U, T)):
        with pytest.raises(ValueError, match="does not match"):
            w.k2.get_rnnt_prune_ranges(px, py, None, 3)
    with pytest.raises(ValueError, match="at least 2"):          # the (B, U, T+1) form keeps its rule
        w.k2.get_rnnt_prune_ranges(px_t1, py, None, 1)
    with pytest.raises(ValueError, match="at least 1"):
        w.k2.get_rnnt_prune_ranges(px_t, py, None, 0)
    for px, s_range in ((px_t, 1), (px_t, 3), (px_t1, 2)):       # accepted: these get as far as the device check
        with pytest.raises(RuntimeError, match="no CPU path"):
            w.k2.get_rnnt_prune_ranges(px, py, None, s_range)
    with pytest.raises(ValueError, match="does not match"):      # the package-level function takes the regular form only
        w.get_rnnt_prune_ranges(px_t, py, None, 3)


class _Enc(torch.nn.Module):
    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)

    def output_size(self):
        return self.proj.out_features


def _model(**kw):
    import wenet_celoss_amd as w
    torch.manual_seed(0)
    return w.Transducer(23, 0, _Enc(8, 12), w.RNNPredictor(23, 10, 10, 0.0, 14, 2, dropout=0.0),
                        w.TransducerJoint(23, 12, 10, 16), ctc_weight=0.0, transducer_weight=1.0, **kw)


def test_transducer_lattice_arguments():
    m = _model(simple_loss_weight=0.5, prune_range=3, rnnt_type="modified", delay_penalty=0.01)
    assert m._lattice_kwargs() == {"rnnt_type": "modified", "delay_penalty": 0.01}
    assert _model(simple_loss_weight=0.5, rnnt_type="regular", delay_penalty=0.0)._lattice_kwargs() == {}
    assert _model()._lattice_kwargs() == {}
    before = set(_model(simple_loss_weight=0.5).state_dict().keys())
    assert set(m.state_dict().keys()) == before                 # no parameters of their own
    for kw in (dict(rnnt_type="modified"), dict(delay_penalty=0.01)):
        with pytest.raises(ValueError, match="simple_loss_weight"):     # the main loss is then the torchaudio-style one
            _model(**kw)
    with pytest.raises(NotImplementedError, match="constrained"):
        _model(simple_loss_weight=0.5, rnnt_type="constrained")
    with pytest.raises(ValueError, match="rnnt_type"):
        _model(simple_loss_weight=0.5, rnnt_type="other")
    with pytest.raises(ValueError, match="delay_penalty"):
        _model(simple_loss_weight=0.5, delay_penalty=-1.0)
    with pytest.raises(ValueError, match="delay_penalty"):
        _model(simple_loss_weight=0.5, delay_penalty=float("nan"))


def test_new_entry_points_reject_bad_arguments_without_launch():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    one = ctypes.c_void_p(256)          # a non-null pointer that is never dereferenced: every check precedes the launches
    big = 1 << 30

    def sweeps(B=2, T=4, U1=3, lat=1, dp=0.0, p=one, ws=big):
        return lib.wr_rnnt_lattice_sweeps(p, p, B, T, U1, lat, dp, p, p, ws, null)

    def export(B=2, T=4, U1=3, lat=1, p=one, ws=big):
        return lib.wr_rnnt_lattice_export(p, ws, p, p, B, T, U1, lat, p, p, null)

    def sgrad(lat=1, p=one, V=8):
        return lib.wr_rnnt_smoothed_grad_lattice(p, p, p, p, p, 2, 4, 3, V, 0, 0.25, 0.0, lat, null, p, p, null, null, p, big,
                                                 p, big, null)

    def pgrad(lat=1, dp=0.0, p=one, R=2):
        return lib.wr_rnnt_pruned_grad_lattice(p, 0, p, p, p, p, 2, 4, 3, R, 8, 0, lat, dp, null, p, p, big, null)

    def ranges(cols=4, p=one, R=2):
        return lib.wr_rnnt_prune_ranges_cols(p, cols, p, p, p, 2, 4, 3, R, p, null)

    for fn in (sweeps, export, sgrad, pgrad):
        assert fn(lat=2) == -1 and b"lattice type" in lib.wr_last_error()
        assert fn(lat=-1) == -1 and b"lattice type" in lib.wr_last_error()
        assert fn(p=null) == -1 and b"null" in lib.wr_last_error()
    for fn in (sweeps, pgrad):
        for dp in (-0.5, float("nan"), float("inf")):
            assert fn(dp=dp) == -1 and b"delay_penalty" in lib.wr_last_error()
    for fn in (sweeps, export):
        assert fn(U1=1100) == -2 and b"1024" in lib.wr_last_error()
        assert fn(B=0) == -1
        assert fn(ws=16) == -3 and b"workspace" in lib.wr_last_error()
    assert sgrad(V=1) == -1 and pgrad(R=4) == -1
    assert ranges(cols=3) == -1 and b"T + 1" in lib.wr_last_error()
    assert ranges(cols=6) == -1
    assert ranges(p=null) == -1 and b"null" in lib.wr_last_error()
    assert ranges(R=4) == -1


def test_general_entry_points_accept_what_the_plain_ones_accept_without_launch():
    """`wr_rnnt_lattice_sweeps(regular, 0)` takes every shape `wr_rnnt_loss_sweeps` takes: the bound on the skewed
    positions, B * (T + U1 - 1) * U1 < 2^31, belongs to the kernels of the other settings.  With both scales 0 the
    smoothed calls need the simple loss's scratch only.  Null data pointers: every check precedes the launches."""
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    one = ctypes.c_void_p(256)
    B, T, U1 = 2047, 1024, 1024
    assert B * T * U1 < 2 ** 31 <= B * (T + U1 - 1) * U1

    def sweeps(lat=0, dp=0.0):
        return lib.wr_rnnt_lattice_sweeps(null, null, B, T, U1, lat, dp, null, null, 0, null)

    assert sweeps() == -1 and b"null" in lib.wr_last_error()            # the shape passed
    assert lib.wr_rnnt_loss_sweeps(null, null, B, T, U1, null, null, 0, null) == -1 and b"null" in lib.wr_last_error()
    assert sweeps(lat=1) == -2 and b"2^31" in lib.wr_last_error()
    assert sweeps(dp=0.01) == -2 and b"2^31" in lib.wr_last_error()

    dims = (2, 5, 4, 7)
    simple = lib.wr_rnnt_simple_workspace_bytes(*dims)
    assert 0 < simple < lib.wr_rnnt_smoothed_workspace_bytes(*dims)

    def stats(ll, la, sws):                                # a null data pointer: the sizes are checked before it
        return lib.wr_rnnt_smoothed_stats(null, one, one, one, one, *dims, 0, ll, la, one, sws, one, 1 << 30, null)

    assert stats(0.0, 0.0, simple - 1) == -3 and b"workspace" in lib.wr_last_error()
    assert stats(0.0, 0.0, simple) == -1 and b"null" in lib.wr_last_error()
    assert stats(0.1, 0.1, simple) == -3 and b"workspace" in lib.wr_last_error()
