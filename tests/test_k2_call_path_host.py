"""What the k2 RNN-T losses ask of the library: one path, whatever the lattice arguments.  No GPU and no library:
tests/joint_call_trace.py's recorder stands in for it (CPU tensors; `_lib.load`, `_lib.current_stream` and
`torch.cuda.device` replaced), and the family's one device check, `rnnt_lattice.require_device`, is replaced as well.

Every case runs forward and backward.  The record must be, to the letter: the scratch query (the simple loss's when both
scales are 0), the RNN-T workspace query, `wr_rnnt_smoothed_stats`, `wr_rnnt_lattice_sweeps`, and the
`wr_rnnt_smoothed_grad_lattice` calls; for the pruned loss `wr_rnnt_pruned_stats`, `wr_rnnt_lattice_sweeps`,
`wr_rnnt_pruned_grad_lattice`; for the ranges `wr_rnnt_prune_ranges_cols`.  The plain twins are never reached.  The
pruned node runs on CPU tensors under these seams like the others, so its record is complete."""
import itertools

import pytest
import torch

import joint_call_trace as tr

B, T, U, V, R = 2, 5, 3, 7, 2
U1 = U + 1
WS = tr.WS_BYTES
BOUNDARY = [[0, 0, 3, 5], [0, 0, 2, 4]]
LATTICES = [("regular", 0.0), ("regular", 0.01), ("modified", 0.01)]
SCALES = [None, (0.25, 0.0), (0.1, 0.1)]                      # None: rnnt_loss_simple
PLAIN_TWINS = {"wr_rnnt_simple_stats", "wr_rnnt_simple_grad", "wr_rnnt_smoothed_grad", "wr_rnnt_pruned_grad",
               "wr_rnnt_prune_ranges", "wr_rnnt_loss_sweeps", "wr_rnnt_export_lattice"}


def _record(fn):
    """The calls `fn(pkg)` makes under the seams; no case reaches a plain twin."""
    import wenet_celoss_amd as pkg
    rec = tr._Recorder(pkg._lib.SIGNATURES, 1007, 1009)       # no scalar here is renamed
    check = pkg.rnnt_lattice.require_device
    pkg.rnnt_lattice.require_device = lambda what, who, *tensors: None
    try:
        with tr._seams(pkg._lib, pkg.joint, rec, "library", True):
            fn(pkg)
    finally:
        pkg.rnnt_lattice.require_device = check
    assert not {c["name"] for c in rec.calls} & PLAIN_TWINS
    return rec.calls


def _call(name, scalars, null):
    return {"name": name, "scalars": list(scalars), "null": list(null)}


def _additive_inputs():
    g = torch.Generator().manual_seed(0)
    lm = torch.randn(B, U1, V, generator=g).requires_grad_()
    am = torch.randn(B, T, V, generator=g).requires_grad_()
    return lm, am, torch.randint(1, V, (B, U), generator=g), torch.tensor(BOUNDARY)


@pytest.mark.parametrize("scales,lattice,return_grad", list(itertools.product(SCALES, LATTICES, (False, True))))
def test_additive_losses_take_the_one_path(scales, lattice, return_grad):
    from wenet_celoss_amd import _lib
    rnnt_type, pen = lattice
    ll, la = scales or (0.0, 0.0)
    lat = _lib.LATTICES[rnnt_type]
    default = lattice == ("regular", 0.0)

    def run(pkg):
        lm, am, symbols, boundary = _additive_inputs()
        mod = pkg if default else pkg.k2                     # the package-level form for the defaults
        kw = {} if default else {"rnnt_type": rnnt_type, "delay_penalty": pen}
        if scales is None:
            out = mod.rnnt_loss_simple(lm, am, symbols, 0, boundary, "sum", return_grad, **kw)
        else:
            out = mod.rnnt_loss_smoothed(lm, am, symbols, 0, ll, la, boundary, "sum", return_grad, **kw)
        if return_grad:
            px_grad, py_grad = out[1]
            assert px_grad.shape == (B, U, T if rnnt_type == "modified" else T + 1) and py_grad.shape == (B, U1, T)
        (out[0] if return_grad else out).backward()
        assert lm.grad.shape == lm.shape and am.grad.shape == am.shape

    simple = ll == 0.0 and la == 0.0
    grad_scalars = [B, T, U1, V, 0, ll, la, lat, WS, WS]
    want = [_call("wr_rnnt_simple_workspace_bytes" if simple else "wr_rnnt_smoothed_workspace_bytes", [B, T, U1, V], []),
            _call("wr_rnnt_workspace_bytes", [B, T, U1], []),
            _call("wr_rnnt_smoothed_stats", [B, T, U1, V, 0, ll, la, WS, WS], [16]),
            _call("wr_rnnt_lattice_sweeps", [B, T, U1, lat, pen, WS], [10])]
    early = return_grad and la == 0.0
    if return_grad:     # grad_costs (13) null, both occupancies given, d_am / d_lm (14, 15) iff the gradient is taken early
        want.append(_call("wr_rnnt_smoothed_grad_lattice", grad_scalars, [13, 22] if early else [13, 14, 15, 22]))
    if not early:       # backward: grad_costs given, the occupancies (16, 17) null
        want.append(_call("wr_rnnt_smoothed_grad_lattice", grad_scalars, [16, 17, 22]))
    assert _record(run) == want


@pytest.mark.parametrize("lattice", LATTICES)
def test_pruned_loss_and_ranges_take_the_one_path(lattice):
    from wenet_celoss_amd import _lib
    rnnt_type, pen = lattice
    lat = _lib.LATTICES[rnnt_type]
    kw = {} if lattice == ("regular", 0.0) else {"rnnt_type": rnnt_type, "delay_penalty": pen}
    g = torch.Generator().manual_seed(1)
    symbols, boundary = torch.randint(1, V, (B, U), generator=g), torch.tensor(BOUNDARY)

    def loss(pkg):
        logits = torch.randn(B, T, R, V, generator=g).requires_grad_()
        ranges = torch.zeros(B, T, R, dtype=torch.int64) + torch.arange(R)
        pkg.k2.rnnt_loss_pruned(logits, symbols, ranges, 0, boundary, "sum", **kw).backward()
        assert logits.grad.shape == logits.shape

    dims = [_lib.WR_F32, B, T, U1, R, V, 0]
    assert _record(loss) == [_call("wr_rnnt_workspace_bytes", [B, T, U1], []),
                             _call("wr_rnnt_pruned_stats", dims + [WS], [14]),
                             _call("wr_rnnt_lattice_sweeps", [B, T, U1, lat, pen, WS], [10]),
                             _call("wr_rnnt_pruned_grad_lattice", dims + [lat, pen, WS], [18])]

    px_cols = T if rnnt_type == "modified" else T + 1

    def ranges(pkg):
        fn = pkg.get_rnnt_prune_ranges if rnnt_type == "regular" else pkg.k2.get_rnnt_prune_ranges
        out = fn(torch.rand(B, U, px_cols, generator=g), torch.rand(B, U1, T, generator=g), boundary, R)
        assert out.shape == (B, T, R) and out.dtype == torch.int64

    assert _record(ranges) == [_call("wr_rnnt_prune_ranges_cols", [px_cols, B, T, U1, R], [10])]

