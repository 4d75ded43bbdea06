"""Lattice types and the delay penalty of the k2 RNN-T losses: what ``rnnt_type=`` and ``delay_penalty=`` of
`k2.rnnt_loss_simple`, `k2.rnnt_loss_smoothed` (k2.py) and `rnnt_loss_pruned` route to (csrc/rnnt_lattice.hip; the
contract is in include/wr_api.h, "Lattice types and the delay penalty"; DESIGN.md, "Modified lattice and delay penalty").

  rnnt_type = "regular"    a label arc stays on its frame, (t,u) -> (t,u+1); a final blank leaves (T_b-1, U_b)
  rnnt_type = "modified"   a label arc consumes a frame, (t,u) -> (t+1,u+1): exactly one arc per frame, T_b >= U_b
  delay_penalty            ``delay_penalty * ((T_b - 1) / 2 - t)`` added to every label arc's log-probability

``"constrained"`` is not offered (NotImplementedError).  The defaults take the code path the functions had before these
arguments existed.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

from . import _lib


def check_lattice(what: str, rnnt_type, delay_penalty) -> Tuple[int, float]:
    """(wr_lattice code, penalty as float) or ValueError / NotImplementedError; needs no device."""
    if rnnt_type == "constrained":
        raise NotImplementedError(f"{what}: rnnt_type 'constrained' is not implemented (\"regular\" and \"modified\" are)")
    if not isinstance(rnnt_type, str) or rnnt_type not in _lib.LATTICES:
        raise ValueError(f"{what}: rnnt_type must be \"regular\" or \"modified\" (got {rnnt_type!r})")
    try:
        pen = float(delay_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: delay_penalty must be a number (got {delay_penalty!r})") from None
    if not (pen >= 0.0 and math.isfinite(pen)):
        raise ValueError(f"{what}: delay_penalty must be finite and not negative (got {delay_penalty})")
    return _lib.LATTICES[rnnt_type], pen


def is_default(lat: int, pen: float) -> bool:
    return lat == 0 and pen == 0.0


def occupancies_to_k2(occ_emit: torch.Tensor, occ_blank: torch.Tensor, lat: int):
    """(B, T, U+1) arc occupancies -> k2's (px_grad, py_grad): px_grad (B, U, T+1) with a zero last column for the
    regular lattice, (B, U, T) for the modified one; py_grad (B, U+1, T)."""
    B, T, U1 = occ_emit.shape
    if lat == _lib.LATTICES["modified"]:
        px_grad = occ_emit[:, :, :U1 - 1].transpose(1, 2).contiguous()
    else:
        px_grad = torch.zeros(B, U1 - 1, T + 1, dtype=torch.float32, device=occ_emit.device)
        px_grad[:, :, :T] = occ_emit[:, :, :U1 - 1].transpose(1, 2)
    return px_grad, occ_blank.transpose(1, 2).contiguous()


def _stats(lm, am, sy, ll, tl, blank, lm_scale, am_scale):
    """Arcs of the (smoothed; both scales 0: simple) lattice into a fresh RNN-T workspace."""
    B, U1, V = lm.shape
    T = am.shape[1]
    dev = lm.device
    sws = _lib.workspace("wr_rnnt_smoothed_workspace_bytes", B, T, U1, V, device=dev)
    rws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
    _lib.call("wr_rnnt_smoothed_stats", am, lm, sy, ll, tl, B, T, U1, V, blank, lm_scale, am_scale, sws, sws.numel(), rws,
              rws.numel(), device=dev)
    return sws, rws


class _RNNTLatticeFn(torch.autograd.Function):
    """`rnnt_loss_simple` / `rnnt_loss_smoothed` with a non-default lattice type or penalty: `_RNNTSmoothedFn` with the
    sweeps and the gradient of that lattice."""

    @staticmethod
    def forward(ctx, lm, am, sy, ll, tl, blank, lm_scale, am_scale, lat, pen, want_occ):
        B, U1, V = lm.shape
        T = am.shape[1]
        dev = lm.device
        lm, am = lm.contiguous(), am.contiguous()
        sws, rws = _stats(lm, am, sy, ll, tl, blank, lm_scale, am_scale)
        costs = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.call("wr_rnnt_lattice_sweeps", ll, tl, B, T, U1, lat, pen, costs, rws, rws.numel(), device=dev)
        ctx.blank, ctx.scales, ctx.lat, ctx.want_occ = blank, (lm_scale, am_scale), lat, want_occ
        # the rule of _RNNTSmoothedFn: with am_only_scale > 0 the gradient cannot be taken with unit grad_costs
        ctx.early = want_occ and am_scale == 0.0
        if not want_occ:
            ctx.save_for_backward(lm, am, sy, ll, tl, sws, rws)
            return costs
        occ_emit = torch.empty(B, T, U1, dtype=torch.float32, device=dev)
        occ_blank = torch.empty_like(occ_emit)
        d_am, d_lm = (torch.empty_like(am), torch.empty_like(lm)) if ctx.early else (None, None)
        _lib.call("wr_rnnt_smoothed_grad_lattice", am, lm, sy, ll, tl, B, T, U1, V, blank, lm_scale, am_scale, lat, None,
                  d_am, d_lm, occ_emit, occ_blank, sws, sws.numel(), rws, rws.numel(), device=dev)
        if ctx.early:
            ctx.save_for_backward(d_lm, d_am)
        else:
            ctx.save_for_backward(lm, am, sy, ll, tl, sws, rws)
        ctx.mark_non_differentiable(occ_emit, occ_blank)
        return costs, occ_emit, occ_blank

    @staticmethod
    def backward(ctx, grad_costs, *unused):
        gc = grad_costs.to(torch.float32).contiguous()
        none = (None,) * 9
        if ctx.early:
            d_lm, d_am = ctx.saved_tensors
            return (d_lm * gc[:, None, None], d_am * gc[:, None, None]) + none
        lm, am, sy, ll, tl, sws, rws = ctx.saved_tensors
        B, U1, V = lm.shape
        T = am.shape[1]
        d_am, d_lm = torch.empty_like(am), torch.empty_like(lm)
        _lib.call("wr_rnnt_smoothed_grad_lattice", am, lm, sy, ll, tl, B, T, U1, V, ctx.blank, ctx.scales[0],
                  ctx.scales[1], ctx.lat, gc, d_am, d_lm, None, None, sws, sws.numel(), rws, rws.numel(), device=lm.device)
        return (d_lm, d_am) + none


def loss(lm, am, sy, ll, tl, blank, lm_scale, am_scale, lat, pen, reduction, return_grad):
    """The tail of rnnt_loss_simple / rnnt_loss_smoothed for a non-default lattice: inputs already checked."""
    out = _RNNTLatticeFn.apply(lm.float(), am.float(), sy, ll, tl, blank, lm_scale, am_scale, lat, pen, bool(return_grad))
    costs = out[0] if return_grad else out
    res = costs.mean() if reduction == "mean" else (costs.sum() if reduction == "sum" else costs)
    if not return_grad:
        return res
    return res, occupancies_to_k2(out[1].detach(), out[2].detach(), lat)


@torch.no_grad()
def lattice(lm, am, sy, ll, tl, blank, lm_scale, am_scale, lat, pen):
    """Diagnostics: (costs, alpha, beta, flag) of the lattice of type `lat`, alpha / beta plain (B, T, U+1)."""
    lm, am = lm.detach().float().contiguous(), am.detach().float().contiguous()
    B, U1, _ = lm.shape
    T = am.shape[1]
    dev = lm.device
    _, rws = _stats(lm, am, sy, ll, tl, blank, lm_scale, am_scale)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    alpha = torch.empty(B, T, U1, dtype=torch.float32, device=dev)
    beta = torch.empty_like(alpha)
    _lib.call("wr_rnnt_lattice_sweeps", ll, tl, B, T, U1, lat, pen, costs, rws, rws.numel(), device=dev)
    _lib.call("wr_rnnt_lattice_export", rws, rws.numel(), ll, tl, B, T, U1, lat, alpha, beta, device=dev)
    flag = rws[-256:-252].view(torch.int32).clone()
    return costs, alpha, beta, flag
