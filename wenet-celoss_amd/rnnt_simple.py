"""The additive-joiner ("simple") RNN-T loss: k2's ``rnnt_loss_simple`` as the reference's second transducer class
calls it (wenet/transducer/transducer_k2_loss.py:140-157), backed by the HIP kernels of csrc/rnnt_simple.hip.

The joiner is a plain sum, ``logit(b,t,u,v) = am[b,t,v] + lm[b,u,v]``, so the loss is the ordinary RNN-T loss on
``am.unsqueeze(2) + lm.unsqueeze(1)`` -- but that tensor is never formed: the row normaliser and both gradients are
contractions over one index ("The additive-joiner loss"), and memory stays at a few floats per lattice cell.

  rnnt_loss_simple            the loss: `loss` with both smoothing scales 0, regular lattice, no delay penalty
  rnnt_simple_forced_align    the best path through the same lattice (row statistics, then `wr_rnnt_align_from_stats`)

`loss` is the one body of the additive-joiner family: `rnnt_loss_simple`, `rnnt_loss_smoothed` (rnnt_smoothed.py) and
their k2-signature forms with ``rnnt_type`` / ``delay_penalty`` (k2.py) are its callers, and `_RNNTAdditiveFn` is its one
autograd node (forward = row statistics + lattice sweeps, backward = gradient).  The defaults run the kernels of the
plain entry points through the general ones.  The forced alignment stays on the regular lattice.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import _lib
from . import rnnt_lattice as _lat


def _check_scales(what: str, lm_only_scale, am_only_scale) -> Tuple[float, float]:
    ll, la = float(lm_only_scale), float(am_only_scale)
    if not ll >= 0.0 or not la >= 0.0:
        raise ValueError(f"{what}: lm_only_scale and am_only_scale must not be negative (got {ll}, {la})")
    if ll + la > 1.0:
        raise ValueError(f"{what}: lm_only_scale + am_only_scale must not exceed 1 (got {ll} + {la})")
    return ll, la


def _prepare(lm, am, symbols, termination_symbol, boundary, what: str, min_frames: int = 0):
    """Shapes, blank, boundary -> (symbols int32, T_b int32, U_b int32, blank), the tensors on the inputs'
    device: `rnnt_lattice.prepare` after the shape checks (one host sync; the device check comes last)."""
    if lm.dim() != 3 or am.dim() != 3:
        raise ValueError(f"{what}: lm must be (B, U+1, V) and am (B, T, V)")
    B, U1, V = lm.shape
    T = am.shape[1]
    if am.shape[0] != B or am.shape[2] != V:
        raise ValueError(f"{what}: lm {tuple(lm.shape)} and am {tuple(am.shape)} do not agree in batch or vocabulary")
    if symbols.dim() != 2 or symbols.shape[0] != B or symbols.shape[1] != U1 - 1:
        raise ValueError(f"{what}: symbols must be (B, U) = ({B}, {U1 - 1}), got {tuple(symbols.shape)}")
    if symbols.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: symbols must be an integer tensor")
    if V < 2:
        raise ValueError(f"{what}: at least 2 classes are needed (V = {V})")
    blank = int(termination_symbol)
    if not 0 <= blank < V:
        raise ValueError(f"{what}: termination_symbol must be within [0, {V})")
    ll, tl, sy = _lat.prepare(what, "lm and am", (lm, am), B, T, U1 - 1, boundary, symbols, V,
                              min_frames=min_frames)
    return sy, ll, tl, blank


def _stats(lm, am, sy, ll, tl, blank, lm_scale=0.0, am_scale=0.0):
    """Arcs of the lattice (interpolated unless both scales are 0) into a fresh RNN-T workspace; returns (scratch
    workspace, RNN-T workspace).  With both scales 0 the calls touch only the simple loss's part of the scratch."""
    B, U1, V = lm.shape
    T = am.shape[1]
    dev = lm.device
    simple = lm_scale == 0.0 and am_scale == 0.0
    sws = _lib.workspace("wr_rnnt_simple_workspace_bytes" if simple else "wr_rnnt_smoothed_workspace_bytes", B, T, U1, V,
                         device=dev)
    rws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
    _lib.call("wr_rnnt_smoothed_stats", am, lm, sy, ll, tl, B, T, U1, V, blank, lm_scale, am_scale, sws, sws.numel(), rws,
              rws.numel(), device=dev)
    return sws, rws


class _RNNTAdditiveFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lm, am, sy, ll, tl, blank, lm_scale, am_scale, lat, pen, want_occ):
        B, U1, V = lm.shape
        T = am.shape[1]
        dev = lm.device
        lm, am = lm.contiguous(), am.contiguous()
        sws, rws = _stats(lm, am, sy, ll, tl, blank, lm_scale, am_scale)
        costs = _lat.sweeps(rws, ll, tl, B, T, U1, lat, pen)
        ctx.blank, ctx.scales, ctx.lat = blank, (lm_scale, am_scale), lat
        # the arc occupancies are a by-product of the gradient: where possible it is taken now (unit grad_costs) and
        # scaled in backward.  With am_only_scale > 0 d_lm of one utterance depends on the grad_costs of the others
        # (through the unigram), so the gradient cannot be taken here and scaled later: only the occupancies are
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


_Loss = Union[torch.Tensor, Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]]


def loss(what: str, lm, am, symbols, termination_symbol, lm_only_scale, am_only_scale, boundary, reduction, return_grad,
         rnnt_type, delay_penalty) -> _Loss:
    """The additive-joiner loss with every option: what `rnnt_loss_simple` / `rnnt_loss_smoothed` and their k2 forms
    document.  Checks in order: lattice arguments, reduction, scales, shapes / boundary / symbols (the one host sync),
    device."""
    lat, pen = _lat.check_lattice(what, rnnt_type, delay_penalty)
    reduce = _lat.reducer(reduction)
    lm_scale, am_scale = _check_scales(what, lm_only_scale, am_only_scale)
    sy, ll, tl, blank = _prepare(lm, am, symbols, termination_symbol, boundary, what)
    out = _RNNTAdditiveFn.apply(lm.float(), am.float(), sy, ll, tl, blank, lm_scale, am_scale, lat, pen, bool(return_grad))
    costs = out[0] if return_grad else out                # float32 whatever the inputs' precision
    res = reduce(costs)
    if not return_grad:
        return res
    return res, _lat.occupancies_to_k2(out[1].detach(), out[2].detach(), lat)


@torch.no_grad()
def lattice(what: str, lm, am, symbols, termination_symbol, lm_only_scale, am_only_scale, boundary, rnnt_type,
            delay_penalty):
    """Diagnostics behind `rnnt_simple_lattice` / `rnnt_smoothed_lattice`: `rnnt_lattice.lattice` of `loss`'s arcs."""
    lm_scale, am_scale = _check_scales(what, lm_only_scale, am_only_scale)
    lat, pen = _lat.check_lattice(what, rnnt_type, delay_penalty)
    sy, ll, tl, blank = _prepare(lm, am, symbols, termination_symbol, boundary, what)
    lm, am = lm.detach().float().contiguous(), am.detach().float().contiguous()
    _, rws = _stats(lm, am, sy, ll, tl, blank, lm_scale, am_scale)
    return _lat.lattice(rws, ll, tl, lm.shape[0], am.shape[1], lm.shape[1], lat, pen)


def rnnt_loss_simple(lm: torch.Tensor, am: torch.Tensor, symbols: torch.Tensor, termination_symbol: int,
                     boundary: Optional[torch.Tensor] = None, reduction: str = "mean", return_grad: bool = False
                     ) -> _Loss:
    """k2.rnnt_loss_simple(lm, am, symbols, termination_symbol, boundary, reduction, return_grad).

    lm (B, U+1, V) and am (B, T, V) are the two un-normalised heads (float32; half precision is upcast), symbols (B, U)
    integer, ``termination_symbol`` the blank.  ``boundary`` (B, 4) int64 rows ``(0, 0, U_b, T_b)``; None = full lengths;
    a row with a non-zero begin raises ValueError.  Returns the negated total log-probability, reduced over the batch
    ("none" | "mean" | "sum"; not length-normalised).  With ``return_grad`` also ``(px_grad (B, U, T+1), py_grad
    (B, U+1, T))``: the occupancies of the emit and blank arcs in k2's layout (px_grad's last frame column is zero),
    detached -- what a pruning step takes its ranges from.  Regular lattice, no delay penalty: `k2.rnnt_loss_simple`
    takes ``rnnt_type`` and ``delay_penalty``."""
    return loss("rnnt_loss_simple", lm, am, symbols, termination_symbol, 0.0, 0.0, boundary, reduction, return_grad,
                "regular", 0.0)


@torch.no_grad()
def rnnt_simple_forced_align(lm: torch.Tensor, am: torch.Tensor, symbols: torch.Tensor, termination_symbol: int,
                             boundary: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Best path of the regular lattice `rnnt_loss_simple` sums over (the modified lattice and the delay penalty are not
    offered here), without a logits tensor.  Arguments as rnnt_loss_simple (every T_b >= 1).  Returns what `rnnt_forced_align` returns: (label_frames (B, U) int32, -1 past U_b; scores (B,)
    float64) on the device; `rnnt_frame_tokens` applies to the result."""
    what = "rnnt_simple_forced_align"
    sy, ll, tl, blank = _prepare(lm, am, symbols, termination_symbol, boundary, what, min_frames=1)
    lm, am = lm.detach().float().contiguous(), am.detach().float().contiguous()
    B, U1, _ = lm.shape
    T = am.shape[1]
    dev = lm.device
    _, rws = _stats(lm, am, sy, ll, tl, blank)
    frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    _lib.call("wr_rnnt_align_from_stats", sy, ll, tl, B, T, U1, frames, scores, rws, rws.numel(), device=dev)
    return frames, scores


def rnnt_simple_lattice(lm, am, symbols, termination_symbol, boundary=None, *, rnnt_type="regular", delay_penalty=0.0):
    """Diagnostics for tests: (costs, alpha, beta, flag) -- alpha / beta as plain (B, T, U+1) tensors, flag the RNN-T
    workspace's "row statistics were redone by the direct kernel" word (a one-element int32 tensor)."""
    return lattice("rnnt_simple_lattice", lm, am, symbols, termination_symbol, 0.0, 0.0, boundary, rnnt_type, delay_penalty)
