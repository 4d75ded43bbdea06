"""The additive-joiner ("simple") RNN-T loss: k2's ``rnnt_loss_simple`` as the reference's second transducer class
calls it (wenet/transducer/transducer_k2_loss.py:140-157), backed by the HIP kernels of csrc/rnnt_simple.hip.

The joiner is a plain sum, ``logit(b,t,u,v) = am[b,t,v] + lm[b,u,v]``, so the loss is the ordinary RNN-T loss on
``am.unsqueeze(2) + lm.unsqueeze(1)`` -- but that tensor is never formed: the row normaliser and both gradients are
contractions over one index ("The additive-joiner loss"), and memory stays at a few floats per lattice cell.

  rnnt_loss_simple            the loss (one autograd node: forward = row statistics + lattice sweeps, backward = gradient)
  rnnt_simple_forced_align    the best path through the same lattice (row statistics, then `wr_rnnt_align_from_stats`)

``rnnt_type="modified"`` and ``delay_penalty`` are offered by the k2-signature form of the loss, `k2.rnnt_loss_simple`
(k2.py, rnnt_lattice.py); the function here keeps its signature.  The forced alignment stays on the regular lattice.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import _lib
from . import rnnt_lattice as _lat


def _prepare(lm, am, symbols, termination_symbol, boundary, what: str):
    """Shapes, blank, boundary -> (symbols int32, T_b int32, U_b int32, blank) on the inputs' device, checked with one
    host sync: begins zero, 0 <= U_b <= U, 0 <= T_b <= T, labels inside each length within [0, V)."""
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
    dev = lm.device
    if boundary is None:
        bd = torch.tensor([0, 0, U1 - 1, T], dtype=torch.int64, device=dev).repeat(B, 1)
    else:
        if boundary.dim() != 2 or boundary.shape[0] != B or boundary.shape[1] != 4:
            raise ValueError(f"{what}: boundary must be (B, 4) = ({B}, 4), got {tuple(boundary.shape)}")
        bd = boundary.to(device=dev, dtype=torch.int64)
    sy = symbols.to(device=dev)
    inside = torch.arange(U1 - 1, device=dev)[None, :] < bd[:, 2:3]
    bad = (inside & ((sy < 0) | (sy >= V))).sum().reshape(1)
    host = torch.cat([bd.reshape(-1), bad]).cpu()                      # the one host sync
    rows = host[:-1].reshape(B, 4)
    if B and int(rows[:, :2].abs().max()) != 0:
        raise ValueError(f"{what}: boundary rows must begin at (0, 0) (got {rows[:, :2].tolist()})")
    if B and (int(rows[:, 2].min()) < 0 or int(rows[:, 2].max()) > U1 - 1):
        raise ValueError(f"{what}: boundary symbol ends must lie in [0, {U1 - 1}] (got {rows[:, 2].tolist()})")
    if B and (int(rows[:, 3].min()) < 0 or int(rows[:, 3].max()) > T):
        raise ValueError(f"{what}: boundary frame ends must lie in [0, {T}] (got {rows[:, 3].tolist()})")
    if int(host[-1]) != 0:
        raise ValueError(f"{what}: a symbol inside its boundary lies outside [0, {V})")
    sy = torch.where(inside, sy, torch.zeros((), dtype=sy.dtype, device=dev)).to(torch.int32).contiguous()
    return sy, bd[:, 3].to(torch.int32).contiguous(), bd[:, 2].to(torch.int32).contiguous(), blank, rows


def _require_device(what: str, *tensors) -> None:
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"wenet_celoss_amd.{what}: lm and am must live on a HIP device (this package has no CPU path)")


def _stats(lm, am, sy, ll, tl, blank):
    """Row statistics of the lattice into a fresh RNN-T workspace; returns (simple workspace, RNN-T workspace)."""
    B, U1, V = lm.shape
    T = am.shape[1]
    dev = lm.device
    sws = _lib.workspace("wr_rnnt_simple_workspace_bytes", B, T, U1, V, device=dev)
    rws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
    _lib.call("wr_rnnt_simple_stats", am, lm, sy, ll, tl, B, T, U1, V, blank, sws, sws.numel(), rws, rws.numel(), device=dev)
    return sws, rws


class _RNNTSimpleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lm, am, sy, ll, tl, blank, want_occ):
        B, U1, V = lm.shape
        T = am.shape[1]
        dev = lm.device
        lm, am = lm.contiguous(), am.contiguous()
        sws, rws = _stats(lm, am, sy, ll, tl, blank)
        costs = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.call("wr_rnnt_loss_sweeps", ll, tl, B, T, U1, costs, rws, rws.numel(), device=dev)
        ctx.blank, ctx.want_occ = blank, want_occ
        if not want_occ:
            ctx.save_for_backward(lm, am, sy, ll, tl, sws, rws)
            return costs
        # the arc occupancies are a by-product of the gradient: take it now (unit grad_costs), scale it in backward
        d_am, d_lm = torch.empty_like(am), torch.empty_like(lm)
        occ_emit = torch.empty(B, T, U1, dtype=torch.float32, device=dev)
        occ_blank = torch.empty_like(occ_emit)
        _lib.call("wr_rnnt_simple_grad", am, lm, sy, ll, tl, B, T, U1, V, blank, None, d_am, d_lm, occ_emit, occ_blank,
                  sws, sws.numel(), rws, rws.numel(), device=dev)
        ctx.save_for_backward(d_lm, d_am)
        ctx.mark_non_differentiable(occ_emit, occ_blank)
        return costs, occ_emit, occ_blank

    @staticmethod
    def backward(ctx, grad_costs, *unused):
        gc = grad_costs.to(torch.float32).contiguous()
        if ctx.want_occ:
            d_lm, d_am = ctx.saved_tensors
            return d_lm * gc[:, None, None], d_am * gc[:, None, None], None, None, None, None, None
        lm, am, sy, ll, tl, sws, rws = ctx.saved_tensors
        B, U1, V = lm.shape
        T = am.shape[1]
        d_am, d_lm = torch.empty_like(am), torch.empty_like(lm)
        _lib.call("wr_rnnt_simple_grad", am, lm, sy, ll, tl, B, T, U1, V, ctx.blank, gc, d_am, d_lm, None, None,
                  sws, sws.numel(), rws, rws.numel(), device=lm.device)
        return d_lm, d_am, None, None, None, None, None


def rnnt_loss_simple(lm: torch.Tensor, am: torch.Tensor, symbols: torch.Tensor, termination_symbol: int,
                     boundary: Optional[torch.Tensor] = None, reduction: str = "mean", return_grad: bool = False
                     ) -> Union[torch.Tensor, Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]]:
    """k2.rnnt_loss_simple(lm, am, symbols, termination_symbol, boundary, reduction, return_grad).

    lm (B, U+1, V) and am (B, T, V) are the two un-normalised heads (float32; half precision is upcast), symbols (B, U)
    integer, ``termination_symbol`` the blank.  ``boundary`` (B, 4) int64 rows ``(0, 0, U_b, T_b)``; None = full lengths;
    a row with a non-zero begin raises ValueError.  Returns the negated total log-probability, reduced over the batch
    ("none" | "mean" | "sum"; not length-normalised).  With ``return_grad`` also ``(px_grad (B, U, T+1), py_grad
    (B, U+1, T))``: the occupancies of the emit and blank arcs in k2's layout (px_grad's last frame column is zero),
    detached -- what a pruning step takes its ranges from.  Regular lattice, no delay penalty: `k2.rnnt_loss_simple`
    takes ``rnnt_type`` and ``delay_penalty``."""
    what = "rnnt_loss_simple"
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("reduction should be one of 'none', 'mean', or 'sum'")
    sy, ll, tl, blank, _ = _prepare(lm, am, symbols, termination_symbol, boundary, what)
    _require_device(what, lm, am)
    out = _RNNTSimpleFn.apply(lm.float(), am.float(), sy, ll, tl, blank, bool(return_grad))
    costs = out[0] if return_grad else out                # float32 whatever the inputs' precision
    loss = costs.mean() if reduction == "mean" else (costs.sum() if reduction == "sum" else costs)
    if not return_grad:
        return loss
    occ_emit, occ_blank = out[1].detach(), out[2].detach()
    B, T, U1 = occ_emit.shape
    px_grad = torch.zeros(B, U1 - 1, T + 1, dtype=torch.float32, device=occ_emit.device)
    px_grad[:, :, :T] = occ_emit[:, :, :U1 - 1].transpose(1, 2)
    py_grad = occ_blank.transpose(1, 2).contiguous()
    return loss, (px_grad, py_grad)


@torch.no_grad()
def rnnt_simple_forced_align(lm: torch.Tensor, am: torch.Tensor, symbols: torch.Tensor, termination_symbol: int,
                             boundary: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """Best path of the regular lattice `rnnt_loss_simple` sums over (the modified lattice and the delay penalty are not
    offered here), without a logits tensor.  Arguments as rnnt_loss_simple (every T_b >= 1).  Returns what `rnnt_forced_align` returns: (label_frames (B, U) int32, -1 past U_b; scores (B,)
    float64) on the device; `rnnt_frame_tokens` applies to the result."""
    what = "rnnt_simple_forced_align"
    sy, ll, tl, blank, rows = _prepare(lm, am, symbols, termination_symbol, boundary, what)
    if lm.shape[0] and int(rows[:, 3].min()) < 1:
        raise ValueError(f"{what}: boundary frame ends must be at least 1 (got {rows[:, 3].tolist()})")
    _require_device(what, lm, am)
    lm, am = lm.detach().float().contiguous(), am.detach().float().contiguous()
    B, U1, _ = lm.shape
    T = am.shape[1]
    dev = lm.device
    _, rws = _stats(lm, am, sy, ll, tl, blank)
    frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    _lib.call("wr_rnnt_align_from_stats", sy, ll, tl, B, T, U1, frames, scores, rws, rws.numel(), device=dev)
    return frames, scores


@torch.no_grad()
def rnnt_simple_lattice(lm, am, symbols, termination_symbol, boundary=None, *, rnnt_type="regular", delay_penalty=0.0):
    """Diagnostics for tests: (costs, alpha, beta, flag) -- alpha / beta as plain (B, T, U+1) tensors, flag the RNN-T
    workspace's "row statistics were redone by the direct kernel" word (a one-element int32 tensor)."""
    what = "rnnt_simple_lattice"
    lat, pen = _lat.check_lattice(what, rnnt_type, delay_penalty)
    sy, ll, tl, blank, _ = _prepare(lm, am, symbols, termination_symbol, boundary, what)
    _require_device(what, lm, am)
    if not _lat.is_default(lat, pen):
        return _lat.lattice(lm, am, sy, ll, tl, blank, 0.0, 0.0, lat, pen)
    lm, am = lm.detach().float().contiguous(), am.detach().float().contiguous()
    B, U1, _ = lm.shape
    T = am.shape[1]
    dev = lm.device
    _, rws = _stats(lm, am, sy, ll, tl, blank)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    alpha = torch.empty(B, T, U1, dtype=torch.float32, device=dev)
    beta = torch.empty_like(alpha)
    _lib.call("wr_rnnt_loss_sweeps", ll, tl, B, T, U1, costs, rws, rws.numel(), device=dev)
    _lib.call("wr_rnnt_export_lattice", rws, rws.numel(), ll, tl, B, T, U1, alpha, beta, device=dev)
    flag = rws[-256:-252].view(torch.int32).clone()       # the last 256-byte slot of the workspace (wr_common.hpp RnntWs)
    return costs, alpha, beta, flag
