"""Pruned RNN-T training: k2's ``get_rnnt_prune_ranges`` / ``do_rnnt_pruning`` / ``rnnt_loss_pruned`` for the regular
and the modified lattice types, backed by the HIP kernels of csrc/rnnt_pruned.hip ("Pruned RNN-T training").

The additive-joiner loss (rnnt_simple.py) is the cheap first pass of the k2 / icefall recipe; its arc occupancies choose,
per frame, a band of ``s_range`` label positions, and the real joiner and the real loss are evaluated on that band only:

  get_rnnt_prune_ranges   occupancies -> ranges (B, T, R): the band's label positions at every frame
  do_rnnt_pruning         the joiner's two addends gathered onto the band: (B, T, R, C) each, differentiable
  rnnt_loss_pruned        the RNN-T loss of logits (B, T, R, V) given on the band (one autograd node)

``rnnt_loss_pruned`` takes ``rnnt_type="modified"`` and ``delay_penalty`` (rnnt_lattice.py); `k2.get_rnnt_prune_ranges`
(k2.py) also takes the (B, U, T) ``px_grad`` of a modified-lattice simple loss.  Not offered: ``rnnt_type="constrained"``.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from . import rnnt_lattice as _lat


def _check_boundary_rows(rows, B: int, T: int, U: int, what: str) -> None:
    if B and int(rows[:, :2].abs().max()) != 0:
        raise ValueError(f"{what}: boundary rows must begin at (0, 0) (got {rows[:, :2].tolist()})")
    if B and (int(rows[:, 2].min()) < 0 or int(rows[:, 2].max()) > U):
        raise ValueError(f"{what}: boundary symbol ends must lie in [0, {U}] (got {rows[:, 2].tolist()})")
    if B and (int(rows[:, 3].min()) < 0 or int(rows[:, 3].max()) > T):
        raise ValueError(f"{what}: boundary frame ends must lie in [0, {T}] (got {rows[:, 3].tolist()})")


def _boundary(boundary, B: int, T: int, U: int, dev, what: str) -> torch.Tensor:
    if boundary is None:
        return torch.tensor([0, 0, U, T], dtype=torch.int64, device=dev).repeat(B, 1)
    if boundary.dim() != 2 or boundary.shape[0] != B or boundary.shape[1] != 4:
        raise ValueError(f"{what}: boundary must be (B, 4) = ({B}, 4), got {tuple(boundary.shape)}")
    return boundary.to(device=dev, dtype=torch.int64)


def _bad_ranges(ranges: torch.Tensor, U1: int) -> torch.Tensor:
    """Number of violations of ``ranges[..., r] == ranges[..., 0] + r`` inside [0, U1 - 1], as a one-element tensor."""
    R = ranges.shape[-1]
    first = ranges[..., :1]
    step = (ranges != first + torch.arange(R, device=ranges.device)).sum()
    return (step + (first < 0).sum() + (first > U1 - R).sum()).reshape(1)


def _require_device(what: str, *tensors) -> None:
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"wenet_celoss_amd.{what}: the inputs must live on a HIP device (this package has no CPU path)")


def get_rnnt_prune_ranges(px_grad: torch.Tensor, py_grad: torch.Tensor, boundary: torch.Tensor, s_range: int
                          ) -> torch.Tensor:
    """`prune_ranges` for the regular lattice's ``px_grad`` (B, U, T+1) only, ``s_range >= 2`` (the rule is spelled out
    there); `k2.get_rnnt_prune_ranges` also takes the modified lattice's (B, U, T)."""
    return prune_ranges(px_grad, py_grad, boundary, s_range, modified_px=False)


def prune_ranges(px_grad: torch.Tensor, py_grad: torch.Tensor, boundary: torch.Tensor, s_range: int,
                 modified_px: bool = True) -> torch.Tensor:
    """k2.get_rnnt_prune_ranges(px_grad, py_grad, boundary, s_range) -> ranges (B, T, R) int64, R = min(s_range, U + 1).

    px_grad (B, U, T+1) and py_grad (B, U+1, T) are the arc occupancies ``rnnt_loss_simple(..., return_grad=True)``
    returns; ``boundary`` (B, 4) int64 rows ``(0, 0, U_b, T_b)`` (None = full lengths).  Per frame the band starts at the
    label position u0 whose window ``sum_{r<R} py[u0+r, t] - px[u0-1, t]`` is largest (float64, lowest u0 on ties), frames
    from T_b - 1 on start at ``max(U_b - R + 1, 0)``, and the starts are then made monotone with steps of at most one
    (the contract is spelled out in include/wr_api.h).  ``ranges[b, t, r] = s_begin[b, t] + r``.

    With ``modified_px`` px_grad may also be (B, U, T), what the losses return with ``rnnt_type="modified"``: the score
    reads only columns ``t < T``, so the rule is the same; ``s_range >= 1`` is then accepted (k2's rule for that lattice),
    with the (B, U, T+1) form it stays ``>= 2``."""
    what = "get_rnnt_prune_ranges"
    if px_grad.dim() != 3 or py_grad.dim() != 3:
        raise ValueError(f"{what}: px_grad must be (B, U, T+1) or (B, U, T) and py_grad (B, U+1, T)")
    B, U1, T = py_grad.shape
    if tuple(px_grad.shape) not in (((B, U1 - 1, T + 1), (B, U1 - 1, T)) if modified_px else ((B, U1 - 1, T + 1),)):
        raise ValueError(f"{what}: px_grad {tuple(px_grad.shape)} does not match py_grad {tuple(py_grad.shape)}")
    px_cols = int(px_grad.shape[2])
    if int(s_range) < (1 if px_cols == T else 2):
        raise ValueError(f"{what}: s_range must be at least {1 if px_cols == T else 2} (got {s_range})")
    if B < 1 or T < 1:
        raise ValueError(f"{what}: empty batch or no frames")
    _require_device(what, px_grad, py_grad)
    dev = py_grad.device
    bd = _boundary(boundary, B, T, U1 - 1, dev, what)
    if boundary is not None:                                                # full lengths need no check and no sync
        _check_boundary_rows(bd.cpu(), B, T, U1 - 1, what)                  # the one host sync
    R = min(int(s_range), U1)
    px = px_grad.detach().to(torch.float32).contiguous()
    py = py_grad.detach().to(torch.float32).contiguous()
    ranges = torch.empty(B, T, R, dtype=torch.int64, device=dev)
    if px_cols == T + 1:
        _lib.call("wr_rnnt_prune_ranges", px if U1 > 1 else None, py, bd[:, 3].to(torch.int32).contiguous(),
                  bd[:, 2].to(torch.int32).contiguous(), B, T, U1, R, ranges, device=dev)
    else:
        _lib.call("wr_rnnt_prune_ranges_cols", px if U1 > 1 else None, px_cols, py, bd[:, 3].to(torch.int32).contiguous(),
                  bd[:, 2].to(torch.int32).contiguous(), B, T, U1, R, ranges, device=dev)
    return ranges


class _PruneFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, am, lm, ranges):
        B, T, C = am.shape
        U1 = lm.shape[1]
        R = ranges.shape[2]
        am, lm = am.contiguous(), lm.contiguous()
        am_p = torch.empty(B, T, R, C, dtype=am.dtype, device=am.device)
        lm_p = torch.empty_like(am_p)
        _lib.call("wr_rnnt_prune_gather", am, lm, ranges, _lib.dtype_code(am.dtype), B, T, U1, R, C, am_p, lm_p,
                  device=am.device)
        ctx.save_for_backward(ranges)
        ctx.dims = (B, T, U1, R, C)
        return am_p, lm_p

    @staticmethod
    def backward(ctx, g_am, g_lm):
        ranges, = ctx.saved_tensors
        B, T, U1, R, C = ctx.dims
        need_am, need_lm = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g_am = g_am.contiguous() if need_am else None
        g_lm = g_lm.contiguous() if need_lm else None
        ref = g_am if need_am else g_lm
        if ref is None:
            return None, None, None
        d_am = torch.empty(B, T, C, dtype=ref.dtype, device=ref.device) if need_am else None
        d_lm = torch.empty(B, U1, C, dtype=ref.dtype, device=ref.device) if need_lm else None
        _lib.call("wr_rnnt_prune_scatter", g_am, g_lm, ranges, _lib.dtype_code(ref.dtype), B, T, U1, R, C, d_am, d_lm,
                  device=ref.device)
        return d_am, d_lm, None


def do_rnnt_pruning(am: torch.Tensor, lm: torch.Tensor, ranges: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """k2.do_rnnt_pruning(am, lm, ranges): am (B, T, C), lm (B, U+1, C) (float32, float16 or bfloat16, the same for
    both), ranges (B, T, R) -> (am_pruned, lm_pruned), both (B, T, R, C): ``am_pruned[b,t,r] = am[b,t]`` and
    ``lm_pruned[b,t,r] = lm[b, ranges[b,t,r]]``.  Differentiable in am and lm; the backward sums in a fixed order
    (bit-identical run to run).  ``ranges`` must be consecutive along r and lie within [0, U] (ValueError otherwise;
    checked with the call's one host sync)."""
    what = "do_rnnt_pruning"
    if am.dim() != 3 or lm.dim() != 3 or ranges.dim() != 3:
        raise ValueError(f"{what}: am must be (B, T, C), lm (B, U+1, C) and ranges (B, T, R)")
    B, T, C = am.shape
    U1 = lm.shape[1]
    R = ranges.shape[2]
    if lm.shape[0] != B or lm.shape[2] != C or ranges.shape[0] != B or ranges.shape[1] != T:
        raise ValueError(f"{what}: am {tuple(am.shape)}, lm {tuple(lm.shape)} and ranges {tuple(ranges.shape)} do not agree")
    if am.dtype != lm.dtype or am.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"{what}: am and lm must share one of float32, float16, bfloat16")
    if not 1 <= R <= U1 or min(B, T, C) < 1:
        raise ValueError(f"{what}: ranges hold R = {R} positions for U + 1 = {U1}")
    if ranges.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: ranges must be an integer tensor")
    _require_device(what, am, lm, ranges)
    rg = ranges.to(torch.int64).contiguous()
    if int(_bad_ranges(rg, U1).item()) != 0:                               # the one host sync
        raise ValueError(f"{what}: ranges must satisfy ranges[..., r] = ranges[..., 0] + r within [0, {U1 - 1}]")
    return _PruneFn.apply(am, lm, rg)


def _prepare(logits, symbols, ranges, termination_symbol, boundary, what: str):
    """Shapes, blank, boundary, ranges -> (symbols int32, T_b int32, U_b int32, blank, ranges int64), checked with one
    host sync as `rnnt_simple._prepare` checks its inputs, plus the band's consecutiveness and bounds."""
    if logits.dim() != 4 or ranges.dim() != 3:
        raise ValueError(f"{what}: logits must be (B, T, R, V) and ranges (B, T, R)")
    B, T, R, V = logits.shape
    if tuple(ranges.shape) != (B, T, R):
        raise ValueError(f"{what}: ranges {tuple(ranges.shape)} do not match logits {tuple(logits.shape)}")
    if ranges.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: ranges must be an integer tensor")
    if symbols.dim() != 2 or symbols.shape[0] != B:
        raise ValueError(f"{what}: symbols must be (B, U) with B = {B}, got {tuple(symbols.shape)}")
    if symbols.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{what}: symbols must be an integer tensor")
    if logits.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise ValueError(f"{what}: logits must be float32, float16 or bfloat16")
    U1 = symbols.shape[1] + 1
    if V < 2:
        raise ValueError(f"{what}: at least 2 classes are needed (V = {V})")
    if not 1 <= R <= U1 or min(B, T) < 1:
        raise ValueError(f"{what}: logits hold R = {R} positions for U + 1 = {U1}")
    blank = int(termination_symbol)
    if not 0 <= blank < V:
        raise ValueError(f"{what}: termination_symbol must be within [0, {V})")
    _require_device(what, logits)
    dev = logits.device
    bd = _boundary(boundary, B, T, U1 - 1, dev, what)
    sy = symbols.to(device=dev)
    rg = ranges.to(device=dev, dtype=torch.int64).contiguous()
    inside = torch.arange(U1 - 1, device=dev)[None, :] < bd[:, 2:3]
    bad = (inside & ((sy < 0) | (sy >= V))).sum().reshape(1)
    host = torch.cat([bd.reshape(-1), bad, _bad_ranges(rg, U1)]).cpu()       # the one host sync
    _check_boundary_rows(host[:-2].reshape(B, 4), B, T, U1 - 1, what)
    if int(host[-2]) != 0:
        raise ValueError(f"{what}: a symbol inside its boundary lies outside [0, {V})")
    if int(host[-1]) != 0:
        raise ValueError(f"{what}: ranges must satisfy ranges[..., r] = ranges[..., 0] + r within [0, {U1 - 1}]")
    sy = torch.where(inside, sy, torch.zeros((), dtype=sy.dtype, device=dev)).to(torch.int32).contiguous()
    return sy, bd[:, 3].to(torch.int32).contiguous(), bd[:, 2].to(torch.int32).contiguous(), blank, rg


def _stats_and_sweeps(logits, sy, rg, ll, tl, blank, lat=0, pen=0.0):
    """Row statistics of the band into a fresh RNN-T workspace, then the lattice sweeps: (costs float32, workspace)."""
    B, T, R, V = logits.shape
    U1 = sy.shape[1] + 1
    dev = logits.device
    ws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    _lib.call("wr_rnnt_pruned_stats", logits, _lib.dtype_code(logits.dtype), sy if U1 > 1 else None, rg, ll, tl, B, T, U1, R,
              V, blank, ws, ws.numel(), device=dev)
    if _lat.is_default(lat, pen):
        _lib.call("wr_rnnt_loss_sweeps", ll, tl, B, T, U1, costs, ws, ws.numel(), device=dev)
    else:
        _lib.call("wr_rnnt_lattice_sweeps", ll, tl, B, T, U1, lat, pen, costs, ws, ws.numel(), device=dev)
    return costs, ws


class _RNNTPrunedFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")          # fp16/bf16 logits are handled natively (fp32 arithmetic inside)
    def forward(ctx, logits, sy, rg, ll, tl, blank, lat=0, pen=0.0):
        logits = logits.contiguous()
        if logits.data_ptr() % 16:                     # a view at an odd storage offset: the gradient kernel needs logits
            logits = logits.clone()                    # and grads at the same 16-byte phase, and fresh tensors are aligned
        costs, ws = _stats_and_sweeps(logits, sy, rg, ll, tl, blank, lat, pen)
        ctx.save_for_backward(logits, sy, rg, ll, tl, ws)
        ctx.blank, ctx.lat, ctx.pen = blank, lat, pen
        return costs

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_costs):
        logits, sy, rg, ll, tl, ws = ctx.saved_tensors
        B, T, R, V = logits.shape
        U1 = sy.shape[1] + 1
        grads = torch.empty_like(logits)
        gc = grad_costs.to(torch.float32).contiguous()
        if _lat.is_default(ctx.lat, ctx.pen):
            _lib.call("wr_rnnt_pruned_grad", logits, _lib.dtype_code(logits.dtype), sy if U1 > 1 else None, rg, ll, tl, B, T,
                      U1, R, V, ctx.blank, gc, grads, ws, ws.numel(), device=logits.device)
        else:
            _lib.call("wr_rnnt_pruned_grad_lattice", logits, _lib.dtype_code(logits.dtype), sy if U1 > 1 else None, rg, ll,
                      tl, B, T, U1, R, V, ctx.blank, ctx.lat, ctx.pen, gc, grads, ws, ws.numel(), device=logits.device)
        return (grads,) + (None,) * (len(ctx.needs_input_grad) - 1)


def rnnt_loss_pruned(logits: torch.Tensor, symbols: torch.Tensor, ranges: torch.Tensor, termination_symbol: int,
                     boundary: Optional[torch.Tensor] = None, reduction: str = "mean", *, rnnt_type: str = "regular",
                     delay_penalty: float = 0.0) -> torch.Tensor:
    """k2.rnnt_loss_pruned(logits, symbols, ranges, termination_symbol, boundary, reduction, rnnt_type=, delay_penalty=).

    logits (B, T, R, V) are the joiner's un-normalised outputs on the band (float32, float16 or bfloat16; the gradient
    comes back in the same dtype), ``logits[b,t,r]`` belonging to the lattice cell ``(t, ranges[b,t,r])``; symbols (B, U)
    integer; ``termination_symbol`` the blank; ``boundary`` (B, 4) int64 rows ``(0, 0, U_b, T_b)``, None = full lengths.
    Returns the negated total log-probability of the paths that stay inside the band (float32), reduced over the batch
    ("none" | "mean" | "sum"; not length-normalised).  A band that holds no complete path gives ``+inf`` for that
    utterance (a value, not an error; its gradient is not finite).  ``ranges`` must be consecutive along r and lie
    within [0, U] (ValueError otherwise).  ``rnnt_type`` and ``delay_penalty`` as in `rnnt_loss_simple`: the penalty is
    added to the band's label arcs; on the "modified" lattice a band of one position per frame (R = 1) is legal."""
    what = "rnnt_loss_pruned"
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("reduction should be one of 'none', 'mean', or 'sum'")
    lat, pen = _lat.check_lattice(what, rnnt_type, delay_penalty)
    sy, ll, tl, blank, rg = _prepare(logits, symbols, ranges, termination_symbol, boundary, what)
    if _lat.is_default(lat, pen):
        costs = _RNNTPrunedFn.apply(logits, sy, rg, ll, tl, blank)
    else:
        costs = _RNNTPrunedFn.apply(logits, sy, rg, ll, tl, blank, lat, pen)
    return costs.mean() if reduction == "mean" else (costs.sum() if reduction == "sum" else costs)


@torch.no_grad()
def rnnt_pruned_lattice(logits, symbols, ranges, termination_symbol, boundary=None, *, rnnt_type="regular",
                        delay_penalty=0.0):
    """Diagnostics for tests: (costs, alpha, beta) of the banded lattice, alpha / beta as plain (B, T, U+1) tensors
    (-inf where no path inside the band reaches a cell, zero outside the boundary)."""
    lat, pen = _lat.check_lattice("rnnt_pruned_lattice", rnnt_type, delay_penalty)
    sy, ll, tl, blank, rg = _prepare(logits, symbols, ranges, termination_symbol, boundary, "rnnt_pruned_lattice")
    logits = logits.detach().contiguous()
    B, T = logits.shape[:2]
    U1 = sy.shape[1] + 1
    costs, ws = _stats_and_sweeps(logits, sy, rg, ll, tl, blank, lat, pen)
    alpha = torch.empty(B, T, U1, dtype=torch.float32, device=logits.device)
    beta = torch.empty_like(alpha)
    if _lat.is_default(lat, pen):
        _lib.call("wr_rnnt_export_lattice", ws, ws.numel(), ll, tl, B, T, U1, alpha, beta, device=logits.device)
    else:
        _lib.call("wr_rnnt_lattice_export", ws, ws.numel(), ll, tl, B, T, U1, lat, alpha, beta, device=logits.device)
    return costs, alpha, beta
