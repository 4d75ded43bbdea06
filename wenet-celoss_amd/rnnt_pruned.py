"""Pruned RNN-T training: k2's ``get_rnnt_prune_ranges`` / ``do_rnnt_pruning`` / ``rnnt_loss_pruned`` for the regular
and the modified lattice types, backed by the HIP kernels of csrc/rnnt_pruned.hip ("Pruned RNN-T training").

The additive-joiner loss (rnnt_simple.py) is the cheap first pass of the k2 / icefall recipe; its arc occupancies choose,
per frame, a band of ``s_range`` label positions, and the real joiner and the real loss are evaluated on that band only:

  get_rnnt_prune_ranges   occupancies -> ranges (B, T, R): the band's label positions at every frame
  do_rnnt_pruning         the joiner's two addends gathered onto the band: (B, T, R, C) each, differentiable
  rnnt_loss_pruned        the RNN-T loss of logits (B, T, R, V) given on the band (one autograd node)

``rnnt_loss_pruned`` takes ``rnnt_type="modified"`` and ``delay_penalty``; `k2.get_rnnt_prune_ranges` (k2.py) also takes
the (B, U, T) ``px_grad`` of a modified-lattice simple loss.  Not offered: ``rnnt_type="constrained"``.  The lattice
arguments, the boundary preparation and the sweeps are rnnt_lattice.py's, shared with the additive-joiner losses; the
defaults go through the same calls as every other setting.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from . import rnnt_lattice as _lat


def _bad_ranges(ranges: torch.Tensor, U1: int) -> torch.Tensor:
    """Number of violations of ``ranges[..., r] == ranges[..., 0] + r`` inside [0, U1 - 1], as a one-element tensor."""
    R = ranges.shape[-1]
    first = ranges[..., :1]
    step = (ranges != first + torch.arange(R, device=ranges.device)).sum()
    return (step + (first < 0).sum() + (first > U1 - R).sum()).reshape(1)


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
    dev = py_grad.device
    # full lengths need no check and no sync
    ll, tl, _ = _lat.prepare(what, "the inputs", (py_grad, px_grad), B, T, U1 - 1, boundary)
    R = min(int(s_range), U1)
    px = px_grad.detach().to(torch.float32).contiguous()
    py = py_grad.detach().to(torch.float32).contiguous()
    ranges = torch.empty(B, T, R, dtype=torch.int64, device=dev)
    _lib.call("wr_rnnt_prune_ranges_cols", px if U1 > 1 else None, px_cols, py, ll, tl, B, T, U1, R, ranges, device=dev)
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
    _lat.require_device(what, "the inputs", am, lm, ranges)
    rg = ranges.to(torch.int64).contiguous()
    if int(_bad_ranges(rg, U1).item()) != 0:                               # the one host sync
        raise ValueError(f"{what}: ranges must satisfy ranges[..., r] = ranges[..., 0] + r within [0, {U1 - 1}]")
    return _PruneFn.apply(am, lm, rg)


def _prepare(logits, symbols, ranges, termination_symbol, boundary, what: str):
    """Shapes, blank, boundary, ranges -> (symbols int32, T_b int32, U_b int32, blank, ranges int64): `rnnt_lattice.prepare`
    after the shape checks, with the band's consecutiveness and bounds added to its one host sync."""
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
    rg = ranges.to(device=logits.device, dtype=torch.int64).contiguous()
    more = [(_bad_ranges(rg, U1), f"{what}: ranges must satisfy ranges[..., r] = ranges[..., 0] + r within [0, {U1 - 1}]")]
    ll, tl, sy = _lat.prepare(what, "the inputs", (logits,), B, T, U1 - 1, boundary, symbols, V, more)
    return sy, ll, tl, blank, rg


def _stats(logits, sy, rg, ll, tl, blank):
    """Row statistics of the band into a fresh RNN-T workspace."""
    B, T, R, V = logits.shape
    U1 = sy.shape[1] + 1
    ws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=logits.device)
    _lib.call("wr_rnnt_pruned_stats", logits, _lib.dtype_code(logits.dtype), sy if U1 > 1 else None, rg, ll, tl, B, T, U1, R,
              V, blank, ws, ws.numel(), device=logits.device)
    return ws


class _RNNTPrunedFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")          # fp16/bf16 logits are handled natively (fp32 arithmetic inside)
    def forward(ctx, logits, sy, rg, ll, tl, blank, lat, pen):
        logits = logits.contiguous()
        if logits.data_ptr() % 16:                     # a view at an odd storage offset: the gradient kernel needs logits
            logits = logits.clone()                    # and grads at the same 16-byte phase, and fresh tensors are aligned
        ws = _stats(logits, sy, rg, ll, tl, blank)
        costs = _lat.sweeps(ws, ll, tl, logits.shape[0], logits.shape[1], sy.shape[1] + 1, lat, pen)
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
        _lib.call("wr_rnnt_pruned_grad_lattice", logits, _lib.dtype_code(logits.dtype), sy if U1 > 1 else None, rg, ll, tl,
                  B, T, U1, R, V, ctx.blank, ctx.lat, ctx.pen, gc, grads, ws, ws.numel(), device=logits.device)
        return (grads,) + (None,) * 7


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
    reduce = _lat.reducer(reduction)
    lat, pen = _lat.check_lattice(what, rnnt_type, delay_penalty)
    sy, ll, tl, blank, rg = _prepare(logits, symbols, ranges, termination_symbol, boundary, what)
    return reduce(_RNNTPrunedFn.apply(logits, sy, rg, ll, tl, blank, lat, pen))


@torch.no_grad()
def rnnt_pruned_lattice(logits, symbols, ranges, termination_symbol, boundary=None, *, rnnt_type="regular",
                        delay_penalty=0.0):
    """Diagnostics for tests: (costs, alpha, beta) of the banded lattice, alpha / beta as plain (B, T, U+1) tensors
    (-inf where no path inside the band reaches a cell, zero outside the boundary)."""
    lat, pen = _lat.check_lattice("rnnt_pruned_lattice", rnnt_type, delay_penalty)
    sy, ll, tl, blank, rg = _prepare(logits, symbols, ranges, termination_symbol, boundary, "rnnt_pruned_lattice")
    logits = logits.detach().contiguous()
    ws = _stats(logits, sy, rg, ll, tl, blank)
    return _lat.lattice(ws, ll, tl, logits.shape[0], logits.shape[1], sy.shape[1] + 1, lat, pen)[:3]
