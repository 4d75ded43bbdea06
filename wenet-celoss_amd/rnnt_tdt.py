"""Token-and-duration transducer (TDT) loss and forced alignment, backed by the HIP kernels (csrc/rnnt_lattice.hip; the
contract is in include/wr_api.h, "Token-and-duration transducer" and "TDT forced alignment"; DESIGN.md, "The
token-and-duration loss" and "TDT forced alignment").

TDT (Xu et al. 2023, the loss of NeMo's Parakeet-TDT models): the joiner's output row holds ``V`` token logits and, after
them, ``D = len(durations)`` duration logits with a softmax of their own.  An arc emits a token -- blank or the next label
-- and jumps ``d = durations[n]`` frames; a blank must jump at least one frame, a label may stay (``d = 0``).  The cost is
the negative log of the summed probability of every path that ends exactly at frame ``T_b`` with all labels emitted, and
the gradient is its exact derivative (no clamp, no FastEmit).  ``sigma`` is NeMo's logit under-normalisation: it is
subtracted from every token log-probability.  An utterance without any path costs ``+inf``.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import Sequence, Tuple

import torch

from . import _lib
from .rnnt_align import _blank, _prepare
from .rnnt_lattice import reducer
from .rnnt_loss import _validate

MAX_DURATION = 8


def check_tdt(what: str, durations, sigma) -> Tuple[Tuple[int, ...], float]:
    """(durations as a tuple of ints, sigma as float) or ValueError; needs no device."""
    try:
        durs = tuple(durations)
    except TypeError:
        raise ValueError(f"{what}: durations must be a sequence of integers (got {durations!r})") from None
    if not 1 <= len(durs) <= MAX_DURATION + 1:
        raise ValueError(f"{what}: durations must hold 1 to {MAX_DURATION + 1} entries (got {len(durs)})")
    for d in durs:
        if isinstance(d, bool) or not isinstance(d, int):
            raise ValueError(f"{what}: durations must be integers (got {d!r})")
        if not 0 <= d <= MAX_DURATION:
            raise ValueError(f"{what}: durations must lie in [0, {MAX_DURATION}] (got {d})")
    if any(b <= a for a, b in zip(durs, durs[1:])):
        raise ValueError(f"{what}: durations must be strictly increasing (got {durs})")
    if durs[-1] < 1:
        raise ValueError(f"{what}: at least one duration must be 1 or more (got {durs}): no arc would consume a frame")
    try:
        sg = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: sigma must be a number (got {sigma!r})") from None
    if not (sg >= 0.0 and math.isfinite(sg)):
        raise ValueError(f"{what}: sigma must be finite and not negative (got {sigma})")
    return durs, sg


def _check_blank(what: str, blank, V: int) -> int:
    if isinstance(blank, bool) or not isinstance(blank, int) or not 0 <= blank < V:
        raise ValueError(f"{what}: blank must be an integer in [0, {V}) -- the token part of the row (got {blank!r})")
    return blank


def _durations_arg(durs):
    """The durations as the library takes them; never empty, so that an empty list still reaches the library's refusal."""
    return (ctypes.c_int32 * max(len(durs), 1))(*[int(d) for d in durs])


def _forward(logits, targets, logit_lengths, target_lengths, blank, durs, sigma):
    B, T, U1, W = logits.shape
    D = len(durs)
    dev = logits.device
    ws = _lib.workspace("wr_rnnt_tdt_workspace_bytes", B, T, U1, D, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    _lib.call("wr_rnnt_tdt_loss_fwd", logits, _lib.dtype_code(logits.dtype), targets, logit_lengths, target_lengths, B, T, U1,
              W - D, blank, _durations_arg(durs), D, sigma, costs, ws, ws.numel(), device=dev)
    return costs, ws


class _TDTLossFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")          # fp16/bf16 logits are handled natively (fp32 arithmetic inside)
    def forward(ctx, logits, targets, logit_lengths, target_lengths, blank, durs, sigma, inplace_grad):
        if not logits.is_cuda:
            raise RuntimeError("wenet_celoss_amd.rnnt_tdt_loss: logits must live on a HIP device "
                               "(this package has no CPU path)")
        costs, ws = _forward(logits, targets, logit_lengths, target_lengths, blank, durs, sigma)
        ctx.save_for_backward(logits, targets, logit_lengths, target_lengths, ws)
        ctx.blank, ctx.durs, ctx.sigma, ctx.inplace_grad = blank, durs, sigma, inplace_grad
        return costs.to(logits.dtype) if logits.dtype != torch.float32 else costs

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_costs):
        logits, targets, logit_lengths, target_lengths, ws = ctx.saved_tensors
        B, T, U1, W = logits.shape
        D = len(ctx.durs)
        dev = logits.device
        grads = logits if ctx.inplace_grad else torch.empty_like(logits)
        gc = grad_costs.to(torch.float32).contiguous()
        _lib.call("wr_rnnt_tdt_loss_bwd", logits, _lib.dtype_code(logits.dtype), targets, logit_lengths, target_lengths, B, T,
                  U1, W - D, ctx.blank, _durations_arg(ctx.durs), D, ctx.sigma, gc, grads, ws, ws.numel(), device=dev)
        return grads, None, None, None, None, None, None, None


def rnnt_tdt_loss(logits: torch.Tensor, targets: torch.Tensor, logit_lengths: torch.Tensor,
                  target_lengths: torch.Tensor, durations: Sequence[int], blank: int = 0, sigma: float = 0.0,
                  reduction: str = "mean", inplace_grad: bool | None = None) -> torch.Tensor:
    """TDT loss of ``logits`` (B, T, U+1, V + D): token logits in columns ``[0, V)``, duration logits behind them,
    ``V = logits.shape[-1] - len(durations)``.  ``targets`` (B, U) int32, lengths int32, as ``rnnt_loss`` takes them.

    ``durations``: strictly increasing integers in [0, 8], at most 9, at least one of them >= 1.  ``blank`` in [0, V).
    ``sigma`` >= 0.  A bad value raises ValueError.  ``reduction`` in {"none", "mean", "sum"}, "mean" a plain batch mean;
    costs come back in the logits' dtype.  ``inplace_grad`` (default from env WR_RNNT_INPLACE_GRAD, off) writes the
    gradient over the logits' storage in backward."""
    reduce = reducer(reduction)
    durs, sg = check_tdt("rnnt_tdt_loss", durations, sigma)
    if logits.dim() == 4:                               # any other rank is _validate's to refuse
        if logits.shape[-1] <= len(durs):
            raise ValueError(f"rnnt_tdt_loss: logits must be (B, T, U+1, V + {len(durs)}) with V >= 1 "
                             f"(got {tuple(logits.shape)})")
        blank = _check_blank("rnnt_tdt_loss", blank, logits.shape[-1] - len(durs))
    _validate(logits, targets, logit_lengths, target_lengths, blank)
    if inplace_grad is None:
        inplace_grad = os.environ.get("WR_RNNT_INPLACE_GRAD", "0") == "1"
    return reduce(_TDTLossFn.apply(logits, targets, logit_lengths, target_lengths, blank, durs, sg, bool(inplace_grad)))


class TDTLoss(torch.nn.Module):
    """Module form of ``rnnt_tdt_loss``."""

    def __init__(self, durations: Sequence[int], blank: int = 0, sigma: float = 0.0, reduction: str = "mean"):
        super().__init__()
        self.durations, self.sigma = check_tdt("TDTLoss", durations, sigma)
        self.blank, self.reduction = blank, reduction

    def forward(self, logits, targets, logit_lengths, target_lengths):
        return rnnt_tdt_loss(logits, targets, logit_lengths, target_lengths, self.durations, self.blank, self.sigma,
                             self.reduction)


@torch.no_grad()
def rnnt_tdt_forced_align(logits: torch.Tensor, targets: torch.Tensor, logit_lengths: torch.Tensor,
                          target_lengths: torch.Tensor, durations: Sequence[int], blank: int = 0, sigma: float = 0.0,
                          return_blank_jumps: bool = False):
    """Best path of the TDT lattice of ``logits`` (B, T, U+1, V + D), float32 / float16 / bfloat16, as ``rnnt_tdt_loss``
    takes them (include/wr_api.h, "TDT forced alignment": the Viterbi pass and its backtrace run on the device).
    targets (B, U); lengths (B,) with 1 <= logit_lengths[b] <= T and 0 <= target_lengths[b] <= U.  ``durations`` and
    ``sigma`` as in ``rnnt_tdt_loss``; ``blank`` in [0, V), negative counts from V.  Returns device tensors
    (label_frames (B, U) int32: the frame at which the arc emitting label u+1 leaves; label_durations (B, U) int32: the
    frames that arc jumps; both -1 past target_lengths[b]; scores (B,) float64: the best path's log-probability, -inf
    for an utterance without a path, whose labels are all -1) and, with ``return_blank_jumps``, blank_jumps (B, T) int32:
    the jump of the blank arc leaving frame t on the path, 0 where none does.  ``rnnt_frame_tokens`` reads label_frames."""
    what = "rnnt_tdt_forced_align"
    durs, sg = check_tdt(what, durations, sigma)
    if logits.dim() != 4:
        raise ValueError(f"{what}: logits must be 4-D (batch, time, target, token + duration)")
    D = len(durs)
    if logits.shape[-1] <= D:
        raise ValueError(f"{what}: logits must be (B, T, U+1, V + {D}) with V >= 1 (got {tuple(logits.shape)})")
    x = logits.detach().contiguous()
    B, T, U1, W = x.shape
    V = W - D
    dev = x.device
    blank = _blank(blank, V, what)
    code = _lib.dtype_code(x.dtype)
    tg, ll, tl = _prepare(targets, logit_lengths, target_lengths, B, T, U1, V, dev, what)
    if not x.is_cuda:
        raise RuntimeError(f"wenet_celoss_amd.{what}: logits must live on a HIP device (this package has no CPU path)")
    frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
    jumps_of = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    blank_jumps = torch.empty(B, T, dtype=torch.int32, device=dev) if return_blank_jumps else None
    ws = _lib.workspace("wr_rnnt_tdt_workspace_bytes", B, T, U1, D, device=dev)
    _lib.call("wr_rnnt_tdt_align", x, code, tg, ll, tl, B, T, U1, V, blank, _durations_arg(durs), D, sg, frames, jumps_of,
              blank_jumps, scores, ws, ws.numel(), device=dev)
    if return_blank_jumps:
        return frames, jumps_of, scores, blank_jumps
    return frames, jumps_of, scores


@torch.no_grad()
def rnnt_tdt_lattice(logits, targets, logit_lengths, target_lengths, durations, blank=0, sigma=0.0):
    """Diagnostics for tests: (costs, alpha, beta) with alpha / beta as plain (B, T, U+1) float tensors, 0 outside the
    lattice."""
    durs, sg = check_tdt("rnnt_tdt_lattice", durations, sigma)
    B, T, U1, _ = logits.shape
    costs, ws = _forward(logits, targets, logit_lengths, target_lengths, blank, durs, sg)
    alpha = torch.empty(B, T, U1, dtype=torch.float32, device=logits.device)
    beta = torch.empty_like(alpha)
    _lib.call("wr_rnnt_tdt_export_lattice", ws, ws.numel(), logit_lengths, target_lengths, B, T, U1, len(durs), alpha, beta,
              device=logits.device)
    return costs, alpha, beta
