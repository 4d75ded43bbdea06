"""RNN-T loss with torchaudio's call signature, backed by the HIP kernels.

Drop-in for ``torchaudio.functional.rnnt_loss`` as the reference calls it:
  wenet/transducer/transducer.py:142-147  (reduction="mean", blank=self.blank)
  wenet/transducer/transducer.py:296-301  (reduction='none', rescoring)

Semantics kept from torchaudio 0.10 (the version the reference pins,
README.md:64): logits (B, T, U+1, V) float (or half), targets (B, U) int32,
lengths int32, ``blank=-1`` means the last class, ``clamp`` clips the gradient,
reduction in {"none", "mean", "sum"} where "mean" is a plain batch mean.  The
same argument checks raise ``RuntimeError``.

Difference in mechanism (not in results): torchaudio computes the gradient in
the forward call and multiplies it by ``grad_output`` in backward (two more
passes over a logits-sized tensor).  Here forward does pass 1 + the lattice
sweeps only and backward writes ``grad_output[b] * d cost_b/d logits`` directly,
so the logits-sized tensor is touched three times in total.
"""
from __future__ import annotations

import math
import os

import torch

from . import _lib
from .rnnt_lattice import check_lattice, reducer


def check_latency(what: str, fastemit_lambda, delay_penalty):
    """(fastemit_lambda, delay_penalty) of a full-lattice loss as floats, or ValueError; needs no device."""
    _, pen = check_lattice(what, "regular", delay_penalty)
    try:
        lam = float(fastemit_lambda)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: fastemit_lambda must be a number (got {fastemit_lambda!r})") from None
    if not (lam >= 0.0 and math.isfinite(lam)):
        raise ValueError(f"{what}: fastemit_lambda must be finite and not negative (got {fastemit_lambda})")
    return lam, pen


def _validate(logits, targets, logit_lengths, target_lengths, blank):
    # Conditions of torchaudio's rnnt_loss (compute.cpp), same error type.
    def req(cond, msg):
        if not cond:
            raise RuntimeError(msg)

    req(logits.device == targets.device == logit_lengths.device == target_lengths.device,
        "logits, targets, logit_lengths and target_lengths must be on the same device")
    req(logits.dtype in (torch.float32, torch.float16, torch.bfloat16), "logits must be float32 or float16 type")
    req(targets.dtype == torch.int32, "targets must be int32 type")
    req(logit_lengths.dtype == torch.int32, "logit_lengths must be int32 type")
    req(target_lengths.dtype == torch.int32, "target_lengths must be int32 type")
    req(logits.is_contiguous(), "logits must be contiguous")
    req(targets.is_contiguous(), "targets must be contiguous")
    req(logit_lengths.is_contiguous(), "logit_lengths must be contiguous")
    req(target_lengths.is_contiguous(), "target_lengths must be contiguous")
    req(logits.dim() == 4, "logits must be 4-D (batch, time, target, class)")
    req(targets.dim() == 2, "targets must be 2-D (batch, max target length)")
    req(logit_lengths.dim() == 1, "logit_lengths must be 1-D")
    req(target_lengths.dim() == 1, "target_lengths must be 1-D")
    B = logits.size(0)
    req(logit_lengths.size(0) == B, "batch dimension mismatch between logits and logit_lengths")
    req(target_lengths.size(0) == B, "batch dimension mismatch between logits and target_lengths")
    req(targets.size(0) == B, "batch dimension mismatch between logits and targets")
    req(0 <= blank < logits.size(-1), "blank must be within [0, logits.shape[-1])")
    lens = torch.stack([logit_lengths, target_lengths]).cpu()     # the one host sync, as torchaudio does
    req(int(lens[0].max()) == logits.size(1), "input length mismatch")
    req(int(lens[1].max()) + 1 == logits.size(2), "output length mismatch")
    req(targets.size(1) == logits.size(2) - 1, "output length mismatch")
    req(int(lens.min()) >= 0, "lengths must be non-negative")


_LATTICE_FORM = {"wr_rnnt_loss_sweeps": "wr_rnnt_lattice_sweeps"}        # every other entry point appends "_lattice"


def call_regularised(name: str, head, tail, pen: float, lam=None, *, device) -> None:
    """Entry point `name`(*head, *tail) or, with a regulariser on, its `_lattice` form, which takes the lattice type
    (0: regular), the delay penalty and -- the gradient passes, which give `lam` -- FastEmit's lambda between `head` and
    `tail`.  With both at 0 it is the plain entry point that runs (and that an error names)."""
    if pen == 0.0 and not lam:
        _lib.call(name, *head, *tail, device=device)
    else:
        _lib.call(_LATTICE_FORM.get(name, name + "_lattice"), *head, 0, pen, *(() if lam is None else (lam,)), *tail,
                  device=device)


def loss_forward(logits, targets, llens, tlens, blank: int, pen: float, costs, ws) -> None:
    """Row pass and lattice sweeps of (B, T, U1, V) logits into `costs` and the RNN-T workspace `ws`."""
    B, T, U1, V = logits.shape
    call_regularised("wr_rnnt_loss_fwd", (logits, _lib.dtype_code(logits.dtype), targets, llens, tlens, B, T, U1, V, blank),
                     (costs, ws, ws.numel()), pen, device=logits.device)


def loss_backward(logits, targets, llens, tlens, blank: int, clamp: float, lam: float, pen: float, gc, grads, ws) -> None:
    """gc[b] * d cost_b / d logits into `grads` (which may be `logits`), from the workspace `loss_forward` left."""
    B, T, U1, V = logits.shape
    call_regularised("wr_rnnt_loss_bwd", (logits, _lib.dtype_code(logits.dtype), targets, llens, tlens, B, T, U1, V, blank,
                                          float(clamp)), (gc, grads, ws, ws.numel()), pen, lam, device=logits.device)


class _RNNTLossFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda")          # fp16/bf16 logits are handled natively (fp32 arithmetic inside)
    def forward(ctx, logits, targets, logit_lengths, target_lengths, blank, clamp, inplace_grad, lam=0.0, pen=0.0):
        if not logits.is_cuda:
            raise RuntimeError("wenet_celoss_amd.rnnt_loss: logits must live on a HIP device "
                               "(this package has no CPU path)")
        B, T, U1, V = logits.shape
        dev = logits.device
        ws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
        costs = torch.empty(B, dtype=torch.float32, device=dev)
        loss_forward(logits, targets, logit_lengths, target_lengths, blank, pen, costs, ws)
        ctx.save_for_backward(logits, targets, logit_lengths, target_lengths, ws)
        ctx.blank, ctx.clamp, ctx.inplace_grad, ctx.lam, ctx.pen = blank, clamp, inplace_grad, lam, pen
        return costs.to(logits.dtype) if logits.dtype != torch.float32 else costs

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_costs):
        logits, targets, logit_lengths, target_lengths, ws = ctx.saved_tensors
        grads = logits if ctx.inplace_grad else torch.empty_like(logits)
        gc = grad_costs.to(torch.float32).contiguous()
        loss_backward(logits, targets, logit_lengths, target_lengths, ctx.blank, ctx.clamp, ctx.lam, ctx.pen, gc, grads, ws)
        return grads, None, None, None, None, None, None, None, None


def rnnt_loss(logits: torch.Tensor, targets: torch.Tensor, logit_lengths: torch.Tensor,
              target_lengths: torch.Tensor, blank: int = -1, clamp: float = -1, reduction: str = "mean",
              inplace_grad: bool | None = None, *, fastemit_lambda: float = 0.0,
              delay_penalty: float = 0.0) -> torch.Tensor:
    """torchaudio.functional.rnnt_loss(logits, targets, logit_lengths,
    target_lengths, blank=-1, clamp=-1, reduction="mean").

    ``fastemit_lambda`` (extension; FastEmit, Yu et al. 2021, as warp-transducer, ESPnet and NeMo name it): a
    gradient-level regulariser towards early emission -- the gradient of every label arc's log-probability is scaled
    by ``1 + fastemit_lambda`` and taken exactly through the log-softmax.  The returned costs do NOT depend on it:
    they are bit-identical to the costs at 0.
    ``delay_penalty`` (extension; k2's rule, as the k2 losses of this package take it): ``delay_penalty * ((T_b - 1) /
    2 - t)`` is added to the log-probability of every label arc at frame t; the returned costs include it and the
    gradient is their derivative.  Both must be finite and not negative (ValueError); with both at 0 this is the call
    it always was.  The contract is in include/wr_api.h ("FastEmit and the delay penalty for the full-lattice loss").

    ``inplace_grad`` (extension; default from env WR_RNNT_INPLACE_GRAD, off):
    write the gradient over the logits storage in backward -- halves the
    footprint of the (B,T,U+1,V) tensors when nothing else needs the logits
    (true for the reference's forward, transducer.py:132-147).
    """
    reduce = reducer(reduction)
    lam, pen = check_latency("rnnt_loss", fastemit_lambda, delay_penalty)
    if blank < 0:
        blank = logits.shape[-1] + blank
    _validate(logits, targets, logit_lengths, target_lengths, blank)
    if inplace_grad is None:
        inplace_grad = os.environ.get("WR_RNNT_INPLACE_GRAD", "0") == "1"
    return reduce(_RNNTLossFn.apply(logits, targets, logit_lengths, target_lengths, int(blank), float(clamp),
                                    bool(inplace_grad), lam, pen))


class RNNTLoss(torch.nn.Module):
    """torchaudio.transforms.RNNTLoss counterpart."""

    def __init__(self, blank: int = -1, clamp: float = -1.0, reduction: str = "mean", fastemit_lambda: float = 0.0,
                 delay_penalty: float = 0.0):
        super().__init__()
        self.blank, self.clamp, self.reduction = blank, clamp, reduction
        self.fastemit_lambda, self.delay_penalty = check_latency("RNNTLoss", fastemit_lambda, delay_penalty)

    def forward(self, logits, targets, logit_lengths, target_lengths):
        return rnnt_loss(logits, targets, logit_lengths, target_lengths, self.blank, self.clamp, self.reduction,
                         fastemit_lambda=getattr(self, "fastemit_lambda", 0.0),
                         delay_penalty=getattr(self, "delay_penalty", 0.0))


def rnnt_lattice(logits, targets, logit_lengths, target_lengths, blank=0):
    """Diagnostics for tests: (costs, alpha, beta) with alpha/beta as plain (B,T,U+1) tensors."""
    B, T, U1, V = logits.shape
    dev = logits.device
    ws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    alpha = torch.empty(B, T, U1, dtype=torch.float32, device=dev)
    beta = torch.empty_like(alpha)
    _lib.call("wr_rnnt_loss_fwd", logits, _lib.dtype_code(logits.dtype), targets, logit_lengths, target_lengths, B, T, U1, V,
              blank, costs, ws, ws.numel(), device=dev)
    _lib.call("wr_rnnt_export_lattice", ws, ws.numel(), logit_lengths, target_lengths, B, T, U1, alpha, beta, device=dev)
    return costs, alpha, beta
