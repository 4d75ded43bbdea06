"""The smoothed additive-joiner RNN-T loss: k2's ``rnnt_loss_smoothed``, the form of the simple loss that the pruned
transducer recipes train with, backed by the smoothing kernels of csrc/rnnt_simple.hip.

Every arc of `rnnt_loss_simple`'s lattice is interpolated with an lm-only and an am-only estimate (include/wr_api.h has
the contract; DESIGN.md, "The smoothed loss"):

    arc = (1 - ll - la) * (am + lm - denom) + ll * (lm - Zl[u]) + la * (am + log pbar - N[t])

so that both vocabulary heads stay usable on their own.  ``rnnt_type="modified"`` and ``delay_penalty`` are offered by
the k2-signature form, `k2.rnnt_loss_smoothed` (k2.py, rnnt_lattice.py); the function here keeps its signature.
"""
from __future__ import annotations

from typing import Optional, Tuple, Union

import torch

from . import _lib
from . import rnnt_lattice as _lat
from .rnnt_simple import _prepare, _require_device, _RNNTSimpleFn


def _check_scales(what: str, lm_only_scale, am_only_scale) -> Tuple[float, float]:
    ll, la = float(lm_only_scale), float(am_only_scale)
    if not ll >= 0.0 or not la >= 0.0:
        raise ValueError(f"{what}: lm_only_scale and am_only_scale must not be negative (got {ll}, {la})")
    if ll + la > 1.0:
        raise ValueError(f"{what}: lm_only_scale + am_only_scale must not exceed 1 (got {ll} + {la})")
    return ll, la


def _stats(lm, am, sy, ll, tl, blank, lm_scale, am_scale):
    """Interpolated arcs of the lattice into a fresh RNN-T workspace; returns (smoothed workspace, RNN-T workspace)."""
    B, U1, V = lm.shape
    T = am.shape[1]
    dev = lm.device
    sws = _lib.workspace("wr_rnnt_smoothed_workspace_bytes", B, T, U1, V, device=dev)
    rws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
    _lib.call("wr_rnnt_smoothed_stats", am, lm, sy, ll, tl, B, T, U1, V, blank, lm_scale, am_scale, sws, sws.numel(), rws,
              rws.numel(), device=dev)
    return sws, rws


class _RNNTSmoothedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lm, am, sy, ll, tl, blank, lm_scale, am_scale, want_occ):
        B, U1, V = lm.shape
        T = am.shape[1]
        dev = lm.device
        lm, am = lm.contiguous(), am.contiguous()
        sws, rws = _stats(lm, am, sy, ll, tl, blank, lm_scale, am_scale)
        costs = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.call("wr_rnnt_loss_sweeps", ll, tl, B, T, U1, costs, rws, rws.numel(), device=dev)
        ctx.blank, ctx.scales, ctx.want_occ = blank, (lm_scale, am_scale), want_occ
        # with am_only_scale > 0 d_lm of one utterance depends on the grad_costs of the others (through the unigram),
        # so the gradient cannot be taken here with unit grad_costs and scaled later: only the occupancies are
        ctx.early = want_occ and am_scale == 0.0
        if not want_occ:
            ctx.save_for_backward(lm, am, sy, ll, tl, sws, rws)
            return costs
        occ_emit = torch.empty(B, T, U1, dtype=torch.float32, device=dev)
        occ_blank = torch.empty_like(occ_emit)
        d_am, d_lm = (torch.empty_like(am), torch.empty_like(lm)) if ctx.early else (None, None)
        _lib.call("wr_rnnt_smoothed_grad", am, lm, sy, ll, tl, B, T, U1, V, blank, lm_scale, am_scale, None, d_am, d_lm,
                  occ_emit, occ_blank, sws, sws.numel(), rws, rws.numel(), device=dev)
        if ctx.early:
            ctx.save_for_backward(d_lm, d_am)
        else:
            ctx.save_for_backward(lm, am, sy, ll, tl, sws, rws)
        ctx.mark_non_differentiable(occ_emit, occ_blank)
        return costs, occ_emit, occ_blank

    @staticmethod
    def backward(ctx, grad_costs, *unused):
        gc = grad_costs.to(torch.float32).contiguous()
        none = (None,) * 7
        if ctx.early:
            d_lm, d_am = ctx.saved_tensors
            return (d_lm * gc[:, None, None], d_am * gc[:, None, None]) + none
        lm, am, sy, ll, tl, sws, rws = ctx.saved_tensors
        B, U1, V = lm.shape
        T = am.shape[1]
        d_am, d_lm = torch.empty_like(am), torch.empty_like(lm)
        _lib.call("wr_rnnt_smoothed_grad", am, lm, sy, ll, tl, B, T, U1, V, ctx.blank, ctx.scales[0], ctx.scales[1], gc,
                  d_am, d_lm, None, None, sws, sws.numel(), rws, rws.numel(), device=lm.device)
        return (d_lm, d_am) + none


def rnnt_loss_smoothed(lm: torch.Tensor, am: torch.Tensor, symbols: torch.Tensor, termination_symbol: int,
                       lm_only_scale: float = 0.1, am_only_scale: float = 0.1, boundary: Optional[torch.Tensor] = None,
                       reduction: str = "mean", return_grad: bool = False
                       ) -> Union[torch.Tensor, Tuple[torch.Tensor, Tuple[torch.Tensor, torch.Tensor]]]:
    """k2.rnnt_loss_smoothed(lm, am, symbols, termination_symbol, lm_only_scale, am_only_scale, boundary, reduction,
    return_grad), regular lattice.

    Arguments and results as `rnnt_loss_simple`; the two scales (each >= 0, their sum <= 1; ValueError otherwise) mix
    into every arc's log-probability an lm-only term ``lm[u,v] - logsumexp(lm[u])`` and an am-only term
    ``am[t,v] + log pbar[v] - log sum_w exp(am[t,w]) pbar[w]``.  ``pbar`` is the mean of ``softmax(lm)`` over ALL
    B * (U+1) rows, rows past ``U_b`` included (k2's definition, kept for parity): with ``am_only_scale > 0`` the padded
    rows of ``lm`` must be finite, they receive a gradient, and ``d_lm`` of one utterance depends on the others'.  A
    scale that is exactly 0 drops its branch (k2 substitutes 1e-20 there, below float32 resolution of any finite term);
    both 0 is `rnnt_loss_simple`, bit for bit.  With ``return_grad`` the occupancies are those of the interpolated
    lattice, in the same ``(px_grad (B, U, T+1), py_grad (B, U+1, T))`` layout.  `k2.rnnt_loss_smoothed` takes
    ``rnnt_type`` and ``delay_penalty``."""
    what = "rnnt_loss_smoothed"
    if reduction not in ("none", "mean", "sum"):
        raise ValueError("reduction should be one of 'none', 'mean', or 'sum'")
    lm_scale, am_scale = _check_scales(what, lm_only_scale, am_only_scale)
    sy, ll, tl, blank, _ = _prepare(lm, am, symbols, termination_symbol, boundary, what)
    _require_device(what, lm, am)
    if lm_scale == 0.0 and am_scale == 0.0:               # the simple loss: the same node, the same kernels
        out = _RNNTSimpleFn.apply(lm.float(), am.float(), sy, ll, tl, blank, bool(return_grad))
    else:
        out = _RNNTSmoothedFn.apply(lm.float(), am.float(), sy, ll, tl, blank, lm_scale, am_scale, bool(return_grad))
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
def rnnt_smoothed_lattice(lm, am, symbols, termination_symbol, lm_only_scale=0.1, am_only_scale=0.1, boundary=None, *,
                          rnnt_type="regular", delay_penalty=0.0):
    """Diagnostics for tests, the twin of `rnnt_simple_lattice`: (costs, alpha, beta, flag) of the interpolated lattice."""
    what = "rnnt_smoothed_lattice"
    lm_scale, am_scale = _check_scales(what, lm_only_scale, am_only_scale)
    lat, pen = _lat.check_lattice(what, rnnt_type, delay_penalty)
    sy, ll, tl, blank, _ = _prepare(lm, am, symbols, termination_symbol, boundary, what)
    _require_device(what, lm, am)
    if not _lat.is_default(lat, pen):
        return _lat.lattice(lm, am, sy, ll, tl, blank, lm_scale, am_scale, lat, pen)
    lm, am = lm.detach().float().contiguous(), am.detach().float().contiguous()
    B, U1, _ = lm.shape
    T = am.shape[1]
    dev = lm.device
    _, rws = _stats(lm, am, sy, ll, tl, blank, lm_scale, am_scale)
    costs = torch.empty(B, dtype=torch.float32, device=dev)
    alpha = torch.empty(B, T, U1, dtype=torch.float32, device=dev)
    beta = torch.empty_like(alpha)
    _lib.call("wr_rnnt_loss_sweeps", ll, tl, B, T, U1, costs, rws, rws.numel(), device=dev)
    _lib.call("wr_rnnt_export_lattice", rws, rws.numel(), ll, tl, B, T, U1, alpha, beta, device=dev)
    flag = rws[-256:-252].view(torch.int32).clone()       # the last 256-byte slot of the workspace (wr_common.hpp RnntWs)
    return costs, alpha, beta, flag
