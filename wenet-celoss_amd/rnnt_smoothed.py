"""The smoothed additive-joiner RNN-T loss: k2's ``rnnt_loss_smoothed``, the form of the simple loss that the pruned
transducer recipes train with, backed by the smoothing kernels of csrc/rnnt_simple.hip.

Every arc of `rnnt_loss_simple`'s lattice is interpolated with an lm-only and an am-only estimate (include/wr_api.h has
the contract; DESIGN.md, "The smoothed loss"):

    arc = (1 - ll - la) * (am + lm - denom) + ll * (lm - Zl[u]) + la * (am + log pbar - N[t])

so that both vocabulary heads stay usable on their own.  The body and the autograd node are `rnnt_simple.loss`, which the
simple loss calls with both scales 0; `k2.rnnt_loss_smoothed` (k2.py) hands the same body ``rnnt_type`` and
``delay_penalty``, the function here keeps its signature.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import rnnt_simple as _simple


def rnnt_loss_smoothed(lm: torch.Tensor, am: torch.Tensor, symbols: torch.Tensor, termination_symbol: int,
                       lm_only_scale: float = 0.1, am_only_scale: float = 0.1, boundary: Optional[torch.Tensor] = None,
                       reduction: str = "mean", return_grad: bool = False) -> _simple._Loss:
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
    return _simple.loss("rnnt_loss_smoothed", lm, am, symbols, termination_symbol, lm_only_scale, am_only_scale, boundary,
                        reduction, return_grad, "regular", 0.0)


def rnnt_smoothed_lattice(lm, am, symbols, termination_symbol, lm_only_scale=0.1, am_only_scale=0.1, boundary=None, *,
                          rnnt_type="regular", delay_penalty=0.0):
    """Diagnostics for tests, the twin of `rnnt_simple_lattice`: (costs, alpha, beta, flag) of the interpolated lattice."""
    return _simple.lattice("rnnt_smoothed_lattice", lm, am, symbols, termination_symbol, lm_only_scale, am_only_scale,
                           boundary, rnnt_type, delay_penalty)
