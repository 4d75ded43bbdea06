"""RNN-T forced alignment: the single best path through the transducer lattice that `rnnt_loss` sums over.

The lattice is the loss's own (torchaudio's, log-softmax fused): for utterance b with T_b frames and labels y_1..y_U_b,
    A(0,0) = 0,  A(t,u) = max(A(t-1,u) + blank(t-1,u), A(t,u-1) + emit(t,u-1)),  score_b = A(T_b-1,U_b) + blank(T_b-1,U_b),
so score_b is the log-probability of the best alignment, at most -cost_b of `rnnt_loss`.  The Viterbi pass and its
backtrace run on the device (`wr_rnnt_align`, csrc/rnnt_align.hip); the CTC head's counterpart is `forced_align_batch`.

  rnnt_forced_align        from a (B, T, U+1, V) logits tensor (fp32, fp16 or bf16)
  joint_rnnt_forced_align  from the joiner's addends, without a logits tensor (`wr_joint_rnnt_stats` then
                           `wr_rnnt_align_from_stats`): memory is the RNN-T workspace plus the joiner's at any T x U
  rnnt_frame_tokens        host helper: per utterance and per frame, the tokens emitted at that frame

Frames are the frames of the logits (encoder frames after subsampling, for a model); converting them to seconds is the
caller's (subsampling rate x frame shift).
"""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _lib
from .joint import _PRECISIONS, _call_precision, activation_code, joiner_workspace


def _prepare(targets, logit_lengths, target_lengths, B: int, T: int, U1: int, V: int, dev, what: str):
    """Lengths and labels on the device, checked with one host sync: 1 <= T_b <= T, 0 <= U_b <= U1 - 1, labels inside each
    length within [0, V).  Labels beyond a length (IGNORE_ID padding) become 0, as forced_align_batch does."""
    tg = targets.to(device=dev, dtype=torch.int32)
    ll = logit_lengths.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    tl = target_lengths.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    if tg.dim() != 2 or tg.shape[0] != B or tg.shape[1] != U1 - 1:
        raise ValueError(f"{what}: targets must be (B, U) = ({B}, {U1 - 1}), got {tuple(tg.shape)}")
    if ll.shape[0] != B or tl.shape[0] != B:
        raise ValueError(f"{what}: logit_lengths and target_lengths must hold B = {B} entries")
    inside = torch.arange(U1 - 1, device=dev)[None, :] < tl[:, None]
    bad = (inside & ((tg < 0) | (tg >= V))).sum().to(torch.int32).reshape(1)
    host = torch.cat([ll, tl, bad]).cpu()                  # the one host sync, as in rnnt_loss
    t_lens, u_lens = host[:B], host[B:2 * B]
    if B and (int(t_lens.min()) < 1 or int(t_lens.max()) > T):
        raise ValueError(f"{what}: logit_lengths must lie in [1, {T}] (got {t_lens.tolist()})")
    if B and (int(u_lens.min()) < 0 or int(u_lens.max()) > U1 - 1):
        raise ValueError(f"{what}: target_lengths must lie in [0, {U1 - 1}] (got {u_lens.tolist()})")
    if int(host[-1]) != 0:
        raise ValueError(f"{what}: a label inside target_lengths lies outside [0, {V})")
    tg = torch.where(inside, tg, torch.zeros((), dtype=torch.int32, device=dev)).contiguous()
    return tg, ll, tl


def _blank(blank: int, V: int, what: str) -> int:
    if blank < 0:
        blank = V + blank
    if not 0 <= blank < V:
        raise ValueError(f"{what}: blank must be within [0, {V})")
    return int(blank)


@torch.no_grad()
def rnnt_forced_align(logits: torch.Tensor, targets: torch.Tensor, logit_lengths: torch.Tensor,
                      target_lengths: torch.Tensor, blank: int = 0) -> Tuple[torch.Tensor, torch.Tensor]:
    """Best path of the RNN-T lattice of `logits` (B, T, U+1, V), float32 / float16 / bfloat16, pre-softmax as
    `rnnt_loss` takes them.  targets (B, U); lengths (B,) with 1 <= logit_lengths[b] <= T and
    0 <= target_lengths[b] <= U (the maxima need not equal the padded sizes).  ``blank`` may be any class (negative counts
    from the end).  Returns device tensors (label_frames (B, U) int32: the frame at which label u+1 is emitted, -1 past
    target_lengths[b]; scores (B,) float64: the best path's log-probability)."""
    what = "rnnt_forced_align"
    if logits.dim() != 4:
        raise ValueError(f"{what}: logits must be 4-D (batch, time, target, class)")
    x = logits.detach().contiguous()
    B, T, U1, V = x.shape
    dev = x.device
    blank = _blank(blank, V, what)
    code = _lib.dtype_code(x.dtype)
    tg, ll, tl = _prepare(targets, logit_lengths, target_lengths, B, T, U1, V, dev, what)
    if not x.is_cuda:
        raise RuntimeError(f"wenet_celoss_amd.{what}: logits must live on a HIP device (this package has no CPU path)")
    frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    ws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
    _lib.call("wr_rnnt_align", x, code, tg, ll, tl, B, T, U1, V, blank, frames, scores, ws, ws.numel(), device=dev)
    return frames, scores


@torch.no_grad()
def joint_rnnt_forced_align(ep: torch.Tensor, pp: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor,
                            targets: torch.Tensor, logit_lengths: torch.Tensor, target_lengths: torch.Tensor,
                            blank: int = 0, precision: Optional[str] = None,
                            activation: str = "tanh") -> Tuple[torch.Tensor, torch.Tensor]:
    """rnnt_forced_align(joint_logits(ep, pp, w_out, b_out, precision=..., activation=...), ...) without the logits
    tensor: the joiner forward writes only the row statistics into the RNN-T workspace (`wr_joint_rnnt_stats`, which
    repairs a row spread over more than 88 nats itself) and the Viterbi kernel reads them (`wr_rnnt_align_from_stats`).
    ep (B, T, J), pp (B, U+1, J) as joint_rnnt_loss takes them.  ``precision``: "fp32", "bf16x3", or "autocast" outside
    autocast; the 16-bit single-term modes keep 16-bit logits and are refused (use rnnt_forced_align on the joiner's
    logits)."""
    what = "joint_rnnt_forced_align"
    precision = _call_precision(precision)
    if precision in ("bf16", "f16"):
        raise ValueError(f"{what}: the 16-bit joiner mode {precision!r} keeps 16-bit logits; use "
                         "rnnt_forced_align(joint_logits(...)) (the logits form)")
    ep, pp = ep.detach().float().contiguous(), pp.detach().float().contiguous()
    w, b = w_out.detach().float().contiguous(), b_out.detach().float().contiguous()
    B, T, J = ep.shape
    U1 = pp.shape[1]
    V = w.shape[0]
    dev = ep.device
    if pp.shape[0] != B or pp.shape[2] != J or w.shape[1] != J or b.shape != (V,):
        raise ValueError(f"{what}: ep (B, T, J), pp (B, U+1, J), w_out (V, J) and b_out (V,) do not agree")
    blank = _blank(blank, V, what)
    terms = _PRECISIONS[precision]
    act = activation_code(activation)
    tg, ll, tl = _prepare(targets, logit_lengths, target_lengths, B, T, U1, V, dev, what)
    if not (ep.is_cuda and pp.is_cuda and w.is_cuda and b.is_cuda):
        raise RuntimeError(f"wenet_celoss_amd.{what}: tensors must live on a HIP device (this package has no CPU path)")
    frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    rws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
    ws = joiner_workspace(terms, J, V, dev)
    _lib.call("wr_joint_rnnt_stats", ep, pp, w, b, ll, tl, tg, B, T, U1, J, V, act, blank, terms, ws, ws.numel(), rws,
              rws.numel(), device=dev)
    _lib.call("wr_rnnt_align_from_stats", tg, ll, tl, B, T, U1, frames, scores, rws, rws.numel(), device=dev)
    return frames, scores


def rnnt_frame_tokens(label_frames: torch.Tensor, targets: torch.Tensor, logit_lengths: torch.Tensor,
                      target_lengths: torch.Tensor) -> List[List[List[int]]]:
    """Per utterance, per frame t < logit_lengths[b]: the labels emitted at frame t on the aligned path, in label order
    (an empty list: the frame emits only its blank).  The transducer counterpart of the per-frame list that
    `forced_align` returns for CTC; a frame can emit several labels."""
    fr = label_frames.detach().cpu().tolist()
    tg = targets.detach().cpu().tolist()
    t_lens = logit_lengths.detach().cpu().reshape(-1).tolist()
    u_lens = target_lengths.detach().cpu().reshape(-1).tolist()
    out = []
    for b in range(len(t_lens)):
        per = [[] for _ in range(int(t_lens[b]))]
        for u in range(int(u_lens[b])):
            per[fr[b][u]].append(int(tg[b][u]))
        out.append(per)
    return out
