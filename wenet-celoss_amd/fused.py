"""Joiner + RNN-T loss as ONE autograd node: the loss block of the reference forward
(wenet/transducer/transducer.py:131-147: `self.joint(...)` followed by `torchaudio.functional.rnnt_loss(...)`).

Why one node.  The unfused pair moves the (B, T, U+1, V) logits tensor through HBM five times (joiner write, loss
pass 1 read, gradient pass read + write, joiner backward read).  A joiner forward workgroup owns every column of
its 64 lattice cells, so it can produce the loss's row statistics (denom, skip / emit log-probabilities) in its
epilogue (`wr_joint_fwd_lse`); the loss then only runs its lattice sweeps (`wr_rnnt_loss_fwd_from_lse`) and pass 1,
one full read of the logits, is gone.  Whether that pays is a measurement (see `forward` below): the split-precision
forward takes the epilogue, the exact-fp32 forward runs the loss's own row pass (14 ms per 32 utterances at the BASELINE
shape since the round-2 launch-shape change).  And because
the logits are internal to the node, the gradient pass writes over them: one logits-sized tensor instead of two.

Both nodes launch the joiner forward through `joint.joint_forward` (the one place that picks its entry point) and hand their
logits gradient to `joint.joint_backward`, whose dispatch is the table in `joint.backward_route`.

Results: costs and every gradient agree with the unfused path to fp32 rounding of the row log-sum-exp (the
statistics are merged in a different order); tests/test_fused_gpu.py states the tolerance (1e-6 relative on costs).

Memory-bounded mode (`logits_budget`, `_JointBoundedFn`): no logits tensor at all.  The forward keeps only the row
statistics (`wr_joint_rnnt_stats`: the joiner forward with a statistics-only epilogue) and runs the lattice sweeps
(`wr_rnnt_loss_sweeps`); the backward walks the lattice in slices (`plan_slices`) and, per slice, recomputes the logits
tile by tile and turns them into the loss gradient in the same kernel's epilogue (`wr_joint_rnnt_grad`), then runs the
joiner backward on that slice.  One extra joiner forward's matrix work buys a footprint that does not grow with the batch
("The memory-bounded loss block").  `joint_rnnt_tdt_loss` is the same node with the token-and-duration loss
(`_TdtLoss` in the place of `_RnntLoss`; DESIGN.md, "The memory-bounded TDT loss block").
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .joint import _PRECISIONS, _call_precision, activation_code, joiner_workspace, joint_backward, joint_forward
from .rnnt_lattice import reducer
from .rnnt_loss import call_regularised, check_latency, loss_backward, loss_forward
from .rnnt_tdt import _check_blank, _durations_arg, check_tdt


class _JointRnntFn(torch.autograd.Function):
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, ep, pp, w, b, targets, llens, tlens, blank, clamp, terms, act=0, lam=0.0, pen=0.0):
        if not ep.is_cuda:
            raise RuntimeError("wenet_celoss_amd.joint_rnnt_loss: tensors must live on a HIP device "
                               "(this package has no CPU path)")
        B, T, J = ep.shape
        U1 = pp.shape[1]
        V = w.shape[0]
        dev = ep.device
        ep, pp, w, b = ep.contiguous(), pp.contiguous(), w.contiguous(), b.contiguous()
        logits = torch.empty(B, T, U1, V, dtype=torch.float32, device=dev)
        rws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
        costs = torch.empty(B, dtype=torch.float32, device=dev)
        # Row statistics of the loss: as the joiner forward's epilogue (wr_joint_fwd*_lse) or as the loss's own row pass.
        # Round 2 measured both ways per 8 utterances at the BASELINE shape: the split-precision forward pays 1.7 ms for
        # the epilogue against 3.5 ms for the row pass (epilogue wins); the exact-fp32 forward, since its fragment-layout
        # rewrite, pays 5.6 ms (54.8 against 49.2 ms: the epilogue's vector work does not hide behind the wave's own
        # MFMAs) against the same 3.5 ms (the row pass wins).  WR_FUSED_LSE_EPILOGUE=1 / 0 forces either.
        epi = os.environ.get("WR_FUSED_LSE_EPILOGUE")
        epilogue = (terms != 0) if epi is None else (epi == "1")
        joint_forward(ep, pp, w, b, llens, tlens, terms, act, out=logits, stats=(targets, blank, rws) if epilogue else None)
        if epilogue:               # a delay penalty goes into the stored label arcs before the sweeps
            call_regularised("wr_rnnt_loss_fwd_from_lse", (logits, targets, llens, tlens, B, T, U1, V, blank),
                             (costs, rws, rws.numel()), pen, device=dev)
        else:
            loss_forward(logits, targets, llens, tlens, blank, pen, costs, rws)
        ctx.save_for_backward(ep, pp, w, b, targets, llens, tlens, logits, rws)
        ctx.blank, ctx.clamp, ctx.terms, ctx.act, ctx.lam, ctx.pen = blank, clamp, terms, act, lam, pen
        ctx.logits_hold_gradient = False
        return costs

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_costs):
        ep, pp, w, b, targets, llens, tlens, logits, rws = ctx.saved_tensors
        gc = grad_costs.to(torch.float32).contiguous()
        if ctx.logits_hold_gradient:
            # A second backward through a retained graph (retain_graph=True, per-loss torch.autograd.grad) finds the
            # gradient of the first one where the logits were: the write went through a raw pointer, which autograd's
            # version counter never sees.  The joiner forward is deterministic and its plain / epilogue variants give
            # bit-identical logits, so the node rebuilds them in the same buffer (one forward's time) instead of failing
            # or -- what it did before -- differentiating gradients-as-logits.  The lattice in `rws` is still the first
            # forward's (the gradient pass only reads it).
            joint_forward(ep, pp, w, b, llens, tlens, ctx.terms, ctx.act, out=logits)
            ctx.logits_hold_gradient = False
        # Nothing else holds the logits, so the gradient overwrites them (one logits-sized tensor instead of two).  With
        # round 1's plain loads that cost the gradient pass ~11 % (a line rewritten microseconds after it was read); with
        # the non-temporal loads of round 2 it costs nothing measurable (46.97 / 46.94 against 47.03 / 47.40 ms per
        # 32-utterance step).  WR_FUSED_INPLACE_BYTES=n keeps a separate buffer below n bytes.
        inplace = logits.numel() * logits.element_size() >= int(os.environ.get("WR_FUSED_INPLACE_BYTES", "0"))
        grads = logits if inplace else torch.empty_like(logits)
        loss_backward(logits, targets, llens, tlens, ctx.blank, ctx.clamp, ctx.lam, ctx.pen, gc, grads, rws)
        ctx.logits_hold_gradient = inplace
        d_ep, d_pp, d_w, d_b = joint_backward(grads, ep, pp, w, llens, tlens, ctx.terms, ctx.needs_input_grad[2],
                                              ctx.needs_input_grad[3], gout_zero_in_padding=True, act=ctx.act)
        return d_ep, d_pp, d_w, d_b, None, None, None, None, None, None, None, None, None


class Slice(NamedTuple):
    """Part of the (B, T, U1) lattice the memory-bounded backward handles at once: utterances [b0, b1), frames [t0, t1)
    of each.  Either a run of whole utterances (t0 = 0, t1 = T: the view ep[b0:b1] is contiguous, so the buffer also
    holds their padded frames, which get a zero gradient and count against the budget) or one utterance's frames
    [t0, t1) with t1 <= its length (b1 = b0 + 1)."""
    b0: int
    b1: int
    t0: int
    t1: int

    def cells(self, U1: int) -> int:
        return (self.b1 - self.b0) * (self.t1 - self.t0) * U1


def plan_slices(t_lens, u_lens, T: int, U1: int, V: int, budget_bytes: int) -> List[Slice]:
    """Cut the lattice of a batch into slices whose fp32 logits gradient, (cells x V) floats, fits `budget_bytes`.

    Utterances are taken in order.  An utterance whose T x U1 cells fit the budget joins the current run of whole
    utterances while the run still fits (else it starts a new one); one that does not fit is cut into frame ranges of
    budget // (4 V U1) frames over [0, T_b).  Frames at or past T_b belong to no frame range, and an utterance with
    T_b = 0 has no cell and no slice.  `u_lens` is accepted for symmetry with plan_buckets: the label axis is never cut.
    Raises ValueError when the budget holds less than one frame row (U1 x V x 4 bytes)."""
    del u_lens
    cap = int(budget_bytes) // (4 * V)
    row = U1 * V * 4
    if cap < U1:
        raise ValueError(f"logits_budget={budget_bytes} bytes is below one frame row of the lattice: at least "
                         f"U1 * V * 4 = {U1} * {V} * 4 = {row} bytes are needed")
    whole = T * U1
    slices: List[Slice] = []
    run0 = None                                   # first utterance of the open run
    for b, tb in enumerate(int(x) for x in t_lens):
        if run0 is not None and (tb == 0 or whole > cap or (b + 1 - run0) * whole > cap):
            slices.append(Slice(run0, b, 0, T))
            run0 = None
        if tb == 0:
            continue
        if whole <= cap:
            if run0 is None:
                run0 = b
            continue
        step = cap // U1
        for t0 in range(0, tb, step):
            slices.append(Slice(b, b + 1, t0, min(t0 + step, tb)))
    if run0 is not None:
        slices.append(Slice(run0, len(t_lens), 0, T))
    return slices


# What the memory-bounded node asks of its loss.  `head` is (ep, pp, w, b, llens, tlens, targets) and `dims`
# (B, T, U1, J, row width) throughout: the arguments every joiner + loss entry point begins with.
@dataclass(frozen=True)
class _RnntLoss:
    """The RNN-T loss in the memory-bounded node: rows of V logits, a joiner of `terms`."""
    blank: int
    clamp: float
    terms: int
    lam: float
    pen: float
    what = "joint_rnnt_loss"

    def workspace(self, B, T, U1, dev):
        return _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)

    def forward(self, head, dims, act, ws, lws, costs, dev):
        """Row statistics into the loss workspace `lws`, then the lattice sweeps into `costs`."""
        _lib.call("wr_joint_rnnt_stats", *head, *dims, act, self.blank, self.terms, ws, ws.numel(), lws, lws.numel(),
                  device=dev)
        call_regularised("wr_rnnt_loss_sweeps", (head[4], head[5], *dims[:3]), (costs, lws, lws.numel()), self.pen, device=dev)

    def grad(self, head, dims, act, gc, lws, begin, end, g, ws, w_ready, dev):
        """The loss gradient of the recomputed logits of lattice cells [begin, end) into `g`."""
        call_regularised("wr_joint_rnnt_grad", (*head, *dims, act, self.blank, float(self.clamp), self.terms),
                         (gc, lws, lws.numel(), begin, end, g, ws, ws.numel(), w_ready), self.pen, self.lam, device=dev)


@dataclass(frozen=True)
class _TdtLoss:
    """The token-and-duration loss in the memory-bounded node: rows of W = V + D logits, the exact fp32 joiner only.
    `durs` is the durations as the library takes them (`_durations_arg`), built once per call of the public function."""
    blank: int
    durs: object
    D: int
    sigma: float
    terms = 0
    what = "joint_rnnt_tdt_loss"

    def workspace(self, B, T, U1, dev):
        return _lib.workspace("wr_rnnt_tdt_workspace_bytes", B, T, U1, self.D, device=dev)

    def forward(self, head, dims, act, ws, lws, costs, dev):
        _lib.call("wr_joint_tdt_stats", *head, *dims, act, self.blank, self.durs, self.D, self.sigma, ws, ws.numel(), lws,
                  lws.numel(), device=dev)
        _lib.call("wr_rnnt_tdt_sweeps", head[4], head[5], *dims[:3], self.durs, self.D, costs, lws, lws.numel(), device=dev)

    def grad(self, head, dims, act, gc, lws, begin, end, g, ws, w_ready, dev):
        _lib.call("wr_joint_tdt_grad", *head, *dims, act, self.blank, self.durs, self.D, self.sigma, gc, lws, lws.numel(),
                  begin, end, g, ws, ws.numel(), w_ready, device=dev)


class _JointBoundedFn(torch.autograd.Function):
    """Joiner + loss with no logits tensor (joint_rnnt_loss(..., logits_budget=n) with an `_RnntLoss`, joint_rnnt_tdt_loss
    with a `_TdtLoss`).  Saves ep, pp, w, b, the lengths and the loss's workspace; `slices` (plan_slices) and the host
    lengths come from the caller's one length sync."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, ep, pp, w, b, targets, llens, tlens, loss, act, slices, host_t, host_u):
        if not ep.is_cuda:
            raise RuntimeError(f"wenet_celoss_amd.{loss.what}: tensors must live on a HIP device "
                               "(this package has no CPU path)")
        B, T, J = ep.shape
        U1 = pp.shape[1]
        W = w.shape[0]                              # the row width: V, or V + D for the TDT loss
        dev = ep.device
        ep, pp, w, b = ep.contiguous(), pp.contiguous(), w.contiguous(), b.contiguous()
        lws = loss.workspace(B, T, U1, dev)
        costs = torch.empty(B, dtype=torch.float32, device=dev)
        ws = joiner_workspace(loss.terms, J, W, dev)
        loss.forward((ep, pp, w, b, llens, tlens, targets), (B, T, U1, J, W), act, ws, lws, costs, dev)
        ctx.save_for_backward(ep, pp, w, b, targets, llens, tlens, lws)
        ctx.slice_lens = _slice_lengths(slices, host_t, host_u, dev)
        ctx.slices, ctx.loss, ctx.act = slices, loss, act
        return costs

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_costs):
        ep, pp, w, b, targets, llens, tlens, lws = ctx.saved_tensors
        B, T, J = ep.shape
        U1 = pp.shape[1]
        W = w.shape[0]
        dev = ep.device
        loss, act = ctx.loss, ctx.act
        need_w, need_b = ctx.needs_input_grad[2], ctx.needs_input_grad[3]
        gc = grad_costs.to(torch.float32).contiguous()
        d_ep = torch.zeros_like(ep)                 # utterances without a slice (no frame) keep zero gradients
        d_pp = torch.zeros_like(pp)
        d_w = torch.zeros(W, J, dtype=torch.float32, device=dev) if need_w else None
        d_b = torch.zeros(W, dtype=torch.float32, device=dev) if need_b else None
        none = (None,) * 8                          # one per non-tensor input of forward
        slices = ctx.slices
        if not slices:
            return (d_ep, d_pp, d_w, d_b) + none
        nmax = max(s.cells(U1) for s in slices)
        # buffers sized to the largest slice, allocated once per backward
        g = torch.empty(nmax * W, dtype=torch.float32, device=dev)
        dz = torch.empty(nmax * J, dtype=torch.float32, device=dev)
        h = torch.empty(nmax * J, dtype=torch.float32, device=dev) if need_w else None
        ws = joiner_workspace(loss.terms, J, W, dev)
        nl = ctx.slice_lens.numel() // 2
        k = 0
        for i, s in enumerate(slices):
            nb, nt = s.b1 - s.b0, s.t1 - s.t0
            cells = nb * nt * U1
            begin = (s.b0 * T + s.t0) * U1
            loss.grad((ep, pp, w, b, llens, tlens, targets), (B, T, U1, J, W), act, gc, lws, begin, begin + cells, g, ws,
                      int(i > 0), dev)
            ll = ctx.slice_lens[k:k + nb]
            tl = ctx.slice_lens[nl + k:nl + k + nb]
            k += nb
            de, dp, dw, db = joint_backward(g[:cells * W].view(nb, nt, U1, W), ep[s.b0:s.b1, s.t0:s.t1], pp[s.b0:s.b1], w,
                                            ll, tl, loss.terms, need_w, need_b, gout_zero_in_padding=True, act=act,
                                            dz_out=dz[:cells * J].view(nb, nt, U1, J),
                                            h_out=h[:cells * J].view(nb, nt, U1, J) if need_w else None)
            d_ep[s.b0:s.b1, s.t0:s.t1] = de
            d_pp[s.b0:s.b1] += dp
            if need_w:
                d_w += dw
            if need_b:
                d_b += db
        return (d_ep, d_pp, d_w, d_b) + none


def _slice_lengths(slices, host_t, host_u, dev):
    """Per-slice length arrays of a bounded node, built once on the host from the caller's length sync:
    [ll of every slice's utterances | tl of them], on `dev`."""
    ll_s, tl_s = [], []
    for s in slices:
        for u in range(s.b0, s.b1):
            ll_s.append(min(host_t[u], s.t1) - s.t0)
            tl_s.append(host_u[u])
    lens = torch.tensor(ll_s + tl_s, dtype=torch.int32)
    with torch.cuda.device(dev):
        return lens.pin_memory().to(dev, non_blocking=True) if lens.numel() else lens.to(dev)


def _lengths(what: str, ep, pp, targets, logit_lengths, target_lengths):
    """The prologue of the two public functions -> (tg, ll, tl, lens): targets, logit_lengths and target_lengths as int32
    on ep's device, and `lens`, a (2, B) CPU tensor [T_b | U_b] from the one host sync.  Like torchaudio's rnnt_loss it
    wants max(T_b) == T and max(U_b) + 1 == U1 (RuntimeError)."""
    dev = ep.device
    tg = targets.to(device=dev, dtype=torch.int32).contiguous()
    ll = logit_lengths.to(device=dev, dtype=torch.int32).contiguous()
    tl = target_lengths.to(device=dev, dtype=torch.int32).contiguous()
    B, T = ep.shape[0], ep.shape[1]
    U1 = pp.shape[1]
    if not (tg.dim() == 2 and tg.shape == (B, U1 - 1) and ll.shape == (B,) and tl.shape == (B,)):
        raise RuntimeError(f"{what}: targets must be (B, U) and lengths (B,) for ep (B,T,J), pp (B,U+1,J)")
    lens = torch.stack([ll, tl]).cpu()                      # the one host sync, as in rnnt_loss
    if int(lens[0].max()) != T:
        raise RuntimeError("input length mismatch")
    if int(lens[1].max()) + 1 != U1:
        raise RuntimeError("output length mismatch")
    if int(lens.min()) < 0:
        raise RuntimeError("lengths must be non-negative")
    return tg, ll, tl, lens


def joint_rnnt_tdt_loss(ep: torch.Tensor, pp: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor,
                        targets: torch.Tensor, logit_lengths: torch.Tensor, target_lengths: torch.Tensor,
                        durations: Sequence[int], blank: int = 0, sigma: float = 0.0, reduction: str = "mean",
                        activation: str = "tanh", precision: str = "fp32", *, logits_budget: int) -> torch.Tensor:
    """rnnt_tdt_loss(ffn_out(act(ep[:, :, None] + pp[:, None])), targets, logit_lengths, target_lengths, durations) with
    no logits tensor at all: the memory-bounded node (`_JointBoundedFn`).  ep (B, T, J), pp (B, U+1, J), and a joiner
    of W = V + len(durations) outputs (w_out (W, J), b_out (W,)): columns [0, V) token logits, the rest duration logits.
    targets (B, U) int32, lengths (B,) int32, max(logit_lengths) == T and max(target_lengths) == U as in
    `joint_rnnt_loss`; ``durations``, ``blank`` in [0, V), ``sigma`` and ``reduction`` as in `rnnt_tdt_loss`.  An utterance
    with T_b = 0 has no slice and costs 0; one without a path costs +inf.
    ``logits_budget`` (bytes, required): the backward recomputes the logits in slices whose fp32 gradient buffer holds at
    most this many bytes (`plan_slices` on rows of W floats; ValueError below one frame row, U1 * W * 4 bytes).
    ``precision``: "fp32" only -- any other joiner precision raises ValueError.  Ragged batches are not bucketed here."""
    what = "joint_rnnt_tdt_loss"
    reduce = reducer(reduction)
    durs, sg = check_tdt(what, durations, sigma)
    if precision != "fp32":
        raise ValueError(f"{what}: precision {precision!r} is not supported, the memory-bounded TDT node runs the exact "
                         "\"fp32\" joiner only")
    W, D = w_out.shape[0], len(durs)
    if W - D < 2:
        raise ValueError(f"{what}: a joiner of {W} outputs with {D} durations leaves {W - D} token columns (at least 2 are "
                         "needed)")
    blank = _check_blank(what, blank, W - D)
    act = activation_code(activation)
    tg, ll, tl, lens = _lengths(what, ep, pp, targets, logit_lengths, target_lengths)
    host_t, host_u = lens[0].tolist(), lens[1].tolist()
    slices = plan_slices(host_t, host_u, ep.shape[1], pp.shape[1], W, int(logits_budget))   # a bad budget fails before any launch
    loss = _TdtLoss(blank, _durations_arg(durs), D, sg)
    return reduce(_JointBoundedFn.apply(ep, pp, w_out, b_out, tg, ll, tl, loss, act, slices, host_t, host_u))


def plan_buckets(t_lens, u_lens, max_buckets: int = 4, min_gain: float = 0.08, min_cells: int = 20000):
    """Group utterances by label length so that each group is padded to its own maxima.

    The joiner kernels skip 64- / 256-cell tiles that lie wholly in padding, which removes the frames beyond an
    utterance's length (runs of U+1 cells) but not the label positions beyond its label count (short runs inside every
    frame): their cost is B * T * (Umax + 1) whatever the individual label counts are.  Sorting the batch by label count
    and cutting it into a few groups, each a joiner + loss call of its own padded to ITS longest label sequence (and
    frame count), removes most of that padding; per-utterance costs and gradients do not change (utterances are
    independent; the weight gradient is the sum over the groups).

    Returns a list of index lists (ascending label length), or None when one call is best: dynamic programming over the
    sorted order with cost sum_g n_g * maxT_g * (maxU_g + 1), at most `max_buckets` groups, and the split must save at
    least `min_gain` of the cells; batches of fewer than `min_cells` lattice cells (a couple of milliseconds of joiner
    work, e.g. the n-best list of a rescoring call) are not worth the extra launches."""
    n = len(t_lens)
    order = sorted(range(n), key=lambda i: (u_lens[i], t_lens[i]))
    whole = n * max(t_lens) * (max(u_lens) + 1)
    if n < 2 or whole < max(min_cells, 1):
        return None
    us = np.asarray([u_lens[i] for i in order], dtype=np.int64)
    ts = np.asarray([t_lens[i] for i in order], dtype=np.int64)
    # cost[a, b] of the group of sorted positions [a, b) = (b - a) * max(ts[a:b]) * (us[b - 1] + 1): the running
    # maximum per start index makes it one vector operation per row (the host runs this every training step; the
    # first version recomputed max(ts[a:b]) inside a triple Python loop, 1 s at 512 utterances).
    INF = np.iinfo(np.int64).max // 4
    cost = np.full((n + 1, n + 1), INF, dtype=np.int64)
    width = us + 1
    for a in range(n):
        cnt = np.arange(1, n - a + 1, dtype=np.int64)
        cost[a, a + 1:] = cnt * np.maximum.accumulate(ts[a:]) * width[a:]
    best = np.full((max_buckets + 1, n + 1), INF, dtype=np.int64)
    cut = np.zeros((max_buckets + 1, n + 1), dtype=np.int64)
    best[0, 0] = 0
    for g in range(1, max_buckets + 1):
        cand = np.minimum(best[g - 1][:, None] + cost, INF)       # [a, b]; INF rows / entries stay INF
        cut[g] = cand.argmin(axis=0)                                # first minimum = smallest a, as the scalar loop did
        best[g] = cand[cut[g], np.arange(n + 1)]
    g_best = min(range(1, max_buckets + 1), key=lambda g: int(best[g][n]))
    if g_best == 1 or best[g_best][n] > (1.0 - min_gain) * whole:
        return None
    groups, b = [], n
    for g in range(g_best, 0, -1):
        a = int(cut[g][b])
        groups.append(order[a:b])
        b = a
    return groups[::-1]


def per_bucket(groups, lens, dev, part, restore_order: bool = True) -> torch.Tensor:
    """The costs of the groups of `plan_buckets` as one tensor.  Each group's come from part(idx, g, tmax, umax): its
    utterances as an index tensor on `dev` and as a list, and its own longest frame and label count, read from the host
    lengths `lens` (2, B).  They come back in the caller's utterance order (differentiable), or in bucket order with
    `restore_order` off."""
    parts, index = [], []
    for g in groups:
        idx = torch.tensor(g, device=dev)
        parts.append(part(idx, g, int(lens[0][g].max()), int(lens[1][g].max())))
        index.append(idx)
    costs = torch.cat(parts)
    return costs[torch.argsort(torch.cat(index))] if restore_order else costs


def joint_rnnt_loss(ep: torch.Tensor, pp: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor,
                    targets: torch.Tensor, logit_lengths: torch.Tensor, target_lengths: torch.Tensor, blank: int = 0,
                    clamp: float = -1.0, reduction: str = "mean", precision: Optional[str] = None,
                    buckets: Optional[int] = None, activation: str = "tanh",
                    logits_budget: Optional[int] = None, *, fastemit_lambda: float = 0.0,
                    delay_penalty: float = 0.0) -> torch.Tensor:
    """rnnt_loss(ffn_out(act(ep[:, :, None] + pp[:, None])), targets, logit_lengths, target_lengths) without the
    logits ever leaving the node.  ep (B, T, J) = enc_ffn(encoder_out), pp (B, U+1, J) = pred_ffn(predictor_out);
    targets (B, U) int32 with padding already mapped to a valid class; lengths (B,) int32; requires
    max(logit_lengths) == T and max(target_lengths) + 1 == U+1 like torchaudio's rnnt_loss.
    ``precision``: "fp32" (exact MFMA, default), "bf16x3" (split precision, joint.py) or "autocast" outside autocast (= "fp32");
    the 16-bit modes are refused; reduction as rnnt_loss.
    ``buckets``: at most this many groups by label length, each padded to its own maxima (`plan_buckets`; default from
    WR_FUSED_BUCKETS, 4; 1 = one call for the whole batch).  Costs come back in the caller's utterance order.
    ``logits_budget``: None (default) = the node above; an int = the memory-bounded node (`_JointBoundedFn`): no
    logits tensor, the backward recomputes the logits in slices whose gradient buffer holds at most this many bytes
    (`plan_slices`; ValueError below one frame row, U1 * V * 4 bytes).  "fp32" and "bf16x3" only, as the node above.
    ``fastemit_lambda`` / ``delay_penalty``: as `rnnt_loss` takes them, in either node (FastEmit scales the gradient of
    the label arcs by 1 + lambda and leaves the costs bit-identical; the delay penalty is inside the costs).  The
    penalty uses each utterance's own length, so buckets and slices do not change it."""
    reduce = reducer(reduction)
    lam, pen = check_latency("joint_rnnt_loss", fastemit_lambda, delay_penalty)
    precision = _call_precision(precision)             # "autocast": "fp32" outside autocast, a 16-bit mode under it
    if precision in ("bf16", "f16"):
        raise ValueError("joint_rnnt_loss: the AMP single-term mode keeps 16-bit logits; use TransducerJoint + rnnt_loss")
    V = w_out.shape[0]
    if blank < 0:
        blank = V + blank
    if not 0 <= blank < V:
        raise RuntimeError("blank must be within [0, logits.shape[-1])")
    tg, ll, tl, lens = _lengths("joint_rnnt_loss", ep, pp, targets, logit_lengths, target_lengths)
    if buckets is None:
        buckets = int(os.environ.get("WR_FUSED_BUCKETS", "4"))
    groups = plan_buckets(lens[0].tolist(), lens[1].tolist(), max_buckets=buckets) if buckets > 1 else None
    terms = _PRECISIONS[precision]
    act = activation_code(activation)

    def node(ep_, pp_, tg_, ll_, tl_, host_t, host_u):
        if logits_budget is None:
            return _JointRnntFn.apply(ep_, pp_, w_out, b_out, tg_, ll_, tl_, int(blank), float(clamp), terms, act, lam, pen)
        slices = plan_slices(host_t, host_u, ep_.shape[1], pp_.shape[1], V, int(logits_budget))
        return _JointBoundedFn.apply(ep_, pp_, w_out, b_out, tg_, ll_, tl_,
                                     _RnntLoss(int(blank), float(clamp), terms, lam, pen), act, slices, host_t, host_u)

    if logits_budget is not None:      # a bad budget fails before any launch
        plan_slices(lens[0].tolist(), lens[1].tolist(), ep.shape[1], pp.shape[1], V, int(logits_budget))
    if groups is None:
        return reduce(node(ep, pp, tg, ll, tl, lens[0].tolist(), lens[1].tolist()))
    return reduce(per_bucket(groups, lens, ep.device, lambda idx, g, tmax, umax: node(
        ep[idx, :tmax], pp[idx, :umax + 1], tg[idx, :umax].contiguous(), ll[idx].contiguous(), tl[idx].contiguous(),
        lens[0][g].tolist(), lens[1][g].tolist())))
