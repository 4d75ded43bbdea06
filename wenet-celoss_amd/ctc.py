"""CTC module with the reference's interface, backed by the HIP kernels.

Mirror of ``wenet/transformer/ctc.py:21-84``: same constructor arguments, same
parameter names (``ctc_lo.weight/bias`` so reference checkpoints load), same
``forward(hs_pad, hlens, ys_pad, ys_lens)`` result
(``CTCLoss(reduction='sum')(log_softmax(ctc_lo(dropout(hs_pad)))) / B``), same
``log_softmax`` / ``argmax`` helpers.  The ``ctc_lo`` projection is a plain
library GEMM (torch.nn.Linear on rocBLAS); log-softmax, the alpha/beta lattice
and the gradient w.r.t. the projection output are the fused HIP path
(``wr_ctc_loss_fwd/bwd``).  Quirk kept: ``F.dropout`` is called with its default
``training=True`` (ctc.py:57), so a non-zero ``dropout_rate`` applies in eval too.

CPU tensors (BASELINE config 1: "torch.nn.CTCLoss on CPU, plumbing, runs without a
GPU"): ``CTC.forward`` then executes the reference's own statement sequence --
``log_softmax(2)`` + stock ``torch.nn.CTCLoss`` (ctc.py:44,58-63) -- on PyTorch's CPU
kernels.  That is the reference's call, not a port of the HIP path; the functional
``ctc_loss`` and every other entry point of this package keep raising on CPU tensors.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib


class _CTCLossFn(torch.autograd.Function):
    # Under AMP ctc_lo produces fp16/bf16; the reference's log_softmax autocasts to fp32 (ctc.py:60), so do we.
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, logits, targets, input_lengths, target_lengths, blank):
        if not logits.is_cuda:
            raise RuntimeError("wenet_celoss_amd.ctc_loss: logits must live on a HIP device "
                               "(this package has no CPU path)")
        B, T, V = logits.shape
        S = targets.shape[1]
        dev = logits.device
        ws = _lib.workspace("wr_ctc_workspace_bytes", B, T, S, device=dev)
        nll = torch.empty(B, dtype=torch.float32, device=dev)
        _lib.call("wr_ctc_loss_fwd", logits, _lib.dtype_code(logits.dtype), targets, input_lengths, target_lengths, B, T, S, V,
                  blank, nll, ws, ws.numel(), device=dev)
        ctx.save_for_backward(logits, targets, input_lengths, target_lengths, ws)
        ctx.blank = blank
        return nll

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, grad_nll):
        logits, targets, input_lengths, target_lengths, ws = ctx.saved_tensors
        B, T, V = logits.shape
        S = targets.shape[1]
        dev = logits.device
        grads = torch.empty_like(logits)
        g = grad_nll.to(torch.float32).contiguous()
        _lib.call("wr_ctc_loss_bwd", logits, _lib.dtype_code(logits.dtype), targets, input_lengths, target_lengths, B, T, S, V,
                  ctx.blank, g, grads, ws, ws.numel(), device=dev)
        return grads, None, None, None, None


def ctc_loss(logits: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
             target_lengths: torch.Tensor, blank: int = 0, reduction: str = "sum") -> torch.Tensor:
    """Fused log-softmax + CTC loss on batch-major pre-softmax activations.

    logits (B, T, V) float32; targets (B, S) any integer dtype, padded with
    anything (``IGNORE_ID`` = -1 in the reference, processor.py:722-724);
    lengths (B,).  reduction: 'none' | 'sum' | 'mean' (mean as torch.nn.CTCLoss:
    nll / target_length, then batch mean).
    """
    if reduction not in ("none", "sum", "mean"):
        raise ValueError(f"{reduction} is not a valid value for reduction")
    if logits.dim() != 3:
        raise RuntimeError("ctc_loss: logits must be (batch, time, vocab)")
    B = logits.size(0)
    if targets.dim() == 1:
        raise RuntimeError("ctc_loss: concatenated 1-D targets are not supported; pass (batch, max_len)")
    if not (input_lengths.numel() == B and target_lengths.numel() == B and targets.size(0) == B):
        raise RuntimeError("ctc_loss: batch size mismatch between logits, targets and lengths")
    dev = logits.device
    tg = targets.to(device=dev, dtype=torch.int32)
    tg = torch.where(tg < 0, torch.zeros_like(tg), tg).contiguous()
    if tg.size(1) == 0:
        tg = torch.zeros(B, 1, dtype=torch.int32, device=dev)
    il = input_lengths.to(device=dev, dtype=torch.int32).contiguous()
    tl = target_lengths.to(device=dev, dtype=torch.int32).contiguous()
    if logits.dtype != torch.float32:
        logits = logits.float()             # fp16/bf16 activations (AMP or not): the CTC kernels take fp32; the
                                            # cast is differentiable, so the gradient returns in the input dtype
    nll = _CTCLossFn.apply(logits.contiguous(), tg, il, tl, int(blank))
    if reduction == "sum":
        return nll.sum()
    if reduction == "mean":
        return (nll / tl.clamp(min=1).to(nll.dtype)).mean()
    return nll


def ctc_greedy_search(logits: torch.Tensor, lens: torch.Tensor, blank: int = 0, eos: int = -1):
    """ASRModel.ctc_greedy_search (wenet/transformer/asr_model.py:281-324) from the ctc_lo output (B, T, V) on:
    returns (hyps: List[List[int]], scores (B,)).  eos defaults to V-1 (asr_model.py:52-53)."""
    if not logits.is_cuda:
        raise RuntimeError("wenet_celoss_amd.ctc_greedy_search: logits must live on a HIP device (no CPU path)")
    x = logits.detach().float().contiguous()
    B, T, V = x.shape
    dev = x.device
    ln = lens.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    ws = _lib.workspace("wr_ctc_decode_workspace_bytes", B, T, 1, device=dev)
    hyps = torch.empty(B, T, dtype=torch.int32, device=dev)
    hl = torch.empty(B, dtype=torch.int32, device=dev)
    sc = torch.empty(B, dtype=torch.float32, device=dev)
    _lib.call("wr_ctc_greedy_search", x, ln, B, T, V, int(blank), int(eos if eos >= 0 else V - 1), hyps, hl, sc, ws,
              ws.numel(), device=dev)
    hc, lc = hyps.cpu(), hl.cpu().tolist()
    return [hc[b, :lc[b]].tolist() for b in range(B)], sc


def ctc_prefix_beam_search(logits: torch.Tensor, lens: torch.Tensor, beam_size: int, blank: int = 0):
    """ASRModel._ctc_prefix_beam_search (asr_model.py:326-409) from the ctc_lo output (B, T, V) on.
    Per utterance: [(prefix tuple, score)] best first (the reference's `hyps` for batch size 1)."""
    if not logits.is_cuda:
        raise RuntimeError("wenet_celoss_amd.ctc_prefix_beam_search: logits must live on a HIP device (no CPU path)")
    x = logits.detach().float().contiguous()
    B, T, V = x.shape
    dev = x.device
    ln = lens.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    ws = _lib.workspace("wr_ctc_decode_workspace_bytes", B, T, beam_size, device=dev)
    hyps = torch.empty(B, beam_size, T, dtype=torch.int32, device=dev)
    hl = torch.empty(B, beam_size, dtype=torch.int32, device=dev)
    sc = torch.empty(B, beam_size, dtype=torch.float64, device=dev)
    nh = torch.empty(B, dtype=torch.int32, device=dev)
    _lib.call("wr_ctc_prefix_beam_search", x, ln, B, T, V, int(beam_size), int(blank), hyps, hl, sc, nh, ws, ws.numel(),
              device=dev)
    hc, lc, scc, nc = hyps.cpu(), hl.cpu().tolist(), sc.cpu().tolist(), nh.cpu().tolist()
    return [[(tuple(hc[b, e, :lc[b][e]].tolist()), scc[b][e]) for e in range(nc[b])] for b in range(B)]


class CtcPrefixBeamStream:
    """CTC prefix beam search continued chunk by chunk, for `n_streams` streams at once, with the Viterbi score and
    the frame of every token of each hypothesis (runtime/core/decoder/ctc_prefix_beam_search.cc:107-211: `Search()` per
    encoder chunk, `viterbi_likelihood()`, `Times()`; the contract is in include/wr_api.h, "Streaming CTC prefix beam
    search").  Owns the state block; `max_frames` bounds the frames (chunk widths summed) between two resets.

    search(logits_chunk (n_streams, T, V) pre-softmax, lens (n_streams,)) consumes lens[b] <= T frames of stream b
    (0 leaves it untouched) and returns per stream [(tokens tuple, score, viterbi_score, times tuple)], best first;
    `frames` then holds the frames each stream has consumed.  `state`: a caller's uint8 device tensor to use as the
    state block (at least wr_ctc_stream_state_bytes(n_streams, beam_size, max_frames) bytes) instead of one allocated by
    the first search; whatever it holds, a new object or a reset() starts every stream fresh."""

    # what the biased stream (CtcContextPrefixBeamStream) does differently: the size of its block and its entry point
    _state_query, _entry = "wr_ctc_stream_state_bytes", "wr_ctc_prefix_beam_search_chunk"

    def __init__(self, n_streams: int, beam_size: int, max_frames: int, blank: int = 0, state: torch.Tensor = None):
        self.n_streams, self.beam_size, self.max_frames, self.blank = int(n_streams), int(beam_size), int(max_frames), int(blank)
        self._name = type(self).__name__            # every message names the class that raised it
        if self.n_streams < 1 or self.max_frames < 1 or not 1 <= self.beam_size <= 16:
            raise RuntimeError(f"{self._name}: n_streams={n_streams}, beam_size={beam_size} (1..16), "
                               f"max_frames={max_frames} must be positive")
        self._state = state             # allocated by the first search (on the chunk's device) unless the caller lends one
        self._vocab = None
        self.reset()

    def reset(self) -> None:
        """Every stream starts fresh with the next search."""
        self._fresh = True
        self._frames_done = 0
        self.frames = [0] * self.n_streams

    def search(self, logits_chunk: torch.Tensor, lens: torch.Tensor):
        return self._search(logits_chunk, lens)

    # the two hooks of the biased stream
    def _more(self, B, dev, finalize):
        """(what the entry point takes between the state block and the outputs, the outputs it writes behind them)"""
        return (), ()

    def _result(self, rows):
        """`rows`, the result of `_call`, completed from the further outputs"""
        return rows

    def _search(self, logits_chunk, lens, finalize=None):
        name = self._name
        if logits_chunk.dim() != 3:
            raise RuntimeError(f"{name}: the chunk must be (n_streams, frames, vocab)")
        B, T, V = logits_chunk.shape
        if B != self.n_streams:
            raise RuntimeError(f"{name}: chunk has {B} streams, the stream set has {self.n_streams}")
        if self._vocab is not None and V != self._vocab:
            raise RuntimeError(f"{name}: vocabulary changed from {self._vocab} to {V}")
        if self._frames_done + T > self.max_frames:
            raise RuntimeError(f"{name}: {self._frames_done} frames done + a chunk of {T} exceeds max_frames={self.max_frames}")
        if not logits_chunk.is_cuda:
            raise RuntimeError(f"wenet_celoss_amd.{name}: logits must live on a HIP device (no CPU path)")
        out = self._call(logits_chunk.detach().float().contiguous(), lens, self._frames_done, finalize)
        self._frames_done += T
        self._vocab = V
        return out

    def _call(self, x, lens, frames_done, finalize):
        """One call of the entry point on chunk `x` (`finalize` is the biased stream's, for `_more`) -> per stream
        [(tokens, score, viterbi_score, times)], passed through `_result`."""
        B, T, V = x.shape
        dev = x.device
        beam, cap = self.beam_size, self.max_frames
        need = getattr(_lib.load(), self._state_query)(B, beam, cap)
        if self._state is None:
            self._state = torch.empty(need, dtype=torch.uint8, device=dev)
        elif self._state.device != dev or self._state.numel() < need or self._state.dtype != torch.uint8:
            raise RuntimeError(f"{self._name}: the state tensor must be uint8 on {dev} with at least {need} bytes")
        ln = lens.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if ln.numel() != B:
            raise RuntimeError(f"{self._name}: lens has {ln.numel()} elements for {B} streams")
        ws = _lib.workspace("wr_ctc_stream_workspace_bytes", B, T, beam, device=dev)
        hyps = torch.empty(B, beam, cap, dtype=torch.int32, device=dev)
        tm = torch.empty(B, beam, cap, dtype=torch.int32, device=dev)
        hl = torch.empty(B, beam, dtype=torch.int32, device=dev)
        sc = torch.empty(B, beam, dtype=torch.float64, device=dev)
        vt = torch.empty(B, beam, dtype=torch.float64, device=dev)
        nh = torch.empty(B, dtype=torch.int32, device=dev)
        nf = torch.empty(B, dtype=torch.int32, device=dev)
        graph_args, more_outputs = self._more(B, dev, finalize)
        _lib.call(self._entry, x, ln, B, T, V, beam, self.blank, int(self._fresh), frames_done, cap, self._state,
                  self._state.numel(), *graph_args, hyps, hl, sc, vt, tm, nh, nf, *more_outputs, ws, ws.numel(), device=dev)
        self._fresh = False
        lc, scc, vtc, nc = hl.cpu().tolist(), sc.cpu().tolist(), vt.cpu().tolist(), nh.cpu().tolist()
        self.frames = nf.cpu().tolist()
        width = max(max(row) for row in lc)
        hc, tc = hyps[:, :, :width].cpu().tolist(), tm[:, :, :width].cpu().tolist()      # nested lists: one conversion each
        return self._result([[(tuple(hc[b][e][:lc[b][e]]), scc[b][e], vtc[b][e], tuple(tc[b][e][:lc[b][e]]))
                              for e in range(nc[b])] for b in range(B)], *more_outputs)


def ctc_prefix_beam_search_times(logits: torch.Tensor, lens: torch.Tensor, beam_size: int, blank: int = 0):
    """ctc_prefix_beam_search over whole utterances (B, T, V) with, per hypothesis, the Viterbi score and the frame of
    every token: per utterance [(prefix tuple, score, viterbi_score, times tuple)] best first.  Prefixes and scores
    are those of ctc_prefix_beam_search, which stays the entry point when the times are not needed."""
    if not logits.is_cuda:
        raise RuntimeError("wenet_celoss_amd.ctc_prefix_beam_search_times: logits must live on a HIP device (no CPU path)")
    return CtcPrefixBeamStream(logits.shape[0], beam_size, logits.shape[1], blank=blank).search(logits, lens)


class CtcContextPrefixBeamStream(CtcPrefixBeamStream):
    """CtcPrefixBeamStream with the context-graph phrase biasing of the reference runtime (context_graph.cc,
    ctc_prefix_beam_search.cc:137-193, 213-234; the contract is in include/wr_api.h, "Context-graph biasing in the CTC
    prefix beam search"): every hypothesis walks `context_graph` (a ContextGraph) and the beam is pruned by score plus
    bonus.  Owns its own state block (wr_ctc_context_stream_state_bytes); `state` lends one, as in CtcPrefixBeamStream.

    search(logits_chunk, lens, finalize=False) returns per stream [(tokens, score, viterbi_score, times, ctc_score,
    context_score, tags)], best first, with score = ctc_score + context_score and one tag per token (bit 0: a phrase
    starts at this token, bit 1: a phrase ends at it).  finalize=True exports as if the stream ended here: a partial
    match gives its bonus back and the list is sorted again; the stream itself is not changed, so it may go on.
    finalize() does that without new frames.  `context_states` holds, per stream, the graph states of the last result."""

    _state_query, _entry = "wr_ctc_context_stream_state_bytes", "wr_ctc_prefix_beam_search_context_chunk"

    def __init__(self, n_streams: int, beam_size: int, max_frames: int, context_graph, blank: int = 0,
                 state: torch.Tensor = None):
        from .context_graph import ContextGraph
        super().__init__(n_streams, beam_size, max_frames, blank, state)
        if not isinstance(context_graph, ContextGraph):
            raise RuntimeError("CtcContextPrefixBeamStream: context_graph must be a ContextGraph")
        if context_graph.blank != self.blank:
            raise RuntimeError(f"CtcContextPrefixBeamStream: the graph was built for blank {context_graph.blank}, "
                               f"the search uses {self.blank}")
        self.context_graph = context_graph
        self._dev = None
        self.context_states = [[] for _ in range(self.n_streams)]

    def search(self, logits_chunk: torch.Tensor, lens: torch.Tensor, finalize: bool = False):
        return self._search(logits_chunk, lens, finalize)

    def finalize(self):
        """The finalised n-best of every stream without new frames: a chunk in which every stream has lens = 0."""
        if self._vocab is None:
            raise RuntimeError("CtcContextPrefixBeamStream: finalize() before the first search")
        x = torch.zeros(self.n_streams, 1, self._vocab, dtype=torch.float32, device=self._dev)
        # the chunk is one frame wide and none of it is consumed: it counts against no capacity
        return self._call(x, torch.zeros(self.n_streams, dtype=torch.int32), min(self._frames_done, self.max_frames - 1), True)

    def _more(self, B, dev, finalize):
        beam, g = self.beam_size, self.context_graph
        cc, cx = (torch.empty(B, beam, dtype=torch.float64, device=dev) for _ in range(2))
        tg = torch.empty(B, beam, self.max_frames, dtype=torch.int32, device=dev)
        cs = torch.empty(B, beam, dtype=torch.int32, device=dev)
        self._dev = dev
        return (*g.to(dev), g.n_states, g.n_arcs, int(bool(finalize))), (cc, cx, tg, cs)

    def _result(self, rows, cc, cx, tg, cs):
        ccc, cxc, csc = cc.cpu().tolist(), cx.cpu().tolist(), cs.cpu().tolist()
        self.context_states = [csc[b][:len(utt)] for b, utt in enumerate(rows)]
        gc = tg[:, :, :max(len(h[0]) for utt in rows for h in utt)].cpu().tolist()
        return [[h + (ccc[b][e], cxc[b][e], tuple(gc[b][e][:len(h[0])])) for e, h in enumerate(utt)]
                for b, utt in enumerate(rows)]

    @staticmethod
    def outputs(result, start_tag_id: int, end_tag_id: int):
        """UpdateOutputs (ctc_prefix_beam_search.cc:63-84) on one stream's result: per hypothesis the tokens with
        `start_tag_id` in front of every token that starts a phrase and `end_tag_id` behind every token that ends one."""
        from .context_graph import mark_phrases
        return [mark_phrases(hyp[0], hyp[6], start_tag_id, end_tag_id) for hyp in result]


def ctc_context_prefix_beam_search(logits: torch.Tensor, lens: torch.Tensor, beam_size: int, context_graph, blank: int = 0):
    """The biased search over whole utterances (B, T, V) in one chunk, finalised: per utterance [(prefix tuple, score,
    viterbi_score, times tuple, ctc_score, context_score, tags tuple)] best first."""
    if not logits.is_cuda:
        raise RuntimeError("wenet_celoss_amd.ctc_context_prefix_beam_search: logits must live on a HIP device (no CPU path)")
    return CtcContextPrefixBeamStream(logits.shape[0], beam_size, logits.shape[1], context_graph, blank=blank).search(
        logits, lens, finalize=True)


def forced_align(ctc_probs: torch.Tensor, y: torch.Tensor, blank_id: int = 0) -> list:
    """wenet/utils/ctc_util.py:27-83: ctc_probs (T, D) log-posteriors, y (L,) label ids -> per-frame token list."""
    return forced_align_batch(ctc_probs.unsqueeze(0), y.reshape(1, -1), torch.tensor([ctc_probs.size(0)]),
                              torch.tensor([y.numel()]), blank_id=blank_id, normalized=True)[0]


def forced_align_batch(logits: torch.Tensor, targets: torch.Tensor, input_lengths: torch.Tensor,
                       target_lengths: torch.Tensor, blank_id: int = 0, normalized: bool = False) -> list:
    """Extension: B utterances at once.  logits (B, T, V) pre-softmax (or log-posteriors with normalized=True)."""
    if not logits.is_cuda:
        raise RuntimeError("wenet_celoss_amd.forced_align: tensors must live on a HIP device (no CPU path)")
    x = logits.detach().float().contiguous()
    B, T, V = x.shape
    dev = x.device
    tg = targets.to(device=dev, dtype=torch.int32)
    tg = torch.where(tg < 0, torch.zeros_like(tg), tg).contiguous()
    S = tg.shape[1]
    il = input_lengths.to(device=dev, dtype=torch.int32).contiguous()
    tl = target_lengths.to(device=dev, dtype=torch.int32).contiguous()
    ws = _lib.workspace("wr_ctc_align_workspace_bytes", B, T, S, device=dev)
    ali = torch.empty(B, T, dtype=torch.int32, device=dev)
    _lib.call("wr_ctc_forced_align", x, int(normalized), tg, il, tl, B, T, S, V, int(blank_id), ali, ws, ws.numel(),
              device=dev)
    ac, ilc = ali.cpu(), il.cpu().tolist()
    return [ac[b, :ilc[b]].tolist() for b in range(B)]


class CTC(torch.nn.Module):
    """CTC module (wenet/transformer/ctc.py:21-84)."""

    def __init__(self, odim: int, encoder_output_size: int, dropout_rate: float = 0.0, reduce: bool = True):
        super().__init__()
        eprojs = encoder_output_size
        self.dropout_rate = dropout_rate
        self.ctc_lo = torch.nn.Linear(eprojs, odim)
        self.reduction_type = "sum" if reduce else "none"
        self.ctc_loss = torch.nn.CTCLoss(reduction=self.reduction_type)     # ctc.py:44; used for CPU tensors only

    @torch.jit.unused      # backed by a ctypes autograd Function: opaque to TorchScript (train.py:203-205 smoke export)
    def forward(self, hs_pad: torch.Tensor, hlens: torch.Tensor, ys_pad: torch.Tensor,
                ys_lens: torch.Tensor) -> torch.Tensor:
        """hs_pad (B, Tmax, D), hlens (B), ys_pad (B, Lmax) padded with -1, ys_lens (B)."""
        ys_hat = self.ctc_lo(F.dropout(hs_pad, p=self.dropout_rate))      # (B, T, V); ctc.py:57
        if not ys_hat.is_cuda:
            # config 1 (CPU plumbing): exactly the reference's statements, on stock PyTorch (ctc.py:58-63)
            ys_hat = ys_hat.transpose(0, 1).log_softmax(2)
            return self.ctc_loss(ys_hat, ys_pad, hlens, ys_lens) / ys_hat.size(1)
        loss = ctc_loss(ys_hat, ys_pad, hlens, ys_lens, blank=0, reduction=self.reduction_type)
        return loss / ys_hat.size(0)                                        # batch-size average; ctc.py:63

    def log_softmax(self, hs_pad: torch.Tensor) -> torch.Tensor:
        return F.log_softmax(self.ctc_lo(hs_pad), dim=2)

    def argmax(self, hs_pad: torch.Tensor) -> torch.Tensor:
        return torch.argmax(self.ctc_lo(hs_pad), dim=2)
