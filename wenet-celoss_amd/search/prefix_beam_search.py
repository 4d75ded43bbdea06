"""Transducer prefix beam search with the reference's interface
(wenet/transducer/search/prefix_beam_search.py:7-148): `Sequence`,
`PrefixBeamSearch(encoder, predictor, joint, ctc, blank)` and
`prefix_beam_search(speech, speech_lengths, decoding_chunk_size, beam_size,
num_decoding_left_chunks, simulate_streaming, ctc_weight, transducer_weight)
-> (beam: List[Sequence], encoder_out)`.

One expansion per hypothesis per frame, CTC/transducer score mixture, top-k,
prefix fusion with float64 log_add and the stable prune all run on the device
(`wr_prefix_beam_search`); unlike the reference (batch 1 only, :54-58) any
number of utterances can be searched together via `prefix_beam_search_batch`."""
from __future__ import annotations

from typing import List

import torch

from ..decoder import DecoderCache


class Sequence:
    __slots__ = {"hyp", "score", "cache"}

    def __init__(self, hyp, score, cache):
        self.hyp = hyp
        self.score = score
        self.cache = cache


def tdt_prefix_beam_search(model: torch.nn.Module, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor,
                           beam_size: int = 5, ctc_weight: float = 0.0, transducer_weight: float = 1.0
                           ) -> List[List[Sequence]]:
    """Prefix beam search of a token-and-duration model (`model.tdt_durations`; the joiner's row is `vocab_size` token
    logits followed by one logit per duration) for any number of utterances, with the whole search on the device
    (`wr_prefix_beam_search_tdt`; the rule is in include/wr_api.h, "TDT prefix beam search").  A hypothesis stands at a
    frame of its own; each step expands those at the earliest frame with their best `beam_size` (token, duration) pairs,
    the others wait; hypotheses with equal tokens at an equal frame fuse with float64 log_add.

    encoder_out (B, T, E), encoder_out_lens scalar or (B,) -> per utterance the pruned beam, best first, each hypothesis
    beginning with the seed blank.  The CTC posterior (`model.ctc`) is computed and mixed in only when
    (ctc_weight, transducer_weight) != (0, 1)."""
    from .greedy_search import _decoder_cache, expand_lens
    lens = expand_lens(encoder_out_lens, encoder_out.shape[0])
    return _search(_decoder_cache(model), model, encoder_out, beam_size,
                   lambda dec, ctc_logp: dec.prefix_beam_tdt(encoder_out, lens, model.tdt_durations, beam_size, model.blank,
                                                             ctc_logp=ctc_logp, ctc_weight=ctc_weight,
                                                             transducer_weight=transducer_weight),
                   with_ctc=(float(ctc_weight), float(transducer_weight)) != (0.0, 1.0))


def _search(cache, owner, encoder_out: torch.Tensor, beam_size: int, search, with_ctc: bool = True) -> List[List[Sequence]]:
    """search(decoder, ctc_logp) on `cache`'s DeviceDecoder for `owner`'s predictor and joiner, sized for a beam search of
    encoder_out (B, T, E); ctc_logp is the (B, T, V) posterior of `owner.ctc`, None unless `with_ctc`.  The n-best lists
    come back as Sequences."""
    B, T, _ = encoder_out.shape
    ctc_logp = None
    if with_ctc:
        with torch.no_grad():
            ctc_logp = owner.ctc.log_softmax(encoder_out)                # (B, T, V), ctc.py:66-75
    dec = cache.get(owner.predictor, owner.joint, lanes=B * beam_size, utts=B, tmax=T, max_hyp=0, beam=beam_size)
    return [[Sequence(hyp=h, score=s, cache=None) for h, s in utt] for utt in search(dec, ctc_logp)]


class TransducerPrefixBeamStream:
    """Transducer prefix beam search continued chunk by chunk, for `n_streams` streams at once, with the Viterbi score and
    the frame of every token of each hypothesis (`wr_prefix_beam_search_chunk`; the rule is in include/wr_api.h,
    "Streaming transducer prefix beam search").  `model` is a Transducer, plain or with `tdt_durations`; `max_frames`
    bounds the encoder frames (chunk widths summed) a stream may take between two resets, `chunk_frames` the width of a
    chunk.  ctc_weight / transducer_weight None: 0.3 / 0.7 for a plain model (`beam_search`), 0 / 1 for a
    token-and-duration model (`tdt_beam_search`).

    reset(streams=None) starts the given streams (all of them by default) fresh with the next search.
    search(encoder_out_chunk (n_streams, T, E), lens, final=False) consumes lens[b] <= T frames of stream b (0 and no
    final flag leaves it untouched; `final` is a bool or one per stream) and returns per stream the current n-best, best
    first: [(tokens incl. the seed blank, score, viterbi_score, times)].  The CTC posterior of the chunk (`model.ctc`) is
    computed here whenever it is mixed in: always for a plain model, and for a token-and-duration model when ctc_weight is
    not 0."""

    def __init__(self, model, n_streams: int, beam_size: int, max_frames: int, chunk_frames: int = 64,
                 ctc_weight: float = None, transducer_weight: float = None):
        self.model = model
        self.n_streams, self.beam_size = int(n_streams), int(beam_size)
        self.max_frames, self.chunk_frames = int(max_frames), int(chunk_frames)
        if self.n_streams < 1 or self.max_frames < 1 or self.chunk_frames < 1 or not 1 <= self.beam_size <= 16:
            raise RuntimeError(f"TransducerPrefixBeamStream: n_streams={n_streams}, beam_size={beam_size} (1..16), "
                               f"max_frames={max_frames}, chunk_frames={chunk_frames} must be positive")
        self.durations = getattr(model, "tdt_durations", None)
        tdt = self.durations is not None
        self.ctc_weight = float((0.0 if tdt else 0.3) if ctc_weight is None else ctc_weight)
        self.transducer_weight = float((1.0 if tdt else 0.7) if transducer_weight is None else transducer_weight)
        self._with_ctc = not tdt or self.ctc_weight != 0.0
        self._dec = None
        self._phase = [0] * self.n_streams          # 0: resets with the next search, 1: running, 2: had its final chunk
        self.frames = [0] * self.n_streams          # chunk widths summed since the stream's reset

    def reset(self, streams=None) -> None:
        for b in (range(self.n_streams) if streams is None else streams):
            self._phase[int(b)] = 0
            self.frames[int(b)] = 0

    # what the biased stream (TransducerContextPrefixBeamStream) does differently: the block it attaches and the call
    def _attached(self, dec):
        return dec.beam_stream

    def _attach(self, dec, B):
        dec.attach_beam_stream(B, self.beam_size, self.max_frames)

    def _chunk(self, dec, encoder_out_chunk, ln, ctc_logp, reset, fin):
        return dec.prefix_beam_chunk(encoder_out_chunk, ln, self.beam_size, self.model.blank, ctc_logp=ctc_logp,
                                     ctc_weight=self.ctc_weight, transducer_weight=self.transducer_weight,
                                     durations=self.durations, reset=reset, final=fin)

    def search(self, encoder_out_chunk: torch.Tensor, lens, final=False):
        from .greedy_search import _decoder_cache, expand_lens
        if encoder_out_chunk.dim() != 3:
            raise RuntimeError("TransducerPrefixBeamStream: the chunk must be (n_streams, frames, encoder dim)")
        B, T, _ = encoder_out_chunk.shape
        if B != self.n_streams:
            raise RuntimeError(f"TransducerPrefixBeamStream: chunk has {B} streams, the stream set has {self.n_streams}")
        if T > self.chunk_frames:
            raise RuntimeError(f"TransducerPrefixBeamStream: a chunk of {T} frames exceeds chunk_frames={self.chunk_frames}")
        fin = [bool(final)] * B if isinstance(final, (bool, int)) else [bool(f) for f in final]
        if len(fin) != B:
            raise RuntimeError(f"TransducerPrefixBeamStream: final has {len(fin)} entries for {B} streams")
        ln = expand_lens(lens, B).reshape(-1)
        if ln.numel() != B:
            raise RuntimeError(f"TransducerPrefixBeamStream: lens has {ln.numel()} elements for {B} streams")
        fed = [int(v) > 0 for v in ln.cpu().tolist()]
        for b in range(B):
            if self._phase[b] == 2 and (fed[b] or fin[b]):
                raise RuntimeError(f"TransducerPrefixBeamStream: stream {b} is fed after its final chunk (reset it first)")
            if self._phase[b] != 2 and self.frames[b] + T > self.max_frames:
                raise RuntimeError(f"TransducerPrefixBeamStream: stream {b}: {self.frames[b]} frames done + a chunk of {T} "
                                   f"exceeds max_frames={self.max_frames}")
        if not encoder_out_chunk.is_cuda:
            raise RuntimeError("wenet_celoss_amd.TransducerPrefixBeamStream: the chunk must live on a HIP device (no CPU path)")
        model = self.model
        dec = _decoder_cache(model).get(model.predictor, model.joint, lanes=B * self.beam_size, utts=B, tmax=self.chunk_frames,
                                        max_hyp=0, beam=self.beam_size)
        if dec is not self._dec:
            if any(p == 1 for p in self._phase):
                raise RuntimeError("the decoder handle was rebuilt (weights changed or capacity grew) in the middle of a "
                                   "stream: call reset() first")
            self._phase = [0] * B                   # finished streams lived on the old handle too
        if self._attached(dec) != (B, self.beam_size, self.max_frames) or dec is not self._dec:
            self._attach(dec, B)
        self._dec = dec
        ctc_logp = None
        if self._with_ctc:
            with torch.no_grad():
                ctc_logp = model.ctc.log_softmax(encoder_out_chunk)
        reset = [p == 0 for p in self._phase]
        try:
            out = self._chunk(dec, encoder_out_chunk, ln, ctc_logp, reset, fin)
        except RuntimeError:
            _decoder_cache(model).discard(dec)
            raise
        for b in range(B):
            if reset[b]:
                self._phase[b], self.frames[b] = 1, 0
            if self._phase[b] == 1:
                self.frames[b] += T
                if fin[b]:
                    self._phase[b] = 2
        return out


class TransducerContextPrefixBeamStream(TransducerPrefixBeamStream):
    """TransducerPrefixBeamStream with context-graph phrase biasing (`wr_prefix_beam_search_context_chunk`; the rule is in
    include/wr_api.h, "Context-graph biasing in the streaming transducer prefix beam search"): every hypothesis walks
    `context_graph` (a ContextGraph, fixed here for the life of the streams) and the beam is pruned by score plus bonus.

    search(encoder_out_chunk, lens, final=False, finalize=None) returns per stream [(tokens incl. the seed blank, score,
    viterbi_score, times, trans_score, context_score, tags, context_state)] best first, score = trans_score +
    context_score, one tag per token after the seed (bit 0: a phrase starts at it, bit 1: a phrase ends at it).
    `finalize` (a bool or one per stream) exports a stream as if it ended here: a partial match gives its bonus back and the
    list is sorted again; the stream itself is not changed.  By default it follows `final`, and stays on for a stream that
    has had its final chunk, so that a finished stream keeps being exported as it ended.  The record of the streams and the
    refusals are TransducerPrefixBeamStream's."""

    def __init__(self, model, n_streams: int, beam_size: int, max_frames: int, chunk_frames: int = 64, context_graph=None,
                 ctc_weight: float = None, transducer_weight: float = None):
        from ..context_graph import ContextGraph
        super().__init__(model, n_streams, beam_size, max_frames, chunk_frames, ctc_weight, transducer_weight)
        if not isinstance(context_graph, ContextGraph):
            raise ValueError("TransducerContextPrefixBeamStream: context_graph must be a ContextGraph")
        if context_graph.blank != int(model.blank):
            raise ValueError(f"TransducerContextPrefixBeamStream: the graph was built for blank {context_graph.blank}, "
                             f"the model's is {model.blank}")
        vocab = int(model.vocab_size)
        worst = int(context_graph.arc_token.max()) if context_graph.n_arcs else -1
        if worst >= vocab:
            raise ValueError(f"TransducerContextPrefixBeamStream: phrase token {worst} lies outside the token vocabulary "
                             f"[0, {vocab})")
        self.context_graph = context_graph

    def _attached(self, dec):
        return dec.beam_context_stream

    def _attach(self, dec, B):
        dec.attach_beam_context_stream(B, self.beam_size, self.max_frames)

    def _chunk(self, dec, encoder_out_chunk, ln, ctc_logp, reset, fin):
        return dec.prefix_beam_context_chunk(encoder_out_chunk, ln, self.beam_size, self.model.blank, self.context_graph,
                                             ctc_logp=ctc_logp, ctc_weight=self.ctc_weight,
                                             transducer_weight=self.transducer_weight, durations=self.durations, reset=reset,
                                             final=fin, finalize=self._finalize)

    def search(self, encoder_out_chunk: torch.Tensor, lens, final=False, finalize=None):
        B = self.n_streams
        fz = final if finalize is None else finalize
        fz = [bool(fz)] * B if isinstance(fz, (bool, int)) else [bool(f) for f in fz]
        if finalize is None:                        # (a `final` of the wrong length is reported below, as `final`)
            fz = [f or p == 2 for f, p in zip(fz + [False] * B, self._phase)]
        elif len(fz) != B:
            raise RuntimeError(f"TransducerContextPrefixBeamStream: finalize has {len(fz)} entries for {B} streams")
        self._finalize = fz                         # read by _chunk
        return super().search(encoder_out_chunk, lens, final=final)

    @staticmethod
    def outputs(result, start_tag_id: int, end_tag_id: int):
        """UpdateOutputs on one stream's result: per hypothesis the tokens after the seed blank with `start_tag_id` in front
        of every token that starts a phrase and `end_tag_id` behind every token that ends one."""
        from ..context_graph import mark_phrases
        return [mark_phrases(hyp[0][1:], hyp[6], start_tag_id, end_tag_id) for hyp in result]


class PrefixBeamSearch:
    def __init__(self, encoder, predictor, joint, ctc, blank):
        self.encoder = encoder
        self.predictor = predictor
        self.joint = joint
        self.ctc = ctc
        self.blank = blank
        self._decoder_cache = DecoderCache()

    def search_encoded(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, beam_size: int = 5,
                       ctc_weight: float = 0.3, transducer_weight: float = 0.7) -> List[List[Sequence]]:
        """encoder_out (B, T, E) already computed -> per utterance the pruned beam (best first)."""
        return _search(self._decoder_cache, self, encoder_out, beam_size,
                       lambda dec, ctc_logp: dec.prefix_beam(encoder_out, encoder_out_lens, ctc_logp, beam_size, ctc_weight,
                                                             transducer_weight, self.blank))

    def prefix_beam_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                           beam_size: int = 5, num_decoding_left_chunks: int = -1, simulate_streaming: bool = False,
                           ctc_weight: float = 0.3, transducer_weight: float = 0.7):
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        assert speech.shape[0] == 1
        encoder_out, _ = self.encoder(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks)
        lens = torch.tensor([encoder_out.size(1)], dtype=torch.int32)
        beam = self.search_encoded(encoder_out, lens, beam_size, ctc_weight, transducer_weight)[0]
        return beam, encoder_out

    def prefix_beam_search_batch(self, speech, speech_lengths, decoding_chunk_size=-1, beam_size=5,
                                 num_decoding_left_chunks=-1, ctc_weight=0.3, transducer_weight=0.7):
        """Extension: B utterances at once.  Returns (List[List[Sequence]], encoder_out)."""
        encoder_out, mask = self.encoder(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks)
        lens = mask.squeeze(1).sum(1).to(torch.int32)
        return self.search_encoded(encoder_out, lens, beam_size, ctc_weight, transducer_weight), encoder_out
