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
