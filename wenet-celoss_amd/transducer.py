"""Transducer model head with the reference's interface
(wenet/transducer/transducer.py:20-629): same constructor keywords, same
`forward(speech, speech_lengths, text, text_lengths, context_list,
context_lengths, hw_label)` returning the dict
{loss, loss_att, loss_ctc, loss_rnnt, hw_loss}, same `greedy_search`,
`beam_search`, `transducer_attention_rescoring`, `_cal_transducer_score` and
step exports -- so wenet/bin/train.py and wenet/bin/recognize.py can drive it.

What runs where
  joiner logits      wenet_celoss_amd.TransducerJoint  (MFMA HIP kernels)
  RNN-T loss + grad  wenet_celoss_amd.rnnt_loss        (HIP, replaces torchaudio, :142-147 / :296-301)
  CTC loss + grad    wenet_celoss_amd.CTC              (HIP, replaces nn.CTCLoss)
  greedy / beam      wenet_celoss_amd.search.*         (HIP decode kernels under hipGraph)
  encoder, attention decoder, ContextBias: whatever modules the caller passes
  (stock PyTorch-ROCm; out of scope).

`context_bias` may be None (no hot words); when a ContextBias module is given it
is called exactly where the reference calls it in `forward`, and `greedy_search`
dispatches on `loss_mode` to the fork's hot-word variants (host-driven control flow
over the HIP step kernels).
"""
from __future__ import annotations

import os
import warnings
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn
from torch.nn.utils.rnn import pad_sequence

from .common import IGNORE_ID, LabelSmoothingLoss, add_blank, add_sos_eos, end_blank, reverse_pad_list
from .decoder import DecoderCache
from .fused import joint_rnnt_loss, joint_rnnt_tdt_loss, per_bucket, plan_buckets
from .joint import TransducerJoint, _call_precision
from .rnnt_align import joint_rnnt_forced_align, rnnt_forced_align
from .rnnt_loss import check_latency, rnnt_loss
from .rnnt_simple import rnnt_simple_forced_align
from . import k2
from .rnnt_lattice import check_lattice, is_default
from .rnnt_pruned import rnnt_loss_pruned
from .rnnt_tdt import check_tdt, rnnt_tdt_forced_align, rnnt_tdt_loss
from .search.greedy_search import (basic_greedy_search, basic_greedy_search_both, basic_greedy_search_hw,
                                   lens_and_decoder, tdt_greedy_search)
from .search.prefix_beam_search import PrefixBeamSearch, tdt_prefix_beam_search


def _output_width(module: nn.Module, role: str, joint: nn.Module, joint_ffn: str) -> int:
    """Feature width of an encoder's / predictor's output: `output_size` (a method on wenet encoders, an attribute on its
    predictors), `_output_size`, the predictor's output projection, else the joiner's pre-join projection for it."""
    for name in ("output_size", "_output_size"):
        width = getattr(module, name, None)
        width = width() if callable(width) else width
        if isinstance(width, int):
            return width
    for owner, name in ((module, "projection"), (joint, joint_ffn)):
        lin = getattr(owner, name, None)
        if isinstance(lin, nn.Linear):
            return lin.out_features if owner is module else lin.in_features
    raise ValueError(f"Transducer: simple_loss_weight > 0 needs the {role}'s output width (no output_size, and the joiner "
                     f"has no {joint_ffn})")


def check_limits(text: torch.Tensor, text_lengths: torch.Tensor, with_ctc: bool) -> None:
    """Shape limits of the loss kernels (INTEGRATION.md "Shape limits"), checked on the padded label width before
    anything is launched, with a message that names the longest utterance.  No device sync unless a limit is hit."""
    width = int(text.shape[1])
    limit = 511 if with_ctc else 1023
    if width <= limit:
        return
    i = int(text_lengths.argmax())
    what = ("the CTC loss kernels take label sequences padded to at most 511" if with_ctc else
            "the RNN-T loss kernels take at most 1023 labels (U + 1 <= 1024 lattice columns)")
    raise RuntimeError(f"wenet_celoss_amd.Transducer: the label batch is padded to {width} (longest: utterance {i} with "
                       f"{int(text_lengths[i])} labels); {what} -- lower filter_conf.token_max_length")


class Transducer(nn.Module):
    """Transducer-ctc-attention hybrid Encoder-Predictor-Decoder model (transducer.py:20)."""

    def __init__(self, vocab_size: int, blank: int, encoder: nn.Module, predictor: nn.Module, joint: nn.Module,
                 attention_decoder: Optional[nn.Module] = None, ctc: Optional[nn.Module] = None,
                 context_bias: Optional[nn.Module] = None, ctc_weight: float = 0, ignore_id: int = IGNORE_ID,
                 reverse_weight: float = 0.0, lsm_weight: float = 0.0, length_normalized_loss: bool = False,
                 transducer_weight: float = 1.0, attention_weight: float = 0.0, hw_weight: float = 0.4,
                 loss_mode: str = "both", prune_range: int = 0, lm_only_scale: float = 0.0,
                 am_only_scale: float = 0.0, rnnt_type: str = "regular", delay_penalty: float = 0.0,
                 fastemit_lambda: float = 0.0, rnnt_delay_penalty: float = 0.0, tdt_durations=None,
                 tdt_sigma: float = 0.0, simple_loss_weight: float = 0.0) -> None:
        assert attention_weight + ctc_weight + transducer_weight == 1.0          # transducer.py:46 (kept as is)
        super().__init__()
        # ASRModel part (asr_model.py:38-70): sos/eos are the last class
        self.sos = vocab_size - 1
        self.eos = vocab_size - 1
        self.vocab_size = vocab_size
        self.ignore_id = ignore_id
        self.ctc_weight = ctc_weight
        self.reverse_weight = reverse_weight
        self.encoder = encoder
        self.decoder = attention_decoder
        self.ctc = ctc

        self.blank = blank
        self.transducer_weight = transducer_weight
        self.attention_decoder_weight = 1 - self.transducer_weight - self.ctc_weight
        self.context_bias = context_bias
        self.predictor = predictor
        self.joint = joint
        self.bs = None
        self.hw_weight = hw_weight
        self.loss_mode = loss_mode
        self.hw_criterion = nn.CrossEntropyLoss()
        if attention_decoder is not None:
            self.criterion_att = LabelSmoothingLoss(size=vocab_size, padding_idx=ignore_id, smoothing=lsm_weight,
                                                    normalize_length=length_normalized_loss)
        # encoder.embed.{subsampling_rate, right_context} as the exports below report them (asr_model.py:542-554); -1 when
        # the encoder module has no `embed` (the reference would fail to script such a model)
        embed = getattr(encoder, "embed", None)
        self._subsampling_rate: int = int(getattr(embed, "subsampling_rate", -1))
        self._right_context: int = int(getattr(embed, "right_context", -1))
        self._decoder_cache = DecoderCache()
        # joiner + RNN-T loss as one autograd node (fused.py): pass 1 of the loss rides on the joiner's epilogue and the
        # logits never leave the node (half the footprint).  WR_FUSED_LOSS=0 (or this attribute) selects the two separate ops.
        self.fused_loss = os.environ.get("WR_FUSED_LOSS", "1") != "0"
        # memory-bounded fused node (fused.joint_rnnt_loss `logits_budget`, bytes): no logits tensor, the backward
        # recomputes them in slices of at most this size.  None: WR_FUSED_LOGITS_BUDGET_MB if set, else the plain node.
        self.logits_budget: Optional[int] = None
        # the additive-joiner ("simple") loss of the reference's second transducer class (transducer_k2_loss.py:73-78,
        # :147-157): two linear heads onto the vocabulary whose sum is the logits of a second RNN-T loss, added with this
        # weight.  Each head is applied to the tensor its name says (the reference builds them with the two widths
        # crossed, which only works when the widths are equal).  0.0: no parameters, no extra loss.
        self.simple_loss_weight = float(simple_loss_weight)
        if self.simple_loss_weight > 0.0:
            self.simple_am_proj = nn.Linear(_output_width(encoder, "encoder", joint, "enc_ffn"), vocab_size)
            self.simple_lm_proj = nn.Linear(_output_width(predictor, "predictor", joint, "pred_ffn"), vocab_size)
        # smoothing of the simple loss (k2's rnnt_loss_smoothed; icefall trains with lm_only_scale = 0.25, am_only_scale
        # = 0): either scale non-zero and loss_simple (and the occupancies the pruning takes) is rnnt_loss_smoothed's.
        self.lm_only_scale, self.am_only_scale = float(lm_only_scale), float(am_only_scale)
        if self.lm_only_scale < 0.0 or self.am_only_scale < 0.0 or self.lm_only_scale + self.am_only_scale > 1.0:
            raise ValueError(f"Transducer: lm_only_scale and am_only_scale must be >= 0 and sum to at most 1 (got "
                             f"{lm_only_scale}, {am_only_scale})")
        if (self.lm_only_scale > 0.0 or self.am_only_scale > 0.0) and not self.simple_loss_weight > 0.0:
            raise ValueError("Transducer: lm_only_scale / am_only_scale smooth the simple loss: simple_loss_weight must be > 0")
        # pruned training (k2 / icefall recipe, rnnt_pruned.py): the simple loss's arc occupancies choose a band of
        # `prune_range` label positions per frame, and loss_rnnt is the RNN-T loss of the joiner evaluated on that band
        # only.  0: the full-lattice loss block above.
        # lattice type and delay penalty of the k2 losses (rnnt_lattice.py): passed to the simple / smoothed loss and to
        # the pruned loss.  Without a simple loss the main loss is the torchaudio-style one, which has neither.
        lat, self.delay_penalty = check_lattice("Transducer", rnnt_type, delay_penalty)
        self.rnnt_type = rnnt_type
        if not is_default(lat, self.delay_penalty) and not self.simple_loss_weight > 0.0:
            raise ValueError("Transducer: rnnt_type / delay_penalty belong to the k2 losses: simple_loss_weight must be > 0")
        # FastEmit and the delay penalty of the full-lattice term (rnnt_loss / joint_rnnt_loss: plain, fused, bounded and
        # AMP routes of compute_loss).  `delay_penalty` above stays the k2 losses' own.
        self.fastemit_lambda, self.rnnt_delay_penalty = check_latency("Transducer", fastemit_lambda, rnnt_delay_penalty)
        self.prune_range = int(prune_range)
        if self.prune_range < 0 or self.prune_range == 1:
            raise ValueError(f"Transducer: prune_range must be 0 (off) or at least 2 (got {prune_range})")
        if self.prune_range > 0 and not self.simple_loss_weight > 0.0:
            raise ValueError("Transducer: prune_range > 0 takes its ranges from the simple loss: simple_loss_weight must be > 0")
        if self.prune_range > 0 and not hasattr(joint, "forward_pruned"):
            raise ValueError("Transducer: prune_range > 0 needs a joiner with forward_pruned (TransducerJoint)")
        # token-and-duration transducer (rnnt_tdt.py): the joiner has vocab_size + D outputs, the last D of them the
        # duration logits, and loss_rnnt is rnnt_tdt_loss on its logits.  CTC, attention and the simple loss keep
        # vocab_size.  None: a plain transducer.
        self.tdt_durations, self.tdt_sigma = None, 0.0
        if tdt_durations is not None:
            self.tdt_durations, self.tdt_sigma = check_tdt("Transducer", tdt_durations, tdt_sigma)
            for name, on in (("prune_range", self.prune_range > 0), ("fastemit_lambda", self.fastemit_lambda > 0.0),
                             ("rnnt_delay_penalty", self.rnnt_delay_penalty > 0.0),
                             ("a context_bias module", context_bias is not None)):
                if on:
                    raise ValueError(f"Transducer: tdt_durations cannot be combined with {name}")
            outputs = getattr(getattr(joint, "ffn_out", None), "out_features", None)
            if outputs != vocab_size + len(self.tdt_durations):
                raise ValueError(f"Transducer: with tdt_durations={self.tdt_durations} the joiner must have vocab_size + "
                                 f"{len(self.tdt_durations)} = {vocab_size + len(self.tdt_durations)} outputs (it has "
                                 f"{outputs})")
        elif float(tdt_sigma) != 0.0:
            raise ValueError("Transducer: tdt_sigma belongs to the TDT loss: tdt_durations must be set")

    # ------------------------------------------------------------- training --
    def _logits_budget(self) -> Optional[int]:
        budget = getattr(self, "logits_budget", None)     # absent on instances built without __init__
        if budget is not None:
            return int(budget)
        mb = os.environ.get("WR_FUSED_LOGITS_BUDGET_MB")
        return None if mb is None or mb == "" else int(float(mb) * (1 << 20))

    def compute_loss(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, predictor_out: torch.Tensor,
                     text: torch.Tensor, text_lengths: torch.Tensor, skip_padding: bool = False
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """The loss block of the reference forward (transducer.py:131-147): joiner -> int32 label prep -> RNN-T loss.
        Returns (joint_out, loss_rnnt).  With `fused_loss` the two run as one autograd node and joint_out is
        None (the logits never leave it); otherwise `skip_padding=True` (extension) lets the joiner skip lattice cells
        that the loss never reads."""
        rnnt_text = self._rnnt_text(text)
        rnnt_text_lengths = text_lengths.to(torch.int32)
        encoder_out_lens = encoder_out_lens.to(torch.int32)
        if self._is_tdt():
            budget = self._logits_budget()
            if budget is not None and self._can_bound_tdt_loss():
                # memory-bounded node: no logits tensor (fused.joint_rnnt_tdt_loss), the exact fp32 joiner only
                jt = self.joint
                ep, pp = jt.pre_activation(encoder_out, predictor_out)
                loss = joint_rnnt_tdt_loss(ep, pp, jt.ffn_out.weight, jt.ffn_out.bias, rnnt_text, encoder_out_lens,
                                           rnnt_text_lengths, self.tdt_durations, blank=self.blank, sigma=self.tdt_sigma,
                                           reduction="mean", activation=jt.activation, logits_budget=budget)
                return None, loss
            if budget is not None:
                self._warn_budget()
            # TDT: the joiner's vocab_size + D logits, in whatever precision it produces them (16-bit under AMP)
            joint_out = self.joint(encoder_out, predictor_out)
            loss = rnnt_tdt_loss(joint_out, rnnt_text.contiguous(), encoder_out_lens.contiguous(),
                                 rnnt_text_lengths.contiguous(), self.tdt_durations, blank=self.blank, sigma=self.tdt_sigma,
                                 reduction="mean", inplace_grad=True)
            return None, loss
        if self._can_fuse_loss():
            jt = self.joint
            ep, pp = jt.pre_activation(encoder_out, predictor_out)
            loss = joint_rnnt_loss(ep, pp, jt.ffn_out.weight, jt.ffn_out.bias,
                                   rnnt_text, encoder_out_lens, rnnt_text_lengths, blank=self.blank, reduction="mean",
                                   precision=jt.precision, activation=jt.activation, logits_budget=self._logits_budget(),
                                   **self._latency_kwargs())
            return None, loss
        if self._logits_budget() is not None:
            self._warn_budget()
        if self.fused_loss and isinstance(self.joint, TransducerJoint):
            # the AMP single-term joiner keeps 16-bit logits (two ops), but a ragged batch is still cut into
            # label-length groups, each padded to its own maxima (fused.plan_buckets): same costs, fewer padded cells
            lens = torch.stack([encoder_out_lens, rnnt_text_lengths]).cpu()
            groups = plan_buckets(lens[0].tolist(), lens[1].tolist(), max_buckets=int(os.environ.get("WR_FUSED_BUCKETS", "4")))
            if groups is not None:
                def part(idx, g, tg, ug):
                    ll, tl = encoder_out_lens[idx].contiguous(), rnnt_text_lengths[idx].contiguous()
                    logits = self.joint(encoder_out[idx, :tg], predictor_out[idx, :ug + 1], ll, tl)
                    return rnnt_loss(logits, rnnt_text[idx, :ug].contiguous(), ll, tl, blank=self.blank, reduction="none",
                                     inplace_grad=True, **self._latency_kwargs())
                # averaged in bucket order, as this branch always did: another order moves the mean's last bit
                return None, per_bucket(groups, lens, encoder_out.device, part, restore_order=False).float().mean()
        if skip_padding:
            joint_out = self.joint(encoder_out, predictor_out, encoder_out_lens, rnnt_text_lengths)
        else:
            joint_out = self.joint(encoder_out, predictor_out)
        loss = rnnt_loss(joint_out, rnnt_text.contiguous(), encoder_out_lens.contiguous(),
                         rnnt_text_lengths.contiguous(), blank=self.blank, reduction="mean", **self._latency_kwargs())
        return joint_out, loss

    def _rnnt_text(self, text: torch.Tensor) -> torch.Tensor:
        """Labels as the loss kernels take them: int32, IGNORE_ID padding mapped to class 0."""
        text = text.to(torch.int64)
        return torch.where(text == self.ignore_id, 0, text).to(torch.int32)

    def _warn_budget(self) -> None:
        """Once per model: a budget is set but this step's joiner keeps a logits tensor (the 16-bit AMP modes, the two-op
        path; for a TDT model anything but the fused "fp32" joiner), so the budget does not apply to it."""
        if not getattr(self, "_warned_budget", False):
            warnings.warn("Transducer: logits_budget / WR_FUSED_LOGITS_BUDGET_MB applies to the fused joiner + loss node with "
                          "the \"fp32\" or \"bf16x3\" joiner only; this step keeps its logits tensor", RuntimeWarning)
            self._warned_budget = True

    def _latency_kwargs(self) -> Dict[str, object]:
        """fastemit_lambda / delay_penalty for the full-lattice loss; empty for the defaults (and for a model pickled
        before they existed)."""
        lam, pen = getattr(self, "fastemit_lambda", 0.0), getattr(self, "rnnt_delay_penalty", 0.0)
        if lam == 0.0 and pen == 0.0:
            return {}
        return {"fastemit_lambda": lam, "delay_penalty": pen}

    def _simple_inputs(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, predictor_out: torch.Tensor,
                       text: torch.Tensor, text_lengths: torch.Tensor):
        """(lm, am, symbols, boundary) of the additive-joiner loss (transducer_k2_loss.py:131-148): the two heads on the
        encoder and predictor outputs the joiner sees, IGNORE_ID mapped to 0, boundary rows (0, 0, U_b, T_b)."""
        symbols = text.to(torch.int64)
        symbols = torch.where(symbols == self.ignore_id, 0, symbols)
        boundary = torch.zeros((text.size(0), 4), dtype=torch.int64, device=encoder_out.device)
        boundary[:, 2] = text_lengths
        boundary[:, 3] = encoder_out_lens
        return self.simple_lm_proj(predictor_out), self.simple_am_proj(encoder_out), symbols, boundary

    def compute_simple_loss(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, predictor_out: torch.Tensor,
                            text: torch.Tensor, text_lengths: torch.Tensor) -> torch.Tensor:
        """rnnt_loss_simple on the two vocabulary heads, reduction "mean" (transducer_k2_loss.py:147-157);
        rnnt_loss_smoothed when the model was built with a non-zero lm_only_scale or am_only_scale."""
        lm, am, symbols, boundary = self._simple_inputs(encoder_out, encoder_out_lens, predictor_out, text, text_lengths)
        return self._simple_loss(lm, am, symbols, boundary, return_grad=False)

    def _simple_loss(self, lm, am, symbols, boundary, return_grad: bool):
        ll, la = self.lm_only_scale, self.am_only_scale
        kw = self._lattice_kwargs()
        if ll != 0.0 or la != 0.0:
            return k2.rnnt_loss_smoothed(lm, am, symbols, self.blank, lm_only_scale=ll, am_only_scale=la, boundary=boundary,
                                         reduction="mean", return_grad=return_grad, **kw)
        return k2.rnnt_loss_simple(lm, am, symbols, self.blank, boundary=boundary, reduction="mean",
                                   return_grad=return_grad, **kw)

    def _lattice_kwargs(self) -> Dict[str, object]:
        """rnnt_type / delay_penalty for the k2 losses; empty for the defaults (and for a model pickled before they
        existed)."""
        rnnt_type, pen = getattr(self, "rnnt_type", "regular"), getattr(self, "delay_penalty", 0.0)
        if rnnt_type == "regular" and pen == 0.0:
            return {}
        return {"rnnt_type": rnnt_type, "delay_penalty": pen}

    def compute_pruned_loss(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, predictor_out: torch.Tensor,
                            text: torch.Tensor, text_lengths: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The pruned loss block: (loss_rnnt, loss_simple), both reduction "mean".  The simple loss returns its arc
        occupancies, `get_rnnt_prune_ranges` turns them into a band of `prune_range` label positions per frame, and
        loss_rnnt is `rnnt_loss_pruned` on the joiner's outputs on that band."""
        lm, am, symbols, boundary = self._simple_inputs(encoder_out, encoder_out_lens, predictor_out, text, text_lengths)
        loss_simple, (px_grad, py_grad) = self._simple_loss(lm, am, symbols, boundary, return_grad=True)
        ranges = k2.get_rnnt_prune_ranges(px_grad, py_grad, boundary, self.prune_range)
        logits = self.joint.forward_pruned(encoder_out, predictor_out, ranges)
        loss_rnnt = rnnt_loss_pruned(logits, symbols, ranges, self.blank, boundary=boundary, reduction="mean",
                                     **self._lattice_kwargs())
        return loss_rnnt, loss_simple

    def _is_tdt(self) -> bool:
        return getattr(self, "tdt_durations", None) is not None      # absent on a model pickled before it existed

    def _refuse_tdt(self, what: str) -> None:
        if self._is_tdt():
            raise NotImplementedError(f"Transducer.{what}: a TDT model (tdt_durations={self.tdt_durations}) decodes with "
                                      "greedy_search and tdt_greedy_search_batch; this method reads every joiner column as "
                                      "a token")

    def _can_fuse_loss(self) -> bool:
        if self._is_tdt():
            return False
        return self._joiner_can_fuse()

    def _joiner_can_fuse(self) -> bool:
        jt = self.joint
        # the AMP single-term modes keep 16-bit logits ("autocast" is one of them under autocast only)
        return (self.fused_loss and isinstance(jt, TransducerJoint)
                and _call_precision(jt.precision) not in ("bf16", "f16"))

    def _can_bound_tdt_loss(self) -> bool:
        """A TDT model whose joiner the memory-bounded TDT node serves: what _can_fuse_loss asks of a plain model's
        joiner, and the exact fp32 precision (the TDT epilogues exist in that forward kernel only)."""
        return self._is_tdt() and self._joiner_can_fuse() and _call_precision(self.joint.precision) == "fp32"

    def _loss_inputs(self, speech: torch.Tensor, speech_lengths: torch.Tensor, text: torch.Tensor,
                     context_list: torch.Tensor, context_lengths: torch.Tensor):
        """The prelude of `forward` up to the loss block (transducer.py:90-120): encoder, ContextBias biasing when a
        module is attached, the blank-prefixed predictor input.  Returns (bias_hidden, encoder_out, encoder_mask,
        encoder_out_lens, encoder_out_bias, predictor_out, predictor_out_bias)."""
        cb = self.context_bias
        bias_hidden = cb.forward_bias_hidden(context_list, context_lengths) if cb is not None else None

        encoder_out, encoder_mask = self.encoder(speech, speech_lengths)
        encoder_out_lens = encoder_mask.squeeze(1).sum(1)
        encoder_out_bias = None
        if cb is not None:
            encoder_out, encoder_out_bias = cb.forward_encoder_bias(bias_hidden, encoder_out)
        ys_in_pad = add_blank(text, self.blank, self.ignore_id)
        predictor_out = self.predictor(ys_in_pad)
        predictor_out_bias = None
        if cb is not None:
            predictor_out, predictor_out_bias = cb.forward_predictor_bias(bias_hidden, predictor_out)
        return (bias_hidden, encoder_out, encoder_mask, encoder_out_lens, encoder_out_bias, predictor_out,
                predictor_out_bias)

    @torch.jit.unused      # wenet/bin/train.py:203-205 scripts the model as an export smoke test; the HIP-backed forward
    def forward(self, speech: torch.Tensor, speech_lengths: torch.Tensor, text: torch.Tensor,  # is opaque to TorchScript
                text_lengths: torch.Tensor, context_list: torch.Tensor = torch.IntTensor([0]),
                context_lengths: torch.Tensor = torch.IntTensor([0]), hw_label=torch.IntTensor([0])
                ) -> Dict[str, Optional[torch.Tensor]]:
        """Frontend + Encoder + predictor + joint + loss (transducer.py:79-270)."""
        assert text_lengths.dim() == 1, text_lengths.shape
        assert (speech.shape[0] == speech_lengths.shape[0] == text.shape[0] == text_lengths.shape[0]), \
            (speech.shape, speech_lengths.shape, text.shape, text_lengths.shape)
        check_limits(text, text_lengths, with_ctc=self.ctc_weight != 0.0 and self.ctc is not None)
        cb = self.context_bias
        (bias_hidden, encoder_out, encoder_mask, encoder_out_lens, encoder_out_bias, predictor_out,
         predictor_out_bias) = self._loss_inputs(speech, speech_lengths, text, context_list, context_lengths)
        predictor_out_unbiased = predictor_out.clone()

        loss_simple: Optional[torch.Tensor] = None
        if getattr(self, "prune_range", 0) > 0:
            loss_rnnt, loss_simple = self.compute_pruned_loss(encoder_out, encoder_out_lens, predictor_out, text, text_lengths)
            loss = self.transducer_weight * loss_rnnt + self.simple_loss_weight * loss_simple
        else:
            _, loss_rnnt = self.compute_loss(encoder_out, encoder_out_lens, predictor_out, text, text_lengths)
            loss = self.transducer_weight * loss_rnnt
            if getattr(self, "simple_loss_weight", 0.0) > 0.0:
                loss_simple = self.compute_simple_loss(encoder_out, encoder_out_lens, predictor_out, text, text_lengths)
                loss = loss + self.simple_loss_weight * loss_simple

        loss_att: Optional[torch.Tensor] = None
        if self.attention_decoder_weight != 0.0 and self.decoder is not None:
            loss_att, _ = self._calc_att_loss(encoder_out, encoder_mask, text, text_lengths)
        loss_ctc: Optional[torch.Tensor] = None
        if self.ctc_weight != 0.0 and self.ctc is not None:
            loss_ctc = self.ctc(encoder_out, encoder_out_lens, text, text_lengths)
        if loss_ctc is not None:
            loss = loss + self.ctc_weight * loss_ctc.sum()
        if loss_att is not None:
            loss = loss + self.attention_decoder_weight * loss_att.sum()

        hw_loss: Optional[torch.Tensor] = None
        if self.hw_weight != 0.0 and cb is not None:
            if self.loss_mode == "pred":
                hw_output = cb.forward_hw_pred(bias_hidden, predictor_out_unbiased).permute(0, 2, 1)
                hw_label_pad = end_blank(hw_label, self.blank, self.ignore_id)[..., :-1]
                hw_loss = self.hw_criterion(hw_output[..., :-1], hw_label_pad)
            elif self.loss_mode == "both":
                hw_output = cb.forward_hw_pred_both(encoder_out_bias, predictor_out_bias).permute(0, 2, 1)
                hw_label_pad = end_blank(hw_label, self.blank, self.ignore_id)[..., :-1]
                hw_loss = self.hw_criterion(hw_output[..., :-1], hw_label_pad)
            else:
                _, hw_output_dec = cb.forward_hw_pred_both_sep(encoder_out_bias, predictor_out_bias)
                hw_label_pad = add_blank(hw_label, self.blank, self.ignore_id)
                hw_loss = self.hw_criterion(hw_output_dec.permute(0, 2, 1), hw_label_pad)
            loss = loss + self.hw_weight * hw_loss
        out = {"loss": loss, "loss_att": loss_att, "loss_ctc": loss_ctc, "loss_rnnt": loss_rnnt, "hw_loss": hw_loss}
        if loss_simple is not None:
            out["loss_simple"] = loss_simple
        return out

    @torch.jit.unused      # HIP-backed, like forward
    def forced_align(self, speech: torch.Tensor, speech_lengths: torch.Tensor, text: torch.Tensor,
                     text_lengths: torch.Tensor, context_list: torch.Tensor = torch.IntTensor([0]),
                     context_lengths: torch.Tensor = torch.IntTensor([0]), head: str = "joint"
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
        """Forced alignment with the transducer head (extension; the reference aligns with the CTC head only,
        wenet/bin/alignment.py): the best path through the lattice whose negative log-sum `forward` reports as
        `loss_rnnt` -- the same encoder, ContextBias biasing and blank / IGNORE_ID label mapping as the loss block.
        With the joiner's precision resolving to "fp32" or "bf16x3" no logits tensor is formed (joint_rnnt_forced_align);
        under a 16-bit (AMP) mode the joiner's logits go to rnnt_forced_align.  Frames are encoder frames (after
        subsampling).  ``head="simple"`` aligns on the lattice of the additive-joiner loss instead (`loss_simple`; the
        model must have been built with `simple_loss_weight > 0`).  Returns (label_frames (B, U) int32, -1 past
        text_lengths; scores (B,) float64) on the device.  Call it in eval mode unless dropout is wanted.  Both heads
        align on the regular lattice without a delay penalty, whatever `rnnt_type` / `delay_penalty` the model trains
        with.  On a token-and-duration model ``head="joint"`` is `tdt_forced_align` (the TDT lattice), of which it
        returns (label_frames, scores)."""
        if head not in ("joint", "simple"):
            raise ValueError(f"forced_align: head must be \"joint\" or \"simple\", got {head!r}")
        if head == "simple" and not hasattr(self, "simple_am_proj"):
            raise ValueError("forced_align: head=\"simple\" needs a model built with simple_loss_weight > 0")
        assert text_lengths.dim() == 1, text_lengths.shape
        assert (speech.shape[0] == speech_lengths.shape[0] == text.shape[0] == text_lengths.shape[0]), \
            (speech.shape, speech_lengths.shape, text.shape, text_lengths.shape)
        check_limits(text, text_lengths, with_ctc=False)
        if head == "joint" and self._is_tdt():              # the joiner's columns are tokens and durations: its own lattice
            frames, _, scores = self.tdt_forced_align(speech, speech_lengths, text, text_lengths, context_list,
                                                      context_lengths)
            return frames, scores
        with torch.no_grad():
            _, encoder_out, _, encoder_out_lens, _, predictor_out, _ = self._loss_inputs(
                speech, speech_lengths, text, context_list, context_lengths)
            if head == "simple":
                lm, am, symbols, boundary = self._simple_inputs(encoder_out, encoder_out_lens, predictor_out, text,
                                                                text_lengths)
                return rnnt_simple_forced_align(lm, am, symbols, self.blank, boundary=boundary)
            rnnt_text = self._rnnt_text(text)
            rnnt_text_lengths = text_lengths.to(torch.int32)
            encoder_out_lens = encoder_out_lens.to(torch.int32)
            jt = self.joint
            if isinstance(jt, TransducerJoint) and _call_precision(jt.precision) not in ("bf16", "f16"):
                ep, pp = jt.pre_activation(encoder_out, predictor_out)
                return joint_rnnt_forced_align(ep, pp, jt.ffn_out.weight, jt.ffn_out.bias, rnnt_text, encoder_out_lens,
                                               rnnt_text_lengths, blank=self.blank, precision=jt.precision,
                                               activation=jt.activation)
            logits = self.joint(encoder_out, predictor_out)
            return rnnt_forced_align(logits, rnnt_text, encoder_out_lens, rnnt_text_lengths, blank=self.blank)

    @torch.jit.unused      # HIP-backed, like forward
    def tdt_forced_align(self, speech: torch.Tensor, speech_lengths: torch.Tensor, text: torch.Tensor,
                         text_lengths: torch.Tensor, context_list: torch.Tensor = torch.IntTensor([0]),
                         context_lengths: torch.Tensor = torch.IntTensor([0]), return_blank_jumps: bool = False):
        """Forced alignment of a token-and-duration model: the best path through the lattice whose negative log-sum
        `forward` reports as `loss_rnnt` (rnnt_tdt_forced_align on the joiner's logits, in whatever precision it produces
        them, with the model's `tdt_durations` and `tdt_sigma`) -- the same encoder, predictor and blank / IGNORE_ID
        label mapping as the loss block.  Returns (label_frames (B, U) int32, label_durations (B, U) int32, both -1 past
        text_lengths; scores (B,) float64[; blank_jumps (B, T) int32]) on the device; frames are encoder frames."""
        if not self._is_tdt():
            raise ValueError("Transducer.tdt_forced_align: the model has no tdt_durations (use forced_align)")
        assert text_lengths.dim() == 1, text_lengths.shape
        assert (speech.shape[0] == speech_lengths.shape[0] == text.shape[0] == text_lengths.shape[0]), \
            (speech.shape, speech_lengths.shape, text.shape, text_lengths.shape)
        check_limits(text, text_lengths, with_ctc=False)
        with torch.no_grad():
            _, encoder_out, _, encoder_out_lens, _, predictor_out, _ = self._loss_inputs(
                speech, speech_lengths, text, context_list, context_lengths)
            rnnt_text = self._rnnt_text(text)
            logits = self.joint(encoder_out, predictor_out)
            return rnnt_tdt_forced_align(logits, rnnt_text, encoder_out_lens.to(torch.int32), text_lengths.to(torch.int32),
                                         self.tdt_durations, blank=self.blank, sigma=self.tdt_sigma,
                                         return_blank_jumps=return_blank_jumps)

    def _calc_att_loss(self, encoder_out, encoder_mask, ys_pad, ys_pad_lens):
        """asr_model.py:115-148 (attention decoder is whatever module the caller attached)."""
        ys_in_pad, ys_out_pad = add_sos_eos(ys_pad, self.sos, self.eos, self.ignore_id)
        ys_in_lens = ys_pad_lens + 1
        r_ys_pad = reverse_pad_list(ys_pad, ys_pad_lens, float(self.ignore_id))
        r_ys_in_pad, r_ys_out_pad = add_sos_eos(r_ys_pad, self.sos, self.eos, self.ignore_id)
        decoder_out, r_decoder_out, _ = self.decoder(encoder_out, encoder_mask, ys_in_pad, ys_in_lens, r_ys_in_pad,
                                                     self.reverse_weight)
        loss_att = self.criterion_att(decoder_out, ys_out_pad)
        r_loss_att = torch.tensor(0.0, device=loss_att.device)
        if self.reverse_weight > 0.0:
            r_loss_att = self.criterion_att(r_decoder_out, r_ys_out_pad)
        loss_att = loss_att * (1 - self.reverse_weight) + r_loss_att * self.reverse_weight
        pred = decoder_out.view(-1, self.vocab_size).argmax(1)
        mask = ys_out_pad.view(-1) != self.ignore_id
        acc = float((pred[mask] == ys_out_pad.view(-1)[mask]).sum()) / max(int(mask.sum()), 1)
        return loss_att, acc

    # -------------------------------------------------------------- decoding --
    def init_bs(self):
        if self.bs is None:
            self.bs = PrefixBeamSearch(self.encoder, self.predictor, self.joint, self.ctc, self.blank)

    def _cal_transducer_score(self, encoder_out: torch.Tensor, encoder_mask: torch.Tensor, hyps_lens: torch.Tensor,
                              hyps_pad: torch.Tensor):
        """-rnnt_loss(reduction='none') per hypothesis (transducer.py:277-302)."""
        xs_in_lens, predictor_out, rnnt_text = self._score_inputs(encoder_mask, hyps_pad)
        if self._can_fuse_loss():                   # same node as the training loss block: no pass 1 over the logits
            ep, pp = self.joint.pre_activation(encoder_out, predictor_out)
            loss_td = joint_rnnt_loss(ep, pp, self.joint.ffn_out.weight, self.joint.ffn_out.bias, rnnt_text,
                                      xs_in_lens, hyps_lens.int(), blank=self.blank, reduction="none",
                                      precision=self.joint.precision, activation=self.joint.activation)
            return loss_td * -1
        joint_out = self.joint(encoder_out, predictor_out)
        loss_td = rnnt_loss(joint_out, rnnt_text.contiguous(), xs_in_lens.contiguous(), hyps_lens.int().contiguous(),
                            blank=self.blank, reduction="none")
        return loss_td * -1

    def _score_inputs(self, encoder_mask: torch.Tensor, hyps_pad: torch.Tensor):
        """(encoder lengths int32, predictor output of the blank-prefixed hypotheses, the hypotheses as loss labels)."""
        hyps_pad_blank = add_blank(hyps_pad, self.blank, self.ignore_id)
        xs_in_lens = encoder_mask.squeeze(1).sum(1).int()
        return xs_in_lens, self.predictor(hyps_pad_blank), self._rnnt_text(hyps_pad)

    def _cal_attn_score(self, encoder_out, encoder_mask, hyps_pad, hyps_lens, reverse_weight: Optional[float] = None):
        """transducer.py:304-330 (decoder called with self.reverse_weight) and the same block inside
        asr_model.py:485-502 (called with the rescoring call's reverse_weight)."""
        if reverse_weight is None:
            reverse_weight = self.reverse_weight
        ori_hyps_pad = hyps_pad
        hyps_pad, _ = add_sos_eos(hyps_pad, self.sos, self.eos, self.ignore_id)
        hyps_lens = hyps_lens + 1
        r_hyps_pad = reverse_pad_list(ori_hyps_pad, hyps_lens, self.ignore_id)
        r_hyps_pad, _ = add_sos_eos(r_hyps_pad, self.sos, self.eos, self.ignore_id)
        decoder_out, r_decoder_out, _ = self.decoder(encoder_out, encoder_mask, hyps_pad, hyps_lens, r_hyps_pad,
                                                     reverse_weight)
        decoder_out = torch.nn.functional.log_softmax(decoder_out, dim=-1).cpu().numpy()
        r_decoder_out = torch.nn.functional.log_softmax(r_decoder_out, dim=-1).cpu().numpy()
        return decoder_out, r_decoder_out

    def _attention_scores(self, hyps, decoder_out, r_decoder_out, reverse_weight: float):
        """Per hypothesis: sum of the attention decoder's log-probabilities of its tokens plus <eos>, mixed with the
        right-to-left decoder's when reverse_weight > 0 (the inner loop shared by asr_model.py:511-525 and
        transducer.py:485-503; numpy fp32 rows summed left to right as there)."""
        out = []
        for i, hyp in enumerate(hyps):
            n = len(hyp)
            score = 0.0
            for j, w in enumerate(hyp):
                score += decoder_out[i][j][w]
            score += decoder_out[i][n][self.eos]
            if reverse_weight > 0:
                r_score = 0.0
                for j, w in enumerate(hyp):
                    r_score += r_decoder_out[i][n - j - 1][w]
                r_score += r_decoder_out[i][n][self.eos]
                score = score * (1 - reverse_weight) + r_score * reverse_weight
            out.append(score)
        return out

    # CTC decode modes inherited from ASRModel in the reference (asr_model.py:281-440)
    def _forward_encoder(self, speech, speech_lengths, decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                         simulate_streaming: bool = False):
        if simulate_streaming and decoding_chunk_size > 0:
            return self.encoder.forward_chunk_by_chunk(speech, decoding_chunk_size=decoding_chunk_size,
                                                       num_decoding_left_chunks=num_decoding_left_chunks)
        return self.encoder(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks)

    def _encoded(self, speech, speech_lengths, *chunking):
        """What every decode mode starts with: the shape asserts and the encoder -> (encoder_out, encoder_out_lens)."""
        assert speech.shape[0] == speech_lengths.shape[0]
        assert chunking[0] != 0                                           # decoding_chunk_size
        encoder_out, encoder_mask = self._forward_encoder(speech, speech_lengths, *chunking)
        return encoder_out, encoder_mask.squeeze(1).sum(1)

    def _ctc_logits(self, speech, speech_lengths, *chunking):
        """`_encoded` and the CTC projection -> (ctc_lo output, encoder_out, encoder_out_lens)."""
        encoder_out, encoder_out_lens = self._encoded(speech, speech_lengths, *chunking)
        with torch.no_grad():
            return self.ctc.ctc_lo(encoder_out), encoder_out, encoder_out_lens

    def ctc_greedy_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                          num_decoding_left_chunks: int = -1, simulate_streaming: bool = False):
        """asr_model.py:281-324 -> (hyps, scores)."""
        from .ctc import ctc_greedy_search
        logits, _, encoder_out_lens = self._ctc_logits(speech, speech_lengths, decoding_chunk_size,
                                                       num_decoding_left_chunks, simulate_streaming)
        return ctc_greedy_search(logits, encoder_out_lens, blank=0, eos=self.eos)

    def _ctc_prefix_beam_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int,
                                decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                                simulate_streaming: bool = False):
        """asr_model.py:326-409 -> (hyps [(prefix, score)], encoder_out)."""
        from .ctc import ctc_prefix_beam_search
        assert speech.shape[0] == 1
        logits, encoder_out, _ = self._ctc_logits(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks,
                                                  simulate_streaming)
        lens = torch.tensor([encoder_out.size(1)], dtype=torch.int32)
        return ctc_prefix_beam_search(logits, lens, beam_size)[0], encoder_out

    def ctc_prefix_beam_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int,
                               decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                               simulate_streaming: bool = False):
        """asr_model.py:411-440"""
        hyps, _ = self._ctc_prefix_beam_search(speech, speech_lengths, beam_size, decoding_chunk_size,
                                               num_decoding_left_chunks, simulate_streaming)
        return hyps[0]

    def ctc_prefix_beam_search_times(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int,
                                     decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                                     simulate_streaming: bool = False):
        """The n-best of ctc_prefix_beam_search with, per hypothesis, the Viterbi score and the frame of every token
        (the runtime's viterbi_likelihood() / Times(), ctc_prefix_beam_search.cc:107-211), for any batch size:
        per utterance [(prefix, score, viterbi_score, times)] best first."""
        from .ctc import ctc_prefix_beam_search_times
        logits, _, encoder_out_lens = self._ctc_logits(speech, speech_lengths, decoding_chunk_size,
                                                       num_decoding_left_chunks, simulate_streaming)
        return ctc_prefix_beam_search_times(logits, encoder_out_lens, beam_size)

    def ctc_context_prefix_beam_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int,
                                       context_graph, decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                                       simulate_streaming: bool = False):
        """ctc_prefix_beam_search_times with the context-graph phrase biasing of the runtime (--context_path /
        --context_score), finalised: per utterance [(prefix, score, viterbi_score, times, ctc_score, context_score,
        tags)] best first, score = ctc_score + context_score."""
        from .ctc import ctc_context_prefix_beam_search
        logits, _, encoder_out_lens = self._ctc_logits(speech, speech_lengths, decoding_chunk_size,
                                                       num_decoding_left_chunks, simulate_streaming)
        return ctc_context_prefix_beam_search(logits, encoder_out_lens, beam_size, context_graph)

    # ------------------------------------------- ASRModel surface the reference class inherits (asr_model.py) --
    # The reference's Transducer IS an ASRModel (transducer.py:20), so wenet/bin/recognize.py may call `recognize`
    # (--mode attention, recognize.py:259) and `attention_rescoring` (--mode attention_rescoring, :351) on it, and
    # the C++ runtime calls the exported helpers below.  Plain host logic over the caller's attention decoder; the
    # n-best list of attention_rescoring comes from the HIP CTC prefix beam search.
    def recognize(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int = 10,
                  decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1, simulate_streaming: bool = False):
        """Beam search on the attention decoder, batched (asr_model.py:175-279) -> (best_hyps (B, L), best_scores (B,)).
        Every step keeps `beam_size` prefixes per utterance: per-prefix top-k, finished prefixes carry one zero-cost
        <eos> branch, top-k again over the beam_size^2 candidates; no length normalisation."""
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        dev = speech.device
        B, N = speech.shape[0], beam_size
        memory, memory_mask = self._forward_encoder(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks,
                                                    simulate_streaming)
        L = memory.size(1)
        memory = memory.repeat_interleave(N, dim=0)                              # utterance-major, beam-minor rows
        memory_mask = memory_mask.repeat_interleave(N, dim=0)
        hyps = torch.full((B * N, 1), self.sos, dtype=torch.long, device=dev)
        scores = torch.full((B, N), -float("inf"), device=dev)
        scores[:, 0] = 0.0                                                       # one live prefix per utterance at start
        scores = scores.view(-1, 1)
        done = torch.zeros(B * N, 1, dtype=torch.bool, device=dev)
        cache: Optional[List[torch.Tensor]] = None
        first_of_utt = torch.arange(B, device=dev).unsqueeze(1) * N            # (B, 1)
        for i in range(1, L + 1):
            if bool(done.all()):
                break
            causal = torch.ones(i, i, dtype=torch.bool, device=dev).tril().unsqueeze(0).expand(B * N, i, i)
            logp, cache = self.decoder.forward_one_step(memory, memory_mask, hyps, causal, cache)
            cand_logp, cand_tok = logp.topk(N)                                   # (B*N, N)
            # a finished prefix keeps exactly one continuation: <eos> at no cost
            cand_logp = cand_logp.masked_fill(done, -float("inf"))
            cand_logp[:, 0] = torch.where(done.squeeze(1), torch.zeros_like(cand_logp[:, 0]), cand_logp[:, 0])
            cand_tok = cand_tok.masked_fill(done, self.eos)
            scores, pick = (scores + cand_logp).view(B, N * N).topk(N)           # (B, N) each
            scores = scores.view(-1, 1)
            parent = (first_of_utt + pick // N).view(-1)                         # row of the prefix each survivor extends
            tok = cand_tok.view(B, N * N).gather(1, pick).view(-1, 1)
            hyps = torch.cat([hyps.index_select(0, parent), tok], dim=1)
            done = tok == self.eos
        best_scores, best = scores.view(B, N).max(dim=-1)
        rows = best + torch.arange(B, device=dev) * N
        return hyps.index_select(0, rows)[:, 1:], best_scores

    def attention_rescoring(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int,
                            decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1, ctc_weight: float = 0.0,
                            simulate_streaming: bool = False, reverse_weight: float = 0.0):
        """CTC prefix beam search n-best rescored by the attention decoder (asr_model.py:443-540) ->
        (best prefix tuple, score)."""
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        if reverse_weight > 0.0:
            assert hasattr(self.decoder, "right_decoder")
        device = speech.device
        assert speech.shape[0] == 1
        hyps, encoder_out = self._ctc_prefix_beam_search(speech, speech_lengths, beam_size, decoding_chunk_size,
                                                         num_decoding_left_chunks, simulate_streaming)
        assert len(hyps) == beam_size
        prefixes = [h[0] for h in hyps]
        hyps_pad = pad_sequence([torch.tensor(h, device=device, dtype=torch.long) for h in prefixes], True, self.ignore_id)
        hyps_lens = torch.tensor([len(h) for h in prefixes], device=device, dtype=torch.long)
        encoder_out = encoder_out.repeat(beam_size, 1, 1)
        encoder_mask = torch.ones(beam_size, 1, encoder_out.size(1), dtype=torch.bool, device=device)
        decoder_out, r_decoder_out = self._cal_attn_score(encoder_out, encoder_mask, hyps_pad, hyps_lens,
                                                          reverse_weight=reverse_weight)
        att = self._attention_scores(prefixes, decoder_out, r_decoder_out, reverse_weight)
        best_score, best_index = -float("inf"), 0
        for i in range(len(hyps)):
            score = att[i] + hyps[i][1] * ctc_weight
            if score > best_score:
                best_score, best_index = score, i
        return hyps[best_index][0], best_score

    def beam_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                    beam_size: int = 5, num_decoding_left_chunks: int = -1, simulate_streaming: bool = False,
                    ctc_weight: float = 0.3, transducer_weight: float = 0.7, **_ignored):
        """transducer.py:332-377.  Extra keyword arguments (recognize.py:303-304 passes context_list /
        context_lengths, which the reference signature lacks) are accepted and ignored."""
        self._refuse_tdt("beam_search")
        self.init_bs()
        beam, _ = self.bs.prefix_beam_search(speech, speech_lengths, decoding_chunk_size, beam_size,
                                             num_decoding_left_chunks, simulate_streaming, ctc_weight,
                                             transducer_weight)
        return beam[0].hyp[1:], beam[0].score

    def transducer_attention_rescoring(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int,
                                       decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                                       simulate_streaming: bool = False, reverse_weight: float = 0.0,
                                       ctc_weight: float = 0.0, attn_weight: float = 0.0,
                                       transducer_weight: float = 0.0, search_ctc_weight: float = 1.0,
                                       search_transducer_weight: float = 0.0, beam_search_type: str = "transducer"):
        """transducer.py:379-513"""
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        if reverse_weight > 0.0:
            assert hasattr(self.decoder, "right_decoder")
        device = speech.device
        assert speech.shape[0] == 1
        if beam_search_type == "transducer":
            self._refuse_tdt("transducer_attention_rescoring(beam_search_type=\"transducer\")")
        self.init_bs()
        if beam_search_type == "transducer":
            beam, encoder_out = self.bs.prefix_beam_search(speech, speech_lengths, decoding_chunk_size=decoding_chunk_size,
                                                           beam_size=beam_size,
                                                           num_decoding_left_chunks=num_decoding_left_chunks,
                                                           ctc_weight=search_ctc_weight,
                                                           transducer_weight=search_transducer_weight)
            beam_score = [s.score for s in beam]
            hyps = [s.hyp[1:] for s in beam]
        elif beam_search_type == "ctc":                                     # transducer.py:447-456
            hyps, encoder_out = self._ctc_prefix_beam_search(speech, speech_lengths, beam_size=beam_size,
                                                             decoding_chunk_size=decoding_chunk_size,
                                                             num_decoding_left_chunks=num_decoding_left_chunks,
                                                             simulate_streaming=simulate_streaming)
            beam_score = [hyp[1] for hyp in hyps]
            hyps = [hyp[0] for hyp in hyps]                                 # prefix tuples, as the reference keeps them
        else:
            raise ValueError(f"unknown beam_search_type {beam_search_type!r}")
        assert len(hyps) == beam_size
        return self._rescore(hyps, beam_score, encoder_out, device, self._cal_transducer_score, reverse_weight, attn_weight,
                             ctc_weight, transducer_weight)

    def _rescore(self, hyps, beam_score, encoder_out, device, cal_td_score, reverse_weight: float, attn_weight: float,
                 ctc_weight: float, transducer_weight: float):
        """The tail of the two rescoring methods: the n-best `hyps` of ONE utterance (encoder_out (1, T, E)) padded, scored
        by `cal_td_score` and by the attention decoder -> (the hypothesis with the largest att * attn_weight + beam score *
        ctc_weight + td_score * transducer_weight, that score)."""
        n = len(hyps)
        hyps_pad = pad_sequence([torch.tensor(h, device=device, dtype=torch.long) for h in hyps], True, self.ignore_id)
        hyps_lens = torch.tensor([len(h) for h in hyps], device=device, dtype=torch.long)
        encoder_out = encoder_out.repeat(n, 1, 1)
        encoder_mask = torch.ones(n, 1, encoder_out.size(1), dtype=torch.bool, device=device)
        td_score = cal_td_score(encoder_out, encoder_mask, hyps_lens, hyps_pad)
        decoder_out, r_decoder_out = self._cal_attn_score(encoder_out, encoder_mask, hyps_pad, hyps_lens)
        att = self._attention_scores(hyps, decoder_out, r_decoder_out, reverse_weight)
        best_score, best_index = -float("inf"), 0
        for i in range(n):
            score = att[i] * attn_weight + beam_score[i] * ctc_weight + td_score[i] * transducer_weight
            if score > best_score:
                best_score, best_index = score, i
        return hyps[best_index], best_score

    def greedy_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                      num_decoding_left_chunks: int = -1, simulate_streaming: bool = False, n_steps: int = 64,
                      context_list: torch.Tensor = torch.IntTensor([0]),
                      context_lengths: torch.Tensor = torch.IntTensor([0]), context_filter_state: str = "on",
                      context_decoder_labels_padded: torch.Tensor = torch.IntTensor([0])):
        """transducer.py:515-598 -> (hyps: List[List[int]], dist).  With no hot-word module the fork's
        variants reduce to the upstream loop and `dist` (an edit distance over the hot-word gate trace) is 0."""
        assert speech.size(0) == 1
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        _ = simulate_streaming
        encoder_out, encoder_mask = self.encoder(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks)
        encoder_out_lens = encoder_mask.squeeze(1).sum()
        if self._is_tdt():                                  # token-and-duration model: its own device search
            return tdt_greedy_search(self, encoder_out, encoder_out_lens, n_steps=n_steps), 0
        if self.context_bias is None:                       # no hot-word module: the variants reduce to the core loop
            return basic_greedy_search(self, encoder_out, encoder_out_lens, n_steps=n_steps), 0
        if self.loss_mode == "pred":                        # transducer.py:559-567
            hyps, dist, _ = basic_greedy_search_hw(self, encoder_out, encoder_out_lens, context_list, context_lengths,
                                                   n_steps=n_steps, context_filter_state=context_filter_state,
                                                   context_decoder_labels_padded=context_decoder_labels_padded)
            return hyps, dist
        # loss_mode 'both' (the default) -- and the reference's final `else` branch, which calls the same function
        # but assigns its (hyps, dist) tuple to `hyps` (transducer.py:589-597, a latent bug); we return (hyps, dist)
        return basic_greedy_search_both(self, encoder_out, encoder_out_lens, context_list, context_lengths,
                                        n_steps=n_steps, context_filter_state=context_filter_state,
                                        context_decoder_labels_padded=context_decoder_labels_padded)

    def greedy_search_batch(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                            num_decoding_left_chunks: int = -1, n_steps: int = 64) -> List[List[int]]:
        """Extension: N independent streams decoded together (BASELINE config 3)."""
        self._refuse_tdt("greedy_search_batch")
        encoder_out, encoder_mask = self.encoder(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks)
        return basic_greedy_search(self, encoder_out, encoder_mask.squeeze(1).sum(1), n_steps=n_steps)

    def tdt_greedy_search_batch(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                                num_decoding_left_chunks: int = -1, n_steps: int = 64, return_frames: bool = False):
        """Extension: N utterances of a token-and-duration model decoded together -> one token list per utterance; with
        `return_frames` also the encoder frame at which each token was emitted."""
        if not self._is_tdt():
            raise ValueError("Transducer.tdt_greedy_search_batch: the model has no tdt_durations (use greedy_search_batch)")
        encoder_out, encoder_mask = self.encoder(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks)
        return tdt_greedy_search(self, encoder_out, encoder_mask.squeeze(1).sum(1), n_steps=n_steps,
                                 return_frames=return_frames)

    # ---------------------------------------------- token-and-duration prefix beam search --
    def _tdt_beam(self, what: str, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int,
                  beam_size: int, num_decoding_left_chunks: int, simulate_streaming: bool, ctc_weight: float,
                  transducer_weight: float):
        """Encoder + `tdt_prefix_beam_search` -> (per utterance the n-best, encoder_out, encoder_mask)."""
        if not self._is_tdt():
            plain = {"tdt_attention_rescoring": "transducer_attention_rescoring"}.get(what, what[len("tdt_"):])
            raise ValueError(f"Transducer.{what}: the model has no tdt_durations (use {plain})")
        assert speech.shape[0] == speech_lengths.shape[0]
        assert decoding_chunk_size != 0
        encoder_out, encoder_mask = self._forward_encoder(speech, speech_lengths, decoding_chunk_size,
                                                          num_decoding_left_chunks, simulate_streaming)
        nbest = tdt_prefix_beam_search(self, encoder_out, encoder_mask.squeeze(1).sum(1), beam_size=beam_size,
                                       ctc_weight=ctc_weight, transducer_weight=transducer_weight)
        return nbest, encoder_out, encoder_mask

    def tdt_beam_search(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                        beam_size: int = 5, num_decoding_left_chunks: int = -1, simulate_streaming: bool = False,
                        ctc_weight: float = 0.0, transducer_weight: float = 1.0, **_ignored):
        """`beam_search` for a token-and-duration model -> (best hypothesis without the seed blank, its score).  The
        search is `tdt_prefix_beam_search`.  The defaults are (0, 1), not `beam_search`'s 0.3 / 0.7: a hypothesis
        that jumps `d` frames is scored with the CTC posterior of the frame it stands at only, and that posterior says
        nothing about the frames the jump skips, so the mixture is opt-in."""
        assert speech.shape[0] == 1
        nbest, _, _ = self._tdt_beam("tdt_beam_search", speech, speech_lengths, decoding_chunk_size, beam_size,
                                     num_decoding_left_chunks, simulate_streaming, ctc_weight, transducer_weight)
        return nbest[0][0].hyp[1:], nbest[0][0].score

    def tdt_beam_search_batch(self, speech: torch.Tensor, speech_lengths: torch.Tensor, decoding_chunk_size: int = -1,
                              beam_size: int = 5, num_decoding_left_chunks: int = -1, simulate_streaming: bool = False,
                              ctc_weight: float = 0.0, transducer_weight: float = 1.0):
        """Extension: the n-best of every utterance of a batch -> per utterance [(hypothesis without the seed blank,
        score)], best first."""
        nbest, _, _ = self._tdt_beam("tdt_beam_search_batch", speech, speech_lengths, decoding_chunk_size, beam_size,
                                     num_decoding_left_chunks, simulate_streaming, ctc_weight, transducer_weight)
        return [[(s.hyp[1:], s.score) for s in utt] for utt in nbest]

    def _cal_tdt_score(self, encoder_out: torch.Tensor, encoder_mask: torch.Tensor, hyps_lens: torch.Tensor,
                       hyps_pad: torch.Tensor):
        """-rnnt_tdt_loss(reduction='none') per hypothesis, with the model's durations and sigma: `_cal_transducer_score`
        for a token-and-duration model."""
        xs_in_lens, predictor_out, rnnt_text = self._score_inputs(encoder_mask, hyps_pad)
        joint_out = self.joint(encoder_out, predictor_out)
        loss_td = rnnt_tdt_loss(joint_out, rnnt_text.contiguous(), xs_in_lens.contiguous(), hyps_lens.int().contiguous(),
                                self.tdt_durations, blank=self.blank, sigma=self.tdt_sigma, reduction="none")
        return loss_td * -1

    def tdt_attention_rescoring(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int,
                                decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                                simulate_streaming: bool = False, reverse_weight: float = 0.0, ctc_weight: float = 0.0,
                                attn_weight: float = 0.0, transducer_weight: float = 0.0, search_ctc_weight: float = 1.0,
                                search_transducer_weight: float = 0.0):
        """`transducer_attention_rescoring` for a token-and-duration model: the n-best of `tdt_prefix_beam_search`
        (searched with search_ctc_weight / search_transducer_weight) rescored as
        att * attn_weight + beam score * ctc_weight + td_score * transducer_weight, td_score from `_cal_tdt_score`
        -> (best hypothesis, its score)."""
        if reverse_weight > 0.0:
            assert hasattr(self.decoder, "right_decoder")
        device = speech.device
        assert speech.shape[0] == 1
        nbest, encoder_out, _ = self._tdt_beam("tdt_attention_rescoring", speech, speech_lengths, decoding_chunk_size,
                                               beam_size, num_decoding_left_chunks, simulate_streaming, search_ctc_weight,
                                               search_transducer_weight)
        beam_score = [s.score for s in nbest[0]]
        hyps = [s.hyp[1:] for s in nbest[0]]
        # no assert on len(hyps): a short utterance may have fewer than beam_size hypotheses
        return self._rescore(hyps, beam_score, encoder_out, device, self._cal_tdt_score, reverse_weight, attn_weight,
                             ctc_weight, transducer_weight)

    # ------------------------------------- streaming greedy ("transducer ref.py":541-606) --
    def reset_cache(self, n_streams: int = 1, chunk_frames: int = 64, n_steps: int = 64) -> None:
        """Start `n_streams` fresh streams (the reference's reset_cache is the n_streams=1 case)."""
        self._stream = dict(n=n_streams, fresh=True, tmax=chunk_frames, n_steps=n_steps)

    def forward_greedy_search(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, n_steps: int = 64,
                              reference_new_cache: bool = True):
        """Decode the next chunk of encoder frames of every stream: encoder_out (N, Tchunk, E) -> tokens of this
        chunk (List[int] for one stream as in the reference, List[List[int]] for several)."""
        self._refuse_tdt("forward_greedy_search")
        st = getattr(self, "_stream", None)
        if st is None:
            self.reset_cache(encoder_out.size(0))
            st = self._stream
        N = encoder_out.size(0)
        assert N == st["n"], "call reset_cache(n_streams) before changing the number of streams"
        lens, dec = lens_and_decoder(self, encoder_out, encoder_out_lens, n_steps, tmax=st["tmax"])
        if not st["fresh"] and getattr(self, "_stream_dec", None) is not dec:
            raise RuntimeError("the decoder handle was rebuilt (weights changed or capacity grew) in the middle of a "
                               "stream: call reset_cache() with the largest chunk size first")
        hyps = dec.greedy_chunk(encoder_out, lens, n_steps=n_steps, blank=self.blank, reset=st["fresh"],
                                reference_new_cache=reference_new_cache)
        st["fresh"] = False
        self._stream_dec = dec
        return hyps[0] if N == 1 else hyps

    # ----- streaming transducer prefix beam search (what runtime/core/decoder/rnnt_prefix_beam_search.{h,cc} drafts) --
    def reset_beam_stream(self, n_streams: int = 1, beam_size: int = 5, max_frames: int = 4096, chunk_frames: int = 64,
                          ctc_weight: Optional[float] = None, transducer_weight: Optional[float] = None) -> None:
        """Start `n_streams` fresh streams of the transducer prefix beam search, plain or token-and-duration
        (`TransducerPrefixBeamStream`).  `max_frames` bounds the encoder frames (chunk widths summed) a stream may take
        before its next reset, `chunk_frames` the width of a chunk.  The weights default to `beam_search`'s 0.3 / 0.7 for
        a plain model and to `tdt_beam_search`'s 0 / 1 for a model with tdt_durations."""
        from .search.prefix_beam_search import TransducerPrefixBeamStream
        self._beam_stream = TransducerPrefixBeamStream(self, n_streams, beam_size, max_frames, chunk_frames, ctc_weight,
                                                       transducer_weight)

    def forward_prefix_beam_search(self, encoder_out_chunk: torch.Tensor, encoder_out_lens: torch.Tensor, final=False):
        """Feed the next chunk of encoder frames of every stream, encoder_out_chunk (N, Tchunk, E) with encoder_out_lens
        (N,) valid frames each (0 without `final`: the stream is left untouched); `final` (a bool or one per stream) marks
        a stream's last chunk -> the current n-best of every stream, [(tokens incl. the seed blank, score, viterbi_score,
        times)] best first; times are encoder frames since the stream's reset."""
        if getattr(self, "_beam_stream", None) is None:
            self.reset_beam_stream(encoder_out_chunk.size(0), chunk_frames=max(64, encoder_out_chunk.size(1)))
        return self._beam_stream.search(encoder_out_chunk, encoder_out_lens, final=final)

    def beam_search_times(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int = 5,
                          ctc_weight: Optional[float] = None, transducer_weight: Optional[float] = None,
                          decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                          simulate_streaming: bool = False):
        """The n-best of `beam_search` (plain model) / `tdt_beam_search` (tdt_durations) over whole utterances, any batch
        size, with the Viterbi score and the encoder frame of every token: per utterance [(tokens without the seed blank,
        score, viterbi_score, times)] best first.  One reset-and-final chunk of the streaming search."""
        from .search.prefix_beam_search import TransducerPrefixBeamStream
        encoder_out, lens = self._encoded(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks,
                                          simulate_streaming)
        B, T, _ = encoder_out.shape
        stream = TransducerPrefixBeamStream(self, B, beam_size, T, T, ctc_weight, transducer_weight)
        nbest = stream.search(encoder_out, lens, final=True)
        return [[(h[1:], s, v, t) for h, s, v, t in utt] for utt in nbest]

    # ---- the same with context-graph phrase biasing (the context_graph_ member rnnt_prefix_beam_search.h drafts) --
    def reset_beam_context_stream(self, n_streams: int, beam_size: int, max_frames: int, chunk_frames: int, context_graph,
                                  ctc_weight: Optional[float] = None, transducer_weight: Optional[float] = None) -> None:
        """Start `n_streams` fresh biased streams of the transducer prefix beam search, plain or token-and-duration, that
        walk `context_graph` (a ContextGraph); the other arguments are those of `reset_beam_stream`."""
        from .search.prefix_beam_search import TransducerContextPrefixBeamStream
        self._beam_context_stream = TransducerContextPrefixBeamStream(self, n_streams, beam_size, max_frames, chunk_frames,
                                                                      context_graph, ctc_weight, transducer_weight)

    def forward_context_prefix_beam_search(self, encoder_out_chunk: torch.Tensor, encoder_out_lens: torch.Tensor, final=False,
                                           finalize=None):
        """forward_prefix_beam_search on the biased streams -> per stream [(tokens incl. the seed blank, score,
        viterbi_score, times, trans_score, context_score, tags, context_state)] best first.  `finalize` (default: `final`)
        exports a stream as if it ended with this chunk; the stream itself goes on unchanged."""
        if getattr(self, "_beam_context_stream", None) is None:
            raise RuntimeError("call reset_beam_context_stream(n_streams, beam_size, max_frames, chunk_frames, context_graph) "
                               "first")
        return self._beam_context_stream.search(encoder_out_chunk, encoder_out_lens, final=final, finalize=finalize)

    def beam_search_context(self, speech: torch.Tensor, speech_lengths: torch.Tensor, beam_size: int, context_graph,
                            ctc_weight: Optional[float] = None, transducer_weight: Optional[float] = None,
                            decoding_chunk_size: int = -1, num_decoding_left_chunks: int = -1,
                            simulate_streaming: bool = False):
        """`beam_search_times` with context-graph phrase biasing, whole utterances of any batch size: per utterance
        [(tokens without the seed blank, score, viterbi_score, times, trans_score, context_score, tags, context_state)]
        best first.  One reset, final and finalised chunk of the biased streaming search."""
        from .search.prefix_beam_search import TransducerContextPrefixBeamStream
        encoder_out, lens = self._encoded(speech, speech_lengths, decoding_chunk_size, num_decoding_left_chunks,
                                          simulate_streaming)
        B, T, _ = encoder_out.shape
        stream = TransducerContextPrefixBeamStream(self, B, beam_size, T, T, context_graph, ctc_weight, transducer_weight)
        nbest = stream.search(encoder_out, lens, final=True, finalize=True)
        return [[(r[0][1:],) + tuple(r[1:]) for r in utt] for utt in nbest]

    # ------------------- streaming CTC prefix beam search (runtime/core/decoder/ctc_prefix_beam_search.cc:107-211) --
    def reset_ctc_stream(self, n_streams: int = 1, beam_size: int = 10, max_frames: int = 4096) -> None:
        """Start `n_streams` fresh CTC prefix-beam streams; `max_frames` bounds the encoder frames (chunk widths summed)
        a stream may take before the next reset."""
        from .ctc import CtcPrefixBeamStream
        self._ctc_stream = CtcPrefixBeamStream(n_streams, beam_size, max_frames, blank=0)

    def forward_ctc_prefix_beam_search(self, encoder_out_chunk: torch.Tensor, encoder_out_lens: torch.Tensor):
        """Feed the next chunk of encoder frames of every stream, encoder_out_chunk (N, Tchunk, E) with encoder_out_lens
        (N,) valid frames each (0: the stream is left untouched) -> the partial n-best of every stream,
        [(prefix, score, viterbi_score, times)] best first; times are encoder frames since the reset."""
        if getattr(self, "_ctc_stream", None) is None:
            self.reset_ctc_stream(encoder_out_chunk.size(0))
        with torch.no_grad():
            logits = self.ctc.ctc_lo(encoder_out_chunk)
        return self._ctc_stream.search(logits, encoder_out_lens)

    # ---- the same with context-graph phrase biasing (context_graph.cc, ctc_prefix_beam_search.cc:137-193, 213-234) --
    def reset_ctc_context_stream(self, n_streams: int, beam_size: int, max_frames: int, context_graph) -> None:
        """Start `n_streams` fresh biased CTC prefix-beam streams that walk `context_graph` (a ContextGraph)."""
        from .ctc import CtcContextPrefixBeamStream
        self._ctc_context_stream = CtcContextPrefixBeamStream(n_streams, beam_size, max_frames, context_graph, blank=0)

    def forward_ctc_context_prefix_beam_search(self, encoder_out_chunk: torch.Tensor, encoder_out_lens: torch.Tensor,
                                               finalize: bool = False):
        """forward_ctc_prefix_beam_search on the biased streams -> per stream [(prefix, score, viterbi_score, times,
        ctc_score, context_score, tags)] best first; finalize=True exports as if every stream ended with this chunk."""
        if getattr(self, "_ctc_context_stream", None) is None:
            raise RuntimeError("call reset_ctc_context_stream(n_streams, beam_size, max_frames, context_graph) first")
        with torch.no_grad():
            logits = self.ctc.ctc_lo(encoder_out_chunk)
        return self._ctc_context_stream.search(logits, encoder_out_lens, finalize=finalize)

    # ----------------------------------------------------- step exports (:600-629) --
    # @torch.jit.export as in the reference, so that torch.jit.script(model) (train.py:203-205, export_jit.py) yields an
    # artefact with the four step methods the C++ runtime calls (runtime/core/decoder/torch_asr_model.cc).  Eager calls
    # run the HIP kernels; inside the scripted artefact -- which cannot reach a ctypes library -- the predictor step and
    # the joiner are their plain module graphs (`_export_step`, `_export_forward`).
    @torch.jit.export
    def forward_encoder_chunk(self, xs: torch.Tensor, offset: int, required_cache_size: int,
                              att_cache: torch.Tensor = torch.zeros(0, 0, 0, 0),
                              cnn_cache: torch.Tensor = torch.zeros(0, 0, 0, 0)
                              ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        return self.encoder.forward_chunk(xs, offset, required_cache_size, att_cache, cnn_cache)

    # The ASRModel exports the C++ runtime calls on every model (asr_model.py:542-634; torch_asr_model.cc reads
    # subsampling_rate / right_context / sos_symbol / eos_symbol / is_bidirectional_decoder at load time).
    @torch.jit.export
    def subsampling_rate(self) -> int:
        if torch.jit.is_scripting():
            return self._subsampling_rate        # captured at construction: a scripted body cannot probe for `embed`
        else:
            return self.encoder.embed.subsampling_rate

    @torch.jit.export
    def right_context(self) -> int:
        if torch.jit.is_scripting():
            return self._right_context
        else:
            return self.encoder.embed.right_context

    @torch.jit.export
    def sos_symbol(self) -> int:
        return self.sos

    @torch.jit.export
    def eos_symbol(self) -> int:
        return self.eos

    @torch.jit.export
    def ctc_activation(self, xs: torch.Tensor) -> torch.Tensor:
        """Linear + log-softmax in front of the CTC search (asr_model.py:597-607)."""
        if self.ctc is not None:
            return self.ctc.log_softmax(xs)
        else:
            raise RuntimeError("ctc_activation: the model was built without a CTC head")

    @torch.jit.export
    def is_bidirectional_decoder(self) -> bool:
        if self.decoder is not None:
            if hasattr(self.decoder, "right_decoder"):
                return True
            else:
                return False
        else:
            return False

    @torch.jit.export
    def forward_attention_decoder(self, hyps: torch.Tensor, hyps_lens: torch.Tensor, encoder_out: torch.Tensor,
                                  reverse_weight: float = 0.0) -> Tuple[torch.Tensor, torch.Tensor]:
        """Score an n-best list (sos-prefixed `hyps` (N, L), lengths counting the sos) on the attention decoder against
        ONE encoder output (asr_model.py:620-710) -> (log-probs (N, L, V), right-to-left log-probs or a zero tensor).
        The right-to-left input is built without pad_sequence (ONNX-friendly in the reference): the label part of every
        row reversed in place, positions beyond its length filled with eos, the sos column kept."""
        if self.decoder is not None:
            assert encoder_out.size(0) == 1
            n = hyps.size(0)
            assert hyps_lens.size(0) == n
            memory = encoder_out.repeat(n, 1, 1)
            memory_mask = torch.ones(n, 1, memory.size(1), dtype=torch.bool, device=memory.device)
            lab_lens = (hyps_lens - 1).unsqueeze(1)                                   # without the sos
            labels = hyps[:, 1:]
            pos = torch.arange(0, int(torch.max(lab_lens)), 1, device=memory.device)
            valid = lab_lens > pos                                                    # (N, Lmax)
            src = (lab_lens - 1 - pos) * valid                                        # mirrored index, 0 where invalid
            flipped = torch.where(valid, torch.gather(labels, 1, src), self.eos)
            r_hyps = torch.cat([hyps[:, 0:1], flipped], dim=1)
            decoder_out, r_decoder_out, _ = self.decoder(memory, memory_mask, hyps, hyps_lens, r_hyps, reverse_weight)
            decoder_out = torch.nn.functional.log_softmax(decoder_out, dim=-1)
            r_decoder_out = torch.nn.functional.log_softmax(r_decoder_out, dim=-1)
            return decoder_out, r_decoder_out
        else:
            raise RuntimeError("forward_attention_decoder: the model was built without an attention decoder")

    @torch.jit.export
    def forward_predictor_step(self, xs: torch.Tensor, cache: List[torch.Tensor]
                               ) -> Tuple[torch.Tensor, List[torch.Tensor]]:
        assert len(cache) == 2
        padding = torch.zeros(1, 1, device=xs.device)
        return self.predictor.forward_step(xs, padding, cache)

    @torch.jit.export
    def forward_joint_step(self, enc_out: torch.Tensor, pred_out: torch.Tensor) -> torch.Tensor:
        if torch.jit.is_scripting():
            return self.joint._export_forward(enc_out, pred_out)
        else:
            return self.joint(enc_out, pred_out)

    @torch.jit.export
    def forward_predictor_init_state(self) -> List[torch.Tensor]:
        return self.predictor.init_state(1, device=self.joint.ffn_out.weight.device)
