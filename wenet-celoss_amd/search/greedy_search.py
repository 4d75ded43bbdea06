"""Transducer greedy search with the upstream core loop's semantics
(wenet/transducer/search/greedy_search copy.py:6-63),
for any number of independent streams at once, with the whole loop on the
device (`wr_greedy_search`); the token-and-duration (TDT) rule likewise
(`wr_greedy_search_tdt`).

The fork's hot-word variants (greedy_search.py:34-430: context gating and "go-back"
re-decoding around ContextBias) follow below: the default one (`basic_greedy_search_both`,
loss_mode 'both') runs its whole loop on the device when the hot-word module has the
reference ContextBias structure (wenet_celoss_amd/hotword.py); other modules and the
'pred' variant keep a host-driven loop over the HIP step kernels.  With no hot words all
of them reduce to the core loop."""
from __future__ import annotations

from typing import List

import torch


def basic_greedy_search(model: torch.nn.Module, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor,
                        context_list: torch.Tensor = None, context_lengths: torch.Tensor = None,
                        n_steps: int = 64) -> List[List[int]]:
    """encoder_out (N, T, E), encoder_out_lens scalar or (N,) -> one token list per stream.

    `model` needs `.blank`, `.predictor` (RNNPredictor), `.joint` (TransducerJoint) and a
    `_decoder_cache` (wenet_celoss_amd.decoder.DecoderCache); Transducer provides all of them.
    context_* are accepted for signature compatibility and ignored (no hot words)."""
    lens, dec = lens_and_decoder(model, encoder_out, encoder_out_lens, n_steps)
    return dec.greedy(encoder_out, lens, n_steps=n_steps, blank=model.blank)


def expand_lens(encoder_out_lens, N: int) -> torch.Tensor:
    """Lengths as a 1-D tensor; a scalar stands for all N streams."""
    lens = torch.as_tensor(encoder_out_lens).reshape(-1)
    return lens.expand(N) if lens.numel() == 1 and N > 1 else lens


def lens_and_decoder(model, encoder_out: torch.Tensor, encoder_out_lens, n_steps: int, tmax: int = 0):
    """(lengths (N,), the model's cached DeviceDecoder sized for a greedy search of encoder_out (N, T, E)): N lanes,
    frames up to max(T, tmax), n_steps tokens per frame."""
    N, T, _ = encoder_out.shape
    T = max(T, tmax)
    dec = _decoder_cache(model).get(model.predictor, model.joint, lanes=N, utts=N, tmax=T, max_hyp=T * n_steps, beam=1)
    return expand_lens(encoder_out_lens, N), dec


def _decoder_cache(model):
    cache = getattr(model, "_decoder_cache", None)
    if cache is None:
        from ..decoder import DecoderCache
        cache = DecoderCache()
        try:
            model._decoder_cache = cache
        except Exception:
            pass
    return cache


def tdt_greedy_search(model: torch.nn.Module, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor,
                      n_steps: int = 64, return_frames: bool = False):
    """Greedy search of a token-and-duration model (`model.tdt_durations`; the joiner's row is `vocab_size` token logits
    followed by one logit per duration) for any number of streams at once, with the whole loop on the device
    (`wr_greedy_search_tdt`).  At frame t: k = argmax of the token part, d = durations[argmax of the duration part]; a
    blank moves max(d, 1) frames on; a label is emitted, steps the predictor and moves d frames on; after `n_steps` labels
    without a frame advance the search moves one frame on.

    encoder_out (N, T, E), encoder_out_lens scalar or (N,) -> one token list per stream; with `return_frames` also the
    frame at which each token was emitted.  Sized like `basic_greedy_search` (max_hyp = T * n_steps).
    WR_TDT_HOST=1 forces the host-driven loop over the HIP step kernels (one stream)."""
    import os
    if os.environ.get("WR_TDT_HOST", "0") == "1":
        hyps, frames = _tdt_greedy_host(model, encoder_out, encoder_out_lens, n_steps)
        return ([hyps], [frames]) if return_frames else [hyps]
    lens, dec = lens_and_decoder(model, encoder_out, encoder_out_lens, n_steps)
    return dec.greedy_tdt(encoder_out, lens, model.tdt_durations, n_steps=n_steps, blank=model.blank,
                          return_frames=return_frames)


def _tdt_greedy_host(model, encoder_out, encoder_out_lens, n_steps):
    """The rule of `tdt_greedy_search` host-driven, one utterance: one predictor.forward_step, one joiner call and one
    host synchronisation per decision -> (tokens, frames)."""
    assert encoder_out.size(0) == 1
    durations = model.tdt_durations
    V = model.vocab_size
    dev = encoder_out.device
    padding = torch.zeros(1, 1, device=dev)
    tok = torch.tensor([[model.blank]], device=dev)
    cache = model.predictor.init_state(1, method="zero", device=dev)
    new_cache = cache
    T = int(encoder_out_lens)
    t, emitted_in_frame, step = 0, 0, True
    hyps: List[int] = []
    frames: List[int] = []
    pred_out = None
    with torch.no_grad():
        while t < T:
            if step:
                pred_out, new_cache = model.predictor.forward_step(tok, padding, cache)
                step = False
            row = model.joint(encoder_out[:, t:t + 1, :].contiguous(), pred_out.contiguous()).reshape(-1).float()
            k, n = torch.stack([row[:V].argmax(), row[V:].argmax()]).tolist()        # one host sync per step
            d = durations[n]
            if k == model.blank:
                t += max(d, 1)
                emitted_in_frame = 0
                continue
            hyps.append(k)
            frames.append(t)
            tok = torch.tensor([[k]], device=dev)
            cache = new_cache
            step = True
            emitted_in_frame = 0 if d > 0 else emitted_in_frame + 1
            t += d
            if emitted_in_frame >= n_steps:
                t += 1
                emitted_in_frame = 0
    return hyps, frames


# ------------------------------------------------------------------------------------------------
# The fork's hot-word variants: wenet/transducer/search/greedy_search.py
#   basic_greedy_search       :34-176   loss_mode 'pred'  -> ([hyps], dist, gate trace)
#   basic_greedy_search_both  :297-430  loss_mode 'both'  -> ([hyps], dist)
# Host-driven, one utterance, exactly the reference's control flow: a hot-word gate (top-1 of the ContextBias
# classifier) per predictor step, and with context_filter_state == 'on' a "go-back" -- when the gate flips
# 0 -> 1 the decoder rewinds to the frame of the last gate-0 step, drops that step's token and re-decodes with
# biasing forced on until the frame where the flip was seen.  The per-step arithmetic runs on the HIP step
# kernels (predictor.forward_step, joint); the ContextBias object is whatever module the caller attached
# (stock PyTorch).  Differences from the reference: nothing is printed to stdout (:363,:428-429 print tensors).
def edit_distance(a, b) -> float:
    """Levenshtein distance (greedy_search.py:6-32), returned as float like the reference's numpy cell."""
    m, n = len(a), len(b)
    prev = list(range(n + 1))
    for i in range(1, m + 1):
        cur = [i] + [0] * n
        for j in range(1, n + 1):
            cost = 0 if int(a[i - 1]) == int(b[j - 1]) else 1
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + cost)
        prev = cur
    return float(prev[n])


def _hotword_greedy(model, encoder_out, encoder_out_lens, context_list, context_lengths, n_steps, filter_on, labels,
                    both: bool):
    dev = encoder_out.device
    cb = model.context_bias
    padding = torch.zeros(1, 1, device=dev)
    tok = torch.tensor([[model.blank]], device=dev)
    cache = model.predictor.init_state(1, method="zero", device=dev)
    new_cache = cache
    hidden = cb.forward_bias_hidden(context_list, context_lengths)
    hidden_none = cb.forward_bias_hidden(torch.zeros((1, 1), dtype=torch.int), context_lengths[0].unsqueeze(0))
    enc_plain = encoder_out.clone()
    enc_hot, enc_hot_feat = cb.forward_encoder_bias(hidden, encoder_out)
    enc_cold, _ = cb.forward_encoder_bias(hidden_none, enc_plain)

    T = int(encoder_out_lens)
    t, emitted_in_frame = 0, 0
    stepped_last = True                    # "previous output was not blank": the predictor must step
    rewinding, rewind_until, frame_of_last_zero = False, -1, 0
    hyps, gates = [], []
    outs, caches, inputs = [], [], []      # one record per predictor step, for the go-back
    pred_out = None
    while t < T:
        if stepped_last:
            pred_out, new_cache = model.predictor.forward_step(tok, padding, cache)
            outs.append(pred_out); caches.append(cache); inputs.append(tok)
            if both:
                raw = pred_out.clone()
                pred_out, pred_feat = cb.forward_predictor_bias(hidden, pred_out)
                gate = int(cb.forward_hw_pred_both(enc_hot_feat[:, t:t + 1, :], pred_feat).squeeze().topk(1).indices.item())
                use_filter = filter_on
            else:
                probe, _ = cb.forward_predictor_bias(hidden, pred_out)
                use_filter = filter_on
                gate = int(cb.forward_hw_pred(hidden, probe).squeeze().topk(1).indices.item()) if filter_on else 1
            if use_filter:
                if not rewinding:
                    if gate == 0:
                        gates.append(0)
                        frame_of_last_zero = t
                    elif gates and gates[-1] == 0:
                        # go back: forget the gate-0 step and its token, resume from its frame with biasing on
                        rewind_until, t, rewinding = t, frame_of_last_zero, True
                        gates.pop(); hyps.pop(); inputs.pop()
                        emitted_in_frame -= 1
                        outs.pop(); caches.pop()
                        pred_out, cache, tok = outs[-1], caches[-1], inputs[-1]
                        continue
                    else:
                        gates.append(1)
                else:
                    gates.append(1)
                    if t >= rewind_until:
                        rewinding = False
            else:
                gates.append(1)
            if both:
                if gates[-1] == 0:
                    pred_out, _ = cb.forward_predictor_bias(hidden_none, raw)
            else:
                # (sic) the 'pred' variant biases with the EMPTY list when the gate is 1, greedy_search.py:145-148
                pred_out, _ = cb.forward_predictor_bias(hidden_none if gates[-1] == 1 else hidden, pred_out)
        enc_step = (enc_hot if gates[-1] == 1 else enc_cold)[:, t:t + 1, :]
        k = int(model.joint(enc_step.contiguous(), pred_out.contiguous()).log_softmax(dim=-1).argmax(dim=-1).squeeze().item())
        if k != model.blank:
            hyps.append(k)
            stepped_last = True
            emitted_in_frame += 1
            tok = torch.tensor([[k]], device=dev)
            cache = new_cache
        if k == model.blank or emitted_in_frame >= n_steps:
            if k == model.blank:
                stepped_last = False
            t += 1
            emitted_in_frame = 0
    lab = labels.squeeze(0) if torch.is_tensor(labels) else labels
    return [hyps], edit_distance(lab.tolist() if torch.is_tensor(lab) else lab, gates), gates


def basic_greedy_search_both(model, encoder_out, encoder_out_lens, context_list=torch.IntTensor([0]),
                             context_lengths=torch.IntTensor([0]), n_steps: int = 64,
                             context_filter_state: str = "off",
                             context_decoder_labels_padded=torch.IntTensor([0])):
    """greedy_search.py:297-430 -> ([hyps], dist).  With a hot-word module of the reference's structure the loop runs
    on the device (hotword.py: gate table, fused predictor biasing, gate / go-back state machine in the update kernel,
    hipGraph replay); WR_HOTWORD_HOST=1 forces the host-driven loop."""
    import os
    from ..hotword import device_capable, greedy_search_both_device, list_fits
    n_ctx = int(context_list.shape[0]) if torch.is_tensor(context_list) and context_list.dim() == 2 else 1
    if (device_capable(model.context_bias) and list_fits(model.context_bias, n_ctx)
            and os.environ.get("WR_HOTWORD_HOST", "0") != "1"):
        hyps, traces = greedy_search_both_device(model, encoder_out, encoder_out_lens, context_list, context_lengths,
                                                 n_steps=n_steps, filter_on=context_filter_state == "on")
        lab = context_decoder_labels_padded
        lab = lab.squeeze(0) if torch.is_tensor(lab) else lab
        return [hyps[0]], edit_distance(lab.tolist() if torch.is_tensor(lab) else lab, traces[0])
    with torch.no_grad():
        h, dist, _ = _hotword_greedy(model, encoder_out, encoder_out_lens, context_list, context_lengths, n_steps,
                                     context_filter_state == "on", context_decoder_labels_padded, both=True)
    return h, dist


def basic_greedy_search_hw(model, encoder_out, encoder_out_lens, context_list=torch.IntTensor([0]),
                           context_lengths=torch.IntTensor([0]), n_steps: int = 64, context_filter_state: str = "off",
                           context_decoder_labels_padded=torch.IntTensor([0])):
    """The fork's `basic_greedy_search` (loss_mode 'pred'), greedy_search.py:34-176 -> ([hyps], dist, gate trace)."""
    with torch.no_grad():
        return _hotword_greedy(model, encoder_out, encoder_out_lens, context_list, context_lengths, n_steps,
                               context_filter_state == "on", context_decoder_labels_padded, both=False)
