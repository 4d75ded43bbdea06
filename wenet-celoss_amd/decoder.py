"""Python owner of a `wr_decoder` handle (include/wr_api.h): packs the predictor /
joiner weights in the reference modules' layouts into `wr_transducer_weights`,
allocates the workspace through torch, and exposes greedy search, prefix beam
search and the predictor step."""
from __future__ import annotations

import ctypes
import os
from typing import List, Tuple

import torch

from . import _lib
from .rnnt_tdt import _durations_arg


def _f32(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t


def _joint_activation_code(joint, default: str = "tanh") -> int:
    """wr_activation of a joiner (or stateless predictor) module: ours carries `act_code`; the reference's modules
    (joint.py:25, predictor.py:237,387) only the instantiated activation under their attribute `activatoin`."""
    code = getattr(joint, "act_code", None)
    if code is not None:
        return int(code)
    act = getattr(joint, "activatoin", None)
    if act is None:
        return _lib.ACTIVATIONS[default]
    by_type = {"Tanh": "tanh", "ReLU": "relu", "Hardtanh": "hardtanh", "SELU": "selu", "SiLU": "swish", "Swish": "swish",
               "GELU": "gelu"}
    name = by_type.get(type(act).__name__)
    if name is None or (name == "gelu" and getattr(act, "approximate", "none") != "none") or \
            (name == "hardtanh" and (act.min_val, act.max_val) != (-1.0, 1.0)):
        raise NotImplementedError(f"wenet_celoss_amd decoding: joiner activation {act!r} is not one of get_activation's")
    return _lib.ACTIVATIONS[name]


class DeviceDecoder:
    """One handle per (predictor, joint) pair and capacity.  Not thread-safe."""

    def __init__(self, predictor, joint, max_lanes: int, max_utt: int, tmax: int, max_hyp: int = 0, max_beam: int = 1):
        lib = _lib.load()
        rnn = getattr(predictor, "rnn", None)
        kind = 0 if rnn is not None else 1 if hasattr(predictor, "pos_embed") else 2 if hasattr(predictor, "conv") else -1
        if kind < 0 or (kind == 0 and not isinstance(rnn, torch.nn.LSTM)):
            raise NotImplementedError("wenet_celoss_amd decoding implements RNNPredictor with an LSTM (the shipped "
                                      "configuration), EmbeddingPredictor and ConvPredictor; got "
                                      f"{type(predictor).__name__}" + (f" / {type(rnn).__name__}" if rnn is not None else ""))
        dev = joint.ffn_out.weight.device
        if joint.enc_ffn is None or joint.pred_ffn is None:
            # prejoin_linear=False (joint.py:30-31 then requires enc == pred == join width): the step kernels multiply by
            # identity weights -- x * 1 + 0 * others is exact in fp32, so the joiner sees enc / pred unchanged
            J = joint.ffn_out.weight.shape[1]
            eye, zero = torch.eye(J, device=dev), torch.zeros(J, device=dev)
            enc_w = pred_w = eye
            enc_b = pred_b = zero
        else:
            enc_w, enc_b = joint.enc_ffn.weight, joint.enc_ffn.bias
            pred_w, pred_b = joint.pred_ffn.weight, joint.pred_ffn.bias
        post = getattr(joint, "post_ffn", None)
        if post is not None:
            # postjoin_linear (joint.py:66-67): post(e + p) = (W e + b) + W p -- a Linear distributes over the sum, so
            # it is folded into the two pre-join projections once (products formed in float64, rounded to fp32 once)
            with torch.no_grad():
                pw64 = post.weight.double()
                enc_b = (pw64 @ enc_b.double() + post.bias.double()).float()
                enc_w = (pw64 @ enc_w.double()).float()
                pred_b = (pw64 @ pred_b.double()).float()
                pred_w = (pw64 @ pred_w.double()).float()
        if dev.type != "cuda":
            raise RuntimeError("wenet_celoss_amd decoding: modules must live on a HIP device (this package has no CPU path)")
        self.device = dev
        self._keep: List[torch.Tensor] = []

        def hold(t):
            t = _f32(t)
            self._keep.append(t)
            return t.data_ptr()

        w = _lib.TransducerWeights()
        w.vocab_size = joint.ffn_out.weight.shape[0]
        w.enc_dim = enc_w.shape[1]
        w.embed_dim = predictor.embed.weight.shape[1]
        w.join_dim = joint.ffn_out.weight.shape[1]
        w.activation = _joint_activation_code(joint)
        w.embed = hold(predictor.embed.weight)
        w.embed_rows = predictor.embed.weight.shape[0]
        w.predictor_type = kind
        if kind == 0:
            w.pred_dim = predictor.projection.weight.shape[0]
            w.hidden = rnn.hidden_size
            w.n_layers = rnn.num_layers
            if rnn.num_layers > 4:
                raise NotImplementedError("at most 4 LSTM layers")
            for l in range(rnn.num_layers):
                w.w_ih[l] = hold(getattr(rnn, f"weight_ih_l{l}"))
                w.w_hh[l] = hold(getattr(rnn, f"weight_hh_l{l}"))
                if rnn.bias:
                    w.b_ih[l] = hold(getattr(rnn, f"bias_ih_l{l}"))
                    w.b_hh[l] = hold(getattr(rnn, f"bias_hh_l{l}"))
                else:                                        # RNNPredictor(bias=False): zero biases
                    w.b_ih[l] = w.b_hh[l] = hold(torch.zeros(4 * rnn.hidden_size, device=dev))
            w.proj_w, w.proj_b = hold(predictor.projection.weight), hold(predictor.projection.bias)
        else:
            # stateless predictors (predictor.py:203-481): the history of context_size - 1 token embeddings takes the
            # place of the LSTM state: that many "layers" of width embed_dim
            ctx = int(predictor.context_size)
            if not 2 <= ctx <= 5:
                raise NotImplementedError(f"history_size must be 1..4 (got {ctx - 1}): the token history travels in the "
                                          "decoder's four state slots")
            w.pred_dim = w.hidden = w.embed_dim
            w.n_layers = ctx - 1
            w.context_size = ctx
            w.pred_activation = _joint_activation_code(predictor, "swish" if kind == 1 else "relu")
            w.ln_eps = float(predictor.norm.eps)
            w.norm_w, w.norm_b = hold(predictor.norm.weight), hold(predictor.norm.bias)
            if kind == 1:
                w.n_head = int(predictor.num_heads)
                w.pos_w = hold(predictor.pos_embed.weight)
                w.ffn_w, w.ffn_b = hold(predictor.ffn.weight), hold(predictor.ffn.bias)
            else:
                w.conv_w = hold(predictor.conv.weight)
                w.conv_b = hold(predictor.conv.bias) if predictor.conv.bias is not None else None
        w.enc_ffn_w, w.enc_ffn_b = hold(enc_w), hold(enc_b)
        w.pred_ffn_w, w.pred_ffn_b = hold(pred_w), hold(pred_b)
        w.out_w, w.out_b = hold(joint.ffn_out.weight), hold(joint.ffn_out.bias)
        self._w = w
        self.dims = dict(V=w.vocab_size, E=w.enc_dim, P=w.pred_dim, D=w.embed_dim, H=w.hidden, L=w.n_layers, J=w.join_dim)
        self.max_lanes, self.max_utt, self.tmax, self.max_hyp, self.max_beam = max_lanes, max_utt, tmax, max_hyp, max_beam
        nbytes = lib.wr_decoder_workspace_bytes(ctypes.byref(w), max_lanes, max_utt, tmax, max_hyp, max_beam)
        if nbytes == 0:
            raise RuntimeError("wr_decoder_workspace_bytes rejected the configuration")
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        handle = ctypes.c_void_p()
        with torch.cuda.device(dev):
            rc = lib.wr_decoder_create(ctypes.byref(w), max_lanes, max_utt, tmax, max_hyp, max_beam, _lib.ptr(self._ws),
                                       nbytes, _lib.current_stream(dev), ctypes.byref(handle))
        _lib.check(rc, "wr_decoder_create")
        self._h = handle
        self._lib = lib
        look = os.environ.get("WR_GREEDY_LOOKAHEAD")      # unset: the library default (adaptive)
        if look is not None:
            self.set_lookahead(int(look))

    def _call(self, name: str, *args) -> None:
        """`_lib.call` on this handle.  A failed search leaves the handle's lane state undefined: mark it so that
        DecoderCache rebuilds it."""
        try:
            _lib.call(name, self._h, *args, device=self.device)
        except RuntimeError:
            self.poisoned = True
            raise

    poisoned = False

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                self._lib.wr_decoder_destroy(h)
            except Exception:
                pass

    def set_graph(self, enable: bool) -> None:
        _lib.check(self._lib.wr_decoder_set_graph(self._h, int(enable)), "wr_decoder_set_graph")

    def set_lookahead(self, frames: int) -> None:
        """Greedy search: encoder frames evaluated per micro-step (1..4, 0 = adaptive); token sequences do not
        depend on it."""
        _lib.check(self._lib.wr_decoder_set_lookahead(self._h, int(frames)), "wr_decoder_set_lookahead")

    def last_counters(self) -> Tuple[int, int, int]:
        """The three counters the last polling search read back (`wr_decoder_last_counters`): greedy searches (lanes
        still active, blank decisions, emissions); TDT prefix beam search (utterances still running, steps taken summed
        over the utterances, hypotheses expanded)."""
        out = (ctypes.c_int32 * 3)()
        _lib.check(self._lib.wr_decoder_last_counters(self._h, out), "wr_decoder_last_counters")
        return tuple(out)

    def _greedy(self, name: str, encoder_out, lens, *args, frames=None):
        """The frame of the greedy searches: `name`(encoder_out (N, T, E) as fp32, lens (N,) int32, N, T, *args, tokens,
        token counts[, frames -- entry points that take that pointer say `frames` True or False]) -> one token list per
        stream; with `frames` also the list of the frames the entry point reported for them."""
        enc = _f32(encoder_out)
        N, T, _ = enc.shape
        lens = lens.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        hyps = torch.empty(N, max(self.max_hyp, 1), dtype=torch.int32, device=self.device)
        fr = torch.empty_like(hyps) if frames else None
        hl = torch.empty(N, dtype=torch.int32, device=self.device)
        self._call(name, enc, lens, N, T, *args, hyps, hl, *(() if frames is None else (fr,)))
        hl_c, hy_c = hl.cpu().tolist(), hyps.cpu()
        if max(hl_c, default=0) > self.max_hyp:
            raise RuntimeError(f"greedy search produced {max(hl_c)} tokens but the decoder was sized for {self.max_hyp}")
        toks = [hy_c[i, :hl_c[i]].tolist() for i in range(N)]
        if not frames:
            return toks
        fr_c = fr.cpu()
        return toks, [fr_c[i, :hl_c[i]].tolist() for i in range(N)]

    def greedy(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, n_steps: int = 64, blank: int = 0
               ) -> List[List[int]]:
        """encoder_out (N, T, E); returns one token list per stream."""
        return self._greedy("wr_greedy_search", encoder_out, encoder_out_lens, int(n_steps), int(blank))

    def greedy_tdt(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, durations, n_steps: int = 64,
                   blank: int = 0, return_frames: bool = False):
        """Greedy search of a token-and-duration model (`wr_greedy_search_tdt`): the joiner's row is its width minus
        len(durations) token logits followed by one logit per duration.  encoder_out (N, T, E) -> one token list per
        stream; with `return_frames` also the frame at which each token was emitted.  `set_graph` and `set_lookahead`
        apply; tokens and frames do not depend on them."""
        return self._greedy("wr_greedy_search_tdt", encoder_out, encoder_out_lens, int(n_steps), int(blank),
                            _durations_arg(durations), len(durations), frames=bool(return_frames))

    def greedy_chunk(self, encoder_chunk: torch.Tensor, chunk_lens: torch.Tensor, n_steps: int = 64, blank: int = 0,
                     reset: bool = False, reference_new_cache: bool = True) -> List[List[int]]:
        """Streaming greedy search: tokens emitted in this chunk for each stream (state carries over)."""
        return self._greedy("wr_greedy_search_chunk", encoder_chunk, chunk_lens, int(n_steps), int(blank), int(reset),
                            int(reference_new_cache))

    def _beam(self, name: str, encoder_out, lens, ctc_logp, beam_size: int, *args) -> List[List[Tuple[List[int], float]]]:
        """The frame of the prefix beam searches: `name`(encoder_out (B, T, E) and ctc_logp (B, T, V) or None as fp32,
        lens (B,) int32, B, T, beam_size, *args, then the n-best buffers) -> per utterance [(hyp, score)] best first."""
        enc = _f32(encoder_out)
        ctc = None if ctc_logp is None else _f32(ctc_logp)
        B, T, _ = enc.shape
        lens = lens.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        lmax = self.tmax + 1
        hyps = torch.empty(B, beam_size, lmax, dtype=torch.int32, device=self.device)
        hl = torch.empty(B, beam_size, dtype=torch.int32, device=self.device)
        sc = torch.empty(B, beam_size, dtype=torch.float64, device=self.device)
        nh = torch.empty(B, dtype=torch.int32, device=self.device)
        self._call(name, enc, lens, ctc, B, T, int(beam_size), *args, hyps, hl, sc, nh)
        hyps, hl, sc, nh = hyps.cpu(), hl.cpu().tolist(), sc.cpu().tolist(), nh.cpu().tolist()
        return [[(hyps[b, e, :hl[b][e]].tolist(), sc[b][e]) for e in range(nh[b])] for b in range(B)]

    def prefix_beam(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, ctc_logp: torch.Tensor,
                    beam_size: int, ctc_weight: float, transducer_weight: float, blank: int = 0
                    ) -> List[List[Tuple[List[int], float]]]:
        """encoder_out (B, T, E), ctc_logp (B, T, V).  Per utterance: [(hyp incl. seed blank, score)] best first."""
        return self._beam("wr_prefix_beam_search", encoder_out, encoder_out_lens, ctc_logp, beam_size, float(ctc_weight),
                          float(transducer_weight), int(blank))

    def prefix_beam_tdt(self, encoder_out: torch.Tensor, encoder_out_lens: torch.Tensor, durations, beam_size: int,
                        blank: int = 0, ctc_logp: torch.Tensor = None, ctc_weight: float = 0.0,
                        transducer_weight: float = 1.0) -> List[List[Tuple[List[int], float]]]:
        """Prefix beam search of a token-and-duration model (`wr_prefix_beam_search_tdt`): the joiner's row is its width
        minus len(durations) token logits followed by one logit per duration.  encoder_out (B, T, E); ctc_logp (B, T, V)
        over the token vocabulary or None (then the weights must be (0, 1)).  Per utterance: [(hyp incl. seed blank,
        score)] best first.  `set_graph` applies; the result does not depend on it."""
        return self._beam("wr_prefix_beam_search_tdt", encoder_out, encoder_out_lens, ctc_logp, beam_size, float(ctc_weight),
                          float(transducer_weight), int(blank), _durations_arg(durations), len(durations))

    def _attach(self, size_query: str, attach: str, n_streams: int, beam: int, max_frames: int):
        """The body of attach_beam_stream / attach_beam_context_stream: size the block with `size_query`, allocate it and
        hand it to the handle with `attach` -> (n_streams, beam, max_frames), what the caller notes as attached."""
        size = (int(n_streams), int(beam), int(max_frames))
        nbytes = getattr(self._lib, size_query)(self._h, *size)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            rc = getattr(self._lib, attach)(self._h, *size, _lib.ptr(ws), nbytes)
        _lib.check(rc, attach)
        self._beam_stream_ws = ws
        return size

    beam_stream = beam_context_stream = None       # the handle holds one form's block at a time

    def attach_beam_stream(self, n_streams: int, beam: int, max_frames: int) -> None:
        """Give the handle the state of `n_streams` streams of `prefix_beam_chunk` (`wr_decoder_attach_beam_stream`): beam
        `beam`, at most `max_frames` encoder frames (chunk widths summed) between two resets of a stream.  Attaching
        again replaces the state and ends every stream."""
        self.beam_stream, self.beam_context_stream = self._attach(
            "wr_decoder_beam_stream_workspace_bytes", "wr_decoder_attach_beam_stream", n_streams, beam, max_frames), None

    def attach_beam_context_stream(self, n_streams: int, beam: int, max_frames: int) -> None:
        """`attach_beam_stream` for the biased streams of `prefix_beam_context_chunk`
        (`wr_decoder_attach_beam_context_stream`).  Attaching one form replaces the other and ends every stream."""
        self.beam_context_stream, self.beam_stream = self._attach(
            "wr_decoder_beam_context_stream_workspace_bytes", "wr_decoder_attach_beam_context_stream", n_streams, beam,
            max_frames), None

    def _beam_chunk(self, name: str, entry: str, attached, encoder_chunk, chunk_lens, beam_size, blank, ctc_logp, ctc_weight,
                    transducer_weight, durations, reset, final, finalize=None, graph=None):
        """The body of prefix_beam_chunk / prefix_beam_context_chunk (`graph` and `finalize` given: the biased one, `name` the
        public method, `entry` its entry point, `attached` what its attach call noted): the masks become the flags, the
        n-best buffers are allocated, the entry point runs and the lists are read back into tuples.  The biased call has a
        third mask, a third list (the tags), two more scores and the graph states."""
        enc = _f32(encoder_chunk)
        ctc = None if ctc_logp is None else _f32(ctc_logp)
        B, T, _ = enc.shape
        biased = graph is not None

        def mask(x):
            return [bool(x)] * B if isinstance(x, (bool, int)) else [bool(v) for v in x]

        rs, fin, fz = mask(reset), mask(final), mask(finalize) if biased else [False] * B
        if len(rs) != B or len(fin) != B or len(fz) != B:
            raise RuntimeError(f"DeviceDecoder.{name}: reset / final{' / finalize' if biased else ''} masks must have one "
                               f"entry per stream ({B})")
        flags = (ctypes.c_int32 * B)(*[int(r) | (int(f) << 1) | (int(z) << 2) for r, f, z in zip(rs, fin, fz)])
        lens = chunk_lens.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        if lens.numel() != B:
            raise RuntimeError(f"DeviceDecoder.{name}: chunk_lens has {lens.numel()} elements for {B} streams")
        cap = attached[2] + 1
        beam_size = int(beam_size)
        hyps = torch.empty(B, beam_size, cap, dtype=torch.int32, device=self.device)
        tm = torch.empty(B, beam_size, cap, dtype=torch.int32, device=self.device)
        hl = torch.empty(B, beam_size, dtype=torch.int32, device=self.device)
        sc = torch.empty(B, beam_size, dtype=torch.float64, device=self.device)
        vs = torch.empty(B, beam_size, dtype=torch.float64, device=self.device)
        nh = torch.empty(B, dtype=torch.int32, device=self.device)
        more = ()
        if biased:
            tg, cs = torch.empty_like(hyps), torch.empty_like(hl)
            ts, cx = torch.empty_like(sc), torch.empty_like(sc)
            more = (*graph.to(self.device), graph.n_states, graph.n_arcs, ts, cx, tg, cs)
        dur = (None, 0) if durations is None else (_durations_arg(durations), len(durations))
        self._call(entry, enc, lens, ctc, B, T, beam_size, float(ctc_weight), float(transducer_weight), int(blank), *dur,
                   flags, hyps, tm, hl, sc, vs, nh, *more)
        hl, sc, vs, nh = hl.cpu().tolist(), sc.cpu().tolist(), vs.cpu().tolist(), nh.cpu().tolist()
        width = max(max(row) for row in hl)
        hyps, tm = hyps[:, :, :width].cpu().tolist(), tm[:, :, :width].cpu().tolist()
        if not biased:
            return [[(hyps[b][e][:hl[b][e]], sc[b][e], vs[b][e], tm[b][e][1:hl[b][e]]) for e in range(nh[b])] for b in range(B)]
        ts, cx, cs, tg = ts.cpu().tolist(), cx.cpu().tolist(), cs.cpu().tolist(), tg[:, :, :width].cpu().tolist()
        return [[(hyps[b][e][:hl[b][e]], sc[b][e], vs[b][e], tm[b][e][1:hl[b][e]], ts[b][e], cx[b][e], tg[b][e][1:hl[b][e]],
                  cs[b][e]) for e in range(nh[b])] for b in range(B)]

    def prefix_beam_chunk(self, encoder_chunk: torch.Tensor, chunk_lens: torch.Tensor, beam_size: int, blank: int = 0,
                          ctc_logp: torch.Tensor = None, ctc_weight: float = 0.0, transducer_weight: float = 1.0,
                          durations=None, reset=False, final=False):
        """The next chunk of every stream of the streaming prefix beam search (`wr_prefix_beam_search_chunk`; the rule is
        in include/wr_api.h, "Streaming transducer prefix beam search").  encoder_chunk (B, T, E) with chunk_lens (B,)
        valid frames each; ctc_logp (B, T, V) of the chunk, or None for a token-and-duration model searched with weights
        (0, 1); `durations` None: a plain model.  `reset` / `final`: a bool for all streams or one per stream -- reset
        the stream before the chunk / the chunk is the stream's last.  Per stream the current n-best, best first:
        [(tokens incl. the seed blank, score, viterbi_score, times)], times[i] the absolute encoder frame at which token
        i + 1 was emitted.  `set_graph` applies; the result does not depend on it."""
        if self.beam_stream is None:
            raise RuntimeError("DeviceDecoder.prefix_beam_chunk: call attach_beam_stream(n_streams, beam, max_frames) first")
        return self._beam_chunk("prefix_beam_chunk", "wr_prefix_beam_search_chunk", self.beam_stream, encoder_chunk,
                                chunk_lens, beam_size, blank, ctc_logp, ctc_weight, transducer_weight, durations, reset, final)

    def prefix_beam_context_chunk(self, encoder_chunk: torch.Tensor, chunk_lens: torch.Tensor, beam_size: int, blank: int,
                                  graph, ctc_logp: torch.Tensor = None, ctc_weight: float = 0.0,
                                  transducer_weight: float = 1.0, durations=None, reset=False, final=False, finalize=False):
        """`prefix_beam_chunk` with context-graph phrase biasing (`wr_prefix_beam_search_context_chunk`; the rule is in
        include/wr_api.h, "Context-graph biasing in the streaming transducer prefix beam search").  `graph` is a
        ContextGraph, the same from a stream's reset to its end.  `reset` / `final` / `finalize`: a bool for all streams or
        one per stream; `finalize` exports the stream as if it ended here (a partial match gives its bonus back and the list
        is sorted again) without changing it.  Per stream the current n-best, best first: [(tokens incl. the seed blank,
        score, viterbi_score, times, trans_score, context_score, tags, context_state)] with score = trans_score +
        context_score and one tag per token after the seed (bit 0: a phrase starts at it, bit 1: a phrase ends at it)."""
        if self.beam_context_stream is None:
            raise RuntimeError("DeviceDecoder.prefix_beam_context_chunk: call attach_beam_context_stream(n_streams, beam, "
                               "max_frames) first")
        return self._beam_chunk("prefix_beam_context_chunk", "wr_prefix_beam_search_context_chunk", self.beam_context_stream,
                                encoder_chunk, chunk_lens, beam_size, blank, ctc_logp, ctc_weight, transducer_weight, durations,
                                reset, final, finalize, graph)

    def predictor_step(self, tokens: torch.Tensor, cache_h: torch.Tensor, cache_c: torch.Tensor):
        """tokens (N,), cache (L, N, H) -> out (N, P), new_h, new_c (L, N, H)."""
        N = tokens.numel()
        tok = tokens.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        ch, cc = _f32(cache_h), _f32(cache_c)
        out = torch.empty(N, self.dims["P"], dtype=torch.float32, device=self.device)
        nh, nc = torch.empty_like(ch), torch.empty_like(cc)
        self._call("wr_predictor_step", tok, ch, cc, N, out, nh, nc)
        return out, nh, nc


def _params(predictor, joint):
    return list(predictor.parameters()) + list(joint.parameters())


def _weights_key(ps):
    return tuple((p.data_ptr(), p._version) for p in ps)


def _fingerprint(ps):
    """Content fingerprint of the weights (L2 norm and plain sum of every parameter, computed on the device):
    `p.data.mul_()`-style edits (EMA, weight averaging) leave data_ptr and _version unchanged, and the handle holds
    re-laid copies of the weights, so identity alone would let it decode with stale weights."""
    with torch.no_grad():
        flat = [p.detach() for p in ps]
        return torch.stack(list(torch._foreach_norm(flat)) + [t.sum(dtype=torch.float32) for t in flat])


class DecoderCache:
    """Keeps a DeviceDecoder alive across calls and rebuilds it when the modules' weights change (identity, version
    counter or -- with `check_content` -- the content fingerprint above) or a call needs more capacity.
    `invalidate()` forces a rebuild.  Copies and pickles of a module that owns a cache get an empty cache (the
    native handle is rebuilt lazily)."""

    def __init__(self, check_content: bool = True):
        self._dec = None
        self._key = None
        self._fp = None
        self._check_content = check_content

    def invalidate(self) -> None:
        self._dec, self._key, self._fp = None, None, None

    def __deepcopy__(self, memo):
        return DecoderCache(self._check_content)

    def __reduce__(self):
        return (DecoderCache, (self._check_content,))

    def discard(self, dec) -> None:
        """Drop `dec` if it is the cached handle (called when a search on it raised: its lane state is undefined)."""
        if self._dec is dec:
            self.invalidate()

    def get(self, predictor, joint, lanes: int, utts: int, tmax: int, max_hyp: int, beam: int) -> DeviceDecoder:
        ps = _params(predictor, joint)
        key = _weights_key(ps)
        d = self._dec
        same = d is not None and key == self._key and not d.poisoned
        fp = None
        if same and self._check_content:
            fp = _fingerprint(ps)
            same = self._fp is not None and self._fp.device == fp.device and torch.equal(fp, self._fp)
        if not same or lanes > d.max_lanes or utts > d.max_utt or tmax > d.tmax or max_hyp > d.max_hyp or beam > d.max_beam:
            grow = (lambda new, old: max(new, old)) if same else (lambda new, old: new)
            caps = (grow(lanes, d.max_lanes if d else 0), grow(utts, d.max_utt if d else 0), grow(tmax, d.tmax if d else 0),
                    grow(max_hyp, d.max_hyp if d else 0), grow(beam, d.max_beam if d else 1))
            self._dec = None            # release the old handle before building the new one
            self._dec = DeviceDecoder(predictor, joint, *caps)
            self._key = key
            self._fp = (fp if fp is not None else _fingerprint(ps)) if self._check_content else None
        return self._dec
