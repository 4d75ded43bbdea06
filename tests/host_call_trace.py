"""Record what the Python host layer asks of the library -- the losses of fused.py, rnnt_loss.py and rnnt_tdt.py, the
searches of `DeviceDecoder`, the loss block of `Transducer` -- on CPU tensors and without the library, and how the public
functions of that layer, the k2-style losses among them, refuse bad calls.

Used twice, like tests/joint_call_trace.py: tests/golden/make_host_calls.py runs it over a checkout of the commit the
fixture is recorded from, tests/test_host_calls_host.py over the working tree; the two records must be identical.

The seams are those of joint_call_trace.py: `_lib.load` returns a recorder (every `*_workspace_bytes` and every
`*_state_bytes` query answers WS_BYTES, everything else 0), `_lib.current_stream` returns None, `torch.cuda.device` is a
null context.  Added here: `torch.Tensor.pin_memory` is the identity, `torch.empty` / `torch.empty_like` are `torch.zeros` / `torch.zeros_like` (so
that read-backs are defined), and the inputs -- and what `torch.empty` allocates, the joiner's logits among it -- are CPU
tensors seen through a `torch.Tensor` subclass whose `is_cuda` is True.  A `DeviceDecoder` is made with `object.__new__`
(its constructor refuses a module that is not on a HIP device), and the search functions get it from a stand-in for
their `DecoderCache` that records the capacities they ask for.

The recorder also plays the library where the host reads results back: the full-lattice forward and the sweeps write
cost_b = 100 * U_b + T_b, so that the order of the costs of a bucketed call can be read off them, and the searches write
token counts, tokens, frames, scores and n-best counts, the streaming searches n-best lists of differing lengths
(`_EFFECTS`).

A record is {"calls": [...], "result" or "raises": ...}.  A call lists the entry point, its scalar arguments in order,
the positions of its null pointers, the contents of its host arrays (the durations), the two length arrays it was given
(`_LENGTHS`: those of a slice or a bucket are built by the host), and the groups of positions that received the same
non-null pointer (a gradient written over the logits shows here).  {"name": "backward"} marks where a
backward pass begins.  "result" is the Python result where it is host data and shape / dtype (with the values of a small
tensor) otherwise; "raises" is [exception type, full message]."""
import contextlib
import ctypes
import itertools
import os
import warnings

import torch

WS_BYTES = 64
ENV = ("WR_FUSED_LSE_EPILOGUE", "WR_FUSED_INPLACE_BYTES", "WR_FUSED_BUCKETS", "WR_RNNT_INPLACE_GRAD", "WR_TDT_HOST",
       "WR_FUSED_LOSS", "WR_FUSED_LOGITS_BUDGET_MB", "WR_JOINT_PRECISION", "WR_AMP_BACKWARD", "WR_GREEDY_LOOKAHEAD")


class _OnDevice(torch.Tensor):
    """A CPU tensor that says it lives on a HIP device."""
    is_cuda = property(lambda self: True)


def dev(t: torch.Tensor) -> torch.Tensor:
    return t.as_subclass(_OnDevice)


def _i32(p, n):
    return (ctypes.c_int32 * n).from_address(p)


def _write_costs(ll, tl, B, costs):
    ll, tl, out = _i32(ll, B), _i32(tl, B), (ctypes.c_float * B).from_address(costs)
    for i in range(B):
        out[i] = 100.0 * tl[i] + ll[i]


def _write_greedy(rec, N, hyps, hl, frames=None):
    width = max(rec.max_hyp, 1)
    for i in range(N):
        _i32(hl, N)[i] = i + 1
        for j in range(width):
            _i32(hyps, N * width)[i * width + j] = 10 * i + j + 1
            if frames:
                _i32(frames, N * width)[i * width + j] = 100 + 10 * i + j
    return 0


def _write_beam(rec, B, beam, hyps, hl, sc, nh):
    lmax = rec.tmax + 1
    for b in range(B):
        _i32(nh, B)[b] = max(beam - b, 1)
        for e in range(beam):
            _i32(hl, B * beam)[b * beam + e] = min(e + 1, lmax)
            (ctypes.c_double * (B * beam)).from_address(sc)[b * beam + e] = -(10 * b + e) - 0.5
            for j in range(lmax):
                _i32(hyps, B * beam * lmax)[(b * beam + e) * lmax + j] = 100 * b + 10 * e + j


def _write_nbest(B, beam, width, hl, nh, lists=(), scores=(), entries=(), streams=()):
    """The n-best lists of a streaming search, of differing lengths: stream b has max(beam - b, 1) hypotheses, hypothesis e
    min(e + 1, width) tokens.  `lists` are int32 [B][beam][width], `scores` double [B][beam], `entries` int32 [B][beam],
    `streams` int32 [B]; every array gets values of its own."""
    for b in range(B):
        _i32(nh, B)[b] = max(beam - b, 1)
        for k, p in enumerate(streams):
            _i32(p, B)[b] = 7 + b + k
        for e in range(beam):
            i = b * beam + e
            _i32(hl, B * beam)[i] = min(e + 1, width)
            for k, p in enumerate(scores):
                (ctypes.c_double * (B * beam)).from_address(p)[i] = -(10 * b + e) - 0.5 - 0.125 * k
            for k, p in enumerate(entries):
                _i32(p, B * beam)[i] = 1000 * (k + 1) + 10 * b + e
            for k, p in enumerate(lists):
                for j in range(width):
                    _i32(p, B * beam * width)[i * width + j] = 1000 * k + 100 * b + 10 * e + j


# entry point -> what the recorder writes through the pointers it was given (arguments as the library receives them)
_EFFECTS = {
    "wr_rnnt_loss_fwd": lambda r, a: _write_costs(a[3], a[4], a[5], a[10]),
    "wr_rnnt_loss_sweeps": lambda r, a: _write_costs(a[0], a[1], a[2], a[5]),
    "wr_greedy_search": lambda r, a: _write_greedy(r, a[3], a[7], a[8]),
    "wr_greedy_search_tdt": lambda r, a: _write_greedy(r, a[3], a[9], a[10], a[11]),
    "wr_greedy_search_chunk": lambda r, a: _write_greedy(r, a[3], a[9], a[10]),
    "wr_prefix_beam_search": lambda r, a: _write_beam(r, a[4], a[6], a[10], a[11], a[12], a[13]),
    "wr_prefix_beam_search_tdt": lambda r, a: _write_beam(r, a[4], a[6], a[12], a[13], a[14], a[15]),
    # the streaming searches (the transducer's lists are max_frames + 1 wide; the cases attach max_frames = tmax)
    "wr_ctc_prefix_beam_search_chunk": lambda r, a: _write_nbest(
        a[2], a[5], a[9], a[13], a[17], lists=(a[12], a[16]), scores=(a[14], a[15]), streams=(a[18],)),
    "wr_ctc_prefix_beam_search_context_chunk": lambda r, a: _write_nbest(
        a[2], a[5], a[9], a[22], a[26], lists=(a[21], a[25], a[30]), scores=(a[23], a[24], a[28], a[29]), entries=(a[31],),
        streams=(a[27],)),
    "wr_prefix_beam_search_chunk": lambda r, a: _write_nbest(
        a[4], a[6], r.tmax + 1, a[15], a[18], lists=(a[13], a[14]), scores=(a[16], a[17])),
    "wr_prefix_beam_search_context_chunk": lambda r, a: _write_nbest(
        a[4], a[6], r.tmax + 1, a[15], a[18], lists=(a[13], a[14], a[29]), scores=(a[16], a[17], a[27], a[28]),
        entries=(a[30],)),
}


# entry point -> positions of (logit lengths, target lengths, B): the lengths are read back into the record, so that the
# per-slice and per-bucket length arrays the host builds are part of it
_LENGTHS = {"wr_rnnt_loss_fwd": (3, 4, 5), "wr_rnnt_loss_bwd": (3, 4, 5), "wr_rnnt_loss_sweeps": (0, 1, 2),
            "wr_rnnt_lattice_sweeps": (0, 1, 2), "wr_rnnt_tdt_sweeps": (0, 1, 2), "wr_joint_fwd": (4, 5, 6),
            "wr_joint_fwd_lse": (4, 5, 7), "wr_joint_rnnt_stats": (4, 5, 7), "wr_joint_tdt_stats": (4, 5, 7),
            "wr_joint_rnnt_grad": (4, 5, 7), "wr_joint_rnnt_grad_lattice": (4, 5, 7), "wr_joint_tdt_grad": (4, 5, 7),
            "wr_joint_bwd_dz": (4, 5, 6)}


class Recorder:
    def __init__(self, signatures, max_hyp=0, tmax=0):
        self.signatures, self.calls, self.max_hyp, self.tmax = signatures, [], max_hyp, tmax

    def __getattr__(self, name):
        if name not in self.signatures:
            raise AttributeError(name)
        argtypes = self.signatures[name][1]

        def fn(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)}"
            scalars, null, arrays, at, plain = [], [], {}, {}, []
            for i, (a, ty) in enumerate(zip(args, argtypes)):
                if ty is not ctypes.c_void_p:
                    scalars.append(a)
                    plain.append(a)
                    continue
                if isinstance(a, ctypes.Array):
                    arrays[str(i)] = list(a)
                    plain.append(a)
                    continue
                a = a.value if isinstance(a, ctypes.c_void_p) else a
                plain.append(a)
                if not a:
                    null.append(i)
                else:
                    at.setdefault(a, []).append(i)
            rec = {"name": name, "scalars": scalars, "null": null}
            if arrays:
                rec["arrays"] = arrays
            same = [v for v in at.values() if len(v) > 1]
            if same:
                rec["same"] = same
            if name in _LENGTHS:
                ll, tl, n = (plain[i] for i in _LENGTHS[name])
                rec["lengths"] = [list(_i32(p, n)) if p else None for p in (ll, tl)]
            self.calls.append(rec)
            if name in _EFFECTS:
                _EFFECTS[name](self, plain)
            return WS_BYTES if name.endswith(("_workspace_bytes", "_state_bytes")) else 0
        return fn


class _NullDevice(contextlib.nullcontext):
    def __init__(self, device=None):
        super().__init__()


@contextlib.contextmanager
def seams(pkg, recorder):
    """The replacements listed in the module docstring, and the package's environment switches unset; undone on exit."""
    lib = pkg._lib
    saved = [(lib, "load", lib.load), (lib, "current_stream", lib.current_stream), (torch.cuda, "device", torch.cuda.device),
             (torch.Tensor, "pin_memory", torch.Tensor.pin_memory), (torch, "empty", torch.empty),
             (torch, "empty_like", torch.empty_like)]
    env = {k: os.environ.pop(k) for k in ENV if k in os.environ}
    try:
        lib.load = lambda: recorder
        lib.current_stream = lambda device=None: None
        torch.cuda.device = _NullDevice
        torch.Tensor.pin_memory = lambda self, *a, **k: self
        zeros, zeros_like = torch.zeros, torch.zeros_like
        torch.empty = lambda *a, **k: dev(zeros(*a, **k))
        torch.empty_like = lambda *a, **k: dev(zeros_like(*a, **k))
        yield
    finally:
        for obj, name, value in saved:
            setattr(obj, name, value)
        for k in ENV:
            os.environ.pop(k, None)
        os.environ.update(env)


def plain(x):
    """A result as the fixture keeps it."""
    if isinstance(x, torch.Tensor):
        out = {"shape": list(x.shape), "dtype": str(x.dtype)}
        if x.numel() <= 64:
            out["values"] = x.detach().to(torch.float64).reshape(-1).tolist()
        return out
    if isinstance(x, (list, tuple)):
        return [plain(v) for v in x]
    if hasattr(x, "hyp") and hasattr(x, "score"):                     # search.prefix_beam_search.Sequence
        return {"hyp": plain(x.hyp), "score": x.score, "cache": x.cache}
    assert x is None or isinstance(x, (bool, int, float, str)), type(x)
    return x


# ---------------------------------------------------------------------------------------------------- the cases --
B, T, U1, J, V = 3, 5, 3, 8, 28
T_LENS, U_LENS = [5, 3, 0], [2, 1, 0]
BUDGETS = {"rows2": lambda width: 2 * U1 * width * 4, "utterance": lambda width: T * U1 * width * 4,
           "unbounded": lambda width: 1 << 40}


def _i(values):
    return dev(torch.tensor(values, dtype=torch.int32))


def _joiner_inputs(width, need_w, batch=B, frames=T, labels1=U1, t_lens=T_LENS, u_lens=U_LENS):
    ep = dev(torch.zeros(batch, frames, J)).requires_grad_()
    pp = dev(torch.zeros(batch, labels1, J)).requires_grad_()
    w = dev(torch.zeros(width, J)).requires_grad_(need_w)
    b = dev(torch.zeros(width)).requires_grad_(need_w)
    return [ep, pp, w, b], (dev(torch.ones(batch, labels1 - 1, dtype=torch.int32)), _i(t_lens), _i(u_lens))


def _grads(calls, loss, leaves, times=1):
    """Run `times` backward passes of `loss`; the result is the loss and which leaves got a gradient of which shape."""
    for k in range(times):
        calls.append({"name": "backward"})
        loss.sum().backward(retain_graph=k + 1 < times)
    return {"loss": plain(loss), "grads": [None if x.grad is None else list(x.grad.shape) for x in leaves]}


def _joint_rnnt(pkg, rec, need_w=True, env=None, times=1, **kw):
    os.environ.update(env or {})
    leaves, rest = _joiner_inputs(V, need_w)
    loss = pkg.joint_rnnt_loss(*leaves, *rest, blank=0, reduction="none", buckets=1, **kw)
    return _grads(rec.calls, loss, leaves, times)


def _joint_tdt(pkg, rec, durations, need_w=True, **kw):
    leaves, rest = _joiner_inputs(V + len(durations), need_w)
    loss = pkg.joint_rnnt_tdt_loss(*leaves, *rest, durations, blank=0, reduction="none", **kw)
    return _grads(rec.calls, loss, leaves)


# a ragged batch that plan_buckets cuts into groups: 8 utterances, 22720 lattice cells, every length different
BUCKET_T, BUCKET_U = [40, 33, 39, 32, 38, 31, 37, 30], [70, 5, 69, 4, 68, 3, 67, 6]


def _bucketed(pkg, rec, **kw):
    groups = pkg.fused.plan_buckets(BUCKET_T, BUCKET_U, max_buckets=4)
    assert groups is not None and len(groups) >= 2, groups
    leaves, rest = _joiner_inputs(V, True, len(BUCKET_T), max(BUCKET_T), max(BUCKET_U) + 1, BUCKET_T, BUCKET_U)
    loss = pkg.joint_rnnt_loss(*leaves, *rest, blank=0, reduction="none", precision="fp32", **kw)
    return _grads(rec.calls, loss, leaves)


LB, LT, LU1, LV = 2, 4, 3, 6
L_T, L_U = [4, 2], [2, 1]


def _logits(width, dtype, grad=True):
    x = dev(torch.zeros(LB, LT, LU1, width, dtype=dtype)).requires_grad_(grad)
    return x, (dev(torch.ones(LB, LU1 - 1, dtype=torch.int32)), _i(L_T), _i(L_U))


def _rnnt_loss(pkg, rec, dtype, **kw):
    x, rest = _logits(LV, dtype)
    return _grads(rec.calls, pkg.rnnt_loss(x, *rest, blank=0, reduction="none", **kw), [x])


def _tdt_loss(pkg, rec, dtype, durations, **kw):
    x, rest = _logits(LV + len(durations), dtype)
    return _grads(rec.calls, pkg.rnnt_tdt_loss(x, *rest, durations, blank=0, reduction="none", **kw), [x])


def _tdt_align(pkg, rec, dtype, durations, **kw):
    x, rest = _logits(LV + len(durations), dtype, grad=False)
    return plain(pkg.rnnt_tdt_forced_align(x, *rest, durations, **kw))


DN, DT, DE, DV, BEAM = 2, 6, 4, 5, 3


def decoder(pkg, rec):
    """A DeviceDecoder over the recorder: built without its constructor, which needs modules on a HIP device."""
    d = object.__new__(pkg.decoder.DeviceDecoder)
    d.device, d._h, d.max_hyp, d.tmax, d._lib = torch.device("cpu"), ctypes.c_void_p(1), rec.max_hyp, rec.tmax, rec
    return d


def _decode(pkg, rec, method, *args, ctc=None, **kw):
    d = decoder(pkg, rec)
    try:
        enc, lens = dev(torch.zeros(DN, DT, DE)), torch.tensor([6, 4])
        if ctc is not None:
            kw["ctc_logp"] = dev(torch.zeros(DN, DT, DV)) if ctc else None
        return plain(getattr(d, method)(enc, lens, *args, **kw))
    finally:
        d._h = None


class _Cache:
    """Stands for a DecoderCache: records the capacities a search asks for and hands out `decoder(pkg, rec)`."""

    def __init__(self, pkg, rec):
        self.rec, self.dec = rec, decoder(pkg, rec)

    def get(self, predictor, joint, **capacities):
        self.rec.calls.append({"name": "DecoderCache.get", "capacities": capacities})
        return self.dec

    def discard(self, dec):
        self.rec.calls.append({"name": "DecoderCache.discard"})


def _search(pkg, rec, what, lens, **kw):
    """The functions of search/ and `Transducer.forward_greedy_search` over a `_Cache`."""
    import types
    cache = _Cache(pkg, rec)
    ctc = types.SimpleNamespace(log_softmax=lambda x: dev(torch.zeros(DN, DT, DV)))
    owner = types.SimpleNamespace(blank=1, predictor=None, joint=None, ctc=ctc, tdt_durations=(0, 1, 2), _decoder_cache=cache)
    enc = dev(torch.zeros(DN, DT, DE))
    try:
        if what == "forward_greedy_search":
            m = model(pkg)
            m._decoder_cache = cache
            m.reset_cache(DN, chunk_frames=8, n_steps=4)
            return [plain(m.forward_greedy_search(enc, lens, n_steps=4)), plain(m.forward_greedy_search(enc, lens, n_steps=4))]
        if what == "search_encoded":
            bs = pkg.PrefixBeamSearch(None, None, None, ctc, 1)
            bs._decoder_cache = cache
            return plain(bs.search_encoded(enc, lens, BEAM, **kw))
        return plain(getattr(pkg, what)(owner, enc, lens, **kw))
    finally:
        cache.dec._h = None


class _Enc(torch.nn.Module):
    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)

    def output_size(self):
        return self.proj.out_features

    def forward(self, speech, speech_lengths, decoding_chunk_size=-1, num_decoding_left_chunks=-1):
        mask = torch.arange(speech.shape[1])[None, None, :] < torch.as_tensor(speech_lengths).reshape(-1, 1, 1)
        return dev(self.proj(speech)), mask


def model(pkg, joint_outputs=23, **kw):
    """The tiny model of tests/test_rnnt_tdt_host.py (`_model`)."""
    torch.manual_seed(0)
    return pkg.Transducer(23, 0, _Enc(8, 12), pkg.RNNPredictor(23, 10, 10, 0.0, 14, 2, dropout=0.0),
                          pkg.TransducerJoint(joint_outputs, 12, 10, 16), ctc_weight=0.0, transducer_weight=1.0, **kw)


def _loss_block(pkg, rec, tdt, budget, fused=True):
    m = model(pkg, 26, tdt_durations=(0, 1, 2), tdt_sigma=0.05) if tdt else model(pkg)
    m.logits_budget, m.fused_loss = budget, fused
    enc, pred = dev(torch.zeros(2, 4, 12)), dev(torch.zeros(2, 3, 10))
    text = dev(torch.tensor([[3, 4], [5, -1]]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits, loss = m.compute_loss(enc, _i([4, 3]), pred, text, dev(torch.tensor([2, 1])))
    return {"logits": plain(logits), "loss": plain(loss)}


def _score(pkg, rec, tdt, fused=True):
    m = model(pkg, 26, tdt_durations=(0, 1, 2), tdt_sigma=0.05) if tdt else model(pkg)
    m.fused_loss = fused
    enc, mask = dev(torch.zeros(2, 4, 12)), dev(torch.ones(2, 1, 4, dtype=torch.bool))
    hyps_pad, hyps_lens = dev(torch.tensor([[3, 4], [5, -1]])), dev(torch.tensor([2, 1]))
    with torch.no_grad():
        fn = m._cal_tdt_score if tdt else m._cal_transducer_score
        return plain(fn(enc, mask, hyps_lens, hyps_pad))


# --------------------------------------------------------- the streaming searches, plain and context-biased --
PHRASES = ((2, 3), (3, 4, 2), (2,))             # one phrase a proper prefix of another; tokens inside DV and 23


def _graph(pkg, blank=1, phrases=PHRASES):
    return pkg.ContextGraph(phrases, 2.0, blank=blank)


def _beam_stream(pkg, rec, ctx, chunks, attach=("own",), beam=BEAM):
    """`DeviceDecoder`'s streaming prefix beam search: the attach calls of `attach` ("own": the form `ctx` says, "other":
    its twin), then one chunk call per entry of `chunks` (its keywords; `streams`, `lens` and `ctc` shape the inputs)."""
    d = decoder(pkg, rec)
    try:
        for which in attach:
            biased = bool(ctx) == (which == "own")
            (d.attach_beam_context_stream if biased else d.attach_beam_stream)(DN, beam, rec.tmax)
        out = [plain([d.beam_stream, d.beam_context_stream])]
        for kw in chunks:
            kw = dict(kw)
            n, lens = kw.pop("streams", DN), kw.pop("lens", torch.tensor([3, 2]))
            if kw.pop("ctc", False):
                kw["ctc_logp"] = dev(torch.zeros(n, 3, DV))
            enc = dev(torch.zeros(n, 3, DE))
            if ctx:
                out.append(plain(d.prefix_beam_context_chunk(enc, lens, beam, 1, _graph(pkg), **kw)))
            else:
                out.append(plain(d.prefix_beam_chunk(enc, lens, beam, 1, **kw)))
        return out
    finally:
        d._h = None


def _ctc_stream(pkg, rec, ctx, chunks, state=None, graph=None, blank=0, streams=DN, beam=BEAM, max_frames=8, vocab=DV,
                on_device=True, then=()):
    """A `CtcPrefixBeamStream` / `CtcContextPrefixBeamStream` (`ctx`) over chunks of the widths `chunks` (a pair: width and
    the keywords of `search`); `state`: the bytes of a lent state tensor, or a tensor.  `then`: "finalize", "reset" and
    further chunks, in order.  The result lists what every call returned and, after each, `frames` / `context_states`."""
    if isinstance(state, int):
        state = dev(torch.zeros(state, dtype=torch.uint8))
    if ctx:
        s = pkg.CtcContextPrefixBeamStream(streams, beam, max_frames, _graph(pkg, blank) if graph is None else graph,
                                           blank=blank, state=state)
    else:
        s = pkg.CtcPrefixBeamStream(streams, beam, max_frames, blank=blank, state=state)
    out = []
    for step in tuple(chunks) + tuple(then):
        if step == "reset":
            s.reset()
        elif step == "finalize":
            out.append(plain(s.finalize()))
        else:
            width, kw = step if isinstance(step, tuple) else (step, {})
            kw = dict(kw)
            x = torch.zeros(kw.pop("shape", (kw.pop("streams", DN), width, kw.pop("vocab", vocab))))
            lens = kw.pop("lens", torch.tensor([width, width - 1]))
            out.append(plain(s.search(x if kw.pop("cpu", not on_device) else dev(x), lens, **kw)))
        out.append(plain([s.frames, getattr(s, "context_states", None)]))
    return out


def _asr(pkg, tdt=False, **kw):
    """`model` with a CTC head, for the decode modes that run the encoder."""
    m = model(pkg, 26, tdt_durations=(0, 1, 2), **kw) if tdt else model(pkg, **kw)
    m.ctc = pkg.CTC(23, 12)
    return m


def _decode_mode(pkg, rec, method, *args, tdt=False, blank=0, **kw):
    """A decode mode of `Transducer` from the speech on: the encoder, then the search."""
    m = _asr(pkg, tdt)
    m.blank = blank
    cache = m._decoder_cache = _Cache(pkg, rec)
    try:
        with torch.no_grad():
            return plain(getattr(m, method)(dev(torch.zeros(DN, DT, 8)), torch.tensor([6, 4]), *args, **kw))
    finally:
        cache.dec._h = None


def _model_streams(pkg, rec, what, tdt=False):
    """The streaming methods of `Transducer`: a reset, then two chunks."""
    m = _asr(pkg, tdt)
    m.blank = 1
    cache = m._decoder_cache = _Cache(pkg, rec)
    enc, lens = dev(torch.zeros(DN, 3, 12)), torch.tensor([3, 2])
    try:
        with torch.no_grad():
            if what == "ctc":
                m.reset_ctc_stream(DN, BEAM, 8)
                return [plain(m.forward_ctc_prefix_beam_search(enc, lens)) for _ in range(2)]
            if what == "ctc context":
                m.reset_ctc_context_stream(DN, BEAM, 8, _graph(pkg, 0))
                return [plain(m.forward_ctc_context_prefix_beam_search(enc, lens, finalize=f)) for f in (False, True)]
            if what == "beam":
                m.reset_beam_stream(DN, BEAM, rec.tmax, 3)
                return [plain(m.forward_prefix_beam_search(enc, lens, final=f)) for f in (False, [True, False])]
            m.reset_beam_context_stream(DN, BEAM, rec.tmax, 3, _graph(pkg))
            return [plain(m.forward_context_prefix_beam_search(enc, lens, **kw))
                    for kw in (dict(finalize=[False, True]), dict(final=[True, False]))]
    finally:
        cache.dec._h = None


def _stream_refusals(pkg, out):
    """The errors the streaming wrappers raise on their own, before or without the library."""
    z = torch.zeros
    for ctx, name in ((False, "CtcPrefixBeamStream"), (True, "CtcContextPrefixBeamStream")):
        def ctc(chunks, ctx=ctx, **kw):
            return lambda rec: _ctc_stream(pkg, rec, ctx, chunks, **kw)
        out[f"{name} beam 17"] = ctc((), beam=17)
        out[f"{name} no stream"] = ctc((), streams=0)
        out[f"{name} max_frames 0"] = ctc((), max_frames=0)
        out[f"{name} chunk rank"] = ctc(((2, dict(shape=(DN, DV))),))
        out[f"{name} wrong stream count"] = ctc(((2, dict(streams=3, lens=torch.tensor([2, 2, 2]))),))
        out[f"{name} vocabulary change"] = ctc((2, (2, dict(vocab=DV + 1))))
        out[f"{name} capacity"] = ctc((5, 4))
        out[f"{name} capacity after reset"] = ctc((5, "reset", 5, 4))
        out[f"{name} cpu"] = ctc((2,), on_device=False)
        out[f"{name} state too small"] = ctc((2,), state=WS_BYTES - 1)
        out[f"{name} state dtype"] = ctc((2,), state=dev(z(WS_BYTES, dtype=torch.int8)))
        out[f"{name} lens length"] = ctc(((2, dict(lens=torch.tensor([2, 2, 2]))),))
        out[f"{name} order: stream count before vocabulary before capacity"] = ctc(
            (2, (7, dict(streams=3, vocab=DV + 1))))
        out[f"{name} order: vocabulary before capacity before cpu"] = ctc((2, (7, dict(vocab=DV + 1, cpu=True))))
        out[f"{name} order: state before lens"] = ctc(((2, dict(lens=torch.tensor([2]))),), state=1)
    cctx = lambda chunks, **kw: (lambda rec: _ctc_stream(pkg, rec, True, chunks, **kw))                    # noqa: E731
    out["CtcContextPrefixBeamStream graph type"] = cctx((), graph=[[2, 3]])
    out["CtcContextPrefixBeamStream graph blank"] = cctx((), graph=_graph(pkg, 1))
    out["CtcContextPrefixBeamStream order: sizes before graph"] = cctx((), graph="phrases", beam=0)
    out["CtcContextPrefixBeamStream finalize() before a search"] = cctx(("finalize",))
    out["CtcContextPrefixBeamStream finalize() before a search, after a reset"] = cctx(("reset", "finalize"))
    out["ctc_prefix_beam_search_times cpu"] = lambda rec: pkg.ctc_prefix_beam_search_times(
        z(DN, DT, DV), torch.tensor([6, 4]), BEAM)
    out["ctc_context_prefix_beam_search cpu"] = lambda rec: pkg.ctc_context_prefix_beam_search(
        z(DN, DT, DV), torch.tensor([6, 4]), BEAM, _graph(pkg, 0))
    out["ctc_context_prefix_beam_search graph type"] = lambda rec: pkg.ctc_context_prefix_beam_search(
        dev(z(DN, DT, DV)), torch.tensor([6, 4]), BEAM, None)
    out["ctc_prefix_beam_search_times beam 17"] = lambda rec: pkg.ctc_prefix_beam_search_times(
        dev(z(DN, DT, DV)), torch.tensor([6, 4]), 17)
    # DeviceDecoder
    for ctx, name in ((False, "prefix_beam_chunk"), (True, "prefix_beam_context_chunk")):
        def dec(chunks, ctx=ctx, **kw):
            return lambda rec: _beam_stream(pkg, rec, ctx, chunks, **kw)
        out[f"DeviceDecoder.{name} not attached"] = dec(({},), attach=())
        out[f"DeviceDecoder.{name} the other form attached"] = dec(({},), attach=("other",))
        out[f"DeviceDecoder.{name} the other form attached last"] = dec(({},), attach=("own", "other"))
        out[f"DeviceDecoder.{name} reset mask length"] = dec((dict(reset=[True]),))
        out[f"DeviceDecoder.{name} final mask length"] = dec((dict(final=[True, False, True]),))
        out[f"DeviceDecoder.{name} lens length"] = dec((dict(reset=True, lens=torch.tensor([3, 2, 1])),))
        out[f"DeviceDecoder.{name} order: mask before lens"] = dec((dict(reset=[True], lens=torch.tensor([3])),))
    out["DeviceDecoder.prefix_beam_context_chunk finalize mask length"] = lambda rec: _beam_stream(
        pkg, rec, True, (dict(finalize=[True]),))
    # the stream classes of search/prefix_beam_search.py and the Transducer methods that need a reset first
    for ctx, name in ((False, "TransducerPrefixBeamStream"), (True, "TransducerContextPrefixBeamStream")):
        def stream(ctx=ctx, model_kw=None, graph=None, blank=1, **kw):
            m = _asr(pkg, **(model_kw or {}))
            m.blank = blank
            if ctx:
                return pkg.TransducerContextPrefixBeamStream(m, context_graph=_graph(pkg) if graph is None else graph, **kw)
            return pkg.TransducerPrefixBeamStream(m, **kw)

        def run(steps, stream=stream, ctx=ctx, **kw):
            def fn(rec):
                s = stream(**dict(dict(n_streams=DN, beam_size=BEAM, max_frames=rec.tmax, chunk_frames=3), **kw))
                cache = s.model._decoder_cache = _Cache(pkg, rec)
                try:
                    return [plain(s.search(dev(z(*shape)), lens, **skw)) for shape, lens, skw in steps]
                finally:
                    cache.dec._h = None
            return fn
        chunk, lens = (DN, 3, 12), torch.tensor([3, 2])
        out[f"{name} beam 17"] = run((), beam_size=17)
        out[f"{name} chunk_frames 0"] = run((), chunk_frames=0)
        out[f"{name} chunk rank"] = run((((DN, 12), lens, {}),))
        out[f"{name} wrong stream count"] = run((((3, 3, 12), lens, {}),))
        out[f"{name} chunk wider than chunk_frames"] = run((((DN, 4, 12), lens, {}),))
        out[f"{name} final length"] = run(((chunk, lens, dict(final=[True])),))
        out[f"{name} lens length"] = run(((chunk, torch.tensor([3, 2, 1]), {}),))
        out[f"{name} fed after final"] = run(((chunk, lens, dict(final=[True, False])), (chunk, lens, {})))
        out[f"{name} final again after final"] = run(((chunk, lens, dict(final=True)),
                                                     (chunk, torch.tensor([0, 0]), dict(final=[False, True]))))
        out[f"{name} capacity"] = run(((chunk, lens, {}), (chunk, lens, {}), (chunk, lens, {})))
        out[f"{name} cpu"] = lambda rec, stream=stream: stream(n_streams=DN, beam_size=BEAM, max_frames=6).search(
            z(*chunk), lens)
    tctx = lambda **kw: (lambda rec: pkg.TransducerContextPrefixBeamStream(                               # noqa: E731
        _asr(pkg), DN, BEAM, 6, 3, **kw))
    out["TransducerContextPrefixBeamStream graph type"] = tctx(context_graph=[[2, 3]])
    out["TransducerContextPrefixBeamStream no graph"] = tctx()
    out["TransducerContextPrefixBeamStream graph blank"] = tctx(context_graph=_graph(pkg, 1))
    out["TransducerContextPrefixBeamStream phrase token outside the vocabulary"] = tctx(
        context_graph=_graph(pkg, 0, ((2, 3), (23,))))
    out["TransducerContextPrefixBeamStream order: sizes before graph"] = lambda rec: pkg.TransducerContextPrefixBeamStream(
        _asr(pkg), DN, 17, 6, 3, None)

    def finalize_length(rec):
        s = pkg.TransducerContextPrefixBeamStream(_asr(pkg), DN, BEAM, 6, 3, _graph(pkg, 0))
        return s.search(dev(z(DN, 3, 12)), torch.tensor([3, 2]), finalize=[True])
    out["TransducerContextPrefixBeamStream finalize length"] = finalize_length
    out["Transducer.forward_context_prefix_beam_search before a reset"] = lambda rec: _asr(
        pkg).forward_context_prefix_beam_search(dev(z(DN, 3, 12)), torch.tensor([3, 2]))
    out["Transducer.forward_ctc_context_prefix_beam_search before a reset"] = lambda rec: _asr(
        pkg).forward_ctc_context_prefix_beam_search(dev(z(DN, 3, 12)), torch.tensor([3, 2]))


def _stream_cases(pkg, add):
    sized = dict(max_hyp=8, tmax=DT)
    # DeviceDecoder: attach, then three chunks -- scalar masks, per-stream masks, the last chunk
    for ctx, durations, ctc in itertools.product((False, True), (None, (0, 1, 2)), (False, True)):
        weights = dict(ctc=True, ctc_weight=0.3, transducer_weight=0.7) if ctc else {}
        last = dict(finalize=True) if ctx else {}
        mixed = dict(finalize=[False, True]) if ctx else {}
        chunks = (dict(reset=True, durations=durations, **weights),
                  dict(reset=[False, True], final=[True, False], durations=durations, **weights, **mixed),
                  dict(final=True, reset=0, durations=durations, **weights, **last))
        add(f"DeviceDecoder streaming prefix beam context={int(bool(ctx))} durations={durations} ctc={int(bool(ctc))}",
            lambda rec, a=(ctx, chunks): _beam_stream(pkg, rec, a[0], a[1]), **sized)
    for ctx in (False, True):
        add(f"DeviceDecoder streaming prefix beam context={int(bool(ctx))} attached after the other form",
            lambda rec, c=ctx: _beam_stream(pkg, rec, c, (dict(reset=True, ctc=True),), attach=("other", "own")), **sized)
        add(f"DeviceDecoder streaming prefix beam context={int(bool(ctx))} beam 1",
            lambda rec, c=ctx: _beam_stream(pkg, rec, c, (dict(reset=True, ctc=True),), beam=1), **sized)
    # the CTC streams: a state tensor of their own or a lent one, two chunks, a reset, a third
    for ctx, lent in itertools.product((False, True), (False, True)):
        fz = (lambda f: dict(finalize=f)) if ctx else (lambda f: {})
        add(f"Ctc{'Context' if ctx else ''}PrefixBeamStream lent={int(bool(lent))}",
            lambda rec, a=(ctx, lent, fz): _ctc_stream(
                pkg, rec, a[0], ((2, a[2](False)), (3, a[2](True))), state=WS_BYTES + 8 if a[1] else None,
                then=(("finalize",) if a[0] else ()) + ("reset", (1, dict(lens=torch.tensor([0, 1]))))))
    add("CtcContextPrefixBeamStream finalize at capacity",
        lambda rec: _ctc_stream(pkg, rec, True, (8,), then=("finalize",)))
    add("CtcContextPrefixBeamStream blank=1 empty graph",
        lambda rec: _ctc_stream(pkg, rec, True, (2,), blank=1, graph=_graph(pkg, 1, ())))
    add("CtcPrefixBeamStream blank=1 beam 1", lambda rec: _ctc_stream(pkg, rec, False, (2,), blank=1, beam=1))
    for blank in (0, 1):
        add(f"ctc_prefix_beam_search_times blank={blank}", lambda rec, b=blank: plain(pkg.ctc_prefix_beam_search_times(
            dev(torch.zeros(DN, DT, DV)), torch.tensor([6, 4]), BEAM, blank=b)))
        add(f"ctc_context_prefix_beam_search blank={blank}", lambda rec, b=blank: plain(pkg.ctc_context_prefix_beam_search(
            dev(torch.zeros(DN, DT, DV)), torch.tensor([6, 4]), BEAM, _graph(pkg, b), blank=b)))
    # Transducer: the decode modes from the speech on, and the streaming methods
    add("Transducer.ctc_greedy_search", lambda rec: _decode_mode(pkg, rec, "ctc_greedy_search"), **sized)
    add("Transducer.ctc_greedy_search chunked", lambda rec: _decode_mode(pkg, rec, "ctc_greedy_search", 4, 2), **sized)
    add("Transducer.ctc_prefix_beam_search_times", lambda rec: _decode_mode(pkg, rec, "ctc_prefix_beam_search_times", BEAM),
        **sized)
    add("Transducer.ctc_context_prefix_beam_search",
        lambda rec: _decode_mode(pkg, rec, "ctc_context_prefix_beam_search", BEAM, _graph(pkg, 0)), **sized)
    for tdt in (False, True):
        add(f"Transducer.beam_search_times tdt={int(bool(tdt))}",
            lambda rec, t=tdt: _decode_mode(pkg, rec, "beam_search_times", BEAM, tdt=t, blank=1), **sized)
        add(f"Transducer.beam_search_context tdt={int(bool(tdt))}",
            lambda rec, t=tdt: _decode_mode(pkg, rec, "beam_search_context", BEAM, _graph(pkg), tdt=t, blank=1), **sized)
    add("Transducer.beam_search_times weights", lambda rec: _decode_mode(
        pkg, rec, "beam_search_times", BEAM, 0.5, 0.5, tdt=True, blank=1), **sized)
    add("Transducer.beam_search_context weights", lambda rec: _decode_mode(
        pkg, rec, "beam_search_context", BEAM, _graph(pkg), 0.5, 0.5, tdt=True, blank=1), **sized)
    for what in ("ctc", "ctc context", "beam", "beam context"):
        add(f"Transducer streaming {what}", lambda rec, w=what: _model_streams(pkg, rec, w), **sized)
    add("Transducer streaming beam context tdt", lambda rec: _model_streams(pkg, rec, "beam context", tdt=True), **sized)


def _refusals(pkg):
    """Bad calls of the public functions, as the test_*_host.py files make them, and the errors they must keep raising."""
    z, ones = torch.zeros, torch.ones
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)                                                   # noqa: E731
    out = {}

    def fused(fn, *extra, width=5, lens=((3, 3), (2, 2)), on_device=False, **kw):
        args = [z(2, 3, 8), z(2, 3, 8), z(width, 8), z(width), ones(2, 2, dtype=torch.int32), i32(*lens[0]), i32(*lens[1])]
        if on_device:
            args = [dev(a) for a in args]
        return lambda rec: fn(*args, *extra, **kw)

    bad_numbers = [-0.1, float("nan"), float("inf"), float("-inf"), "x", None]
    bad_durations = [(), tuple(range(9)) + (9,), (0, 9), (-1, 1), (1, 1), (2, 1), (0,), (0.0, 1.0), (True, 2), 3]
    for key, bad in itertools.product(("fastemit_lambda", "delay_penalty"), bad_numbers):
        out[f"rnnt_loss {key}={bad!r}"] = lambda rec, kw={key: bad}: pkg.rnnt_loss(
            z(2, 3, 3, 5), ones(2, 2, dtype=torch.int32), i32(3, 3), i32(2, 2), blank=0, **kw)
        out[f"joint_rnnt_loss {key}={bad!r}"] = fused(pkg.joint_rnnt_loss, **{key: bad})
        out[f"joint_rnnt_loss budget {key}={bad!r}"] = fused(pkg.joint_rnnt_loss, logits_budget=1 << 20, **{key: bad})
    for name, fn, extra in (("joint_rnnt_loss", pkg.joint_rnnt_loss, ()),
                            ("joint_rnnt_loss budget", pkg.joint_rnnt_loss, ()),
                            ("joint_rnnt_tdt_loss", pkg.joint_rnnt_tdt_loss, ((0, 1, 2),))):
        kw = {"logits_budget": 1 << 20} if name != "joint_rnnt_loss" else {}
        width = 5 + len(extra[0]) if extra else 5
        out[f"{name} cpu"] = fused(fn, *extra, width=width, **kw)
        out[f"{name} reduction"] = fused(fn, *extra, width=width, reduction="average", **kw)
        out[f"{name} targets shape"] = lambda rec, fn=fn, extra=extra, width=width, kw=kw: fn(
            z(2, 3, 8), z(2, 3, 8), z(width, 8), z(width), ones(2, 3, dtype=torch.int32), i32(3, 3), i32(2, 2), *extra, **kw)
        out[f"{name} input length"] = fused(fn, *extra, width=width, lens=((2, 2), (2, 2)), **kw)
        out[f"{name} output length"] = fused(fn, *extra, width=width, lens=((3, 3), (1, 1)), **kw)
        out[f"{name} negative length"] = fused(fn, *extra, width=width, lens=((3, -1), (2, 2)), **kw)
        out[f"{name} budget below a row"] = fused(fn, *extra, width=width, on_device=True, **dict(kw, logits_budget=59))
    for precision in ("bf16", "f16"):
        out[f"joint_rnnt_loss budget precision={precision}"] = fused(pkg.joint_rnnt_loss, precision=precision,
                                                                     logits_budget=1 << 30)
    out["joint_rnnt_loss blank"] = fused(pkg.joint_rnnt_loss, blank=5)
    for precision in ("bf16x3", "autocast"):
        out[f"joint_rnnt_tdt_loss precision={precision}"] = fused(pkg.joint_rnnt_tdt_loss, (0, 1, 2), width=8,
                                                                  precision=precision, logits_budget=1 << 20)
    for bad in bad_durations:
        out[f"joint_rnnt_tdt_loss durations={bad!r}"] = fused(pkg.joint_rnnt_tdt_loss, bad, width=8, logits_budget=1 << 20)
    out["joint_rnnt_tdt_loss sigma"] = fused(pkg.joint_rnnt_tdt_loss, (0, 1, 2), width=8, sigma=-0.5, logits_budget=1 << 20)
    out["joint_rnnt_tdt_loss blank"] = fused(pkg.joint_rnnt_tdt_loss, (0, 1, 2), width=8, blank=5, logits_budget=1 << 20)
    out["joint_rnnt_tdt_loss token columns"] = fused(pkg.joint_rnnt_tdt_loss, tuple(range(9)), width=10,
                                                     logits_budget=1 << 20)
    out["joint_rnnt_tdt_loss no budget"] = fused(pkg.joint_rnnt_tdt_loss, (0, 1, 2), width=8)

    def tdt(fn, durations=(0, 1, 2), blank=0, sigma=0.0, logits=None, targets=None, llens=(2,), tlens=(1,), **kw):
        D = len(durations) if hasattr(durations, "__len__") else 1
        logits = z(1, 2, 2, 6 + D) if logits is None else logits
        targets = ones(1, 1, dtype=torch.int32) if targets is None else targets
        return lambda rec: fn(logits, targets, i32(*llens), i32(*tlens), durations, blank=blank, sigma=sigma, **kw)

    for name, fn in (("rnnt_tdt_loss", pkg.rnnt_tdt_loss), ("rnnt_tdt_forced_align", pkg.rnnt_tdt_forced_align)):
        for bad in bad_durations:
            out[f"{name} durations={bad!r}"] = tdt(fn, durations=bad)
        for bad in (-0.1, float("inf"), float("nan"), "x"):
            out[f"{name} sigma={bad!r}"] = tdt(fn, sigma=bad)
        for bad in (6, -1, 7, 1.0, -7):
            out[f"{name} blank={bad!r}"] = tdt(fn, blank=bad)
        out[f"{name} cpu"] = tdt(fn)
        out[f"{name} cpu bf16"] = tdt(fn, logits=z(1, 2, 2, 9, dtype=torch.bfloat16))
        out[f"{name} rank"] = tdt(fn, logits=z(2, 2, 9))
        out[f"{name} no token column"] = tdt(fn, logits=z(1, 2, 2, 3))
        for key, bad in (("llens", (0,)), ("llens", (3,)), ("tlens", (2,)), ("tlens", (-1,)), ("llens", (2, 2))):
            out[f"{name} {key}={bad!r}"] = tdt(fn, **{key: bad})
        for what, bad in (("label 6", torch.full((1, 1), 6, dtype=torch.int32)),
                          ("label -1", torch.full((1, 1), -1, dtype=torch.int32)), ("width", ones(1, 2, dtype=torch.int32))):
            out[f"{name} targets {what}"] = tdt(fn, targets=bad)
    out["rnnt_tdt_loss reduction"] = tdt(pkg.rnnt_tdt_loss, reduction="average")
    out["rnnt_tdt_forced_align cpu blank jumps"] = tdt(pkg.rnnt_tdt_forced_align, return_blank_jumps=True)
    out["rnnt_loss cpu"] = lambda rec: pkg.rnnt_loss(z(2, 3, 3, 5), ones(2, 2, dtype=torch.int32), i32(3, 3), i32(2, 2), blank=0)
    out["rnnt_loss reduction"] = lambda rec: pkg.rnnt_loss(z(2, 3, 3, 5), ones(2, 2, dtype=torch.int32), i32(3, 3),
                                                           i32(2, 2), blank=0, reduction="average")
    out["RNNTLoss cpu"] = lambda rec: pkg.RNNTLoss(blank=0)(z(2, 3, 3, 5), ones(2, 2, dtype=torch.int32), i32(3, 3), i32(2, 2))
    out["TDTLoss cpu"] = lambda rec: pkg.TDTLoss((0, 1, 2))(z(1, 2, 2, 9), ones(1, 1, dtype=torch.int32), i32(2), i32(1))
    # the k2-style losses, whose reduction check and tail moved: the bad calls of test_rnnt_simple_host.py,
    # test_rnnt_smoothed_host.py and test_rnnt_lattice_host.py, all on CPU tensors (every refusal precedes the device check)
    lm, am = z(3, 4, 7), z(3, 6, 7)
    sy = ones(3, 3, dtype=torch.int64)
    simple = lambda fn=pkg.rnnt_loss_simple, lm=lm, am=am, sy=sy, blank=0, **kw: (                        # noqa: E731
        lambda rec: fn(lm, am, sy, blank, **kw))
    smoothed = lambda *scales, fn=pkg.rnnt_loss_smoothed, sy=sy, blank=0, **kw: (                         # noqa: E731
        lambda rec: fn(lm, am, sy, blank, *scales, **kw))
    ranges = torch.zeros(3, 6, 2, dtype=torch.int64) + torch.arange(2)
    pruned = lambda logits=z(3, 6, 2, 7), **kw: lambda rec: pkg.rnnt_loss_pruned(logits, sy, ranges, 0, **kw)  # noqa: E731

    def boundary(row, column, value):
        bd = torch.tensor([[0, 0, 3, 6], [0, 0, 1, 4], [0, 0, 0, 2]])
        bd[row, column] = value
        return bd

    out["rnnt_loss_simple cpu"] = simple()
    out["rnnt_loss_simple boundary symbol begin"] = simple(boundary=boundary(1, 1, 1))
    out["rnnt_loss_simple boundary frame begin"] = simple(boundary=boundary(2, 0, 1))
    out["rnnt_loss_simple boundary frame ends"] = simple(boundary=boundary(0, 3, 7))
    out["rnnt_loss_simple boundary symbol ends"] = simple(boundary=boundary(0, 2, 4))
    out["rnnt_loss_simple termination_symbol"] = simple(blank=7)
    out["rnnt_loss_simple reduction"] = simple(reduction="avg")
    out["rnnt_loss_simple symbols shape"] = simple(sy=sy[:, :2])
    out["rnnt_loss_simple symbol outside"] = simple(sy=torch.tensor([[9, 1, 1], [1, 1, 1], [1, 1, 1]]))
    out["rnnt_loss_simple delay_penalty keyword"] = simple(delay_penalty=0.1)
    for ll, la in ((-0.1, 0.0), (0.0, -1e-3), (0.6, 0.5), (1.5, 0.0), (float("nan"), 0.0)):
        out[f"rnnt_loss_smoothed scales=({ll!r}, {la!r})"] = smoothed(lm_only_scale=ll, am_only_scale=la)
    out["rnnt_loss_smoothed reduction"] = smoothed(reduction="avg")
    out["rnnt_loss_smoothed termination_symbol"] = smoothed(blank=7)
    out["rnnt_loss_smoothed symbols shape"] = smoothed(sy=sy[:, :2])
    out["rnnt_loss_smoothed cpu"] = smoothed()
    out["rnnt_loss_smoothed cpu scales=(0.0, 0.0)"] = smoothed(0.0, 0.0)
    out["rnnt_loss_pruned cpu"] = pruned()
    out["rnnt_loss_pruned reduction"] = pruned(reduction="avg")
    lattice = (("k2.rnnt_loss_simple", lambda **kw: simple(fn=pkg.k2.rnnt_loss_simple, **kw)),
               ("k2.rnnt_loss_smoothed", lambda **kw: smoothed(0.25, 0.0, fn=pkg.k2.rnnt_loss_smoothed, **kw)),
               ("rnnt_loss_pruned", pruned))
    for name, make in lattice:
        for bad in ("constrained", "Modified", "", "simple", None, 1):
            out[f"{name} rnnt_type={bad!r}"] = make(rnnt_type=bad)
        for bad, rnnt_type in itertools.product((-0.01, float("nan"), float("inf"), -float("inf")), ("regular", "modified")):
            out[f"{name} {rnnt_type} delay_penalty={bad!r}"] = make(rnnt_type=rnnt_type, delay_penalty=bad)
        for kw in (dict(rnnt_type="modified"), dict(delay_penalty=0.003), dict(rnnt_type="regular", delay_penalty=0.0)):
            out[f"{name} cpu {kw}"] = make(**kw)
        for bad in (None, ["mean"], "Mean"):
            out[f"{name} reduction={bad!r}"] = make(reduction=bad)
    # the order of the refusals: lattice, reduction, scales, shapes in the additive losses; reduction, lattice, shapes in
    # the pruned one.  Each call is wrong in two ways or more; the record keeps which error comes first
    for name, make in lattice[:2]:
        out[f"{name} order: lattice before reduction"] = make(rnnt_type="other", reduction="avg", sy=sy[:, :2])
        out[f"{name} order: reduction before shapes"] = make(reduction="avg", sy=sy[:, :2], blank=7)
    out["k2.rnnt_loss_smoothed order: lattice before scales"] = simple(
        fn=pkg.k2.rnnt_loss_smoothed, lm_only_scale=-0.1, delay_penalty=-1.0)
    out["k2.rnnt_loss_smoothed order: reduction before scales"] = simple(
        fn=pkg.k2.rnnt_loss_smoothed, lm_only_scale=-0.1, reduction="avg")
    out["k2.rnnt_loss_smoothed order: scales before shapes"] = simple(
        fn=pkg.k2.rnnt_loss_smoothed, lm_only_scale=-0.1, sy=sy[:, :2])
    out["rnnt_loss_pruned order: reduction before lattice"] = pruned(reduction="avg", rnnt_type="other")
    out["rnnt_loss_pruned order: lattice before shapes"] = pruned(z(3, 6, 2), rnnt_type="other")
    # the decoder was sized for fewer tokens than the search reports (the recorder reports 1 and 2)
    for method, args in (("greedy", ()), ("greedy_tdt", ((0, 1, 2),)), ("greedy_chunk", ())):
        out[f"DeviceDecoder.{method} more tokens than max_hyp"] = lambda rec, m=method, a=args: _decode(pkg, rec, m, *a)
    # Transducer methods that refuse the other kind of model before they touch their inputs
    none = (None, None)
    out["Transducer plain tdt_attention_rescoring"] = lambda rec: model(pkg).tdt_attention_rescoring(z(1, 4, 8), i32(4), 3)
    out["Transducer plain tdt_beam_search"] = lambda rec: model(pkg).tdt_beam_search(z(1, 4, 8), i32(4))
    out["Transducer plain tdt_greedy_search_batch"] = lambda rec: model(pkg).tdt_greedy_search_batch(*none)
    out["Transducer tdt transducer_attention_rescoring"] = lambda rec: model(
        pkg, 26, tdt_durations=(0, 1, 2)).transducer_attention_rescoring(z(1, 4, 8), i32(4), 3)
    out["Transducer tdt forward_greedy_search"] = lambda rec: model(
        pkg, 26, tdt_durations=(0, 1, 2)).forward_greedy_search(*none)
    out["Transducer tdt greedy_search_batch"] = lambda rec: model(pkg, 26, tdt_durations=(0, 1, 2)).greedy_search_batch(*none)
    _stream_refusals(pkg, out)
    return out


def cases(pkg):
    """case id -> (function of the recorder, recorder settings).  The ids are the fixture's."""
    out = {}

    def add(name, fn, **rec):
        assert name not in out, name
        out[name] = (fn, rec)

    flag = lambda x: int(bool(x))                                                                          # noqa: E731
    # the memory-bounded nodes: three budgets; an utterance without a frame has no slice and breaks the run
    for budget, need_w, lam, pen, precision in itertools.product(BUDGETS, (True, False), (0.0, 0.5), (0.0, 0.25),
                                                                 ("fp32", "bf16x3")):
        add(f"bounded rnnt budget={budget} need_w={flag(need_w)} lambda={lam} penalty={pen} {precision}",
            lambda rec, a=(budget, need_w, lam, pen, precision): _joint_rnnt(
                pkg, rec, a[1], logits_budget=BUDGETS[a[0]](V), fastemit_lambda=a[2], delay_penalty=a[3], precision=a[4]))
    for budget, need_w, durations, sigma in itertools.product(BUDGETS, (True, False), ((0, 1, 2), (1,)), (0.0, 0.05)):
        add(f"bounded tdt budget={budget} need_w={flag(need_w)} durations={durations} sigma={sigma}",
            lambda rec, a=(budget, need_w, durations, sigma): _joint_tdt(
                pkg, rec, a[2], a[1], sigma=a[3], logits_budget=BUDGETS[a[0]](V + len(a[2]))))
    # the node that keeps the logits
    for precision, epilogue, lam, pen in itertools.product(("fp32", "bf16x3"), (None, "0", "1"), (0.0, 0.5), (0.0, 0.25)):
        env = {} if epilogue is None else {"WR_FUSED_LSE_EPILOGUE": epilogue}
        add(f"fused {precision} epilogue={epilogue} lambda={lam} penalty={pen}",
            lambda rec, a=(precision, env, lam, pen): _joint_rnnt(pkg, rec, env=a[1], precision=a[0], fastemit_lambda=a[2],
                                                                  delay_penalty=a[3]))
    for precision in ("fp32", "bf16x3"):
        add(f"fused {precision} second backward", lambda rec, p=precision: _joint_rnnt(pkg, rec, precision=p, times=2))
        add(f"fused {precision} separate gradient buffer",
            lambda rec, p=precision: _joint_rnnt(pkg, rec, precision=p, env={"WR_FUSED_INPLACE_BYTES": str(1 << 40)}))
    add("fused weights without gradient", lambda rec: _joint_rnnt(pkg, rec, need_w=False, precision="fp32"))
    add("bucketed", lambda rec: _bucketed(pkg, rec))
    add("bucketed budget", lambda rec: _bucketed(pkg, rec, logits_budget=1 << 40))
    add("bucketed buckets=2", lambda rec: _bucketed(pkg, rec, buckets=2))
    # the losses that take logits, and TDT alignment
    for name, dtype in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        for lam, pen, inplace in itertools.product((0.0, 0.5), (0.0, 0.25), (False, True)):
            add(f"rnnt_loss {name} lambda={lam} penalty={pen} inplace={flag(inplace)}",
                lambda rec, a=(dtype, lam, pen, inplace): _rnnt_loss(pkg, rec, a[0], fastemit_lambda=a[1], delay_penalty=a[2],
                                                                     inplace_grad=a[3]))
        for durations, sigma, inplace in itertools.product(((0, 1, 2), (1,)), (0.0, 0.05), (False, True)):
            add(f"rnnt_tdt_loss {name} durations={durations} sigma={sigma} inplace={flag(inplace)}",
                lambda rec, a=(dtype, durations, sigma, inplace): _tdt_loss(pkg, rec, a[0], a[1], sigma=a[2],
                                                                            inplace_grad=a[3]))
        for jumps in (False, True):
            add(f"rnnt_tdt_forced_align {name} blank_jumps={flag(jumps)}",
                lambda rec, a=(dtype, jumps): _tdt_align(pkg, rec, a[0], (0, 1, 2), sigma=0.05, return_blank_jumps=a[1]))
    add("rnnt_loss inplace from the environment",
        lambda rec: (os.environ.update(WR_RNNT_INPLACE_GRAD="1"), _rnnt_loss(pkg, rec, torch.float32))[1])
    add("rnnt_tdt_loss inplace from the environment",
        lambda rec: (os.environ.update(WR_RNNT_INPLACE_GRAD="1"), _tdt_loss(pkg, rec, torch.float32, (0, 1, 2)))[1])
    # DeviceDecoder
    sized = dict(max_hyp=8, tmax=DT)
    add("DeviceDecoder.greedy", lambda rec: _decode(pkg, rec, "greedy", n_steps=4, blank=1), **sized)
    add("DeviceDecoder.greedy defaults", lambda rec: _decode(pkg, rec, "greedy"), **sized)
    for durations, frames in itertools.product(((0, 1, 2), ()), (False, True)):
        add(f"DeviceDecoder.greedy_tdt durations={durations} return_frames={flag(frames)}",
            lambda rec, a=(durations, frames): _decode(pkg, rec, "greedy_tdt", a[0], n_steps=4, blank=1, return_frames=a[1]),
            **sized)
    for reset in (False, True):
        add(f"DeviceDecoder.greedy_chunk reset={flag(reset)}",
            lambda rec, r=reset: _decode(pkg, rec, "greedy_chunk", n_steps=4, blank=1, reset=r, reference_new_cache=not r),
            **sized)
    add("DeviceDecoder.prefix_beam", lambda rec: _decode(pkg, rec, "prefix_beam", dev(torch.zeros(DN, DT, DV)), BEAM, 0.3,
                                                         0.7, 1), **sized)
    for durations, ctc in itertools.product(((0, 1, 2), ()), (False, True)):
        weights = dict(ctc_weight=0.3, transducer_weight=0.7) if ctc else {}
        add(f"DeviceDecoder.prefix_beam_tdt durations={durations} ctc={flag(ctc)}",
            lambda rec, a=(durations, ctc, weights): _decode(pkg, rec, "prefix_beam_tdt", a[0], BEAM, 1, ctc=a[1], **a[2]),
            **sized)
    # search/: the lengths and the decoder a search asks its cache for, then the DeviceDecoder call
    for name, lens in (("scalar", torch.tensor(6)), ("vector", torch.tensor([6, 4]))):
        add(f"basic_greedy_search lens={name}", lambda rec, l=lens: _search(pkg, rec, "basic_greedy_search", l, n_steps=4),
            **sized)
        add(f"tdt_greedy_search lens={name}",
            lambda rec, l=lens: _search(pkg, rec, "tdt_greedy_search", l, n_steps=4, return_frames=l.dim() == 0), **sized)
        add(f"forward_greedy_search lens={name}", lambda rec, l=lens: _search(pkg, rec, "forward_greedy_search", l), **sized)
        add(f"tdt_prefix_beam_search lens={name}",
            lambda rec, l=lens: _search(pkg, rec, "tdt_prefix_beam_search", l, beam_size=BEAM,
                                        **(dict(ctc_weight=0.3, transducer_weight=0.7) if l.dim() else {})), **sized)
    add("PrefixBeamSearch.search_encoded", lambda rec: _search(pkg, rec, "search_encoded", torch.tensor([6, 4])), **sized)
    add("PrefixBeamSearch.search_encoded weights",
        lambda rec: _search(pkg, rec, "search_encoded", torch.tensor([6, 4]), ctc_weight=0.5, transducer_weight=0.5), **sized)
    # Transducer: the loss block and the hypothesis scores of a tiny plain and a tiny TDT model
    for tdt, budget in itertools.product((False, True), (None, 1 << 20)):
        add(f"Transducer.compute_loss tdt={flag(tdt)} budget={budget}",
            lambda rec, a=(tdt, budget): _loss_block(pkg, rec, a[0], a[1]))
    for tdt in (False, True):
        add(f"Transducer.compute_loss tdt={flag(tdt)} two ops", lambda rec, t=tdt: _loss_block(pkg, rec, t, None, fused=False))
        add(f"Transducer score tdt={flag(tdt)}", lambda rec, t=tdt: _score(pkg, rec, t))
    add("Transducer score tdt=0 two ops", lambda rec: _score(pkg, rec, False, fused=False))
    _stream_cases(pkg, add)
    for name, fn in _refusals(pkg).items():
        add("refusal: " + name, fn, max_hyp=1, tmax=DT)
    return out


def record(pkg, case):
    """The record of one case (an entry of `cases`), as described in the module docstring."""
    fn, settings = case
    rec = Recorder(pkg._lib.SIGNATURES, **settings)
    out = {"calls": rec.calls}
    with seams(pkg, rec):
        try:
            out["result"] = fn(rec)
        except Exception as e:                                        # a refusal is part of the record
            out["raises"] = [type(e).__name__, str(e)]
    return out


def record_all(pkg):
    return {name: record(pkg, case) for name, case in cases(pkg).items()}
