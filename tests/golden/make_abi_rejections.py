"""Record what the entry points of the library answer to bad arguments: tests/golden/abi_rejections.json.

    python tests/golden/make_abi_rejections.py            # rewrites the table from the library as built

Every row is one call that an argument check rejects BEFORE the first HIP call: (entry point, arguments, return code,
exact wr_last_error() text).  tests/test_abi.py replays the table, so a change to the host code between `extern "C"`
and the launches keeps codes, texts and the order of the checks.  Run it on the commit whose behaviour is to be kept.

Arguments are written by parameter name (include/wr_api.h) over a base call per entry point: small positive sizes,
every pointer a never-dereferenced placeholder, every workspace size 0.  The base call itself is rejected (its
workspace is too small, or, where an entry point takes no workspace, a row overrides an argument that is checked).
Pointers are encoded as "null", "ptr" (16-byte aligned placeholder) or "ptr+8"; the one pointer that is read, the
decoder's weight description, as {"weights": {field: value}} over WEIGHTS_BASE (every weight pointer a placeholder).  A
row that comes back WR_OK or WR_ELAUNCH reached a launch: the generator refuses to write the table.

The size queries of the decoder answer a bad argument with 0 and set no error text: SIZE_ZERO lists those calls, the
generator checks them and tests/test_abi.py repeats them; they are not rows of the table.
"""
import ctypes
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
TABLE = os.path.join(HERE, "abi_rejections.json")
PLACEHOLDER = 0x100000
WR_OK, WR_ELAUNCH = 0, -4


def prototypes():
    """{entry point: [(kind, name), ...]} from include/wr_api.h; kind is 'ptr', 'int', 'float' or 'size'."""
    text = open(os.path.join(ROOT, "include", "wr_api.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(?:int|size_t)\s+(wr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        params = []
        for p in m.group(2).split(","):
            p = " ".join(p.split())
            if p in ("", "void"):
                continue
            name = re.search(r"([A-Za-z_0-9]+)$", p).group(1)
            if "*" in p:
                kind = "ptr"
            elif re.search(r"\b(float|double)\b", p):
                kind = "float"
            elif "size_t" in p:
                kind = "size"
            else:
                kind = "int"
            params.append((kind, name))
        out[m.group(1)] = params
    return out


# base value of an integer / float parameter, by name (every other integer is 0, every float 0.0)
BASE = {"B": 2, "T": 4, "Tmax": 4, "U1": 3, "U1max": 3, "Smax": 2, "V": 8, "J": 8, "R": 2, "C": 4, "terms": 3, "h_ld": 8,
        "px_cols": 5, "cell_end": 1, "clamp": -1.0,
        "max_lanes": 4, "max_utt": 2, "max_hyp": 8, "max_beam": 2, "beam": 2, "N": 2, "n_steps": 1, "trace_cap": 4,
        "max_ctx": 2, "n_ctx_hot": 1, "n_ctx_cold": 1}

# wr_transducer_weights of the smallest LSTM decoder; a pointer field is "ptr" unless a row says "null"
WEIGHTS_BASE = {"vocab_size": 32, "enc_dim": 16, "pred_dim": 16, "embed_dim": 16, "hidden": 16, "n_layers": 1, "join_dim": 32}
_keep = []              # the weight structs of decoded calls stay alive


def weights_struct(over):
    from wenet_celoss_amd import _lib
    w = _lib.TransducerWeights()
    vals = dict(WEIGHTS_BASE, **over)
    assert not set(vals) - {n for n, _ in w._fields_}, vals
    for name, ctype in w._fields_:
        v = vals.get(name)
        if ctype is ctypes.c_void_p:
            setattr(w, name, None if v == "null" else PLACEHOLDER)
        elif issubclass(ctype, ctypes.Array):
            setattr(w, name, ctype(*([None if v == "null" else PLACEHOLDER] * len(ctype()))))
        elif v is not None:
            setattr(w, name, v)
    _keep.append(w)
    return ctypes.byref(w)


def decode(kind, v):
    if isinstance(v, dict):
        return weights_struct(v["weights"])
    if kind == "ptr":
        return None if v == "null" else ctypes.c_void_p(PLACEHOLDER + (8 if v == "ptr+8" else 0))
    return v


def arguments(proto, over):
    unknown = set(over) - {n for _, n in proto}
    assert not unknown, unknown
    args = []
    for kind, name in proto:
        if name in over:
            args.append(over[name])
        elif name == "stream":
            args.append("null")
        elif kind == "ptr":
            args.append("ptr")
        elif kind == "float":
            args.append(float(BASE.get(name, 0.0)))
        else:
            args.append(BASE.get(name, 0))
    return args


NULLS = "null"
BIG = 1 << 40           # a workspace size that passes every size check

# (entry point, class of the check, overrides of the base call)
ROWS = []


def row(fn, what, **over):
    ROWS.append((fn, what, over))


def rnnt_loss_family():
    for fn, has_v, ptr0, has_dtype, has_targets in [
            ("wr_rnnt_loss_fwd", True, "logits_d", True, True), ("wr_rnnt_loss_fwd_from_lse", True, "logits_d", False, True),
            ("wr_rnnt_loss_sweeps", False, "costs_d", False, False), ("wr_rnnt_loss_bwd", True, "grads_d", True, True),
            ("wr_rnnt_export_lattice", False, "alpha_d", False, False)]:
        row(fn, "sizes", B=0)
        if has_v:
            row(fn, "blank range", blank=8)
            row(fn, "blank range", blank=-1)
        row(fn, "U1 limit", U1max=1025)
        row(fn, "cell count", B=1 << 15, Tmax=1 << 15, U1max=4)
        row(fn, "null pointer", **{ptr0: NULLS})
        row(fn, "null pointer", logit_lengths_d=NULLS)
        if has_targets:
            row(fn, "targets null", targets_d=NULLS)
        if has_dtype:
            row(fn, "dtype code", dtype=3)
        row(fn, "workspace size")
        row(fn, "workspace size", workspace_bytes=255)


def lattice_family():
    for fn in ("wr_rnnt_lattice_sweeps", "wr_rnnt_lattice_export"):
        row(fn, "sizes", T=0)
        row(fn, "U1 limit", U1=1025)
        row(fn, "cell count", B=1 << 15, T=1 << 15, U1=4)
        row(fn, "lattice code", lattice_type=2)
        row(fn, "null pointer", logit_lengths_d=NULLS)
        row(fn, "workspace size")
        row(fn, "workspace size", lattice_type=1)
    row("wr_rnnt_lattice_sweeps", "delay penalty", delay_penalty=-0.5)
    row("wr_rnnt_lattice_sweeps", "position count", B=1025, T=1 << 10, U1=1024, delay_penalty=0.5)
    row("wr_rnnt_lattice_sweeps", "null pointer", costs_d=NULLS, delay_penalty=0.5)


def pruned_family():
    for fn in ("wr_rnnt_prune_ranges", "wr_rnnt_prune_ranges_cols"):
        row(fn, "sizes", R=0)
        row(fn, "band width", R=4)
        row(fn, "row count", B=1 << 15, T=1 << 15, U1=4)
        row(fn, "null pointer", ranges_d=NULLS)
        row(fn, "null pointer", py_grad_d=NULLS)
        row(fn, "px_grad null", px_grad_d=NULLS)
        row(fn, "alignment", ranges_d="ptr+8")
    row("wr_rnnt_prune_ranges_cols", "px_cols", px_cols=6)
    row("wr_rnnt_prune_ranges_cols", "px_cols", px_cols=3, ranges_d=NULLS)
    for fn, p in (("wr_rnnt_prune_gather", "am_pruned_d"), ("wr_rnnt_prune_scatter", "ranges_d")):
        row(fn, "sizes", U1=0)
        row(fn, "band width", R=4)
        row(fn, "sizes", C=0)
        row(fn, "dtype code", dtype=-1)
        row(fn, "dtype code", dtype=3)
        row(fn, "null pointer", **{p: NULLS})
    row("wr_rnnt_prune_scatter", "null pointer", d_am_d=NULLS, d_lm_d=NULLS)
    row("wr_rnnt_prune_scatter", "output without gradient", g_am_pruned_d=NULLS)
    row("wr_rnnt_prune_scatter", "output without gradient", g_lm_pruned_d=NULLS, d_am_d=NULLS)
    for fn in ("wr_rnnt_pruned_stats", "wr_rnnt_pruned_grad", "wr_rnnt_pruned_grad_lattice"):
        row(fn, "sizes", B=-1)
        row(fn, "band width", R=4)
        row(fn, "sizes", V=0)
        row(fn, "blank range", blank=8)
        row(fn, "dtype code", dtype=3)
        row(fn, "U1 limit", U1=1025, R=2)
        row(fn, "null pointer", ranges_d=NULLS)
        row(fn, "symbols null", symbols_d=NULLS)
        row(fn, "workspace size")
        row(fn, "workspace size", rnnt_workspace_bytes=4096)
    for fn in ("wr_rnnt_pruned_grad", "wr_rnnt_pruned_grad_lattice"):
        row(fn, "null pointer", grads_d=NULLS)
        row(fn, "alignment", grads_d="ptr+8")
    row("wr_rnnt_pruned_grad_lattice", "lattice code", lattice_type=-1)
    row("wr_rnnt_pruned_grad_lattice", "delay penalty", delay_penalty=-1.0)


def simple_family():
    for fn in ("wr_rnnt_simple_stats", "wr_rnnt_simple_grad", "wr_rnnt_smoothed_stats", "wr_rnnt_smoothed_grad",
               "wr_rnnt_smoothed_grad_lattice"):
        smoothed = "smoothed" in fn
        big = "smoothed_workspace_bytes" if smoothed else "simple_workspace_bytes"
        row(fn, "sizes", U1=0)
        row(fn, "sizes", V=1)
        row(fn, "blank range", blank=8)
        row(fn, "U1 limit", U1=1025)
        row(fn, "cell count", B=1 << 15, T=1 << 15, U1=4)
        row(fn, "grid limit", B=65536, T=1, U1=1)
        if smoothed:
            row(fn, "scales", lm_only_scale=-0.25)
            row(fn, "scales", lm_only_scale=0.75, am_only_scale=0.5)
            row(fn, "vocabulary limit", V=256 * 65535 + 1, lm_only_scale=0.25)
            row(fn, "workspace size", lm_only_scale=0.25, am_only_scale=0.25)
        row(fn, "workspace size")
        row(fn, "workspace size", **{big: BIG})
        # the null checks follow the size checks, so these rows need sizes that pass: their pointers are all null
        nulls = {n: NULLS for n in ("am_d", "lm_d", "symbols_d", "logit_lengths_d", "target_lengths_d", "rnnt_workspace_d")}
        nulls["smoothed_workspace_d" if smoothed else "simple_workspace_d"] = NULLS
        if "grad" in fn:
            nulls.update(grad_costs_d=NULLS, d_am_d=NULLS, d_lm_d=NULLS, occ_emit_d=NULLS, occ_blank_d=NULLS)
        row(fn, "null pointer", rnnt_workspace_bytes=BIG, **{big: BIG}, **nulls)
    row("wr_rnnt_smoothed_grad_lattice", "lattice code", lattice_type=2)


def ctc_family():
    for fn, p in (("wr_ctc_loss_fwd", "nll_d"), ("wr_ctc_loss_bwd", "grads_d"), ("wr_ctc_forced_align", "alignment_d")):
        row(fn, "sizes", Tmax=0)
        row(fn, "sizes", Smax=-1)
        row(fn, "blank range", blank=8)
        row(fn, "label limit", Smax=512)
        row(fn, "vocabulary limit", V=16385)
        row(fn, "null pointer", **{p: NULLS})
        row(fn, "targets null", targets_d=NULLS)
        row(fn, "workspace size")
        row(fn, "workspace size", workspace_bytes=1024)
    for fn in ("wr_ctc_loss_fwd", "wr_ctc_loss_bwd"):
        row(fn, "dtype code", dtype=1)
        row(fn, "dtype code", dtype=2)
        row(fn, "workspace size", Smax=0, targets_d=NULLS)
    row("wr_ctc_forced_align", "empty labels", Smax=0)


def joint_family():
    exact = [("wr_joint_fwd", "out_d"), ("wr_joint_fwd_lse", "out_d"), ("wr_joint_rnnt_stats", "ep_d"),
             ("wr_joint_rnnt_grad", "w_out_d"), ("wr_joint_bwd_dz", "dz_d"), ("wr_joint_bwd_dw", "dw_d")]
    for fn, p in exact:
        row(fn, "sizes", J=0)
        if fn != "wr_joint_bwd_dw":
            row(fn, "activation code", activation=6)
            row(fn, "activation code", activation=-1)
        row(fn, "join_dim", J=6)
        row(fn, "join_dim", J=516)
        row(fn, "null pointer", **{p: NULLS})
    for fn in ("wr_joint_fwd", "wr_joint_bwd_dz", "wr_joint_bwd_dw"):
        row(fn, "length pair", logit_lengths_d=NULLS)
        row(fn, "length pair", target_lengths_d=NULLS)
    row("wr_joint_fwd", "workspace size")
    row("wr_joint_fwd", "workspace size", logit_lengths_d=NULLS, target_lengths_d=NULLS, workspace_bytes=16)
    row("wr_joint_bwd_dw", "workspace size")
    row("wr_joint_bwd_dw", "workspace size", workspace_bytes=64)
    for fn in ("wr_joint_fwd_lse", "wr_joint_fwd_split_lse"):
        row(fn, "length pair", logit_lengths_d=NULLS)
        row(fn, "length pair", logit_lengths_d=NULLS, target_lengths_d=NULLS)
    for fn in ("wr_joint_fwd_lse", "wr_joint_fwd_split_lse", "wr_joint_rnnt_stats", "wr_joint_rnnt_grad"):
        row(fn, "null pointer", rnnt_workspace_d=NULLS)
        row(fn, "targets null", targets_d=NULLS)
        row(fn, "targets null", targets_d=NULLS, blank=9)
        row(fn, "blank range", blank=8)
        row(fn, "blank range", blank=-1, U1=1025)
        row(fn, "U1 limit", U1=1025)
        row(fn, "workspace size")
        row(fn, "workspace size", rnnt_workspace_bytes=4096, workspace_bytes=BIG)
    for fn in ("wr_joint_rnnt_stats", "wr_joint_rnnt_grad"):
        row(fn, "null pointer", logit_lengths_d=NULLS)
        row(fn, "terms code", terms=1)
        row(fn, "terms code", terms=2, blank=8)
        row(fn, "blank range", terms=0, blank=8)
        row(fn, "cell count", B=1 << 15, T=1 << 15, U1=4)
        row(fn, "workspace size", terms=0)
    # the joiner's own workspace, the first statement of the launch functions behind the RNN-T side checks
    row("wr_joint_fwd_lse", "joiner workspace size", rnnt_workspace_bytes=BIG)
    row("wr_joint_fwd_lse", "joiner workspace size", rnnt_workspace_bytes=BIG, workspace_bytes=16)
    for terms in (3, 1):
        row("wr_joint_fwd_split_lse", "joiner workspace size", rnnt_workspace_bytes=BIG, terms=terms)
        row("wr_joint_fwd_split_lse", "joiner workspace size", rnnt_workspace_bytes=BIG, terms=terms, workspace_bytes=16)
    for terms in (0, 3):
        row("wr_joint_rnnt_stats", "joiner workspace size", rnnt_workspace_bytes=BIG, terms=terms)
        row("wr_joint_rnnt_stats", "joiner workspace size", rnnt_workspace_bytes=BIG, terms=terms, workspace_bytes=16)
        row("wr_joint_rnnt_grad", "joiner workspace size", rnnt_workspace_bytes=BIG, terms=terms)
        row("wr_joint_rnnt_grad", "joiner workspace size", rnnt_workspace_bytes=BIG, terms=terms, cell_begin=5, cell_end=24,
            workspace_bytes=16, w_ready=1)
    # past the shared checks: the cell range (every pointer null but the ones checked before it; sizes that pass)
    row("wr_joint_rnnt_grad", "null pointer", rnnt_workspace_bytes=BIG, g_out_d=NULLS)
    row("wr_joint_rnnt_grad", "cell range", rnnt_workspace_bytes=BIG, cell_begin=-1)
    row("wr_joint_rnnt_grad", "cell range", rnnt_workspace_bytes=BIG, cell_begin=3, cell_end=3)
    row("wr_joint_rnnt_grad", "cell range", rnnt_workspace_bytes=BIG, cell_begin=0, cell_end=25)

    split = [("wr_joint_fwd_split", "out_d", True), ("wr_joint_fwd_f16", "workspace_d", False),
             ("wr_joint_fwd_split_lse", "b_out_d", True), ("wr_joint_bwd_dz_split", "dz_d", True),
             ("wr_joint_bwd_dz_split_bf16", "gout_bf16_d", True), ("wr_joint_bwd_dz_f16", "w_out_d", False),
             ("wr_joint_bwd_dw_split", "dw_d", True), ("wr_joint_bwd_dw_split_bf16", "h_d", True),
             ("wr_joint_bwd_dw_f16", "gout_d", False)]
    for fn, p, has_terms in split:
        dw = "bwd_dw" in fn
        v = {"V": 32} if "bwd_d" in fn else {}
        if not dw:
            row(fn, "activation code", activation=6, **v)
        row(fn, "sizes", B=0, **v)
        row(fn, "join_dim", J=516, **v)
        row(fn, "join_dim", J=10, **v)
        if has_terms:
            row(fn, "terms code", terms=0, **v)
            row(fn, "terms code", terms=2, **v)
        row(fn, "null pointer", **{p: NULLS}, **v)
        if fn != "wr_joint_fwd_split_lse":
            row(fn, "length pair", logit_lengths_d=NULLS, **v)
            row(fn, "length pair", target_lengths_d=NULLS, **v)
        if "bwd_d" in fn:
            row(fn, "vocabulary shape", V=30)
            row(fn, "workspace size", **v)
            row(fn, "workspace size", workspace_bytes=256, **v)
            row(fn, "workspace size", logit_lengths_d=NULLS, target_lengths_d=NULLS, **v)
    for fn in ("wr_joint_fwd_split", "wr_joint_fwd_f16"):
        row(fn, "dtype code", out_dtype=3)
        row(fn, "dtype code", out_dtype=-1)
        row(fn, "workspace size")
        row(fn, "workspace size", workspace_bytes=128, out_dtype=2)
    row("wr_joint_fwd_split", "workspace size", terms=1, out_dtype=1)
    for fn in ("wr_joint_bwd_dz_split", "wr_joint_bwd_dz_split_bf16", "wr_joint_bwd_dz_f16"):
        row(fn, "vocabulary shape", V=16)
    row("wr_joint_bwd_dz_split_bf16", "vocabulary shape", V=36)
    for fn in ("wr_joint_bwd_dz_f16", "wr_joint_bwd_dw_f16"):
        row(fn, "dtype code", gout_dtype=2)
        row(fn, "dtype code", gout_dtype=-1)
    row("wr_joint_bwd_dz_f16", "vocabulary shape", V=36, gout_dtype=1)
    for fn in ("wr_joint_db_bf16", "wr_joint_db_f16"):
        row(fn, "sizes", V=0)
        row(fn, "sizes", V=12)
        row(fn, "null pointer", db_d=NULLS)
        row(fn, "length pair", target_lengths_d=NULLS)
        row(fn, "workspace size")
        row(fn, "workspace size", workspace_bytes=4096)
    fn = "wr_joint_dz_act"
    row(fn, "sizes", J=6)
    row(fn, "sizes", T=0)
    row(fn, "activation code", activation=7)
    row(fn, "null pointer", dz_d=NULLS)
    row(fn, "length pair", logit_lengths_d=NULLS)
    row(fn, "activation copy", h_dtype=3)
    row(fn, "activation copy", h_ld=4)
    row(fn, "activation copy", h_ld=10)


def W(**over):
    return {"weights": over}


STATELESS = dict(predictor_type=1, context_size=2, n_layers=1, n_head=2, ln_eps=1e-5)


def decoder_family():
    fn = "wr_decoder_create"

    def create(what, w=None, **over):
        row(fn, what, w=W() if w is None else w, **over)
    create("weights null", w=NULLS)
    create("weight sizes", W(vocab_size=1))
    create("weight sizes", W(join_dim=0))
    create("layer count", W(n_layers=0))
    create("layer count", W(n_layers=5))
    create("activation code", W(activation=6))
    create("layer width", W(hidden=1025))
    create("vocabulary limit", W(vocab_size=16385))
    create("null weight", W(embed=NULLS))
    create("null weight", W(out_b=NULLS))
    create("predictor type", W(predictor_type=3))
    create("predictor type", W(predictor_type=-1))
    create("null weight", W(proj_w=NULLS))                    # LSTM
    create("null weight", W(w_hh=NULLS))
    create("null weight", W(n_layers=2, b_ih=NULLS))
    for t in (1, 2):                                          # embedding / conv: the checks the stateless predictors share
        sl = dict(STATELESS, predictor_type=t)
        create("context size", W(**dict(sl, context_size=1)))
        create("context size", W(**dict(sl, context_size=6, n_layers=4)))
        create("context size", W(**dict(sl, context_size=3)))
        create("stateless widths", W(**dict(sl, hidden=32)))
        create("stateless widths", W(**dict(sl, pred_dim=8)))
        create("activation code", W(**dict(sl, pred_activation=6)))
        create("layer norm", W(**dict(sl, ln_eps=0.0)))
        create("layer norm", W(**dict(sl, norm_b=NULLS)))
        create("workspace size", W(**sl))
    emb = dict(STATELESS, predictor_type=1)
    create("head count", W(**dict(emb, n_head=0)))
    create("head count", W(**dict(emb, n_head=33)))
    create("null weight", W(**dict(emb, ffn_w=NULLS)))
    create("null weight", W(**dict(STATELESS, predictor_type=2, conv_w=NULLS)))
    create("null pointer", out=NULLS)
    create("null pointer", workspace_d=NULLS)
    create("lanes", max_lanes=0)
    create("lanes", max_lanes=1025)
    create("sizes", max_utt=0)
    create("sizes", max_utt=5)
    create("sizes", Tmax=0)
    create("sizes", max_hyp=-1)
    create("beam", max_beam=17)
    create("workspace size")
    create("workspace size", max_beam=0, workspace_bytes=4096)
    # everything else a decoder offers needs a handle: the null handle is what can be rejected without one
    for fn in ("wr_decoder_set_graph", "wr_decoder_set_lookahead", "wr_greedy_search", "wr_greedy_search_chunk",
               "wr_prefix_beam_search", "wr_predictor_step", "wr_decoder_attach_hotword", "wr_greedy_search_hotword"):
        row(fn, "null handle", h=NULLS)
    row("wr_decoder_attach_hotword", "null handle", h=NULLS, hw=NULLS)


def ctc_decode_family():
    for fn in ("wr_ctc_greedy_search", "wr_ctc_prefix_beam_search"):
        row(fn, "sizes", B=0)
        row(fn, "sizes", T=-1)
        row(fn, "sizes", V=1)
        row(fn, "blank range", blank=8)
        row(fn, "blank range", blank=-1)
        row(fn, "vocabulary limit", V=16321)
        row(fn, "null pointer", logits_d=NULLS)
        row(fn, "null pointer", workspace_d=NULLS)
        row(fn, "workspace size")
        row(fn, "workspace size", workspace_bytes=64)
    fn = "wr_ctc_prefix_beam_search"
    row(fn, "null pointer", n_hyps_d=NULLS)
    row(fn, "beam", beam=0)
    row(fn, "beam", beam=17, V=32)
    row(fn, "beam", beam=9)


def rnnt_align_family():
    for fn, ws in (("wr_rnnt_align", "workspace_bytes"), ("wr_rnnt_align_from_stats", "rnnt_workspace_bytes")):
        row(fn, "sizes", Tmax=0)
        row(fn, "U1 limit", U1max=1025)
        row(fn, "cell count", B=1 << 15, Tmax=1 << 15, U1max=4)
        row(fn, "null pointer", scores_d=NULLS)
        row(fn, "null pointer", logit_lengths_d=NULLS)
        row(fn, "targets null", targets_d=NULLS)
        row(fn, "targets null", label_frames_d=NULLS)
        row(fn, "workspace size")
        row(fn, "workspace size", **{ws: 255})
        row(fn, "workspace size", U1max=1, targets_d=NULLS, label_frames_d=NULLS)
    fn = "wr_rnnt_align"
    row(fn, "sizes", V=0)
    row(fn, "blank range", blank=8)
    row(fn, "blank range", blank=-1)
    row(fn, "null pointer", logits_d=NULLS)
    row(fn, "dtype code", dtype=3)
    row(fn, "dtype code", dtype=-1)


# size queries that answer a bad argument with 0: (entry point, overrides of the base call)
SIZE_ZERO = [("wr_decoder_workspace_bytes", dict(w=NULLS)), ("wr_decoder_workspace_bytes", dict(w=W(), max_lanes=0)),
             ("wr_decoder_workspace_bytes", dict(w=W(), max_utt=0)), ("wr_decoder_workspace_bytes", dict(w=W(), Tmax=-1)),
             ("wr_hotword_workspace_bytes", dict(h=NULLS)), ("wr_ctc_decode_workspace_bytes", dict(B=0)),
             ("wr_ctc_decode_workspace_bytes", dict(T=0)), ("wr_ctc_decode_workspace_bytes", dict(beam=0))]


def size_zero_answers(lib):
    """[(entry point, overrides, what the library returned)] for SIZE_ZERO"""
    protos = prototypes()
    return [(fn, over, getattr(lib, fn)(*[decode(k, a) for (k, _), a in zip(protos[fn], arguments(protos[fn], over))]))
            for fn, over in SIZE_ZERO]


def all_rows():
    del ROWS[:]
    rnnt_loss_family()
    lattice_family()
    pruned_family()
    simple_family()
    ctc_family()
    joint_family()
    decoder_family()
    ctc_decode_family()
    rnnt_align_family()
    return list(ROWS)


def call(lib, fn, proto, args):
    """(return code, wr_last_error() text) of one encoded call"""
    rc = getattr(lib, fn)(*[decode(k, a) for (k, _), a in zip(proto, args)])
    return rc, lib.wr_last_error().decode()


def main():
    sys.path.insert(0, ROOT)
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    protos = prototypes()
    for fn, over, got in size_zero_answers(lib):
        if got != 0:
            raise SystemExit(f"{fn} {over}: returned {got}, not 0")
    table, seen = [], set()
    for fn, what, over in all_rows():
        args = arguments(protos[fn], over)
        key = json.dumps([fn, args])
        if key in seen:
            continue
        seen.add(key)
        rc, err = call(lib, fn, protos[fn], args)
        if rc in (WR_OK, WR_ELAUNCH) or rc > 0:
            raise SystemExit(f"{fn} {over}: returned {rc} ({err!r}) -- the row reaches a launch, it must not be recorded")
        table.append({"fn": fn, "check": what, "args": args, "rc": rc, "error": err})
    with open(TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in table) + "\n]\n")
    print(f"{len(table)} rows, {len({r['fn'] for r in table})} entry points -> {TABLE}")


if __name__ == "__main__":
    main()
