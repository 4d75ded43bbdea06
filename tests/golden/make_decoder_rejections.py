"""Record what the decoder answers to bad arguments on a LIVE handle: tests/golden/decoder_rejections.json.

    python tests/golden/make_decoder_rejections.py        # needs a GPU; rewrites the table from the library as built

The companion of make_abi_rejections.py (whose prototypes, base values and argument encoding it uses) for the checks
that need a handle: capacities, Tmax, n_steps / blank, the chunk call without stream state, beam limits, the
look-ahead range, the hot-word search before and after wr_decoder_attach_hotword, every limit of the attach call that
this decoder can reach, and a short workspace.  Every row is rejected before the first HIP call of its entry point, so
the placeholder pointers are never read.  tests/test_decode_gpu.py replays the rows on a handle of its own and then
decodes with it.  Run it on the commit whose behaviour is to be kept.

The decoder is the smallest that has every path: V=32, E=P=D=H=16, J=32, one LSTM layer, 4 lanes, 2 utterances,
Tmax=8, 8 tokens, beam 2; the hot-word module dim 16, 2 heads, hw_dim 8, 1 label, lists of at most 2 entries.
"""
import ctypes
import importlib.util
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = os.path.join(HERE, "decoder_rejections.json")
DEV = "cuda:0"
V, E, J, LANES, UTT, TMAX, MAX_HYP, BEAM = 32, 16, 32, 4, 2, 8, 8, 2
HOTWORD_BASE = {"dim": 16, "heads": 2, "hw_dim": 8, "n_labels": 1}
MAX_CTX = 2

_spec = importlib.util.spec_from_file_location("make_abi_rejections", os.path.join(HERE, "make_abi_rejections.py"))
abi = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(abi)
NULLS = abi.NULLS


def HW(**over):
    return {"hotword": over}


def rows_before_attach():
    r = []

    def row(fn, **over):
        r.append((fn, dict(over, h="handle")))
    for fn in ("wr_greedy_search", "wr_greedy_search_chunk"):
        row(fn, N=LANES + 1)                      # lanes
        row(fn, N=UTT + 1)                        # utterances
        row(fn, N=0)
        row(fn, T=TMAX + 1)
        row(fn, T=0)
        row(fn, n_steps=0)
        row(fn, blank=V)
        row(fn, blank=-1)
        row(fn, hyps_d=NULLS)
    row("wr_greedy_search_chunk", reset=0)        # no stream state yet
    row("wr_greedy_search_chunk", reset=0, reference_new_cache=1, N=1)
    fn = "wr_prefix_beam_search"
    row(fn, beam=BEAM + 1)
    row(fn, beam=0)
    row(fn, B=UTT + 1)                            # B * beam over the lanes as well
    row(fn, B=UTT + 1, beam=1)
    row(fn, B=0)
    row(fn, T=TMAX + 1)
    row(fn, blank=V)
    row(fn, ctc_logp_d=NULLS)
    row("wr_predictor_step", N=LANES + 1)
    row("wr_predictor_step", N=0)
    row("wr_predictor_step", out_d=NULLS)
    row("wr_decoder_set_lookahead", frames=5)
    row("wr_decoder_set_lookahead", frames=-1)
    row("wr_greedy_search_hotword")               # before attach
    fn = "wr_decoder_attach_hotword"
    for hw in (HW(dim=0), HW(n_labels=0), HW(dim=32), HW(hw_dim=257), HW(n_labels=9), HW(heads=3), HW(heads=32),
               HW(q_w=NULLS), HW(hw_out_b=NULLS), HW()):
        row(fn, hw=hw)                            # the last one: the base call's workspace of 0 bytes
    row(fn, hw=HW(), max_ctx=0)
    row(fn, hw=HW(), max_ctx=8000)                # the bias kernel's LDS
    row(fn, hw=NULLS)
    row(fn, hw=HW(), workspace_d=NULLS)
    row(fn, hw=HW(), workspace_bytes=4096)
    return r


def rows_after_attach():
    r = []

    def row(**over):
        r.append(("wr_greedy_search_hotword", dict(over, h="handle")))
    row(N=LANES + 1)
    row(N=UTT + 1)
    row(T=TMAX + 1)
    row(n_steps=0)
    row(blank=V)
    row(trace_cap=0)
    row(n_ctx_hot=MAX_CTX + 1)
    row(n_ctx_hot=0)
    row(n_ctx_cold=MAX_CTX + 1)
    row(n_ctx_cold=0)
    row(trace_d=NULLS)
    return r


def modules():
    import torch
    import wenet_celoss_amd as w
    torch.manual_seed(0)
    pred = w.RNNPredictor(V, E, E, 0.0, E, 1).eval()
    joint = w.TransducerJoint(V, E, E, J).eval()
    return pred.to(DEV), joint.to(DEV)


def decoder(pred, joint):
    from wenet_celoss_amd.decoder import DeviceDecoder
    return DeviceDecoder(pred, joint, LANES, UTT, TMAX, MAX_HYP, BEAM)


def hotword_struct(over, keep, real=False):
    """wr_hotword_weights: placeholder pointers (never read by a rejected call), or with `real` zero-filled tensors"""
    import torch
    from wenet_celoss_amd import _lib
    w = _lib.HotwordWeights()
    vals = dict(HOTWORD_BASE, **over)
    assert not set(vals) - {n for n, _ in w._fields_}, vals
    for name, ctype in w._fields_:
        if ctype is ctypes.c_void_p:
            if real:
                keep.append(torch.zeros(2 * vals["dim"] * vals["dim"], device=DEV))
            setattr(w, name, None if vals.get(name) == NULLS else keep[-1].data_ptr() if real else abi.PLACEHOLDER)
        else:
            setattr(w, name, vals[name])
    keep.append(w)
    return ctypes.byref(w)


def answers(dec, rows, keep):
    """[{fn, args, rc, error}] of the encoded calls on the handle of `dec`"""
    protos = abi.prototypes()
    out = []
    for fn, over in rows:
        args = abi.arguments(protos[fn], over)
        real = [dec._h if a == "handle" else hotword_struct(a["hotword"], keep) if isinstance(a, dict) else abi.decode(k, a)
                for (k, _), a in zip(protos[fn], args)]
        rc = getattr(dec._lib, fn)(*real)
        out.append({"fn": fn, "args": args, "rc": rc, "error": dec._lib.wr_last_error().decode()})
    return out


def attach(dec, keep):
    """the real attach, with zero weights: only rejected hot-word searches follow"""
    import torch
    from wenet_celoss_amd import _lib
    hw = hotword_struct({}, keep, real=True)
    nbytes = dec._lib.wr_hotword_workspace_bytes(dec._h, hw, MAX_CTX)
    assert nbytes > 0
    keep.append(torch.empty(nbytes, dtype=torch.uint8, device=DEV))
    with torch.cuda.device(DEV):
        rc = dec._lib.wr_decoder_attach_hotword(dec._h, hw, MAX_CTX, _lib.ptr(keep[-1]), nbytes, _lib.current_stream(DEV))
    _lib.check(rc, "wr_decoder_attach_hotword")


def run(dec):
    """every rejected call, in order, on `dec` (which ends with the hot-word module attached)"""
    keep = []
    dec._rejection_keep = keep
    table = answers(dec, rows_before_attach(), keep)
    attach(dec, keep)
    return table + answers(dec, rows_after_attach(), keep)


def main():
    sys.path.insert(0, abi.ROOT)
    table = run(decoder(*modules()))
    for r in table:
        if r["rc"] not in (-1, -2, -3) or not r["error"]:
            raise SystemExit(f"{r['fn']} {r['args']}: returned {r['rc']} ({r['error']!r}) -- not a rejection")
    with open(TABLE, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in table) + "\n]\n")
    print(f"{len(table)} rows -> {TABLE}")


if __name__ == "__main__":
    main()
