#!/usr/bin/env python3
"""Secondary measurements (SURVEY.md 8d "Secondary"): joiner TFLOP/s, CTC loss+grad utt/s.
Not the headline metric (bench.py is); prints one JSON line per measurement."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, steps, warmup=1):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2]


def bench_joint(args):
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, U1, J, V = args.B, args.T, args.U + 1, 512, args.V
    ep = torch.randn(B, T, J, device=dev); pp = torch.randn(B, U1, J, device=dev)
    w = torch.randn(V, J, device=dev) * 0.05; b = torch.randn(V, device=dev)
    out = torch.empty(B, T, U1, V, device=dev)
    ws_bytes = lib.wr_joint_workspace_bytes(J, V)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    st = _lib.current_stream(dev); P = _lib.ptr
    f = lambda: _lib.check(lib.wr_joint_fwd(P(ep), P(pp), P(w), P(b), None, None, B, T, U1, J, V, 0, P(out), P(ws), ws_bytes, st))
    flops = 2.0 * B * T * U1 * J * V
    ms = timeit(f, args.steps)
    print(json.dumps({"what": "joint_fwd", "shape": [B, T, U1, J, V], "ms": round(ms, 3),
                      "TFLOPs": round(flops / ms / 1e9, 2), "peak_f32_mfma": 157.3,
                      "frac": round(flops / ms / 1e9 / 157.3, 4), "probe": float(out[0, 0, 0, :8].abs().sum())}), flush=True)
    if args.fwd_only:
        return
    # split-precision variants on the bf16 matrix cores, checked against the exact-fp32 logits just computed
    wsb_s = lib.wr_joint_split_workspace_bytes(J, V)
    ws_s = torch.empty(wsb_s, dtype=torch.uint8, device=dev)
    scale = float(out[0, :8].std())
    for terms, odt, code, parts in ((3, torch.float32, 0, 1), (3, torch.float32, 0, 2), (3, torch.float32, 0, 4),
                                    (1, torch.float32, 0, 1), (1, torch.float32, 0, 2), (1, torch.bfloat16, 2, 1), (1, torch.bfloat16, 2, 2)):
        lib.wr_tune_set(7, parts)
        out_s = torch.empty(B, T, U1, V, dtype=odt, device=dev)
        fs = lambda: _lib.check(lib.wr_joint_fwd_split(P(ep), P(pp), P(w), P(b), None, None, B, T, U1, J, V, 0, terms,
                                                       P(out_s), code, P(ws_s), wsb_s, st))
        ms = timeit(fs, args.steps)
        err = float((out_s[:1].float() - out[:1]).abs().max())
        print(json.dumps({"what": "joint_fwd_split", "terms": terms, "parts": parts, "out": str(odt).split(".")[-1],
                          "shape": [B, T, U1, J, V], "ms": round(ms, 3), "TFLOPs_fp32_equiv": round(flops / ms / 1e9, 2),
                          "bf16_TFLOPs": round(terms * flops / ms / 1e9, 1), "frac_of_2500": round(terms * flops / ms / 1e9 / 2500, 4),
                          "max_abs_err_vs_fp32": err, "logit_std": scale, "rel_to_scale": err / scale}), flush=True)
        del out_s
    lib.wr_tune_set(7, 0)
    # the single-term forward with bf16 operands (wr_joint_fwd_split, terms=1) and with f16 operands (wr_joint_fwd_f16) on
    # the same shape, bf16 / f16 logits (the fp16-autocast configuration), alternating in one process; default launch form
    out16 = torch.empty(B, T, U1, V, dtype=torch.bfloat16, device=dev)
    outh = torch.empty(B, T, U1, V, dtype=torch.float16, device=dev)
    fb = lambda: _lib.check(lib.wr_joint_fwd_split(P(ep), P(pp), P(w), P(b), None, None, B, T, U1, J, V, 0, 1, P(out16),
                                                   _lib.WR_BF16, P(ws_s), wsb_s, st))
    fh = lambda: _lib.check(lib.wr_joint_fwd_f16(P(ep), P(pp), P(w), P(b), None, None, B, T, U1, J, V, 0, P(outh),
                                                 _lib.WR_F16, P(ws_s), wsb_s, st))
    for rep_ in range(2):
        for name, fn, o in (("bf16", fb, out16), ("f16", fh, outh)):
            ms = timeit(fn, args.steps)
            err = float((o[:1].float() - out[:1]).abs().max())
            print(json.dumps({"what": "joint_fwd_single_term", "operands": name, "logits": str(o.dtype).split(".")[-1],
                              "rep": rep_, "shape": [B, T, U1, J, V], "ms": round(ms, 3), "TFLOPs": round(flops / ms / 1e9, 1),
                              "max_abs_err_vs_fp32": err, "rel_to_scale": err / scale}), flush=True)
    del out16, outh
    dz = torch.empty(B, T, U1, J, device=dev); h = torch.empty_like(dz)
    g = lambda: _lib.check(lib.wr_joint_bwd_dz(P(out), P(ep), P(pp), P(w), None, None, B, T, U1, J, V, 0, P(dz), P(h), st))
    dz_blocks = None
    for blocks in (1, 0):                              # knob 10: 0 = 256 x 256 block tiling (default), 1 = 64-cell tiling
        lib.wr_tune_set(10, 0 if blocks else 1)
        ms = timeit(g, args.steps)
        rec = {"what": "joint_bwd_dz", "tiling": "blocks" if blocks else "cells64", "shape": [B, T, U1, J, V], "ms": round(ms, 3),
               "TFLOPs": round(flops / ms / 1e9, 2), "frac": round(flops / ms / 1e9 / 157.3, 4)}
        if blocks:
            dz_blocks = dz[:1].clone()
        else:
            rec["max_abs_diff_blocks_vs_cells64"] = float((dz[:1] - dz_blocks).abs().max())
        print(json.dumps(rec), flush=True)
    lib.wr_tune_set(10, 0)
    wsz = lib.wr_joint_dz_split_workspace_bytes(J, V)
    wz = torch.empty(wsz, dtype=torch.uint8, device=dev)
    dz_ref = dz.clone()
    for terms in (3, 1):
        gs = lambda: _lib.check(lib.wr_joint_bwd_dz_split(P(out), P(ep), P(pp), P(w), None, None, B, T, U1, J, V, 0, terms,
                                                           P(dz), P(h), P(wz), wsz, st))
        ms = timeit(gs, args.steps)
        err = float((dz[:1] - dz_ref[:1]).abs().max())
        print(json.dumps({"what": "joint_bwd_dz_split", "terms": terms, "shape": [B, T, U1, J, V], "ms": round(ms, 3),
                          "TFLOPs_fp32_equiv": round(flops / ms / 1e9, 2), "max_abs_err_vs_fp32": err,
                          "dz_rms": float(dz_ref[:1].pow(2).mean().sqrt())}), flush=True)
    g()
    wsb2 = lib.wr_joint_dw_workspace_bytes(J, V)
    ws2 = torch.empty(wsb2, dtype=torch.uint8, device=dev)
    dwt = torch.empty(V, J, device=dev); dbt = torch.empty(V, device=dev)
    kdw = lambda: _lib.check(lib.wr_joint_bwd_dw(P(out), P(h), None, None, B, T, U1, J, V, P(dwt), P(dbt), P(ws2), wsb2, st))
    for slabs in (1, 0):                               # knob 9: 1 = first tiling (128-row slabs), 0 = 256 x 256 blocks (default)
        lib.wr_tune_set(9, slabs)
        ms = timeit(kdw, args.steps)
        print(json.dumps({"what": "joint_bwd_dw", "tiling": "slabs" if slabs else "blocks", "shape": [B, T, U1, J, V],
                          "ms": round(ms, 3), "TFLOPs": round(flops / ms / 1e9, 2),
                          "frac": round(flops / ms / 1e9 / 157.3, 4)}), flush=True)
    dw_ref, db_ref = dwt.clone(), dbt.clone()
    wsb3 = lib.wr_joint_dw_split_workspace_bytes(B, T, U1, J, V)
    ws3 = torch.empty(wsb3, dtype=torch.uint8, device=dev)
    for terms in (3, 1):
        ks = lambda: _lib.check(lib.wr_joint_bwd_dw_split(P(out), P(h), None, None, B, T, U1, J, V, terms, P(dwt), P(dbt),
                                                           P(ws3), wsb3, st))
        ms = timeit(ks, args.steps)
        rms = float(dw_ref.pow(2).mean().sqrt())
        print(json.dumps({"what": "joint_bwd_dw_split", "terms": terms, "shape": [B, T, U1, J, V], "ms": round(ms, 3),
                          "TFLOPs_fp32_equiv": round(flops / ms / 1e9, 2),
                          "max_err_over_rms": float((dwt - dw_ref).abs().max()) / rms,
                          "db_max_err_over_rms": float((dbt - db_ref).abs().max() / db_ref.pow(2).mean().sqrt())}), flush=True)
    if args.dw:
        # yardstick, not product: the library's fp32 GEMM (hipBLASLt / rocBLAS through torch) on the three contractions
        g2, h2 = out.view(-1, V), h.view(-1, J)
        dz2 = dz.view(-1, J)
        for name, k in (("forward  H @ W^T + b", lambda: torch.addmm(b, h2, w.t(), out=g2)),
                        ("dZ       dY @ W", lambda: torch.mm(g2, w, out=dz2)),
                        ("dW       dY^T @ H", lambda: g2.t().mm(h2))):
            ms = timeit(k, max(1, args.steps // 2))
            print(json.dumps({"what": "library fp32 GEMM (yardstick)", "contraction": name, "ms": round(ms, 3),
                              "TFLOPs": round(flops / ms / 1e9, 2), "frac": round(flops / ms / 1e9 / 157.3, 4)}), flush=True)


def bench_ctc(args):
    import wenet_celoss_amd as wc
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B, T, S, V = 32, 1000, 150, 5000
    x = torch.randn(B, T, V, device=dev)
    y = torch.randint(1, V, (B, S), dtype=torch.int32, device=dev)
    il = torch.full((B,), T, dtype=torch.int32, device=dev); tl = torch.full((B,), S, dtype=torch.int32, device=dev)
    ws_bytes = lib.wr_ctc_workspace_bytes(B, T, S)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    nll = torch.empty(B, device=dev); g = torch.empty_like(x); go = torch.full((B,), 1.0 / B, device=dev)
    st = _lib.current_stream(dev); P = _lib.ptr

    def step():
        _lib.check(lib.wr_ctc_loss_fwd(P(x), 0, P(y), P(il), P(tl), B, T, S, V, 0, P(nll), P(ws), ws_bytes, st))
        _lib.check(lib.wr_ctc_loss_bwd(P(x), 0, P(y), P(il), P(tl), B, T, S, V, 0, P(go), P(g), P(ws), ws_bytes, st))
    ms = timeit(step, 20, warmup=3)
    # CPU reference, exactly the reference's call (ctc.py:60-61), on the host cores
    import time
    xc = x.cpu().requires_grad_(True)
    torch.set_num_threads(min(os.cpu_count(), 16))
    t0 = time.perf_counter()
    for _ in range(3):
        lp = xc.transpose(0, 1).log_softmax(2)
        l = torch.nn.CTCLoss(reduction="sum")(lp, y.cpu().long(), il.cpu().long(), tl.cpu().long()) / B
        l.backward()
    cpu_ms = (time.perf_counter() - t0) / 3 * 1e3
    print(json.dumps({"what": "ctc_loss+grad", "shape": [B, T, S, V], "ms": round(ms, 4), "utt_per_s": round(B / ms * 1e3, 1),
                      "GBps_algorithmic(3*4*T*B*V)": round(3 * 4.0 * T * B * V / ms / 1e6, 1),
                      "steps_per_s": round(T / ms * 1e3), "cpu_torch_ctcloss_ms": round(cpu_ms, 1),
                      "cpu_utt_per_s": round(B / cpu_ms * 1e3, 1), "cpu_threads": torch.get_num_threads()}), flush=True)


def bench_ctcdec(args):
    """CTC decode modes and forced alignment from the ctc_lo output on: B=16, T=1500, V=5000."""
    import time
    import wenet_celoss_amd as wc
    from oracle import decode_oracle as do
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    B, T, V, S = (args.B if args.B != 32 else 16), (args.T if args.T != 1000 else 1500), 5000, 150
    x = torch.randn(B, T, V, device=dev) * 3
    x[..., 0] += 14.0                                  # blank-heavy, like a trained CTC head (about one label per 12 frames)
    lens = torch.full((B,), T)
    y = torch.randint(1, V, (B, S))

    def timed(fn, n):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n, r

    dt, (hyps, _) = timed(lambda: wc.ctc_greedy_search(x, lens), args.steps)
    print(json.dumps({"what": "ctc_greedy_search", "B": B, "T": T, "V": V, "ms_per_call": round(dt * 1e3, 3),
                      "utt_per_s": round(B / dt, 1), "frames_per_s": round(B * T / dt), "tokens": sum(len(h) for h in hyps)}), flush=True)
    dt, res = timed(lambda: wc.ctc_prefix_beam_search(x, lens, 10), args.steps)
    print(json.dumps({"what": "ctc_prefix_beam_search", "beam": 10, "B": B, "T": T, "V": V, "ms_per_call": round(dt * 1e3, 3),
                      "utt_per_s": round(B / dt, 1), "frames_per_s": round(B * T / dt), "best_len": len(res[0][0][0])}), flush=True)
    dt, ali = timed(lambda: wc.forced_align_batch(x, y, lens, torch.full((B,), S)), args.steps)
    print(json.dumps({"what": "ctc_forced_align", "B": B, "T": T, "S": S, "ms_per_call": round(dt * 1e3, 3),
                      "utt_per_s": round(B / dt, 1), "frames_per_s": round(B * T / dt)}), flush=True)
    # CPU: the numpy restatement of the reference's prefix beam search on one utterance of 200 frames
    lp = do.log_softmax(x[0, :200].cpu().numpy())
    t0 = time.perf_counter()
    ref = do.ctc_prefix_beam_search(lp, 200, 10)
    cdt = time.perf_counter() - t0
    print(json.dumps({"what": "ctc_prefix_beam_search_cpu_oracle", "frames": 200, "s": round(cdt, 3),
                      "frames_per_s": round(200 / cdt)}), flush=True)


def bench_ctcstream(args):
    """Streaming CTC prefix beam search at the BASELINE CTC shape (B=32, T=1000, V=5000, beam=10), in one run: the
    existing whole-utterance search, the streaming entry point in one chunk, and in 16-frame chunks (total and per
    chunk).  Device time of the raw entry points on preallocated buffers (median of event timings), then the Python
    wrappers end to end (they also copy the n-best to the host)."""
    import time
    import wenet_celoss_amd as wc
    from wenet_celoss_amd import _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    B, T, V, beam, W = args.B, args.T, args.V, 10, 16
    x = torch.randn(B, T, V, device=dev) * 3
    x[..., 0] += 14.0                                  # blank-heavy, like a trained CTC head (about one label per 12 frames)
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    base = {"B": B, "T": T, "V": V, "beam": beam}
    i32 = dict(dtype=torch.int32, device=dev)
    hl, nh, nf = torch.empty(B, beam, **i32), torch.empty(B, **i32), torch.empty(B, **i32)
    sc, vt = torch.empty(B, beam, dtype=torch.float64, device=dev), torch.empty(B, beam, dtype=torch.float64, device=dev)
    hyps, tm = torch.empty(B, beam, T, **i32), torch.empty(B, beam, T, **i32)

    ws0 = _lib.workspace("wr_ctc_decode_workspace_bytes", B, T, beam, device=dev)
    ms = timeit(lambda: _lib.call("wr_ctc_prefix_beam_search", x, lens, B, T, V, beam, 0, hyps, hl, sc, nh, ws0, ws0.numel(),
                                  device=dev), args.steps)
    old = (hyps.clone(), hl.clone(), sc.clone(), nh.clone())
    print(json.dumps({"what": "wr_ctc_prefix_beam_search", **base, "ms_per_call": round(ms, 3),
                      "frames_per_s": round(B * T / ms * 1e3)}), flush=True)

    state = _lib.workspace("wr_ctc_stream_state_bytes", B, beam, T, device=dev)
    ws1 = _lib.workspace("wr_ctc_stream_workspace_bytes", B, T, beam, device=dev)

    def chunk(xc, ln, Tc, reset, done, ws):
        _lib.call("wr_ctc_prefix_beam_search_chunk", xc, ln, B, Tc, V, beam, 0, reset, done, T, state, state.numel(), hyps, hl,
                  sc, vt, tm, nh, nf, ws, ws.numel(), device=dev)

    ms1 = timeit(lambda: chunk(x, lens, T, 1, 0, ws1), args.steps)
    same = all(torch.equal(a, b) for a, b in zip(old, (hyps, hl, sc, nh)))
    one = (hyps.clone(), hl.clone(), sc.clone(), vt.clone(), tm.clone())
    print(json.dumps({"what": "wr_ctc_prefix_beam_search_chunk, one chunk", **base, "ms_per_call": round(ms1, 3),
                      "frames_per_s": round(B * T / ms1 * 1e3), "vs_existing": round(ms1 / ms, 3),
                      "bit_identical_to_existing": same}), flush=True)

    parts = [x[:, t0:t0 + W].contiguous() for t0 in range(0, T, W)]
    plens = [torch.full((B,), p.shape[1], dtype=torch.int32, device=dev) for p in parts]
    wsc = _lib.workspace("wr_ctc_stream_workspace_bytes", B, W, beam, device=dev)

    def chunked():
        done = 0
        for p, ln in zip(parts, plens):
            chunk(p, ln, p.shape[1], int(done == 0), done, wsc)
            done += p.shape[1]

    msc = timeit(chunked, args.steps)
    same = all(torch.equal(a, b) for a, b in zip(one, (hyps, hl, sc, vt, tm)))
    print(json.dumps({"what": "wr_ctc_prefix_beam_search_chunk, 16-frame chunks", **base, "chunks": len(parts),
                      "ms_total": round(msc, 3), "ms_per_chunk": round(msc / len(parts), 4),
                      "frames_per_s": round(B * T / msc * 1e3), "vs_one_chunk": round(msc / ms1, 3),
                      "bit_identical_to_one_chunk": same}), flush=True)

    def timed(fn, n):
        fn(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    def stream_py():
        s = wc.CtcPrefixBeamStream(B, beam, T)
        for p, ln in zip(parts, plens):
            s.search(p, ln)

    print(json.dumps({"what": "python wrappers end to end", **base,
                      "ctc_prefix_beam_search_ms": round(timed(lambda: wc.ctc_prefix_beam_search(x, lens, beam), args.steps), 3),
                      "ctc_prefix_beam_search_times_ms": round(timed(lambda: wc.ctc_prefix_beam_search_times(x, lens, beam),
                                                                     args.steps), 3),
                      "CtcPrefixBeamStream_16_frame_chunks_ms": round(timed(stream_py, args.steps), 3)}), flush=True)


def bench_ctcctx(args):
    """The biased chunk call beside the plain one on the shape of `ctcstream` (B=32 streams x T=1000 frames, V=5000,
    beam 10, 16-frame chunks), the graph 1000 random 3-token phrases: device time of the raw entry points on preallocated
    buffers (median of event timings), in one chunk and in 16-frame chunks, and the biased call again with an empty
    graph, which isolates what the added state traffic and export cost from what the arc lookups cost."""
    import numpy as np
    import wenet_celoss_amd as wc
    from wenet_celoss_amd import _lib
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    B, T, V, beam, W = args.B, args.T, args.V, 10, 16
    x = torch.randn(B, T, V, device=dev) * 3
    x[..., 0] += 14.0                                  # the input of bench_ctcstream
    lens = torch.full((B,), T, dtype=torch.int32, device=dev)
    base = {"B": B, "T": T, "V": V, "beam": beam}
    i32, f64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float64, device=dev)
    hl, cs, nh, nf = torch.empty(B, beam, **i32), torch.empty(B, beam, **i32), torch.empty(B, **i32), torch.empty(B, **i32)
    sc, vt, cc, cx = (torch.empty(B, beam, **f64) for _ in range(4))
    hyps, tm, tg = (torch.empty(B, beam, T, **i32) for _ in range(3))
    rng = np.random.default_rng(11)
    graph = wc.ContextGraph(rng.integers(1, V, size=(1000, 3)).tolist(), 3.0)
    empty = wc.ContextGraph([])
    state = _lib.workspace("wr_ctc_stream_state_bytes", B, beam, T, device=dev)
    cstate = _lib.workspace("wr_ctc_context_stream_state_bytes", B, beam, T, device=dev)

    def plain(xc, ln, Tc, reset, done, ws):
        _lib.call("wr_ctc_prefix_beam_search_chunk", xc, ln, B, Tc, V, beam, 0, reset, done, T, state, state.numel(), hyps, hl,
                  sc, vt, tm, nh, nf, ws, ws.numel(), device=dev)

    def biased(g):
        def call(xc, ln, Tc, reset, done, ws):
            _lib.call("wr_ctc_prefix_beam_search_context_chunk", xc, ln, B, Tc, V, beam, 0, reset, done, T, cstate,
                      cstate.numel(), *g.to(dev), g.n_states, g.n_arcs, 0, hyps, hl, sc, vt, tm, nh, nf, cc, cx, tg, cs, ws,
                      ws.numel(), device=dev)
        return call

    ws1 = _lib.workspace("wr_ctc_stream_workspace_bytes", B, T, beam, device=dev)
    wsc = _lib.workspace("wr_ctc_stream_workspace_bytes", B, W, beam, device=dev)
    parts = [x[:, t0:t0 + W].contiguous() for t0 in range(0, T, W)]
    plens = [torch.full((B,), p.shape[1], dtype=torch.int32, device=dev) for p in parts]

    def chunked(call):
        done = 0
        for p, ln in zip(parts, plens):
            call(p, ln, p.shape[1], int(done == 0), done, wsc)
            done += p.shape[1]

    rows = {}
    for name, call in (("plain", plain), ("biased", biased(graph)), ("biased, empty graph", biased(empty))):
        one = timeit(lambda: call(x, lens, T, 1, 0, ws1), args.steps)
        ref = (hyps.clone(), sc.clone())
        many = timeit(lambda: chunked(call), args.steps)
        rows[name] = (one, many)
        extra = {}
        if name != "plain":
            extra = {"one_chunk_vs_plain": round(one / rows["plain"][0], 3), "chunks_vs_plain": round(many / rows["plain"][1], 3),
                     "chunked_bit_identical_to_one_chunk": bool(torch.equal(ref[0], hyps) and torch.equal(ref[1], sc))}
        if name == "biased":
            extra.update({"states": graph.n_states, "arcs": graph.n_arcs, "hyps_with_a_bonus": int((cx != 0).sum()),
                          "tokens_per_hyp": round(float(hl.float().mean()), 1)})
        print(json.dumps({"what": f"ctc prefix beam chunk call, {name}", **base, "one_chunk_ms": round(one, 3),
                          "chunks": len(parts), "chunks_ms_total": round(many, 3), "ms_per_chunk": round(many / len(parts), 4),
                          **extra}), flush=True)


def bench_greedy(args):
    """BASELINE config 3: B=64 streams, chunks of 16 encoder frames, V=5000, LSTM 2x256, J=512, n_steps=64."""
    import time
    import types
    import wenet_celoss_amd as w
    from oracle import decode_oracle as do
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    V, E, P, J, H, L, N = 5000, 256, 256, 512, 256, 2, args.streams
    T = 16 * args.chunks
    pred = w.RNNPredictor(V, P, P, 0.1, H, L).to(dev).eval()
    joint = w.TransducerJoint(V, E, P, J).to(dev).eval()
    with torch.no_grad():
        joint.ffn_out.weight *= 10
        joint.ffn_out.bias[0] += 16.0
    model = types.SimpleNamespace(blank=0, predictor=pred, joint=joint)
    enc = torch.randn(N, T, E, device=dev)
    lens = torch.full((N,), T)
    for use_graph in (True, False):
        hyps = w.basic_greedy_search(model, enc, lens, n_steps=64)          # builds the handle / graph
        model._decoder_cache._dec.set_graph(use_graph)
        w.basic_greedy_search(model, enc, lens, n_steps=64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            hyps = w.basic_greedy_search(model, enc, lens, n_steps=64)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        ntok = sum(len(h) for h in hyps)
        micro = ntok + N * T                                     # joiner evaluations actually needed
        print(json.dumps({"what": "greedy_search", "hipGraph": use_graph, "streams": N, "frames": T, "tokens": ntok,
                          "ms_per_call": round(dt * 1e3, 3), "utt_per_s": round(N / dt, 1),
                          "lane_steps_per_s": round(micro / dt)}), flush=True)
    # look-ahead: frames per micro-step (token sequences must not change).  Second scenario shaped like speech: most
    # frames quiet (blank), a quarter of them loud, at most 2 symbols per frame -> about one token per five frames
    # (the dense scenario above keeps emitting until n_steps stops it, which no trained model does).
    scenarios = [("dense", enc, 64, 0.0)]
    gq = torch.Generator(device=dev).manual_seed(11)
    quiet = torch.randn(N, T, E, device=dev, generator=gq) * 0.1
    loud = torch.randn(N, T, E, device=dev, generator=gq) * 2.5
    spikes = torch.rand(N, T, device=dev, generator=gq) < 0.25
    scenarios.append(("speech-like", torch.where(spikes[..., None], loud, quiet), 2, 1.0))
    for name, e_s, n_steps_s, extra_blank in scenarios:
        with torch.no_grad():
            joint.ffn_out.bias[0] += extra_blank
        m_s = types.SimpleNamespace(blank=0, predictor=pred, joint=joint)
        ref_hyps = w.basic_greedy_search(m_s, e_s, lens, n_steps=n_steps_s)
        for look in (1, 2, 4, 0):                      # 0: adaptive
            dec = m_s._decoder_cache._dec
            dec.set_lookahead(look)
            got = w.basic_greedy_search(m_s, e_s, lens, n_steps=n_steps_s)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                got = w.basic_greedy_search(m_s, e_s, lens, n_steps=n_steps_s)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) / args.steps
            print(json.dumps({"what": "greedy_search_lookahead", "scenario": name, "frames_per_micro_step": look,
                              "streams": N, "frames": T, "n_steps": n_steps_s, "tokens": sum(len(h) for h in got),
                              "max_tokens_per_stream": max(len(h) for h in got), "ms_per_call": round(dt * 1e3, 3),
                              "utt_per_s": round(N / dt, 1), "tokens_identical": got == ref_hyps}), flush=True)
        with torch.no_grad():
            joint.ffn_out.bias[0] -= extra_blank
        m_s._decoder_cache._dec.set_lookahead(0)
    # CPU reference: the reference's loop restated in numpy (oracle), one stream, scaled to 64
    p = do.Predictor({k: v.detach().cpu().numpy() for k, v in pred.state_dict().items()}, L)
    j = do.Joint({k: v.detach().cpu().numpy() for k, v in joint.state_dict().items()})
    t0 = time.perf_counter()
    ref = do.greedy_search(p, j, enc[0].cpu().numpy(), T, n_steps=64)
    cdt = time.perf_counter() - t0
    print(json.dumps({"what": "greedy_search_cpu_oracle", "one_stream_s": round(cdt, 3), "utt_per_s": round(1 / cdt, 2),
                      "tokens_match": ref == hyps[0]}), flush=True)


def bench_beam(args):
    """BASELINE config 5: beam=8, B=16, T=1500, V=5000."""
    import time
    import wenet_celoss_amd as w
    dev = torch.device("cuda:0")
    torch.manual_seed(6)
    V, E, P, J, H, L, B, T, beam = 5000, 256, 256, 512, 256, 2, args.B if args.B != 32 else 16, args.T if args.T != 1000 else 1500, 8
    pred = w.RNNPredictor(V, P, P, 0.1, H, L).to(dev).eval()
    joint = w.TransducerJoint(V, E, P, J).to(dev).eval()
    ctc = w.CTC(V, E).to(dev).eval()
    with torch.no_grad():
        joint.ffn_out.weight *= 10
        joint.ffn_out.bias[0] += 16.0
    bs = w.PrefixBeamSearch(None, pred, joint, ctc, 0)
    enc = torch.randn(B, T, E, device=dev)
    lens = torch.full((B,), T, dtype=torch.int32)
    for use_graph in (True, False):
        out = bs.search_encoded(enc, lens, beam_size=beam)
        bs._decoder_cache._dec.set_graph(use_graph)
        bs.search_encoded(enc, lens, beam_size=beam)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = bs.search_encoded(enc, lens, beam_size=beam)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        print(json.dumps({"what": "prefix_beam_search", "hipGraph": use_graph, "B": B, "T": T, "beam": beam,
                          "ms_per_call": round(dt * 1e3, 2), "frames_per_s": round(B * T / dt),
                          "utt_per_s": round(B / dt, 2), "best_len": len(out[0][0].hyp)}), flush=True)


def bench_hotword(args):
    """Hot-word greedy search (the fork's default decode path, greedy_search.py:297-430) at the shipped dimensions:
    the loop on the device (gate table + fused predictor biasing + state machine in the update kernel, hipGraph) next
    to the host-driven loop of round 1, one utterance as the reference decodes, and several streams together."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
    from context_bias_mirror import ContextBiasMirror
    import wenet_celoss_amd as w
    from wenet_celoss_amd.hotword import greedy_search_both_device
    dev = torch.device("cuda:0")
    torch.manual_seed(12)
    V, D, J, H, L, HW, T = args.V, 256, 512, 256, 2, 100, args.T
    pred = w.RNNPredictor(V, D, D, 0.1, H, L).eval()
    joint = w.TransducerJoint(V, D, D, J).eval()
    cb = ContextBiasMirror(V, D, layers=1, heads=4, hw_dim=HW, hw_heads=4).eval()
    with torch.no_grad():
        joint.ffn_out.weight *= 10
        joint.ffn_out.bias[0] += 10.0
        cb.hw_output_layer_enc.weight.mul_(6.0)
        cb.hw_output_layer.weight.mul_(4.0)
    n_ctx = 50
    ctx = torch.randint(1, V, (n_ctx, 6)); ctx_len = torch.randint(2, 7, (n_ctx,)).to(torch.int32); ctx[0, 0] = 0; ctx_len[0] = 1
    m = w.Transducer(V, 0, torch.nn.Identity(), pred.to(dev), joint.to(dev), context_bias=cb.to(dev), ctc_weight=0.0,
                     transducer_weight=1.0, loss_mode="both")
    for N in (1, args.streams):
        enc = torch.randn(N, T, D, device=dev)
        lens = torch.full((N,), T)
        run = lambda: greedy_search_both_device(m, enc, lens, ctx, ctx_len, n_steps=args.n_steps, filter_on=True)
        hyps, traces = run()
        ms = timeit(run, args.steps)
        ntok = sum(len(h) for h in hyps)
        decisions = ntok + N * T                       # lower bound: go-back re-decodes more
        print(json.dumps({"what": "hotword_greedy device", "streams": N, "T": T, "V": V, "n_ctx": n_ctx, "ms_per_call": round(ms, 2),
                          "tokens": ntok, "gate_zeros": sum(t.count(0) for t in traces), "gate_ones": sum(t.count(1) for t in traces),
                          "us_per_decision": round(ms * 1e3 / (decisions / N), 1), "utt_per_s": round(N / ms * 1e3, 1)}), flush=True)
    os.environ["WR_HOTWORD_HOST"] = "1"
    enc = torch.randn(1, T, D, device=dev)
    run = lambda: w.basic_greedy_search_both(m, enc, torch.tensor(T), ctx, ctx_len, n_steps=args.n_steps, context_filter_state="on",
                                             context_decoder_labels_padded=torch.zeros(1, 4, dtype=torch.long))
    out = run()
    ms = timeit(run, max(1, args.steps // 2))
    print(json.dumps({"what": "hotword_greedy host-driven (round 1)", "streams": 1, "T": T, "ms_per_call": round(ms, 2),
                      "tokens": len(out[0][0]), "us_per_decision": round(ms * 1e3 / (len(out[0][0]) + T), 1)}), flush=True)
    os.environ.pop("WR_HOTWORD_HOST")


def latency_settings(args):
    """step: (fastemit_lambda, delay_penalty) pairs timed beside (0, 0) when --fastemit-lambda / --delay-penalty are given"""
    out = [(0.0, 0.0)]
    if args.fastemit_lambda > 0:
        out.append((args.fastemit_lambda, 0.0))
    if args.delay_penalty > 0:
        out.append((0.0, args.delay_penalty))
    return out if len(out) > 1 else []


def alternating(fns, reps):
    """{key: (median, min, max) ms} of the callables `fns`, one run of each in turn, `reps` rounds after one warm-up"""
    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    runs = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            runs[k].append(a.elapsed_time(b))
    return {k: (sorted(v)[len(v) // 2], min(v), max(v)) for k, v in runs.items()}


def bench_grad_pass_latency(args, settings):
    """The gradient pass alone (wr_rnnt_loss_bwd / wr_rnnt_loss_bwd_lattice on fp32 logits, separate gradient buffer) at
    each setting, alternating, with the share of dead and faint rows: the kernel's three bounds (rnnt_loss.hip) evaluated
    in float64 from the exported lattice and the log-probabilities of the logits."""
    import math
    from wenet_celoss_amd import _lib
    dev = torch.device("cuda:0")
    B, T, U, V = args.B, args.T, args.U, args.V
    U1 = U + 1
    torch.manual_seed(3)
    logits = torch.empty(B, T, U1, V, device=dev)
    for b in range(B):
        logits[b].normal_()
    grads = torch.empty_like(logits)
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=dev)
    ll = torch.full((B,), T, dtype=torch.int32, device=dev); tl = torch.full((B,), U, dtype=torch.int32, device=dev)
    gc = torch.full((B,), 1.0 / B, device=dev)
    blank_lp = torch.empty(B, T, U1, dtype=torch.float64, device=dev)
    emit_lp = torch.zeros(B, T, U1, dtype=torch.float64, device=dev)
    for b in range(B):
        for t0 in range(0, T, 100):
            x = logits[b, t0:t0 + 100]
            d = torch.logsumexp(x, -1)
            blank_lp[b, t0:t0 + 100] = (x[..., 0] - d).double()
            emit_lp[b, t0:t0 + 100, :U] = (x[:, :U].gather(-1, y[b].long()[None, :, None].expand(x.shape[0], U, 1))[..., 0]
                                           - d[:, :U]).double()
    fns, shares = {}, {}
    for lam, pen in settings:
        ws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
        costs = torch.empty(B, device=dev)
        _lib.call("wr_rnnt_loss_fwd_lattice", logits, _lib.WR_F32, y, ll, tl, B, T, U1, V, 0, 0, pen, costs, ws, ws.numel(),
                  device=dev)
        alpha = torch.empty(B, T, U1, device=dev); beta = torch.empty_like(alpha)
        _lib.call("wr_rnnt_export_lattice", ws, ws.numel(), ll, tl, B, T, U1, alpha, beta, device=dev)
        alpha, beta = alpha.double(), beta.double()
        ninf = torch.full_like(beta[:, :1], -math.inf)
        b1 = torch.cat([beta[:, 1:], ninf], 1)                              # beta(t+1, u)
        b2 = torch.cat([beta[:, :, 1:], torch.full_like(beta[:, :, :1], -math.inf)], 2)    # beta(t, u+1)
        ac = alpha + costs.double()[:, None, None]
        tt = torch.arange(T, device=dev, dtype=torch.float64)[None, :, None]
        em = emit_lp + pen * ((T - 1) / 2.0 - tt)
        has_lab = torch.arange(U1, device=dev)[None, None, :] < U
        be_eff = torch.logaddexp(beta, math.log(lam) + em + b2) if lam > 0 else beta
        be_eff = torch.where(has_lab, be_eff, beta)
        thr = -93.3
        main_dead = ac + be_eff < thr
        final = torch.zeros(B, T, U1, dtype=torch.bool, device=dev); final[:, T - 1, U] = True
        blank_bound = torch.where(final, ac, ac + b1)
        blank_dead = (blank_bound < thr) | ((tt == T - 1) & ~final)
        label_dead = ~has_lab | (ac + b2 + pen * ((T - 1) / 2.0 - tt) + math.log1p(lam) < thr)
        n = float(B * T * U1)
        shares[(lam, pen)] = (float((main_dead & blank_dead & label_dead).sum()) / n,
                              float((main_dead & ~(blank_dead & label_dead)).sum()) / n)
        if lam == 0.0 and pen == 0.0:
            fns[(lam, pen)] = lambda ws=ws: _lib.call("wr_rnnt_loss_bwd", logits, _lib.WR_F32, y, ll, tl, B, T, U1, V, 0, -1.0,
                                                      gc, grads, ws, ws.numel(), device=dev)
        else:
            fns[(lam, pen)] = lambda ws=ws, lam=lam, pen=pen: _lib.call(
                "wr_rnnt_loss_bwd_lattice", logits, _lib.WR_F32, y, ll, tl, B, T, U1, V, 0, -1.0, 0, pen, lam, gc, grads, ws,
                ws.numel(), device=dev)
    for (lam, pen), (med, lo, hi) in alternating(fns, args.reps).items():
        print(json.dumps({"what": "rnnt gradient pass (fp32 logits, separate buffer)", "shape": [B, T, U1, V],
                          "fastemit_lambda": lam, "delay_penalty": pen, "ms": round(med, 3), "ms_min": round(lo, 3),
                          "ms_max": round(hi, 3), "reps": args.reps, "dead_share": round(shares[(lam, pen)][0], 4),
                          "faint_share": round(shares[(lam, pen)][1], 4)}), flush=True)
    del logits, grads


def bench_step(args):
    """The loss block of Transducer.forward (transducer.py:131-147) through the autograd path: pre-join
    projections -> joiner -> RNN-T loss -> backward to enc/pred outputs and all joiner weights.
    --fastemit-lambda / --delay-penalty: also the gradient pass alone and every configuration's step at (0, 0),
    (lambda, 0) and (0, delta), alternating, median of --reps with min and max."""
    import wenet_celoss_amd as w
    settings = latency_settings(args)
    if settings:
        bench_grad_pass_latency(args, settings)
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    B, T, U, V, E, P, J = args.B, args.T, args.U, args.V, 256, 256, 512
    enc = torch.randn(B, T, E, device=dev, requires_grad=True)
    pred = torch.randn(B, U + 1, P, device=dev, requires_grad=True)
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=dev)
    ll = torch.full((B,), T, dtype=torch.int32, device=dev); tl = torch.full((B,), U, dtype=torch.int32, device=dev)
    if args.ragged:                                    # utterances sorted by frames (processor.py:704), label counts spread
        gcpu = torch.Generator().manual_seed(5)
        ll = torch.sort(torch.randint(int(0.8 * T), T + 1, (B,), generator=gcpu), descending=True).values.to(torch.int32).to(dev)
        tl = torch.randint(U // 3, U + 1, (B,), generator=gcpu).to(torch.int32).to(dev)
        ll[0], tl[-1] = T, U
    base = None
    precs = ("fp32", "fp32-fused", "bf16x3", "bf16x3-fused", "bf16-autocast", "bf16-autocast-f16", "f16-autocast-f16")
    if args.budget_mb:                                 # the memory-bounded node beside the one that keeps the logits
        precs = ("fp32-fused", "fp32-bounded", "bf16x3-fused", "bf16x3-bounded")
    if args.only:
        precs = tuple(x for x in precs if x in args.only.split(","))
    for prec in precs:
        amp = "-autocast" in prec                      # the --use_amp configuration (executor.py:91)
        adt = torch.float16 if prec.endswith("-f16") else torch.bfloat16      # "-f16": fp16 autocast, the reference's default
        bounded = prec.endswith("-bounded")            # the same node without a logits tensor (logits_budget)
        fused = prec.endswith("-fused") or bounded     # joiner + loss as one node (fused.py): no pass 1, gradient in place
        jprec = prec.split("-")[0] if amp else prec.replace("-fused", "").replace("-bounded", "")
        budget = int(args.budget_mb * (1 << 20)) if bounded else None
        joint = w.TransducerJoint(V, E, P, J, precision=jprec).to(dev)
        torch.manual_seed(4)
        with torch.no_grad():
            for prm in joint.parameters():
                prm.copy_(torch.randn_like(prm) * 0.05)

        def step(**kw):
            joint.zero_grad(set_to_none=True); enc.grad = None; pred.grad = None
            with torch.autocast("cuda", dtype=adt, enabled=amp):
                if fused:
                    loss = w.joint_rnnt_loss(joint.enc_ffn(enc), joint.pred_ffn(pred), joint.ffn_out.weight,
                                             joint.ffn_out.bias, y, ll, tl, blank=0, reduction="mean", precision=jprec,
                                             buckets=args.buckets, logits_budget=budget, **kw)
                else:
                    logits = joint(enc, pred, ll, tl) if args.ragged else joint(enc, pred)
                    loss = w.rnnt_loss(logits, y, ll, tl, blank=0, reduction="mean", inplace_grad=True, **kw)
            loss.backward()
            return loss
        loss = step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        ms = timeit(step, args.steps)
        rec = {"what": "joint+rnnt_loss fwd+bwd (autograd)", "precision": prec, "shape": [B, T, U + 1, J, V],
               "ragged": bool(args.ragged), "buckets": args.buckets if fused else None,
               "ms": round(ms, 2), "utt_per_s": round(B / ms * 1e3, 1), "loss": float(loss),
               "peak_gb": round(torch.cuda.max_memory_allocated() / 1e9, 2)}
        if bounded:
            rec["budget_mb"] = args.budget_mb
        if base is None:
            base = (float(loss), enc.grad.clone(), joint.ffn_out.weight.grad.clone())
        else:
            rec["loss_rel_diff_vs_fp32"] = abs(float(loss) - base[0]) / abs(base[0])
            for name, got, ref in (("grad_enc", enc.grad, base[1]), ("grad_w", joint.ffn_out.weight.grad, base[2])):
                rms = ref.pow(2).mean().sqrt()
                rec[name + "_max_err_over_rms"] = float((got - ref).abs().max() / rms)
                rec[name + "_rms_err_over_rms"] = float((got - ref).pow(2).mean().sqrt() / rms)
        print(json.dumps(rec), flush=True)
        if settings:
            fns = {(lam, pen): (lambda lam=lam, pen=pen: step(**({} if lam == pen == 0.0 else
                                                                  {"fastemit_lambda": lam, "delay_penalty": pen})))
                   for lam, pen in settings}
            for (lam, pen), (med, lo, hi) in alternating(fns, args.reps).items():
                print(json.dumps({"what": "joint+rnnt_loss fwd+bwd (autograd), latency options", "precision": prec,
                                  "shape": [B, T, U + 1, J, V], "fastemit_lambda": lam, "delay_penalty": pen,
                                  "ms": round(med, 3), "ms_min": round(lo, 3), "ms_max": round(hi, 3), "reps": args.reps}),
                      flush=True)
        del joint


def bench_align(args):
    """RNN-T forced alignment.  At B utterances (default 32) of the BASELINE lattice, fp32 logits: rnnt_forced_align
    (pass 1 + Viterbi), wr_rnnt_align alone, the Viterbi kernel alone (wr_rnnt_align_from_stats on the workspace pass 1
    filled) and wr_rnnt_loss_fwd (pass 1 + both sweeps) on the same logits.  At 8 utterances: joint_rnnt_forced_align
    ("fp32", "bf16x3") beside wr_joint_rnnt_stats + wr_rnnt_loss_sweeps, J = 512."""
    import wenet_celoss_amd as w
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    P = _lib.ptr
    T, U1, V, J = args.T, args.U + 1, args.V, 512
    for B in (args.B, 8):
        tg = torch.randint(1, V, (B, U1 - 1), dtype=torch.int32, device=dev)
        ll = torch.full((B,), T, dtype=torch.int32, device=dev)
        tl = torch.full((B,), U1 - 1, dtype=torch.int32, device=dev)
        rws_bytes = lib.wr_rnnt_workspace_bytes(B, T, U1)
        rws = torch.empty(rws_bytes, dtype=torch.uint8, device=dev)
        costs = torch.empty(B, device=dev)
        frames = torch.empty(B, U1 - 1, dtype=torch.int32, device=dev)
        scores = torch.empty(B, dtype=torch.float64, device=dev)
        st = _lib.current_stream(dev)
        viterbi = lambda: _lib.check(lib.wr_rnnt_align_from_stats(P(tg), P(ll), P(tl), B, T, U1, P(frames), P(scores),
                                                                  P(rws), rws_bytes, st))
        if B == args.B:
            logits = torch.randn(B, T, U1, V, device=dev)
            rec = {"what": "rnnt_align", "shape": [B, T, U1, V], "dtype": "fp32"}
            rec["rnnt_forced_align_ms"] = timeit(lambda: w.rnnt_forced_align(logits, tg, ll, tl), args.steps)
            rec["wr_rnnt_align_ms"] = timeit(lambda: _lib.check(lib.wr_rnnt_align(
                P(logits), 0, P(tg), P(ll), P(tl), B, T, U1, V, 0, P(frames), P(scores), P(rws), rws_bytes, st)),
                args.steps)
            rec["viterbi_kernel_ms"] = timeit(viterbi, max(args.steps, 20))
            rec["wr_rnnt_loss_fwd_ms"] = timeit(lambda: _lib.check(lib.wr_rnnt_loss_fwd(
                P(logits), 0, P(tg), P(ll), P(tl), B, T, U1, V, 0, P(costs), P(rws), rws_bytes, st)), args.steps)
            rec["loss_sweeps_ms"] = timeit(lambda: _lib.check(lib.wr_rnnt_loss_sweeps(
                P(ll), P(tl), B, T, U1, P(costs), P(rws), rws_bytes, st)), max(args.steps, 20))
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)
            del logits
            torch.cuda.empty_cache()
            continue
        g = torch.Generator(device=dev).manual_seed(0)
        ep = torch.randn(B, T, J, device=dev, generator=g)
        pp = torch.randn(B, U1, J, device=dev, generator=g)
        wt = torch.randn(V, J, device=dev, generator=g) * (2.0 / J ** 0.5)
        bt = torch.randn(V, device=dev, generator=g)
        for precision, terms in (("fp32", 0), ("bf16x3", 3)):
            ws_bytes = lib.wr_joint_workspace_bytes(J, V) if terms == 0 else lib.wr_joint_split_workspace_bytes(J, V)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)

            def stats_sweeps():
                _lib.check(lib.wr_joint_rnnt_stats(P(ep), P(pp), P(wt), P(bt), P(ll), P(tl), P(tg), B, T, U1, J, V, 0, 0,
                                                   terms, P(ws), ws_bytes, P(rws), rws_bytes, st))
                _lib.check(lib.wr_rnnt_loss_sweeps(P(ll), P(tl), B, T, U1, P(costs), P(rws), rws_bytes, st))
            rec = {"what": "joint_rnnt_align", "shape": [B, T, U1, J, V], "precision": precision}
            rec["joint_rnnt_forced_align_ms"] = timeit(
                lambda: w.joint_rnnt_forced_align(ep, pp, wt, bt, tg, ll, tl, precision=precision), args.steps)
            rec["stats_plus_loss_sweeps_ms"] = timeit(stats_sweeps, args.steps)
            print(json.dumps({k: (round(v, 3) if isinstance(v, float) else v) for k, v in rec.items()}), flush=True)


def lattice_variants(args):
    """{suffix: keywords} of the k2 losses' lattice forms to time beside the regular one in the same run (simple, smoothed,
    pruned): --rnnt-type modified adds "_modified", --delay-penalty x adds "_regular_pen", both add "_modified_pen" too."""
    out = {}
    if args.rnnt_type != "regular":
        out["_" + args.rnnt_type] = {"rnnt_type": args.rnnt_type}
    if args.delay_penalty > 0:
        out["_regular_pen"] = {"delay_penalty": args.delay_penalty}
        if args.rnnt_type != "regular":
            out["_" + args.rnnt_type + "_pen"] = {"rnnt_type": args.rnnt_type, "delay_penalty": args.delay_penalty}
    return out


def bench_simple(args):
    """The additive-joiner loss step (rnnt_loss_simple forward + backward) beside the composite it replaces:
    am.unsqueeze(2) + lm.unsqueeze(1) -> rnnt_loss, fp32, which writes and re-reads a (B,T,U+1,V) tensor.  N(0,1) inputs,
    full lengths.  HIP events around each step after warm-up, the two alternating, median of --steps runs; peak memory of
    each above what the inputs hold.  One JSON line.  --only simple: the new step alone (for a kernel trace)."""
    import wenet_celoss_amd as w
    dev = torch.device("cuda:0")
    B, T, U, V = args.B, args.T, args.U, args.V
    gen = torch.Generator(device=dev).manual_seed(0)
    am = torch.randn(B, T, V, device=dev, generator=gen).requires_grad_(True)
    lm = torch.randn(B, U + 1, V, device=dev, generator=gen).requires_grad_(True)
    sy = torch.randint(1, V, (B, U), device=dev, generator=gen)
    sy32 = sy.to(torch.int32)
    ll = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl = torch.full((B,), U, dtype=torch.int32, device=dev)

    def simple():
        am.grad = lm.grad = None
        loss = w.rnnt_loss_simple(lm, am, sy, 0, reduction="mean")
        loss.backward()
        return loss

    def composite():
        am.grad = lm.grad = None
        loss = w.rnnt_loss(am.unsqueeze(2) + lm.unsqueeze(1), sy32, ll, tl, blank=0, reduction="mean")
        loss.backward()
        return loss

    def variant(kw):
        def run():
            am.grad = lm.grad = None
            loss = w.k2.rnnt_loss_simple(lm, am, sy, 0, reduction="mean", **kw)
            loss.backward()
            return loss
        return run

    fns = {"simple": simple} if args.only == "simple" else {"simple": simple, "composite": composite}
    fns.update({"simple" + sfx: variant(kw) for sfx, kw in lattice_variants(args).items()})
    peak, loss = {}, {}
    for name, fn in fns.items():                       # warm-up, and the memory peak of one step
        fn()
        am.grad = lm.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss[name] = float(fn())
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    times = {name: [] for name in fns}
    for _ in range(max(args.steps, 1)):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    med = {name: sorted(ts)[len(ts) // 2] for name, ts in times.items()}
    rec = {"what": "rnnt_loss_simple fwd+bwd", "shape": [B, T, U + 1, V], "runs": max(args.steps, 1),
           "simple_ms": round(med["simple"], 3), "simple_ms_min_max": [round(min(times["simple"]), 3), round(max(times["simple"]), 3)],
           "simple_peak_mib": round(peak["simple"] / 2**20, 1), "simple_loss": loss["simple"],
           "contraction_gflop": round(3 * 2.0 * B * T * (U + 1) * V / 1e9, 1),
           "logits_gib": round(B * T * (U + 1) * V * 4 / 2**30, 2)}
    if "composite" in med:
        rec.update({"composite_ms": round(med["composite"], 3),
                    "composite_ms_min_max": [round(min(times["composite"]), 3), round(max(times["composite"]), 3)],
                    "composite_peak_mib": round(peak["composite"] / 2**20, 1), "composite_loss": loss["composite"],
                    "composite_over_simple": round(med["composite"] / med["simple"], 1)})
    for name in fns:
        if name not in ("simple", "composite"):
            rec.update({name + "_ms": round(med[name], 3),
                        name + "_ms_min_max": [round(min(times[name]), 3), round(max(times[name]), 3)],
                        name + "_peak_mib": round(peak[name] / 2**20, 1), name + "_loss": loss[name]})
    print(json.dumps(rec), flush=True)


def bench_smoothed(args):
    """rnnt_loss_smoothed forward + backward beside rnnt_loss_simple, at the shape and by the timing method of `simple`:
    N(0,1) inputs, full lengths, HIP events around each step after warm-up, the three alternating, median of --steps
    runs (9 for the figures in DESIGN.md).  Configurations: simple, smoothed (0.25, 0) -- the icefall setting --, and
    smoothed (0.1, 0.1) -- k2's defaults.  One JSON line.  --only NAME[,NAME]: a subset (for a kernel trace)."""
    import wenet_celoss_amd as w
    dev = torch.device("cuda:0")
    B, T, U, V = args.B, args.T, args.U, args.V
    gen = torch.Generator(device=dev).manual_seed(0)
    am = torch.randn(B, T, V, device=dev, generator=gen).requires_grad_(True)
    lm = torch.randn(B, U + 1, V, device=dev, generator=gen).requires_grad_(True)
    sy = torch.randint(1, V, (B, U), device=dev, generator=gen)

    def step(fn):
        def run():
            am.grad = lm.grad = None
            loss = fn()
            loss.backward()
            return loss
        return run

    fns = {"simple": step(lambda: w.rnnt_loss_simple(lm, am, sy, 0, reduction="mean")),
           "smoothed_0.25_0": step(lambda: w.rnnt_loss_smoothed(lm, am, sy, 0, 0.25, 0.0, reduction="mean")),
           "smoothed_0.1_0.1": step(lambda: w.rnnt_loss_smoothed(lm, am, sy, 0, 0.1, 0.1, reduction="mean"))}
    if args.only:
        fns = {k: v for k, v in fns.items() if k in args.only.split(",")}
    for sfx, kw in lattice_variants(args).items():     # the icefall setting on the other lattice forms
        fns["smoothed_0.25_0" + sfx] = step(lambda kw=kw: w.k2.rnnt_loss_smoothed(lm, am, sy, 0, 0.25, 0.0, reduction="mean", **kw))
    loss = {}
    for name, fn in fns.items():                       # warm-up
        fn()
        loss[name] = float(fn())
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(max(args.steps, 1)):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    rec = {"what": "rnnt_loss_smoothed fwd+bwd", "shape": [B, T, U + 1, V], "runs": max(args.steps, 1)}
    for name, ts in times.items():
        rec[name + "_ms"] = round(sorted(ts)[len(ts) // 2], 3)
        rec[name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
        rec[name + "_loss"] = loss[name]
    print(json.dumps(rec), flush=True)


def bench_pruned(args):
    """Pruned RNN-T training beside the full-lattice paths, fp32, N(0,1) inputs, full lengths, R = 5 (--R):
      loss:  rnnt_loss_pruned forward + backward on (B,T,R,V) logits  |  rnnt_loss on the (B,T,U+1,V) logits the band was
             gathered from;
      step:  simple loss + prune ranges + TransducerJoint.forward_pruned + pruned loss, forward + backward down to the
             encoder / predictor outputs  |  joint_rnnt_loss on the same joiner (E = P = 256, J = 512, tanh).
    HIP events around each step after warm-up, the configurations alternating, median of --steps runs (9 for the figures
    in DESIGN.md); peak memory of each above what its inputs hold.  One JSON line.  --only pruned: the two pruned
    configurations alone (for a kernel trace)."""
    import wenet_celoss_amd as w
    dev = torch.device("cuda:0")
    B, T, U, V, R = args.B, args.T, args.U, args.V, min(args.R, args.U + 1)
    E = P = 256
    J = 512
    gen = torch.Generator(device=dev).manual_seed(0)
    sy = torch.randint(1, V, (B, U), device=dev, generator=gen)
    sy32 = sy.to(torch.int32)
    ll = torch.full((B,), T, dtype=torch.int32, device=dev)
    tl = torch.full((B,), U, dtype=torch.int32, device=dev)
    only = args.only == "pruned"

    # loss: a diagonal band through the lattice
    start = (torch.arange(T, device=dev) * max(U + 1 - R, 0)) // max(T - 1, 1)
    ranges = (start[None, :, None] + torch.arange(R, device=dev)).expand(B, T, R).contiguous()
    if only:
        band = torch.randn(B, T, R, V, device=dev, generator=gen)
        full = None
    else:
        full = torch.empty(B, T, U + 1, V, device=dev)
        for b in range(B):
            full[b].normal_(generator=gen)
        band = torch.stack([full[b].gather(1, ranges[b, :, :, None].expand(T, R, V)) for b in range(B)])
        full.requires_grad_(True)
    band.requires_grad_(True)

    def loss_pruned():
        band.grad = None
        loss = w.rnnt_loss_pruned(band, sy, ranges, 0, reduction="mean")
        loss.backward()
        return loss

    def loss_full():
        full.grad = None
        loss = w.rnnt_loss(full, sy32, ll, tl, blank=0, reduction="mean")
        loss.backward()
        return loss

    # step: the whole training step from the encoder / predictor outputs
    torch.manual_seed(0)
    joint = w.TransducerJoint(V, E, P, J).to(dev)
    am_head, lm_head = torch.nn.Linear(E, V).to(dev), torch.nn.Linear(P, V).to(dev)
    enc = torch.randn(B, T, E, device=dev, generator=gen).requires_grad_(True)
    pred = torch.randn(B, U + 1, P, device=dev, generator=gen).requires_grad_(True)
    params = list(joint.parameters()) + list(am_head.parameters()) + list(lm_head.parameters())
    boundary = torch.tensor([0, 0, U, T], device=dev).repeat(B, 1)

    def clear():
        enc.grad = pred.grad = None
        for p in params:
            p.grad = None

    def step_pruned():
        clear()
        simple, (px, py) = w.rnnt_loss_simple(lm_head(pred), am_head(enc), sy, 0, boundary=boundary, reduction="mean",
                                              return_grad=True)
        rg = w.get_rnnt_prune_ranges(px, py, boundary, R)
        loss = w.rnnt_loss_pruned(joint.forward_pruned(enc, pred, rg), sy, rg, 0, boundary=boundary, reduction="mean")
        (loss + 0.5 * simple).backward()
        return loss

    def step_full():
        clear()
        ep, pp = joint.pre_activation(enc, pred)
        loss = w.joint_rnnt_loss(ep, pp, joint.ffn_out.weight, joint.ffn_out.bias, sy32, ll, tl, blank=0, reduction="mean",
                                 precision=joint.precision, activation=joint.activation)
        loss.backward()
        return loss

    def loss_pruned_variant(kw):
        def run():
            band.grad = None
            loss = w.rnnt_loss_pruned(band, sy, ranges, 0, reduction="mean", **kw)
            loss.backward()
            return loss
        return run

    def step_pruned_variant(kw):
        def run():
            clear()
            simple, (px, py) = w.k2.rnnt_loss_simple(lm_head(pred), am_head(enc), sy, 0, boundary=boundary,
                                                     reduction="mean", return_grad=True, **kw)
            rg = w.k2.get_rnnt_prune_ranges(px, py, boundary, R)
            loss = w.rnnt_loss_pruned(joint.forward_pruned(enc, pred, rg), sy, rg, 0, boundary=boundary, reduction="mean",
                                      **kw)
            (loss + 0.5 * simple).backward()
            return loss
        return run

    fns = {"loss_pruned": loss_pruned, "step_pruned": step_pruned}
    if not only:
        fns.update({"loss_full": loss_full, "step_full": step_full})
    for sfx, kw in lattice_variants(args).items():
        fns.update({"loss_pruned" + sfx: loss_pruned_variant(kw), "step_pruned" + sfx: step_pruned_variant(kw)})
    peak, loss = {}, {}
    for name, fn in fns.items():                       # warm-up, and the memory peak of one step
        fn()
        clear()
        band.grad = None
        if full is not None:
            full.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss[name] = float(fn().detach())
        torch.cuda.synchronize()
        peak[name] = torch.cuda.max_memory_allocated() - base
    times = {name: [] for name in fns}
    for _ in range(max(args.steps, 1)):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    rec = {"what": "pruned RNN-T training, fwd+bwd", "shape": [B, T, U + 1, V], "R": R, "runs": max(args.steps, 1),
           "band_logits_gib": round(B * T * R * V * 4 / 2**30, 2), "full_logits_gib": round(B * T * (U + 1) * V * 4 / 2**30, 2)}
    for name, ts in times.items():
        rec[name + "_ms"] = round(sorted(ts)[len(ts) // 2], 3)
        rec[name + "_ms_min_max"] = [round(min(ts), 3), round(max(ts), 3)]
        rec[name + "_peak_mib"] = round(peak[name] / 2**20, 1)
        rec[name + "_loss"] = loss[name]
    print(json.dumps(rec), flush=True)


def bench_tdt(args):
    """The token-and-duration loss through the C-ABI on fp32 N(0,1) logits (B, T, U+1, V + D), full lengths, durations
    0 .. D-1: the forward call (row statistics, sweeps, records) and the gradient pass, each alternating with its sibling of
    rnnt_loss on the same (B, T, U+1, V + D) tensor with the dead-row skip off (wr_tune_set(14, 0): the TDT kernels have
    none).  HIP events, median of --steps rounds after one warm-up.  --only tdt runs one TDT step alone (for a profiler)."""
    import ctypes
    from wenet_celoss_amd import _lib
    dev = torch.device("cuda:0")
    B, T, U, V, D = args.B, args.T, args.U, args.V, args.durations
    U1, W = U + 1, V + D
    durs = (ctypes.c_int32 * D)(*range(D))
    torch.manual_seed(3)
    logits = torch.empty(B, T, U1, W, device=dev)
    for b in range(B):
        logits[b].normal_()
    grads = torch.empty_like(logits)
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=dev)
    ll = torch.full((B,), T, dtype=torch.int32, device=dev); tl = torch.full((B,), U, dtype=torch.int32, device=dev)
    gc = torch.full((B,), 1.0 / B, device=dev)
    tws = _lib.workspace("wr_rnnt_tdt_workspace_bytes", B, T, U1, D, device=dev)
    rws = _lib.workspace("wr_rnnt_workspace_bytes", B, T, U1, device=dev)
    tcosts, rcosts = torch.empty(B, device=dev), torch.empty(B, device=dev)
    fns = {
        "tdt_fwd": lambda: _lib.call("wr_rnnt_tdt_loss_fwd", logits, _lib.WR_F32, y, ll, tl, B, T, U1, V, 0, durs, D, 0.0,
                                     tcosts, tws, tws.numel(), device=dev),
        "rnnt_fwd": lambda: _lib.call("wr_rnnt_loss_fwd", logits, _lib.WR_F32, y, ll, tl, B, T, U1, W, 0, rcosts, rws,
                                      rws.numel(), device=dev),
        "tdt_bwd": lambda: _lib.call("wr_rnnt_tdt_loss_bwd", logits, _lib.WR_F32, y, ll, tl, B, T, U1, V, 0, durs, D, 0.0, gc,
                                     grads, tws, tws.numel(), device=dev),
        "rnnt_bwd": lambda: _lib.call("wr_rnnt_loss_bwd", logits, _lib.WR_F32, y, ll, tl, B, T, U1, W, 0, -1.0, gc, grads,
                                      rws, rws.numel(), device=dev),
    }
    if args.only == "tdt":
        fns = {k: f for k, f in fns.items() if k.startswith("tdt")}
    lib = _lib.load()
    lib.wr_tune_set(14, 0)
    try:
        res = alternating(fns, args.steps)
    finally:
        lib.wr_tune_set(14, 1)
    rec = {"what": "tdt loss vs rnnt_loss (fp32 logits, separate gradient buffer, no dead-row skip)", "shape": [B, T, U1, W],
           "durations": list(range(D)), "reps": args.steps, "logits_gb": round(logits.numel() * 4 / 1e9, 2),
           "tdt_workspace_gb": round(tws.numel() / 1e9, 3), "rnnt_workspace_gb": round(rws.numel() / 1e9, 3),
           "tdt_cost_mean": round(float(tcosts.mean()), 4)}
    for k, (med, lo, hi) in res.items():
        rec[k + "_ms"] = round(med, 3)
        rec[k + "_ms_min_max"] = [round(lo, 3), round(hi, 3)]
    for k in ("tdt", "rnnt"):
        if k + "_fwd" in res:
            rec[k + "_step_ms"] = round(res[k + "_fwd"][0] + res[k + "_bwd"][0], 3)
    print(json.dumps(rec), flush=True)


def bench_tdtstep(args):
    """The TDT loss block of Transducer.forward through the autograd path, two ways in one run: the materialised pair
    (joiner logits (B, T, U+1, V + D) -> rnnt_tdt_loss(inplace_grad=True), what a TDT model runs without a budget) and
    the memory-bounded node joint_rnnt_tdt_loss(logits_budget=--budget-mb, default 1 GiB).  Forward + backward to enc /
    pred and all joiner weights, exact fp32 joiner, J = 512, durations 0 .. D-1, full lengths; alternating, HIP events,
    median of --steps rounds after one warm-up, and the growth of max_memory_allocated over one step of each."""
    import wenet_celoss_amd as w
    dev = torch.device("cuda:0")
    torch.manual_seed(3)
    B, T, U, V, D, E, P, J = args.B, args.T, args.U, args.V, args.durations, 256, 256, 512
    durations = tuple(range(D))
    budget = int((args.budget_mb or 1024.0) * (1 << 20))
    enc = torch.randn(B, T, E, device=dev, requires_grad=True)
    pred = torch.randn(B, U + 1, P, device=dev, requires_grad=True)
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=dev)
    ll = torch.full((B,), T, dtype=torch.int32, device=dev); tl = torch.full((B,), U, dtype=torch.int32, device=dev)
    joint = w.TransducerJoint(V + D, E, P, J, precision="fp32").to(dev)
    torch.manual_seed(4)
    with torch.no_grad():
        for prm in joint.parameters():
            prm.copy_(torch.randn_like(prm) * 0.05)
    last = {}

    def step(bounded):
        joint.zero_grad(set_to_none=True); enc.grad = None; pred.grad = None
        if bounded:
            loss = w.joint_rnnt_tdt_loss(joint.enc_ffn(enc), joint.pred_ffn(pred), joint.ffn_out.weight, joint.ffn_out.bias,
                                         y, ll, tl, durations, blank=0, reduction="mean", logits_budget=budget)
        else:
            loss = w.rnnt_tdt_loss(joint(enc, pred), y, ll, tl, durations, blank=0, reduction="mean", inplace_grad=True)
        loss.backward()
        last["loss"] = loss.detach()

    fns = {"materialised": lambda: step(False), "bounded": lambda: step(True)}
    if args.only:
        fns = {k: f for k, f in fns.items() if k in args.only.split(",")}
    rec = {"what": "joint+rnnt_tdt_loss fwd+bwd (autograd): materialised logits vs memory-bounded node",
           "shape": [B, T, U + 1, J, V + D], "durations": list(durations), "budget_mb": budget / (1 << 20), "reps": args.steps,
           "logits_gb": round(B * T * (U + 1) * (V + D) * 4 / 1e9, 2)}
    grads = {}
    for k, fn in fns.items():                          # one step of each alone: loss, gradients, peak memory
        joint.zero_grad(set_to_none=True); enc.grad = None; pred.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        rec[k + "_peak_gb"] = round((torch.cuda.max_memory_allocated() - base) / 1e9, 3)
        rec[k + "_loss"] = float(last["loss"])
        grads[k] = (enc.grad.clone(), joint.ffn_out.weight.grad.clone())
    if len(grads) == 2:
        for name, i in (("grad_enc", 0), ("grad_w", 1)):
            got, ref = grads["bounded"][i], grads["materialised"][i]
            rec[name + "_max_err_over_max"] = float((got - ref).abs().max() / ref.abs().max())
    del grads
    for k, (med, lo, hi) in alternating(fns, args.steps).items():
        rec[k + "_ms"] = round(med, 2)
        rec[k + "_ms_min_max"] = [round(lo, 2), round(hi, 2)]
    if len(fns) == 2:
        rec["bounded_over_materialised"] = round(rec["bounded_ms"] / rec["materialised_ms"], 3)
    print(json.dumps(rec), flush=True)


def bench_tdtalign(args):
    """TDT forced alignment at the `tdt` sweep's shape (fp32 N(0,1) logits (B, T, U+1, V + D), full lengths, durations
    0 .. D-1): rnnt_tdt_forced_align (Python entry: label check, pass 1, Viterbi + backtrace), wr_rnnt_tdt_align alone and
    wr_rnnt_tdt_loss_fwd (pass 1, both sweeps, records) on the same logits, alternating.  HIP events, median of --steps
    rounds after one warm-up.  --only tdtalign runs wr_rnnt_tdt_align and wr_rnnt_tdt_loss_fwd once each (for a profiler)."""
    import ctypes
    import wenet_celoss_amd as w
    from wenet_celoss_amd import _lib
    dev = torch.device("cuda:0")
    B, T, U, V, D = args.B, args.T, args.U, args.V, args.durations
    U1, W = U + 1, V + D
    durations = tuple(range(D))
    durs = (ctypes.c_int32 * D)(*durations)
    torch.manual_seed(3)
    logits = torch.empty(B, T, U1, W, device=dev)
    for b in range(B):
        logits[b].normal_()
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=dev)
    ll = torch.full((B,), T, dtype=torch.int32, device=dev); tl = torch.full((B,), U, dtype=torch.int32, device=dev)
    ws = _lib.workspace("wr_rnnt_tdt_workspace_bytes", B, T, U1, D, device=dev)
    frames, jumps_of = (torch.empty(B, U, dtype=torch.int32, device=dev) for _ in range(2))
    blank_jumps = torch.empty(B, T, dtype=torch.int32, device=dev)
    scores = torch.empty(B, dtype=torch.float64, device=dev)
    costs = torch.empty(B, device=dev)
    fns = {
        "wr_rnnt_tdt_align": lambda: _lib.call("wr_rnnt_tdt_align", logits, _lib.WR_F32, y, ll, tl, B, T, U1, V, 0, durs, D, 0.0,
                                               frames, jumps_of, blank_jumps, scores, ws, ws.numel(), device=dev),
        "wr_rnnt_tdt_loss_fwd": lambda: _lib.call("wr_rnnt_tdt_loss_fwd", logits, _lib.WR_F32, y, ll, tl, B, T, U1, V, 0, durs,
                                                  D, 0.0, costs, ws, ws.numel(), device=dev),
        "rnnt_tdt_forced_align": lambda: w.rnnt_tdt_forced_align(logits, y, ll, tl, durations, return_blank_jumps=True),
    }
    if args.only == "tdtalign":
        del fns["rnnt_tdt_forced_align"]
    res = alternating(fns, 1 if args.only == "tdtalign" else args.steps)
    rec = {"what": "tdt forced alignment vs tdt loss forward (fp32 logits)", "shape": [B, T, U1, W],
           "durations": list(durations), "reps": args.steps, "logits_gb": round(logits.numel() * 4 / 1e9, 2),
           "workspace_gb": round(ws.numel() / 1e9, 3), "score_mean": round(float(scores.mean()), 4),
           "cost_mean": round(float(costs.mean()), 4)}
    for k, (med, lo, hi) in res.items():
        rec[k + "_ms"] = round(med, 3)
        rec[k + "_ms_min_max"] = [round(lo, 3), round(hi, 3)]
    print(json.dumps(rec), flush=True)


def tdt_decision_traces(model, enc, lens, n_steps):
    """Every stream's decisions [(frame, token, duration)] by a lock-step torch loop over the HIP step kernels (all streams
    step together; a stream that has not emitted repeats its predictor step, which gives the same output)."""
    N, dev = enc.size(0), enc.device
    V, durs = model.vocab_size, model.tdt_durations
    pad = torch.zeros(N, 1, device=dev)
    tok = torch.full((N, 1), model.blank, device=dev)
    cache = model.predictor.init_state(N, method="zero", device=dev)
    t, nb, traces = [0] * N, [0] * N, [[] for _ in range(N)]
    T = [int(x) for x in lens]
    rows_of = torch.arange(N, device=dev)
    with torch.no_grad():
        while any(t[n] < T[n] for n in range(N)):
            out, new_cache = model.predictor.forward_step(tok, pad, cache)
            at = torch.tensor([min(t[n], T[n] - 1) for n in range(N)], device=dev)
            rows = model.joint(enc[rows_of, at][:, None, :].contiguous(), out.contiguous()).reshape(N, -1).float()
            ks, js = rows[:, :V].argmax(1).tolist(), rows[:, V:].argmax(1).tolist()
            emitted = []
            for n in range(N):
                if t[n] >= T[n]:
                    continue
                k, d = ks[n], durs[js[n]]
                traces[n].append((t[n], k, d))
                if k == model.blank:
                    t[n] += max(d, 1)
                    nb[n] = 0
                    continue
                emitted.append(n)
                nb[n] = 0 if d > 0 else nb[n] + 1
                t[n] += d
                if nb[n] >= n_steps:
                    t[n] += 1
                    nb[n] = 0
            if emitted:                                             # commit the stepped state and feed the new token
                tok[emitted, 0] = torch.tensor([ks[n] for n in emitted], device=dev)
                for c, nc in zip(cache, new_cache):
                    c[:, emitted] = nc[:, emitted]
    return traces


def tdt_row_counts(traces, look, blank=0):
    """Replay of the look-ahead walk over recorded decisions -> (micro-steps, joiner rows evaluated for active streams,
    rows consulted)."""
    N = len(traces)
    pos = [0] * N
    micro = evaluated = consulted = 0
    while any(pos[n] < len(traces[n]) for n in range(N)):
        micro += 1
        for n in range(N):
            if pos[n] >= len(traces[n]):
                continue
            t0 = traces[n][pos[n]][0]
            evaluated += look
            while pos[n] < len(traces[n]) and traces[n][pos[n]][0] - t0 < look:
                k = traces[n][pos[n]][1]
                pos[n] += 1
                consulted += 1
                if k != blank:
                    break
    return micro, evaluated, consulted


def bench_tdtdec(args):
    """TDT greedy search on the device at the shape of the `greedy` sweep: 64 streams, V = 5000 tokens + D durations
    0 .. D-1, LSTM 2x256, J = 512; look-ahead 1 / 2 / 4 / 0, plain greedy on the same handle, the host-driven loop for one
    stream.  Per line: ms per call, us per decision, the share of joiner rows evaluated but never consulted."""
    import time
    import types
    import wenet_celoss_amd as w
    dev = torch.device("cuda:0")
    torch.manual_seed(5)
    D = args.durations
    V, E, P, J, H, L, N = 5000, 256, 256, 512, 256, 2, args.streams
    T = 16 * args.chunks
    durations = tuple(range(D))
    # the embedding table has a row for every joiner column, so that the plain search may run on the same handle
    pred = w.RNNPredictor(V + D, P, P, 0.1, H, L).to(dev).eval()
    joint = w.TransducerJoint(V + D, E, P, J).to(dev).eval()
    with torch.no_grad():
        joint.ffn_out.weight *= 10
        joint.ffn_out.bias[0] += 17.0
    gq = torch.Generator(device=dev).manual_seed(11)                # the speech-like input of the `greedy` sweep
    quiet = torch.randn(N, T, E, device=dev, generator=gq) * 0.1
    loud = torch.randn(N, T, E, device=dev, generator=gq) * 2.5
    spikes = torch.rand(N, T, device=dev, generator=gq) < 0.25
    enc = torch.where(spikes[..., None], loud, quiet)
    lens = torch.full((N,), T)
    n_steps = 2

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, out

    for n_str in (N, 1):
        model = types.SimpleNamespace(blank=0, predictor=pred, joint=joint, vocab_size=V, tdt_durations=durations)
        e_s, l_s = enc[:n_str].contiguous(), lens[:n_str]
        traces = tdt_decision_traces(model, e_s, l_s, n_steps)
        decisions = sum(len(tr) for tr in traces)
        want = [[k for _, k, _ in tr if k != 0] for tr in traces]
        taken = sorted({d for tr in traces for _, _, d in tr})
        w.tdt_greedy_search(model, e_s, l_s, n_steps=n_steps)      # builds the handle
        dec = model._decoder_cache._dec
        for look in (1, 2, 4, 0):
            dec.set_lookahead(look)
            dt, got = timed(lambda: w.tdt_greedy_search(model, e_s, l_s, n_steps=n_steps))
            micro, evaluated, consulted = tdt_row_counts(traces, look or 1)      # 0 means 1 for TDT
            print(json.dumps({"what": "tdt_greedy_search device", "streams": n_str, "frames": T, "durations": durations,
                              "frames_per_micro_step": look, "tokens": sum(len(h) for h in got), "decisions": decisions,
                              "durations_taken": taken, "micro_steps": micro, "ms_per_call": round(dt * 1e3, 3),
                              "us_per_decision": round(dt * 1e6 / max(decisions, 1), 2),
                              "rows_never_consulted": round(1.0 - consulted / max(evaluated, 1), 3),
                              "tokens_identical": got == want}), flush=True)
        dec.set_lookahead(0)
        if n_str == N:
            dt, got = timed(lambda: dec.greedy(e_s, l_s, n_steps=n_steps, blank=0))
            plain_decisions = sum(len(h) for h in got) + n_str * T          # one per token, one blank per frame (an upper bound)
            print(json.dumps({"what": "greedy_search (plain, same handle, every column a token)", "streams": n_str, "frames": T,
                              "tokens": sum(len(h) for h in got), "ms_per_call": round(dt * 1e3, 3),
                              "us_per_decision": round(dt * 1e6 / plain_decisions, 2)}), flush=True)
    os.environ["WR_TDT_HOST"] = "1"
    try:
        dt, got = timed(lambda: w.tdt_greedy_search(model, e_s, l_s, n_steps=n_steps))
    finally:
        del os.environ["WR_TDT_HOST"]
    print(json.dumps({"what": "tdt_greedy_search host-driven loop", "streams": 1, "frames": T, "decisions": decisions,
                      "ms_per_call": round(dt * 1e3, 2), "us_per_decision": round(dt * 1e6 / max(decisions, 1), 1),
                      "tokens_identical": got == want}), flush=True)


def bench_tdtbeam(args):
    """TDT prefix beam search at BASELINE config 5 (B = 16, T = 1500, beam 8, LSTM 2x256, J = 512): the plain prefix beam
    search on a plain joiner of width 5000 (the first 5000 outputs), the TDT search on the joiner of width V + D = 5005
    with durations 0 .. 4, and the TDT search with durations (1,) on the same handle (then 5004 token columns), all in one
    run.  Per line: ms per call, us per step, steps taken against T (mean over the utterances), and the share of
    lane-steps (beam slots of a step) that were expanded."""
    import time
    import wenet_celoss_amd as w
    from wenet_celoss_amd.decoder import DeviceDecoder
    dev = torch.device("cuda:0")
    torch.manual_seed(6)
    D = args.durations
    V, E, P, J, H, L, beam = 5000, 256, 256, 512, 256, 2, 8
    B, T = (args.B if args.B != 32 else 16), (args.T if args.T != 1000 else 1500)
    # the embedding table has a row for every joiner column: with durations (1,) all but one of them are tokens
    pred = w.RNNPredictor(V + D, P, P, 0.1, H, L).to(dev).eval()
    joint = w.TransducerJoint(V + D, E, P, J).to(dev).eval()
    with torch.no_grad():
        joint.ffn_out.weight *= 10
        joint.ffn_out.bias[0] += 16.0
    plain_joint = w.TransducerJoint(V, E, P, J).to(dev).eval()
    plain_joint.load_state_dict({k: (v[:V] if k.startswith("ffn_out.") else v) for k, v in joint.state_dict().items()})
    ctc = w.CTC(V, E).to(dev).eval()
    enc = torch.randn(B, T, E, device=dev)
    lens = torch.full((B,), T, dtype=torch.int32)
    with torch.no_grad():
        ctc_logp = ctc.log_softmax(enc)
    plain = DeviceDecoder(pred, plain_joint, B * beam, B, T, 0, beam)
    tdt = DeviceDecoder(pred, joint, B * beam, B, T, 0, beam)

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, out

    only = set(args.only.split(",")) if args.only else {"plain", "tdt", "tdt1"}
    if "plain" in only:
        dt, out = timed(lambda: plain.prefix_beam(enc, lens, ctc_logp, beam, 0.3, 0.7, 0))
        print(json.dumps({"what": "prefix_beam_search (plain joiner, width 5000)", "B": B, "T": T, "beam": beam,
                          "ms_per_call": round(dt * 1e3, 2), "us_per_step": round(dt * 1e6 / T, 1), "steps": T,
                          "expanded_share": 1.0, "best_len": len(out[0][0][0])}), flush=True)
    for key, durations in (("tdt", tuple(range(D))), ("tdt1", (1,))):
        if key not in only:
            continue
        dt, out = timed(lambda: tdt.prefix_beam_tdt(enc, lens, durations, beam, 0))
        _, utt_steps, expanded = tdt.last_counters()
        steps = utt_steps / B
        print(json.dumps({"what": "prefix_beam_search_tdt", "durations": durations, "B": B, "T": T, "beam": beam,
                          "ms_per_call": round(dt * 1e3, 2), "us_per_step": round(dt * 1e6 / max(steps, 1), 1),
                          "steps": round(steps, 1), "steps_over_T": round(steps / T, 3),
                          "expanded_share": round(expanded / max(utt_steps * beam, 1), 3),
                          "best_len": len(out[0][0][0])}), flush=True)


def bench_beamstream(args):
    """Streaming transducer prefix beam search at the shape of `beam` / `tdtbeam` (B = 16, T = 1500, beam 8, LSTM 2x256,
    J = 512, V = 5000), plain (joiner of width 5000) and token-and-duration (width 5005, durations 0 .. 4), in one run per
    model: the whole-utterance search, one reset-and-final chunk call over the whole utterance, and the utterance in chunks
    of --chunk-frames frames (16), with the time per chunk call.  Per line: ms per utterance batch and, for the chunked
    run, us per chunk."""
    import time
    import wenet_celoss_amd as w
    from wenet_celoss_amd.decoder import DeviceDecoder
    dev = torch.device("cuda:0")
    torch.manual_seed(6)
    D = args.durations
    V, E, P, J, H, L, beam = 5000, 256, 256, 512, 256, 2, 8
    B, T = (args.B if args.B != 32 else 16), (args.T if args.T != 1000 else 1500)
    C = args.chunk_frames
    pred = w.RNNPredictor(V + D, P, P, 0.1, H, L).to(dev).eval()
    joint = w.TransducerJoint(V + D, E, P, J).to(dev).eval()
    with torch.no_grad():
        joint.ffn_out.weight *= 10
        joint.ffn_out.bias[0] += 16.0
    plain_joint = w.TransducerJoint(V, E, P, J).to(dev).eval()
    plain_joint.load_state_dict({k: (v[:V] if k.startswith("ffn_out.") else v) for k, v in joint.state_dict().items()})
    ctc = w.CTC(V, E).to(dev).eval()
    enc = torch.randn(B, T, E, device=dev)
    lens = torch.full((B,), T, dtype=torch.int32)
    with torch.no_grad():
        ctc_logp = ctc.log_softmax(enc)
    starts = list(range(0, T, C))
    chunks = [(enc[:, p:p + C].contiguous(), ctc_logp[:, p:p + C].contiguous(),
               torch.full((B,), min(C, T - p), dtype=torch.int32, device=dev)) for p in starts]

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            out = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps, out

    for name, jn, durations, mix in (("plain", plain_joint, None, (0.3, 0.7)), ("tdt", joint, tuple(range(D)), (0.0, 1.0))):
        if args.only and name not in args.only.split(","):
            continue
        dec = DeviceDecoder(pred, jn, B * beam, B, T, 0, beam)
        dec.attach_beam_stream(B, beam, T)
        post = (lambda c: c) if durations is None else (lambda c: None)

        def whole():
            if durations is None:
                return dec.prefix_beam(enc, lens, ctc_logp, beam, *mix, 0)
            return dec.prefix_beam_tdt(enc, lens, durations, beam, 0)

        def one_chunk():
            return dec.prefix_beam_chunk(enc, lens, beam, 0, ctc_logp=post(ctc_logp), ctc_weight=mix[0], transducer_weight=mix[1],
                                         durations=durations, reset=True, final=True)

        def chunked():
            out = None
            for i, (e, c, n) in enumerate(chunks):
                out = dec.prefix_beam_chunk(e, n, beam, 0, ctc_logp=post(c), ctc_weight=mix[0], transducer_weight=mix[1],
                                            durations=durations, reset=i == 0, final=i == len(chunks) - 1)
            return out

        t_whole, out_w = timed(whole)
        t_one, out_1 = timed(one_chunk)
        t_chunked, out_c = timed(chunked)
        base = {"model": name, "durations": durations, "B": B, "T": T, "beam": beam}
        print(json.dumps({"what": "whole-utterance search", **base, "ms_per_call": round(t_whole * 1e3, 2)}), flush=True)
        print(json.dumps({"what": "prefix_beam_search_chunk, one reset-and-final call", **base,
                          "ms_per_call": round(t_one * 1e3, 2), "over_whole": round(t_one / t_whole, 3),
                          "equals_whole": [[(h, s) for h, s, _, _ in u] for u in out_1] == out_w}), flush=True)
        print(json.dumps({"what": "prefix_beam_search_chunk, chunked", **base, "chunk_frames": C, "chunks": len(chunks),
                          "ms_per_utterance": round(t_chunked * 1e3, 2), "us_per_chunk": round(t_chunked * 1e6 / len(chunks), 1),
                          "over_one_chunk": round(t_chunked / t_one, 3), "over_whole": round(t_chunked / t_whole, 3),
                          "equals_one_chunk": out_c == out_1}), flush=True)


def bench_beamctx(args):
    """Context-graph biasing in the streaming transducer prefix beam search, at the shape of `beamstream` (16 streams x
    1500 frames, beam 8, V = 5000, chunks of --chunk-frames = 16 frames; a plain model and durations 0 .. 4): the unbiased
    stream, the biased stream with an empty graph and with 1000 random three-token phrases, in the same process and
    alternating, --reps rounds after one warm-up round.  Per line: the median ms per utterance batch, ms per chunk call,
    and the ratio to the unbiased stream of the same model (the median of the per-round ratios)."""
    import statistics
    import time
    import wenet_celoss_amd as w
    from wenet_celoss_amd.decoder import DeviceDecoder
    dev = torch.device("cuda:0")
    torch.manual_seed(6)
    D = args.durations
    V, E, P, J, H, L, beam = 5000, 256, 256, 512, 256, 2, 8
    B, T = (args.B if args.B != 32 else 16), (args.T if args.T != 1000 else 1500)
    C = args.chunk_frames
    pred = w.RNNPredictor(V + D, P, P, 0.1, H, L).to(dev).eval()
    joint = w.TransducerJoint(V + D, E, P, J).to(dev).eval()
    with torch.no_grad():
        joint.ffn_out.weight *= 10
        joint.ffn_out.bias[0] += 16.0
    plain_joint = w.TransducerJoint(V, E, P, J).to(dev).eval()
    plain_joint.load_state_dict({k: (v[:V] if k.startswith("ffn_out.") else v) for k, v in joint.state_dict().items()})
    ctc = w.CTC(V, E).to(dev).eval()
    enc = torch.randn(B, T, E, device=dev)
    with torch.no_grad():
        ctc_logp = ctc.log_softmax(enc)
    chunks = [(enc[:, p:p + C].contiguous(), ctc_logp[:, p:p + C].contiguous(),
               torch.full((B,), min(C, T - p), dtype=torch.int32, device=dev)) for p in range(0, T, C)]
    phrases = torch.randint(1, V, (1000, 3), generator=torch.Generator().manual_seed(7)).tolist()
    graphs = {"empty graph": w.ContextGraph([], 3.0), "1000 phrases": w.ContextGraph(phrases, 3.0)}

    for name, jn, durations, mix in (("plain", plain_joint, None, (0.3, 0.7)), ("tdt", joint, tuple(range(D)), (0.0, 1.0))):
        if args.only and name not in args.only.split(","):
            continue
        plain_dec, ctx_dec = DeviceDecoder(pred, jn, B * beam, B, T, 0, beam), DeviceDecoder(pred, jn, B * beam, B, T, 0, beam)
        plain_dec.attach_beam_stream(B, beam, T)
        ctx_dec.attach_beam_context_stream(B, beam, T)
        post = (lambda c: c) if durations is None else (lambda c: None)

        def run(graph):
            out = None
            for i, (e, c, n) in enumerate(chunks):
                kw = dict(ctc_logp=post(c), ctc_weight=mix[0], transducer_weight=mix[1], durations=durations, reset=i == 0,
                          final=i == len(chunks) - 1)
                if graph is None:
                    out = plain_dec.prefix_beam_chunk(e, n, beam, 0, **kw)
                else:
                    out = ctx_dec.prefix_beam_context_chunk(e, n, beam, 0, graph, finalize=i == len(chunks) - 1, **kw)
            return out

        variants = [("unbiased stream", None)] + list(graphs.items())
        times = {k: [] for k, _ in variants}
        outs = {}
        for r in range(args.reps + 1):
            for k, g in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                outs[k] = run(g)
                torch.cuda.synchronize()
                if r > 0:
                    times[k].append(time.perf_counter() - t0)
        base = {"model": name, "durations": durations, "B": B, "T": T, "beam": beam, "chunk_frames": C, "chunks": len(chunks),
                "rounds": args.reps}
        for k, g in variants:
            med = statistics.median(times[k])
            line = {"what": k, **base, "ms_per_utterance": round(med * 1e3, 2), "ms_per_chunk": round(med * 1e3 / len(chunks), 4),
                    "min_ms": round(min(times[k]) * 1e3, 2), "max_ms": round(max(times[k]) * 1e3, 2)}
            if g is not None:
                line["over_unbiased"] = round(statistics.median(a / b for a, b in zip(times[k], times["unbiased stream"])), 4)
                line["states"], line["arcs"] = g.n_states, g.n_arcs
                if g.n_arcs == 0:
                    line["equals_unbiased"] = [[x[:4] for x in u] for u in outs[k]] == outs["unbiased stream"]
                else:
                    line["hyps_with_bonus"] = sum(1 for u in outs[k] for x in u if x[5] != 0.0)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["joint", "ctc", "ctcdec", "greedy", "beam", "step", "hotword", "align", "simple", "smoothed", "pruned", "tdt",
                                     "tdtstep", "tdtalign", "tdtdec", "tdtbeam", "ctcstream", "ctcctx", "beamstream", "beamctx"])
    ap.add_argument("--chunk-frames", type=int, default=16, help="beamstream: encoder frames per chunk")
    ap.add_argument("--durations", type=int, default=5, help="tdt, tdtstep, tdtalign: number of durations D (the set is 0 .. D-1)")
    ap.add_argument("--n-steps", type=int, default=64)
    ap.add_argument("--chunks", type=int, default=4)
    ap.add_argument("--B", type=int, default=None, help="batch size (default 32; simple, smoothed, pruned, tdt, tdtstep, tdtalign: 16)")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--U", type=int, default=150)
    ap.add_argument("--V", type=int, default=5000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--R", type=int, default=5, help="pruned: label positions per frame (s_range)")
    ap.add_argument("--rnnt-type", default="regular", choices=["regular", "modified"],
                    help="simple, smoothed, pruned: also time this lattice type beside the regular form")
    ap.add_argument("--delay-penalty", type=float, default=0.0,
                    help="simple, smoothed, pruned: also time this delay penalty beside the regular form; step: the "
                         "full-lattice loss's delay_penalty, timed beside (0, 0)")
    ap.add_argument("--fastemit-lambda", type=float, default=0.0,
                    help="step: the full-lattice loss's fastemit_lambda, timed beside (0, 0)")
    ap.add_argument("--reps", type=int, default=9, help="step: alternating rounds of the latency-option timings")
    ap.add_argument("--dw", action="store_true", help="joint: also time the library fp32 GEMM on the three contractions (yardstick)")
    ap.add_argument("--fwd-only", action="store_true", help="joint: stop after the exact forward sweep")
    ap.add_argument("--ragged", action="store_true", help="step: frames in [0.8 T, T] sorted, labels in [U/3, U]")
    ap.add_argument("--buckets", type=int, default=4, help="step: label-length groups of the fused node (1 = off)")
    ap.add_argument("--only", default="", help="step: comma-separated subset of the configurations; simple: \"simple\" "
                                              "skips the composite; pruned: \"pruned\" skips the full-lattice siblings; tdt: \"tdt\", "
                                              "tdtalign: \"tdtalign\" run one call of each entry point (for a profiler)")
    ap.add_argument("--budget-mb", type=float, default=0.0,
                    help="step: time the memory-bounded fused node (logits_budget = this many MiB) beside the plain one, "
                         "fp32 and bf16x3, with max_memory_allocated of each")
    ap.add_argument("--streams", type=int, default=64, help="greedy: independent streams decoded together")
    ap.add_argument("--tile", type=int, default=0, help="lane-GEMM tile policy of the decoders (wr_tune_set key 6)")
    a = ap.parse_args()
    if a.B is None:
        a.B = 16 if a.what in ("simple", "smoothed", "pruned", "tdt", "tdtstep", "tdtalign") else 32
    if a.tile:
        from wenet_celoss_amd import _lib
        _lib.load().wr_tune_set(6, a.tile)
    {"joint": bench_joint, "ctc": bench_ctc, "greedy": bench_greedy, "beam": bench_beam, "step": bench_step, "ctcdec": bench_ctcdec, "hotword": bench_hotword,
     "align": bench_align, "simple": bench_simple, "smoothed": bench_smoothed, "pruned": bench_pruned,
     "tdt": bench_tdt, "tdtstep": bench_tdtstep, "tdtalign": bench_tdtalign, "tdtdec": bench_tdtdec,
     "tdtbeam": bench_tdtbeam, "ctcstream": bench_ctcstream, "ctcctx": bench_ctcctx, "beamstream": bench_beamstream,
     "beamctx": bench_beamctx}[a.what](a)
