"""Float64 reference of context-graph biasing in the streaming transducer prefix beam search (include/wr_api.h,
"Context-graph biasing in the streaming transducer prefix beam search"): the rule of tests/beam_stream_ref.py where every
entry also walks a ContextGraph and the beam is pruned by score plus bonus.

Plain module (not a conftest): test_beam_context_ref.py checks it on scripted joiner rows with hand-worked answers, the GPU
tests in test_beam_context_gpu.py compare the device search with it.  Written from the header text, on top of
beam_stream_ref / tdt_beam_ref (their log_add, log_softmax and row sources) and ContextGraph.next:

  entry = (tokens, t, score, vscore, times, ctx_state, ctx_score, tags); the seed is ((blank,), 0, 0.0, 0.0, (), 0, 0.0, ())
  a waiting entry and a blank arc copy the three new fields; a label arc appending k, whatever its duration, takes
    (st, sc, start, end) = graph.next(ctx_state, k): ctx_state = st, ctx_score += sc (float64), tags + (start | end << 1,)
  score and vscore are beam_stream_ref's: float32(.) + float32(v), the bonus never enters them
  fusion as there; all members of a class agree on the three fields (asserted on every class), the representative's stay
  prune, and the fuse-and-re-sort of a final chunk: stable, descending by total = fused score + ctx_score; the first `beam`
  export after a chunk: (tokens, total, vscore, times, score, ctx_score, tags, ctx_state) in beam order; finalised: an entry
    with ctx_state != 0 gains float(escape[ctx_state]) in the exported bonus and the list is stably re-sorted by the new
    totals; the entries themselves are not changed
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from beam_stream_ref import Modules, Scripted, log_add, log_softmax  # noqa: F401  (re-exported for the tests)

# beam: the entries after the last chunk, best first; margin: the margin of beam_stream_ref.search where the sort's key is the
# total -- the token and pair rank-`beam` boundaries of every expansion, the two largest member vscores of every class with
# more than one member, the gap between every neighbouring pair of TOTALS down to the first pruned class in every step's (and
# every final begin's) sorted list -- and between neighbours of every finalised export list; steps; after: the entries after
# every chunk; exports: what every chunk's call returns; stats: what the bonus did (Stats)
Result = namedtuple("Result", "beam margin steps after exports stats")


class Stats:
    """saved: prunes in which the first `beam` by total are not the first `beam` by pure score; taken_back: label arcs that
    broke a partial match and gave bonus back (escape != 0); reordered: finalised exports whose order differs from the
    beam's; finalised_back: entries whose exported bonus a finalisation lowered; walked: label arcs that took a graph arc"""

    def __init__(self):
        self.saved = self.taken_back = self.reordered = self.finalised_back = self.walked = 0

    def __repr__(self):
        return (f"Stats(saved={self.saved}, taken_back={self.taken_back}, reordered={self.reordered}, "
                f"finalised_back={self.finalised_back}, walked={self.walked})")


def export(entries, graph, finalize):
    """[(tokens, total, vscore, times, score, ctx_score, tags, ctx_state)] of a beam, finalised or not"""
    rows = []
    for toks, _, sc, vs, tm, st, cx, tg in entries:
        if finalize and st != 0:
            cx = cx + float(graph.escape[st])
        rows.append((toks, sc + cx, vs, tm, sc, cx, tg, st))
    if finalize:
        rows.sort(key=lambda r: -r[1])                         # stable
    return rows


def search(source, widths, V, durations, beam, graph, blank=0, ctc_logp=None, ctc_weight=0.0, transducer_weight=1.0,
           final=True, finalize=None, trace=None):
    """beam_stream_ref.search with the context graph `graph` (a ContextGraph).  `finalize`: one bool per chunk -- that
    chunk's export is finalised; None: the last chunk's is, if it is final.  `trace`: a list that receives the beam after the
    begin of a final chunk and after every step."""
    plain = durations is None
    durs = (1,) if plain else tuple(durations)
    D = len(durs)
    tw, cw = float(np.float32(transducer_weight)), float(np.float32(ctc_weight))
    entries = [((blank,), 0, 0.0, 0.0, (), 0, 0.0, ())]
    margin, steps = math.inf, 0
    after, exports, stats = [], [], Stats()
    if finalize is None:
        finalize = [final and ci == len(widths) - 1 for ci in range(len(widths))]
    assert len(finalize) == len(widths)

    def gap(a, b):
        nonlocal margin
        g = a - b
        if math.isfinite(g):
            margin = min(margin, g)

    def fuse_sort(pool):
        fused = []
        for toks, t, sc, vs, tm, st, cx, tg in pool:
            for c in fused:
                if c[0] == toks and c[1] == t:
                    # purity: the three fields are a function of the tokens alone
                    assert (c[5], c[6], c[7]) == (st, cx, tg), ("members of a class disagree", toks, c[5:8], (st, cx, tg))
                    c[2] = log_add(c[2], sc)
                    c[8].append(vs)
                    if vs > c[3]:                              # strictly: a tie stays with the first in pool order
                        c[3], c[4] = vs, tm
                    break
            else:
                fused.append([toks, t, sc, vs, tm, st, cx, tg, [vs]])
        for c in fused:
            if len(c[8]) > 1:
                top = sorted(c[8], reverse=True)
                gap(top[0], top[1])
        pure = sorted(fused, key=lambda c: -c[2])[:beam]       # what the unbiased prune would keep
        fused.sort(key=lambda c: -(c[2] + c[6]))               # stable; one float64 add
        for a, b in zip(fused[:beam], fused[1:beam + 1]):
            gap(a[2] + a[6], b[2] + b[6])
        if any(all(k is not q for q in pure) for k in fused[:beam]):
            stats.saved += 1
        return [tuple(c[:8]) for c in fused[:beam]]

    F = 0
    for ci, width in enumerate(widths):
        F += width
        last = final and ci == len(widths) - 1
        T = F if last else None
        if last:
            entries = fuse_sort([(e[0], min(e[1], T)) + e[2:] for e in entries])
            if trace is not None:
                trace.append(list(entries))
        while any(e[1] < F for e in entries):
            f = min(e[1] for e in entries)
            pool = []
            for ent in entries:
                toks, t, score, vscore, tm, st, cx, tg = ent
                if t != f:
                    pool.append(ent)
                    continue
                row = np.array(source.row(t, toks), dtype=np.float64).reshape(-1)
                assert row.size == (V if plain else V + D), (row.size, V, D)
                mix = log_softmax(row[:V])
                ld = np.zeros(1) if plain else log_softmax(row[V:])
                if ctc_logp is not None:
                    mix = np.log(tw * np.exp(mix) + cw * np.exp(np.asarray(ctc_logp[t], dtype=np.float64)))
                order = np.argsort(-mix, kind="stable")
                top = order[:beam]                             # the first prune is unbiased
                if V > beam:
                    gap(mix[order[beam - 1]], mix[order[beam]])
                pairs = [(mix[k] + ld[j], r, j) for r, k in enumerate(top) for j in range(D)]
                pairs.sort(key=lambda p: -p[0])                # stable: r, then j on ties
                if len(pairs) > beam:
                    gap(pairs[beam - 1][0], pairs[beam][0])
                for v, r, j in pairs[:beam]:
                    k = int(top[r])
                    sc = float(np.float32(score) + np.float32(v))
                    vs = float(np.float32(vscore) + np.float32(v))
                    tn = t + max(durs[j], 1)
                    if last:
                        tn = min(tn, T)
                    if k == blank:
                        pool.append((toks, tn, sc, vs, tm, st, cx, tg))
                        continue
                    nst, nsc, start, end = graph.next(st, k)   # once per token, whatever the duration
                    if nst != 0 or end:                        # an arc was taken (a leaf's arc ends at the root, final)
                        stats.walked += 1
                    elif nsc != 0.0:                           # a miss away from the root and from a final state
                        stats.taken_back += 1
                    pool.append((toks + (k,), tn, sc, vs, tm + (t,), nst, cx + float(nsc), tg + (int(start) | int(end) << 1,)))
            entries = fuse_sort(pool)
            steps += 1
            if trace is not None:
                trace.append(list(entries))
        after.append(list(entries))
        rows = export(entries, graph, finalize[ci])
        if finalize[ci]:
            for a, b in zip(rows, rows[1:]):
                gap(a[1], b[1])
            if [r[0] for r in rows] != [e[0] for e in entries]:
                stats.reordered += 1
            stats.finalised_back += sum(1 for e in entries if e[5] != 0 and float(graph.escape[e[5]]) != 0.0)
        exports.append(rows)
    return Result(entries, margin, steps, after, exports, stats)


def decode(predictor, joint, enc, lens, V, durations, beam, graph, blank=0, ctc_logp=None, ctc_weight=0.0,
           transducer_weight=1.0, widths=None, final=True, finalize=None):
    """One Result per utterance of enc (B, T, E) with lengths `lens`, as beam_stream_ref.decode."""
    out = []
    for b in range(enc.shape[0]):
        n = int(lens[b])
        cut, left = [], n
        for w in (widths or [n]):
            cut.append(min(w, left))
            left -= cut[-1]
        assert left == 0, "the chunk widths do not cover the utterance"
        out.append(search(Modules(predictor, joint, enc[b]), cut, V, durations, beam, graph, blank,
                          None if ctc_logp is None else np.asarray(ctc_logp[b]), ctc_weight, transducer_weight, final, finalize))
    return out


def outputs(result, start_tag_id, end_tag_id):
    """UpdateOutputs on an exported list: the tokens after the seed blank, the start tag in front of a token with bit 0,
    the end tag behind a token with bit 1."""
    outs = []
    for hyp in result:
        o = []
        for tok, tag in zip(hyp[0][1:], hyp[6]):
            if tag & 1:
                o.append(start_tag_id)
            o.append(tok)
            if tag & 2:
                o.append(end_tag_id)
        outs.append(o)
    return outs


def phrases_from(tokens):
    """Phrases for a test graph from a hypothesis (ctc_context_ref.phrases_from): its tokens cut into pieces of 2, 3, 2, 3,
    ... tokens (a shorter last piece is kept), plus one nested pair -- the first piece extended by the token that follows."""
    tokens = [int(t) for t in tokens]
    out, i, w = [], 0, 2
    while i < len(tokens):
        out.append(tokens[i:i + w])
        i += w
        w = 5 - w
    if out and len(tokens) > len(out[0]):
        out.append(tokens[:len(out[0]) + 1])
    return out
