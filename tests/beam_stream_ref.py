"""Float64 reference of the streaming transducer prefix beam search (include/wr_api.h, "Streaming transducer prefix beam
search"): the rule of tests/tdt_beam_ref.py continued across encoder chunks, where every entry also carries a Viterbi score
and the frame of each of its tokens.

Plain module (not a conftest): test_beam_stream_ref.py checks it on scripted joiner rows with hand-worked answers, the GPU
tests in test_beam_stream_gpu.py compare the device search with it.  Written from the rule, not from the kernels:

  entry = (tokens, t, score, vscore, times); the seed is ((blank,), 0, 0.0, 0.0, ()), frames are absolute
  a chunk adds frames: F += width.  A final chunk first sets T = F, clamps every t > T to T, fuses and stably re-sorts.
  while an entry has t < F:  the step of tdt_beam_ref.search with
    an arc of an entry (t, pair value v): score and vscore each float32(.) + float32(v); times + (t,) for a label
    t' = t + max(d, 1), clamped to T only in a final chunk
    fusion: score by log_add in pool order; vscore the maximum of the members, times those of the member holding it, an
      exact tie to the first in pool order

The plain search is the rule with durations = (1,): a row then has V columns and the duration part is log 1 = 0.
"""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

from tdt_beam_ref import Modules, Scripted, log_add, log_softmax  # noqa: F401  (re-exported for the tests)

# beam: [(tokens incl. the seed blank, t, score, vscore, times)] best first; margin: the margin of tdt_beam_ref.search plus,
# for every class with more than one member, the gap between its two largest member vscores (the decision that is new);
# steps: steps taken, over all chunks; after: the beam after every chunk
Result = namedtuple("Result", "beam margin steps after")


def search(source, widths, V, durations, beam, blank=0, ctc_logp=None, ctc_weight=0.0, transducer_weight=1.0, final=True,
           trace=None):
    """`source.row(t, tokens)` as in tdt_beam_ref.search, with V + len(durations) columns -- or V columns when `durations`
    is None (the plain search).  `widths`: the chunk widths; the last chunk is the final one if `final`.  ctc_logp
    [sum(widths), V] or None.  `trace`: a list that receives the beam after the begin of a final chunk and after every
    step."""
    plain = durations is None
    durs = (1,) if plain else tuple(durations)
    D = len(durs)
    tw, cw = float(np.float32(transducer_weight)), float(np.float32(ctc_weight))
    entries = [((blank,), 0, 0.0, 0.0, ())]
    margin, steps = math.inf, 0
    after = []

    def gap(a, b):
        nonlocal margin
        g = a - b
        if math.isfinite(g):
            margin = min(margin, g)

    def fuse_sort(pool):
        fused = []
        for toks, t, sc, vs, tm in pool:
            for c in fused:
                if c[0] == toks and c[1] == t:
                    c[2] = log_add(c[2], sc)
                    c[5].append(vs)
                    if vs > c[3]:                              # strictly: a tie stays with the first in pool order
                        c[3], c[4] = vs, tm
                    break
            else:
                fused.append([toks, t, sc, vs, tm, [vs]])
        for c in fused:
            if len(c[5]) > 1:
                top = sorted(c[5], reverse=True)
                gap(top[0], top[1])
        fused.sort(key=lambda c: -c[2])                        # stable
        for a, b in zip(fused[:beam], fused[1:beam + 1]):
            gap(a[2], b[2])
        return [tuple(c[:5]) for c in fused[:beam]]

    F = 0
    for ci, width in enumerate(widths):
        F += width
        last = final and ci == len(widths) - 1
        T = F if last else None
        if last:
            entries = fuse_sort([(toks, min(t, T), sc, vs, tm) for toks, t, sc, vs, tm in entries])
            if trace is not None:
                trace.append(list(entries))
        while any(e[1] < F for e in entries):
            f = min(e[1] for e in entries)
            pool = []
            for toks, t, score, vscore, tm in entries:
                if t != f:
                    pool.append((toks, t, score, vscore, tm))
                    continue
                row = np.array(source.row(t, toks), dtype=np.float64).reshape(-1)
                assert row.size == (V if plain else V + D), (row.size, V, D)
                mix = log_softmax(row[:V])
                ld = np.zeros(1) if plain else log_softmax(row[V:])
                if ctc_logp is not None:
                    mix = np.log(tw * np.exp(mix) + cw * np.exp(np.asarray(ctc_logp[t], dtype=np.float64)))
                order = np.argsort(-mix, kind="stable")
                top = order[:beam]
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
                    pool.append((toks, tn, sc, vs, tm) if k == blank else (toks + (k,), tn, sc, vs, tm + (t,)))
            entries = fuse_sort(pool)
            steps += 1
            if trace is not None:
                trace.append(list(entries))
        after.append(list(entries))
    return Result(entries, margin, steps, after)


def decode(predictor, joint, enc, lens, V, durations, beam, blank=0, ctc_logp=None, ctc_weight=0.0, transducer_weight=1.0,
           widths=None, final=True):
    """One Result per utterance of enc (B, T, E) with lengths `lens`; ctc_logp (B, T, V) or None.  `widths`: the chunk
    widths every utterance is cut into (an utterance takes what is left of its frames from each chunk, possibly nothing);
    None: one chunk."""
    out = []
    for b in range(enc.shape[0]):
        n = int(lens[b])
        cut, left = [], n
        for w in (widths or [n]):
            cut.append(min(w, left))
            left -= cut[-1]
        assert left == 0, "the chunk widths do not cover the utterance"
        out.append(search(Modules(predictor, joint, enc[b]), cut, V, durations, beam, blank,
                          None if ctc_logp is None else np.asarray(ctc_logp[b]), ctc_weight, transducer_weight, final))
    return out
