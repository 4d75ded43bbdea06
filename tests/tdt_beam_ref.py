"""Float64 reference of the token-and-duration (TDT) prefix beam search (include/wr_api.h, "TDT prefix beam search").

Plain module (not a conftest): test_tdt_beam_ref.py checks it on scripted joiner rows with hand-worked answers, the GPU
tests in test_tdt_beam_gpu.py compare the device search with it.  Written from the rule, not from the kernels:

  beam = [([blank], t = 0, score 0.0)], best first; while an entry has t < T:
    f = min t; entries with t == f are expanded, the others wait as they are
    expanded entry: l = log_softmax(row[:V]), ld = log_softmax(row[V:]) of the row for (frame t, predictor stepped on its
      last token); mix = l, or log(tw * exp(l) + cw * exp(ctc[t])); the `beam` best tokens by mix (ties: lowest index) get
      ranks r; of the beam x D pairs v = mix[k_r] + ld[j] the best `beam` (ties: lower r, then lower j) become arcs with
      score float32(score) + float32(v), t' = min(t + max(durations[j], 1), T), tokens + [k] unless k is blank
    pool in beam order (a waiting entry itself, an expanded entry's arcs in their order); entries with equal tokens and equal
    t' fuse into the first of them with float64 log_add in pool order; stable sort, descending; the first `beam` stay

The predictor state of a hypothesis is a function of its tokens, so a source is asked for `row(t, tokens)`.
"""
from __future__ import annotations

import copy
import math
from collections import namedtuple

import numpy as np
import torch

# beam: [(tokens incl. the seed blank, t, score)] best first; margin: the smallest gap that decided anything visible -- at
# the token rank-`beam` boundary and the pair rank-`beam` boundary of every expansion, and between neighbours of the sorted
# fused classes down to the first pruned one, over all steps; steps: steps taken; expanded: entries expanded in all;
# fused: pool entries that joined an earlier entry's class, in all steps
Result = namedtuple("Result", "beam margin steps expanded fused")


def log_softmax(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    return x - m - math.log(np.exp(x - m).sum())


def log_add(a, b):
    if a == -math.inf and b == -math.inf:
        return -math.inf
    mx, mn = max(a, b), min(a, b)
    return mx + math.log(1.0 + math.exp(mn - mx))


def search(source, T, V, durations, beam, blank=0, ctc_logp=None, ctc_weight=0.0, transducer_weight=1.0, dup=(), trace=None):
    """`source.row(t, tokens)`: the V + D logits of frame t against the predictor stepped on tokens[-1] from the state
    that tokens[:-1] left.  ctc_logp [T, V] or None.  `dup` {column: lower column} (the exact-tie tests): columns whose
    weights are copies of a lower column's; their logits ARE the lower column's (a CPU BLAS need not round two equal
    columns alike, so the value is copied), and a gap of exactly 0.0, which only such a copy produces and which the index
    rules decide, is left out of the margin.  `trace`: a list that receives the beam after every step."""
    dup = dict(dup)
    D = len(durations)
    tw, cw = float(np.float32(transducer_weight)), float(np.float32(ctc_weight))
    entries = [((blank,), 0, 0.0)]
    margin, steps, expanded, n_fused = math.inf, 0, 0, 0

    def gap(a, b):
        nonlocal margin
        g = a - b
        if math.isfinite(g) and not (dup and g == 0.0):
            margin = min(margin, g)

    while any(t < T for _, t, _ in entries):
        f = min(t for _, t, _ in entries)
        pool = []
        for toks, t, score in entries:
            if t != f:
                pool.append((toks, t, score))
                continue
            expanded += 1
            row = np.array(source.row(t, toks), dtype=np.float64).reshape(-1)
            assert row.size == V + D, (row.size, V, D)
            for hi, lo in dup.items():
                assert lo < hi
                row[hi] = row[lo]
            mix, ld = log_softmax(row[:V]), log_softmax(row[V:])
            if ctc_logp is not None:
                mix = np.log(tw * np.exp(mix) + cw * np.exp(np.asarray(ctc_logp[t], dtype=np.float64)))
            order = np.argsort(-mix, kind="stable")
            top = order[:beam]
            if V > beam:
                gap(mix[order[beam - 1]], mix[order[beam]])
            pairs = [(mix[k] + ld[j], r, j) for r, k in enumerate(top) for j in range(D)]
            pairs.sort(key=lambda p: -p[0])                    # stable: r, then j on ties
            if len(pairs) > beam:
                gap(pairs[beam - 1][0], pairs[beam][0])
            for v, r, j in pairs[:beam]:
                k = int(top[r])
                sc = float(np.float32(score) + np.float32(v))
                pool.append((toks if k == blank else toks + (k,), min(t + max(durations[j], 1), T), sc))
        fused = []
        for toks, t, sc in pool:
            for c in fused:
                if c[0] == toks and c[1] == t:
                    c[2] = log_add(c[2], sc)
                    n_fused += 1
                    break
            else:
                fused.append([toks, t, sc])
        fused.sort(key=lambda c: -c[2])                        # stable
        for a, b in zip(fused[:beam], fused[1:beam + 1]):
            gap(a[2], b[2])
        entries = [tuple(c) for c in fused[:beam]]
        steps += 1
        if trace is not None:
            trace.append(list(entries))
    return Result(entries, margin, steps, expanded, n_fused)


class Scripted:
    """Joiner rows from a table keyed by (frame, tokens); a row the table lacks must not be consulted."""

    def __init__(self, table):
        self.table = table

    def row(self, t, toks):
        return self.table[(t, toks)]


class Modules:
    """Float64 CPU copies of a predictor and a joiner of the package (their plain torch graphs) over one utterance's
    encoder frames enc (T, E); predictor steps are kept per token sequence."""

    def __init__(self, predictor, joint, enc):
        self.pred = copy.deepcopy(predictor).cpu().double().eval()
        self.joint = copy.deepcopy(joint).cpu().double().eval()
        self.enc = enc.detach().cpu().double()
        self.pad = torch.zeros(1, 1, dtype=torch.double)
        self.memo = {}

    def _step(self, toks):
        got = self.memo.get(toks)
        if got is None:
            if len(toks) == 1:
                state = [s.double() for s in self.pred.init_state(1, device=torch.device("cpu"))]
            else:
                state = self._step(toks[:-1])[1]
            with torch.no_grad():
                got = self.memo[toks] = self.pred._export_step(torch.tensor([[toks[-1]]]), self.pad, state)
        return got

    def row(self, t, toks):
        with torch.no_grad():
            return self.joint._export_forward(self.enc[None, t:t + 1], self._step(toks)[0]).reshape(-1).numpy()


def decode(predictor, joint, enc, lens, V, durations, beam, blank=0, ctc_logp=None, ctc_weight=0.0, transducer_weight=1.0,
           dup=()):
    """One Result per utterance of enc (B, T, E) with lengths `lens`; ctc_logp (B, T, V) or None."""
    return [search(Modules(predictor, joint, enc[b]), int(lens[b]), V, durations, beam, blank,
                   None if ctc_logp is None else np.asarray(ctc_logp[b]), ctc_weight, transducer_weight, dup)
            for b in range(enc.shape[0])]
