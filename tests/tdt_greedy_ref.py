"""Float64 reference of the token-and-duration (TDT) greedy search (include/wr_api.h, "TDT greedy search").

Plain module (not a conftest): test_tdt_greedy_ref.py checks it on scripted joiner rows with hand-worked answers, the GPU
tests in test_tdt_greedy_gpu.py compare the device search with it.  Written from the rule, not from the product's loop:

  t = 0, nb = 0; while t < T:
      k = argmax of the token part of the row for (frame t, predictor state), j = argmax of its duration part
      d = durations[j]
      k == blank:  t += max(d, 1); nb = 0
      otherwise:   emit k at frame t; the predictor steps on k; nb = 0 if d > 0 else nb + 1; t += d
                   if nb >= n_steps: t += 1; nb = 0

numpy's argmax takes the lowest index on an exact tie.  `durations=None` is the plain transducer rule over the whole row
(every label stays on its frame, a blank moves one frame on): the rule above with d = 0 throughout.
"""
from __future__ import annotations

import copy
from collections import namedtuple

import numpy as np
import torch

# tokens, frames: the emissions and the frame of each; gap: the smallest top-1 / top-2 difference over every token and
# every duration decision; trace: one (t, k, d) per decision, in order; end: the value of t that ended the loop
Result = namedtuple("Result", "tokens frames gap trace end")


def _gap(part, dup):
    keep = [i for i in range(len(part)) if i not in dup]
    if len(keep) < 2:
        return float("inf")
    top = np.sort(np.asarray(part, dtype=np.float64)[keep])
    return float(top[-1] - top[-2])


def walk(source, T, V, durations, blank=0, n_steps=64, dup=()):
    """`source.row(t)` gives the V + D logits of frame t against the current predictor state, `source.emit(k)` steps the
    predictor on k.  `dup` {column: lower column} (the exact-tie tests): columns whose weights are copies of a lower
    column's.  Their logits ARE the lower column's -- a CPU BLAS need not round two equal columns alike, so the value is
    copied; they take part in the argmax and are left out of the gap."""
    dup = dict(dup)
    t, nb, gap = 0, 0, float("inf")
    tokens, frames, trace = [], [], []
    while t < T:
        row = np.array(source.row(t), dtype=np.float64).reshape(-1)
        for hi, lo in dup.items():
            assert lo < hi
            row[hi] = row[lo]
        if durations is None:
            tok, d = row, 0
        else:
            assert row.size == V + len(durations), (row.size, V, durations)
            tok, dur = row[:V], row[V:]
            d = durations[int(np.argmax(dur))]
            gap = min(gap, _gap(dur, {c - V for c in dup if c >= V}))
        k = int(np.argmax(tok))
        gap = min(gap, _gap(tok, {c for c in dup if c < V}))
        trace.append((t, k, d))
        if k == blank:
            t += max(d, 1)
            nb = 0
            continue
        tokens.append(k)
        frames.append(t)
        source.emit(k)
        nb = 0 if d > 0 else nb + 1
        t += d
        if nb >= n_steps:
            t += 1
            nb = 0
    return Result(tokens, frames, gap, trace, t)


class Scripted:
    """Joiner rows from a table keyed by (frame, tokens emitted so far); a row the table lacks must not be consulted."""

    def __init__(self, table):
        self.table, self.u = table, 0

    def row(self, t):
        return self.table[(t, self.u)]

    def emit(self, k):
        self.u += 1


class Modules:
    """Float64 CPU copies of a predictor and a joiner of the package (their plain torch graphs) over one stream's
    encoder frames enc (T, E)."""

    def __init__(self, predictor, joint, enc, blank=0):
        self.pred = copy.deepcopy(predictor).cpu().double().eval()
        self.joint = copy.deepcopy(joint).cpu().double().eval()
        self.enc = enc.detach().cpu().double()
        self.pad = torch.zeros(1, 1, dtype=torch.double)
        self.state = [s.double() for s in self.pred.init_state(1, device=torch.device("cpu"))]
        self._step(blank)

    def _step(self, k):
        with torch.no_grad():
            self.out, self.new_state = self.pred._export_step(torch.tensor([[k]]), self.pad, self.state)

    def row(self, t):
        with torch.no_grad():
            return self.joint._export_forward(self.enc[None, t:t + 1], self.out).reshape(-1).numpy()

    def emit(self, k):
        self.state = self.new_state
        self._step(k)


def decode(predictor, joint, enc, lens, V, durations, blank=0, n_steps=64, dup=()):
    """One Result per stream of enc (N, T, E) with lengths `lens`."""
    return [walk(Modules(predictor, joint, enc[n], blank), int(lens[n]), V, durations, blank, n_steps, dup)
            for n in range(enc.shape[0])]
