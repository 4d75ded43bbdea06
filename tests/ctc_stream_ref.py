"""Float64 reference of the streaming CTC prefix beam search with Viterbi scores and token times, numpy only.

Written from the contract in include/wr_api.h ("Streaming CTC prefix beam search"), which restates
runtime/core/decoder/ctc_prefix_beam_search.cc:107-211 in the Python search's visiting order (symbol outer, entries
inner).  The summed scores follow tests/ctc_decode_ref.py statement for statement, so hypotheses and scores equal
`prefix_beam_search_logp` value for value.

  Stream(beam, blank)            one stream's state: `a_next` and `entries`; `consume(logp_rows)` runs frames,
                                 `nbest()` exports [(tokens, score, viterbi, times)]
  search_logp(logp, T, beam, blank, chunks=None)     whole search from log-probabilities, optionally chunked
  search(logits_f32, T, beam, blank, chunks=None)    the same from fp32 logits (float64 log-softmax)

Statistics (class StreamStats) extend ctc_decode_ref.Stats to the Viterbi decisions: `min_gap` / `ties` also cover
every `vnb < candidate` comparison with both sides finite and every `vb > vnb` choice of a non-empty prefix; `kept`
counts how often vnb improved while `ctp < p` was false, so that the times were kept.
"""
from dataclasses import dataclass

import numpy as np

from ctc_decode_ref import NINF, Stats, log_add, log_softmax_f64, peaky_logits  # noqa: F401


@dataclass
class StreamStats(Stats):
    kept: int = 0

    def decide_any(self, x, y):
        """One comparison between two finite values, whichever is larger."""
        self.decide(max(x, y), min(x, y))


class Entry:
    __slots__ = ("tokens", "pb", "pnb", "vb", "vnb", "times_b", "times_nb", "ctp")

    def __init__(self, tokens=(), pb=NINF, pnb=NINF, vb=NINF, vnb=NINF, times_b=(), times_nb=()):
        self.tokens, self.pb, self.pnb, self.vb, self.vnb = tokens, pb, pnb, vb, vnb
        self.times_b, self.times_nb, self.ctp = times_b, times_nb, NINF

    def vit(self):
        return self.vb if self.vb > self.vnb else self.vnb

    def times(self):
        return self.times_b if self.vb > self.vnb else self.times_nb

    def score(self):
        return log_add([self.pb, self.pnb])


class Stream:
    def __init__(self, beam, blank=0, stats=None):
        self.beam, self.blank = beam, blank
        self.stats = stats if stats is not None else StreamStats()
        self.reset()

    def reset(self):
        self.a_next = 0
        self.entries = [Entry((), 0.0, NINF, 0.0, 0.0)]

    def _choice(self, e):
        if len(e.tokens) > 0:
            self.stats.decide_any(e.vb, e.vnb)

    def _frame(self, row):
        st, beam, blank, a = self.stats, self.beam, self.blank, self.a_next
        V = row.shape[0]
        st.max_ncur = max(st.max_ncur, len(self.entries))
        nxt, bases = {}, {}
        full = np.argsort(-row, kind="stable")
        if beam < V:
            st.decide(float(row[full[beam - 1]]), float(row[full[beam]]))
        slots = 0

        def key(tokens, bi):
            bases.setdefault(tokens, set()).add(bi)
            if tokens not in nxt:
                nxt[tokens] = Entry(tokens)
            return nxt[tokens]

        def improve(n, cand):
            st.decide_any(n.vnb, cand)
            return n.vnb < cand

        for s in full[:beam]:
            s = int(s)
            p = float(row[s])
            for bi, e in enumerate(self.entries):
                last = e.tokens[-1] if len(e.tokens) > 0 else None
                if s == blank:
                    n = key(e.tokens, bi)
                    n.pb = log_add([n.pb, e.pb + p, e.pnb + p])
                    self._choice(e)
                    n.vb = e.vit() + p
                    n.times_b = e.times()
                    slots += 1
                elif s == last:
                    n = key(e.tokens, bi)
                    n.pnb = log_add([n.pnb, e.pnb + p])
                    if improve(n, e.vnb + p):
                        n.vnb = e.vnb + p
                        if n.ctp < p:
                            n.ctp = p
                            n.times_nb = e.times_nb[:-1] + (a,)
                        else:
                            st.kept += 1
                    n = key(e.tokens + (s,), bi)
                    n.pnb = log_add([n.pnb, e.pb + p])
                    if improve(n, e.vb + p):
                        n.vnb, n.ctp, n.times_nb = e.vb + p, p, e.times_b + (a,)
                    slots += 2
                    st.pairs += 1
                else:
                    n = key(e.tokens + (s,), bi)
                    n.pnb = log_add([n.pnb, e.pb + p, e.pnb + p])
                    self._choice(e)
                    if improve(n, e.vit() + p):
                        n.vnb, n.ctp, n.times_nb = e.vit() + p, p, e.times() + (a,)
                    slots += 1
        st.max_slots = max(st.max_slots, slots)
        st.merges += sum(1 for v in bases.values() if len(v) > 1)
        nh = sorted(nxt.values(), key=lambda n: n.score(), reverse=True)       # stable
        if len(nh) > beam:
            st.decide(nh[beam - 1].score(), nh[beam].score())
        self.entries = nh[:beam]
        self.a_next += 1

    def consume(self, logp_rows):
        for row in np.asarray(logp_rows):
            self._frame(row)

    def nbest(self, final=False):
        """[(tokens, score, viterbi, times)], best first.  final=True also records the decisions of the exported list
        (neighbouring scores, the vb > vnb choice of each hypothesis) in the statistics."""
        out = [(e.tokens, e.score(), e.vit(), e.times()) for e in self.entries]
        if final:
            for (_, x, _, _), (_, y, _, _) in zip(out[:-1], out[1:]):
                self.stats.decide(x, y)
            for e in self.entries:
                self._choice(e)
        return out


def search_logp(logp, T, beam, blank=0, chunks=None):
    """logp (T', V) log-probabilities; the first T frames, split into `chunks` (widths summing to T; None: one chunk).
    Returns (nbest, StreamStats)."""
    logp = np.asarray(logp)
    s = Stream(beam, blank)
    t = 0
    for w in (chunks if chunks is not None else [T]):
        s.consume(logp[t:t + w])
        t += w
    assert t == T
    return s.nbest(final=True), s.stats


def search(logits_f32, T, beam, blank=0, chunks=None):
    lp = log_softmax_f64(logits_f32)
    return search_logp(lp, min(int(T), lp.shape[0]), beam, blank, chunks)


def check_times(nbest, a_next):
    """The invariant of the contract: as many times as tokens, strictly increasing, inside [0, a_next)."""
    for tokens, _, _, times in nbest:
        assert len(times) == len(tokens), (tokens, times)
        assert all(x < y for x, y in zip(times[:-1], times[1:])), times
        assert all(0 <= x < a_next for x in times), (times, a_next)
