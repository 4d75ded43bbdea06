"""Float64 reference of the CTC prefix beam search with context-graph phrase biasing, numpy only.

Written from the contract in include/wr_api.h ("Context-graph biasing in the CTC prefix beam search") on top of
tests/ctc_stream_ref.py, whose per-frame statements (summed scores, Viterbi riders, times) are repeated here unchanged.
The graph is any object with `next(state, token) -> (state', score, start, end)` and an `escape` array -- the package's
ContextGraph, or a stand-in.

  ContextStream(beam, graph, blank)   one stream: `consume(logp_rows)`, `nbest(final=False, finalize=False)` exports
                                      [(tokens, score, viterbi, times, ctc_score, context_score, tags)] and leaves the
                                      entries' graph states, in that order, in `exported_states`
  search_logp(logp, T, beam, graph, blank, chunks=None, finalize=True)
  search(logits_f32, T, beam, graph, blank, chunks=None, finalize=True)
  outputs(result, start_tag_id, end_tag_id)     UpdateOutputs, ctc_prefix_beam_search.cc:63-84

Purity.  Every contributor to a key computes the key's (ctx_state, ctx_score, tags) and the reference asserts that they
agree with what the first contributor set (`purity` counts the comparisons made).

Statistics (class ContextStats) extend StreamStats: `min_gap` / `ties` also cover every comparison of totals between
neighbours of a frame's sorted list up to and including the cut, and of the finalised list.  Further:
  ends        end boundaries set (tags with bit 1) over all contributions that created a key
  starts      start boundaries likewise
  saved       frames in which an entry was kept that a prune by log_add(pb, pnb) alone would have dropped
  taken_back  entries of a finalised export whose bonus finalisation reduced (ctx_state != 0 with escape != 0)
  reordered   finalised exports whose order differs from the stream's
  states      the graph states of the entries of the last export, in its order
"""
from dataclasses import dataclass

import numpy as np

from ctc_stream_ref import NINF, Entry, Stream, StreamStats, log_add, log_softmax_f64, peaky_logits  # noqa: F401


@dataclass
class ContextStats(StreamStats):
    purity: int = 0
    ends: int = 0
    starts: int = 0
    saved: int = 0
    taken_back: int = 0
    reordered: int = 0
    states: tuple = ()          # the graph states of the last exported list, in its order


class CEntry(Entry):
    __slots__ = ("ctx_state", "ctx_score", "tags", "has_context")

    def __init__(self, tokens=(), pb=NINF, pnb=NINF, vb=NINF, vnb=NINF, times_b=(), times_nb=()):
        super().__init__(tokens, pb, pnb, vb, vnb, times_b, times_nb)
        self.ctx_state, self.ctx_score, self.tags, self.has_context = 0, 0.0, (), False

    def total(self):
        return self.score() + self.ctx_score


class ContextStream(Stream):
    def __init__(self, beam, graph, blank=0, stats=None):
        self.graph = graph
        super().__init__(beam, blank, stats if stats is not None else ContextStats())

    def reset(self):
        self.a_next = 0
        e = CEntry((), 0.0, NINF, 0.0, 0.0)
        e.has_context = True
        self.entries = [e]

    def _context(self, n, e, s):
        """The context of key n as contributor e gives it: a copy (s is None) or one step of the graph on token s."""
        st = self.stats
        if s is None:
            ctx = (e.ctx_state, e.ctx_score, e.tags)
        else:
            state, sc, start, end = self.graph.next(e.ctx_state, s)
            ctx = (state, e.ctx_score + float(sc), e.tags + (int(start) | int(end) << 1,))
        if n.has_context:
            st.purity += 1
            assert (n.ctx_state, n.ctx_score, n.tags) == ctx, (n.tokens, (n.ctx_state, n.ctx_score, n.tags), ctx)
        else:
            n.ctx_state, n.ctx_score, n.tags = ctx
            n.has_context = True
            if s is not None:
                st.starts += ctx[2][-1] & 1
                st.ends += ctx[2][-1] >> 1

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
                nxt[tokens] = CEntry(tokens)
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
                    self._context(n, e, None)
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
                    self._context(n, e, None)
                    n = key(e.tokens + (s,), bi)
                    n.pnb = log_add([n.pnb, e.pb + p])
                    if improve(n, e.vb + p):
                        n.vnb, n.ctp, n.times_nb = e.vb + p, p, e.times_b + (a,)
                    self._context(n, e, s)
                    slots += 2
                    st.pairs += 1
                else:
                    n = key(e.tokens + (s,), bi)
                    n.pnb = log_add([n.pnb, e.pb + p, e.pnb + p])
                    self._choice(e)
                    if improve(n, e.vit() + p):
                        n.vnb, n.ctp, n.times_nb = e.vit() + p, p, e.times() + (a,)
                    self._context(n, e, s)
                    slots += 1
        st.max_slots = max(st.max_slots, slots)
        st.merges += sum(1 for v in bases.values() if len(v) > 1)
        nh = sorted(nxt.values(), key=lambda n: n.total(), reverse=True)       # stable; total_score()
        for x, y in zip(nh[:beam], nh[1:beam + 1]):                            # every neighbour up to and across the cut
            st.decide(x.total(), y.total())
        if len(nh) > beam:
            plain = sorted(nxt.values(), key=lambda n: n.score(), reverse=True)[:beam]
            if any(all(k is not q for q in plain) for k in nh[:beam]):
                st.saved += 1
        self.entries = nh[:beam]
        self.a_next += 1

    def nbest(self, final=False, finalize=False):
        """[(tokens, score, viterbi, times, ctc_score, context_score, tags)], best first; finalize=True is
        UpdateFinalContext on the exported copy (the stream keeps its entries).  final=True records the decisions of the
        exported list in the statistics, as ctc_stream_ref does."""
        st = self.stats
        rows = []
        for e in self.entries:
            ctx = e.ctx_score
            if finalize and e.ctx_state != 0:
                ctx = ctx + float(self.graph.escape[e.ctx_state])
                if final and ctx != e.ctx_score:
                    st.taken_back += 1
            ctc = e.score()
            rows.append((e.tokens, ctc + ctx, e.vit(), e.times(), ctc, ctx, e.tags, e.ctx_state))
        rows = sorted(rows, key=lambda r: r[1], reverse=True) if finalize else rows     # stable
        self.exported_states = [r[7] for r in rows]                # the graph states, in the order of the exported list
        st.states = tuple(self.exported_states)
        out = [r[:7] for r in rows]
        rows = [(e.tokens,) for e in self.entries]
        if final:
            if [r[0] for r in out] != [r[0] for r in rows]:
                st.reordered += 1
            for x, y in zip(out[:-1], out[1:]):
                st.decide(x[1], y[1])
            for e in self.entries:
                self._choice(e)
        return out


def search_logp(logp, T, beam, graph, blank=0, chunks=None, finalize=True):
    """logp (T', V) log-probabilities; the first T frames, split into `chunks` (widths summing to T; None: one chunk).
    Returns (nbest, ContextStats)."""
    logp = np.asarray(logp)
    s = ContextStream(beam, graph, blank)
    t = 0
    for w in (chunks if chunks is not None else [T]):
        s.consume(logp[t:t + w])
        t += w
    assert t == T
    return s.nbest(final=True, finalize=finalize), s.stats


def search(logits_f32, T, beam, graph, blank=0, chunks=None, finalize=True):
    lp = log_softmax_f64(logits_f32)
    return search_logp(lp, min(int(T), lp.shape[0]), beam, graph, blank, chunks, finalize)


def outputs(result, start_tag_id, end_tag_id):
    """UpdateOutputs (ctc_prefix_beam_search.cc:63-84): the start tag in front of a token with bit 0, the end tag behind
    a token with bit 1."""
    outs = []
    for hyp in result:
        o = []
        for tok, tag in zip(hyp[0], hyp[6]):
            if tag & 1:
                o.append(start_tag_id)
            o.append(tok)
            if tag & 2:
                o.append(end_tag_id)
        outs.append(o)
    return outs


def check_tags(nbest):
    for hyp in nbest:
        assert len(hyp[6]) == len(hyp[0]) and all(0 <= g <= 3 for g in hyp[6]), hyp


def phrases_from(tokens):
    """Phrases for a test graph from a hypothesis: its tokens cut into pieces of 2, 3, 2, 3, ... tokens (a shorter last
    piece is kept), plus one nested pair -- the first piece extended by the token that follows it."""
    tokens = [int(t) for t in tokens]
    out, i, w = [], 0, 2
    while i < len(tokens):
        out.append(tokens[i:i + w])
        i += w
        w = 5 - w
    if len(tokens) > len(out[0]):
        out.append(tokens[:len(out[0]) + 1])
    return out
