"""The context graph of the biased CTC prefix beam search, as a deterministic table.

The reference runtime compiles the user's phrases into an OpenFST graph (runtime/core/decoder/context_graph.{h,cc}) and
asks it one question, `GetNextState` (context_graph.cc:86-108).  This module builds the table that answers the same
question (include/wr_api.h, "Context-graph biasing in the CTC prefix beam search"):

  arc_begin int32[S+1]   CSR offsets into the arcs            arc_token int32[A]   strictly increasing within a state
  arc_next  int32[A]                                          arc_score float32[A]
  escape    float32[S]   escape[0] = 0                        final     int32[S]   final[0] = 1

  next(state, token) = (arc_next, arc_score, state == 0, final[arc_next] != 0)    if state has an arc on token
                     = (0, escape[state], False, False)                            otherwise

The table is the prefix trie of the de-duplicated phrases; every arc scores float32(context_score).  The arc on the last
token of a phrase that no other phrase extends goes back to state 0, the root.  A phrase that is a proper prefix of
another ends in a trie node with final = 1: the match commits there and its bonus stays whatever follows (determinising
the reference's FST would take it back; this builder does not).  escape[s] is minus the sum of the arc scores since the
last final state or the root, +0.0 at final states and at the root.  States are numbered in insertion order and every
state is reachable.  The caller tokenises: phrases are sequences of token ids.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import numpy as np

MAX_PHRASES = 5000          # ContextConfig::max_contexts (context_graph.h)
MAX_PHRASE_LEN = 100        # ContextConfig::max_context_length


class ContextGraph:
    def __init__(self, phrases: Sequence[Sequence[int]], context_score: float = 3.0, blank: int = 0):
        score = float(context_score)
        if not math.isfinite(score) or abs(score) > float(np.finfo(np.float32).max):
            raise ValueError(f"ContextGraph: context_score={context_score} is not finite")
        phrases = [tuple(int(t) for t in p) for p in phrases]
        if len(phrases) > MAX_PHRASES:
            raise ValueError(f"ContextGraph: {len(phrases)} phrases, at most {MAX_PHRASES}")
        for p in phrases:
            if len(p) == 0:
                raise ValueError("ContextGraph: empty phrase")
            if len(p) > MAX_PHRASE_LEN:
                raise ValueError(f"ContextGraph: a phrase of {len(p)} tokens, at most {MAX_PHRASE_LEN}")
            for t in p:
                if t < 0 or t == int(blank):
                    raise ValueError(f"ContextGraph: token {t} in phrase {list(p)} (negative, or the blank {blank})")
        self.context_score, self.blank = score, int(blank)
        self.phrases = list(dict.fromkeys(phrases))                    # de-duplicated, first occurrence kept
        whole = set(self.phrases)
        extended = {p[:n] for p in self.phrases for n in range(1, len(p))}     # proper prefixes of some phrase
        sc = np.float32(score)
        arcs: List[dict] = [{}]               # per state: token -> next state
        node = {(): 0}                        # trie prefix -> state
        escape, final = [np.float32(0.0)], [1]
        for p in self.phrases:
            s = 0
            for n in range(1, len(p) + 1):
                pre = p[:n]
                if pre in whole and pre not in extended:                # a leaf: the match is complete, back to the root
                    arcs[s][p[n - 1]] = 0
                    break
                if pre not in node:
                    node[pre] = len(arcs)
                    arcs[s][p[n - 1]] = node[pre]
                    arcs.append({})
                    fin = pre in whole
                    final.append(1 if fin else 0)
                    escape.append(np.float32(0.0) if fin else np.float32(escape[s] - sc))
                s = node[pre]
        self.n_states = len(arcs)
        begin, tok, nxt = [0], [], []
        for a in arcs:
            for t in sorted(a):
                tok.append(t)
                nxt.append(a[t])
            begin.append(len(tok))
        self.arc_begin = np.asarray(begin, np.int32)
        self.arc_token = np.asarray(tok, np.int32)
        self.arc_next = np.asarray(nxt, np.int32)
        self.arc_score = np.full(len(tok), sc, np.float32)
        self.escape = np.asarray(escape, np.float32)
        self.final = np.asarray(final, np.int32)
        self.n_arcs = len(tok)
        self._device = {}

    def next(self, state: int, token: int) -> Tuple[int, float, bool, bool]:
        """GetNextState on the host: (state', score, start boundary, end boundary); the score is the float32's value."""
        lo, hi = int(self.arc_begin[state]), int(self.arc_begin[state + 1])
        k = lo + int(np.searchsorted(self.arc_token[lo:hi], token))
        if k < hi and int(self.arc_token[k]) == token:
            st = int(self.arc_next[k])
            return st, float(self.arc_score[k]), state == 0, bool(self.final[st] != 0)
        return 0, float(self.escape[state]), False, False

    def to(self, device):
        """The six tensors on `device`: (arc_begin, arc_token, arc_next, arc_score, escape, final).  Empty arc arrays
        are padded to one element so that every tensor has storage."""
        import torch
        device = torch.device(device)
        if device not in self._device:
            pad = (lambda a: a if a.size else np.zeros(1, a.dtype))
            self._device[device] = tuple(torch.from_numpy(pad(a).copy()).to(device) for a in (
                self.arc_begin, self.arc_token, self.arc_next, self.arc_score, self.escape, self.final))
        return self._device[device]


def mark_phrases(tokens, tags, start_tag_id: int, end_tag_id: int) -> list:
    """UpdateOutputs (ctc_prefix_beam_search.cc:63-84) on one hypothesis: its tokens with `start_tag_id` in front of every
    token whose tag has bit 0 (a phrase starts at it) and `end_tag_id` behind every token whose tag has bit 1 (one ends)."""
    out = []
    for tok, tag in zip(tokens, tags):
        if tag & 1:
            out.append(start_tag_id)
        out.append(tok)
        if tag & 2:
            out.append(end_tag_id)
    return out
