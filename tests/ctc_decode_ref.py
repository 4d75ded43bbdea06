"""Float64 references of the CTC decode modes with the blank as a parameter, numpy only.

  prefix_beam_search(logits_f32, T, beam, blank)   ASRModel._ctc_prefix_beam_search (asr_model.py:326-409) restated: the
        log-softmax in float64 from the fp32 logits, then prefix_beam_search_logp.  Returns (nbest, stats).
  prefix_beam_search_logp(logp, T, beam, blank)    the search itself from log-probabilities (T, V): the reference's
        visiting order (top-k symbol outer, current prefix inner), its log_add (n-ary sums left to right) and a stable
        sort.  At blank 0 and fp32 log-probs it is oracle.decode_oracle.ctc_prefix_beam_search value for value.
  greedy_search(logits, lens, blank, eos)          ASRModel.ctc_greedy_search (asr_model.py:281-324): eos-fill BEFORE
        the collapse, score = maximum over ALL T frames; argmax on the raw logits (first index), float64 score.
  forced_align(lp, y, blank_id)                    wenet/utils/ctc_util.py:27-83 as oracle.decode_oracle.forced_align
        restates it (fp32 sums, first maximum of [s, s-1, s-2], the s-1 = -1 wrap), plus what a test needs to know
        about ties; an empty y is the one all-blank path.

stats of the prefix search (class Stats):
  max_ncur    largest number of current prefixes at the start of a frame
  max_slots   largest number of contributions in one frame: one per (symbol, prefix) pair, two for a pair whose symbol
              repeats the prefix's last token (it feeds the unchanged prefix and the extended one)
  pairs       number of such same-symbol pairs over all frames
  merges      number of next prefixes that received contributions from two different current prefixes in one frame
  min_gap     smallest strictly positive decision gap: per frame logp[k-th] - logp[(k+1)-th] at the top-k cut (beam < V)
              and score[beam-th] - score[(beam+1)-th] at the prune cut (more candidates than beam), and the gaps
              between neighbours of the final list
  ties        number of those decisions whose two values are exactly equal (ties are not gaps)
"""
import math
from dataclasses import dataclass

import numpy as np

NINF = -float("inf")


def log_add(args):
    """wenet/utils/common.py:268-276 (Python floats; sum() adds left to right)."""
    if all(a == NINF for a in args):
        return NINF
    a_max = max(args)
    return a_max + math.log(sum(math.exp(a - a_max) for a in args))


def log_softmax_f64(logits):
    x = np.asarray(logits, np.float32).astype(np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


@dataclass
class Stats:
    max_ncur: int = 0
    max_slots: int = 0
    pairs: int = 0
    merges: int = 0
    min_gap: float = float("inf")
    ties: int = 0

    def decide(self, hi, lo):
        """One decision between two values, hi ranked in front of lo."""
        if not (math.isfinite(hi) and math.isfinite(lo)):
            return
        if hi == lo:
            self.ties += 1
        else:
            self.min_gap = min(self.min_gap, hi - lo)


def peaky_logits(seed, T, V, blank=0, scale=1.0, bonus=2.5, blank_bonus=2.0):
    """Test input (T, V) fp32 for the prefix search: normal * scale, a bonus on a favourite label that changes every
    three frames and a bonus on the blank -- repeats of the last token and prefixes reached along several routes are
    then frequent."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(T, V)) * scale
    labels = [v for v in range(V) if v != blank]
    for t0 in range(0, T, 3):
        x[t0:t0 + 3, labels[int(rng.integers(len(labels)))]] += bonus
    x[:, blank] += blank_bonus
    return x.astype(np.float32)


def prefix_beam_search_logp(logp, T, beam, blank=0):
    logp = np.asarray(logp)
    V = logp.shape[1]
    st = Stats()
    cur_hyps = [(tuple(), (0.0, NINF))]
    for t in range(T):
        row = logp[t]
        st.max_ncur = max(st.max_ncur, len(cur_hyps))
        next_hyps = {}                              # insertion-ordered, missing = (-inf, -inf)
        bases = {}

        def get(p):
            return next_hyps.get(p, (NINF, NINF))

        full = np.argsort(-row, kind="stable")      # larger first, lower index on ties (torch.topk)
        order = full[:beam]
        if beam < V:
            st.decide(float(row[full[beam - 1]]), float(row[full[beam]]))
        slots = 0
        for s in order:
            s = int(s)
            ps = float(row[s])
            for bi, (prefix, (pb, pnb)) in enumerate(cur_hyps):
                last = prefix[-1] if len(prefix) > 0 else None
                if s == blank:
                    n_pb, n_pnb = get(prefix)
                    next_hyps[prefix] = (log_add([n_pb, pb + ps, pnb + ps]), n_pnb)
                    bases.setdefault(prefix, set()).add(bi)
                    slots += 1
                elif s == last:
                    n_pb, n_pnb = get(prefix)
                    next_hyps[prefix] = (n_pb, log_add([n_pnb, pnb + ps]))
                    bases.setdefault(prefix, set()).add(bi)
                    n_prefix = prefix + (s,)
                    n_pb, n_pnb = get(n_prefix)
                    next_hyps[n_prefix] = (n_pb, log_add([n_pnb, pb + ps]))
                    bases.setdefault(n_prefix, set()).add(bi)
                    slots += 2
                    st.pairs += 1
                else:
                    n_prefix = prefix + (s,)
                    n_pb, n_pnb = get(n_prefix)
                    next_hyps[n_prefix] = (n_pb, log_add([n_pnb, pb + ps, pnb + ps]))
                    bases.setdefault(n_prefix, set()).add(bi)
                    slots += 1
        st.max_slots = max(st.max_slots, slots)
        st.merges += sum(1 for v in bases.values() if len(v) > 1)
        nh = sorted(next_hyps.items(), key=lambda x: log_add(list(x[1])), reverse=True)   # stable
        if len(nh) > beam:
            st.decide(log_add(list(nh[beam - 1][1])), log_add(list(nh[beam][1])))
        cur_hyps = nh[:beam]
    out = [(y[0], log_add([y[1][0], y[1][1]])) for y in cur_hyps]
    for (_, a), (_, b) in zip(out[:-1], out[1:]):
        st.decide(a, b)
    return out, st


def prefix_beam_search(logits_f32, T, beam, blank=0):
    """logits (T', V) fp32 pre-softmax, the first min(T, T') frames are searched.  Returns (nbest, Stats)."""
    lp = log_softmax_f64(logits_f32)
    return prefix_beam_search_logp(lp, min(int(T), lp.shape[0]), beam, blank)


def greedy_search(logits, lens, blank=0, eos=-1):
    """logits (B, T, V).  Returns (hyps, scores float64 (B,)); eos < 0 means V - 1."""
    x = np.asarray(logits, np.float32)
    B, T, V = x.shape
    eos = V - 1 if eos < 0 else eos
    best = x.argmax(-1)                             # first maximum; log-softmax is monotone in the logits
    top = log_softmax_f64(x).max(-1)
    hyps = []
    for b in range(B):
        seq = [int(best[b, t]) if t < lens[b] else eos for t in range(T)]
        out, cur = [], 0
        while cur < len(seq):                       # remove_duplicates_and_blank, common.py:256-265
            if seq[cur] != blank:
                out.append(seq[cur])
            prev = cur
            while cur < len(seq) and seq[cur] == seq[prev]:
                cur += 1
        hyps.append(out)
    return hyps, top.max(1)


def forced_align(lp, y, blank_id=0, return_ties=False):
    """lp (T, V) fp32 log-posteriors, y label ids.  Returns the per-frame token list; with return_ties also the number
    of cells ON the backtraced path whose candidates [s, s-1(, s-2)] held their maximum more than once, split by which
    candidates tied: {(0, 1): n, (0, 2): n, (1, 2): n} keyed by the positions of the first two maxima.  Only ties
    between candidates with different tokens are counted: resolving one of those the other way changes the result."""
    lp = np.asarray(lp, np.float32)
    T = lp.shape[0]
    y = [int(v) for v in y]
    if len(y) == 0:
        return ([blank_id] * T, {}) if return_ties else [blank_id] * T
    ext = [blank_id]
    for tok in y:
        ext += [tok, blank_id]
    NS = len(ext)
    ext_a = np.array(ext)
    three = np.zeros(NS, bool)                      # states with the third candidate s-2
    three[2:] = (ext_a[2:] != blank_id) & (ext_a[2:] != ext_a[:-2])
    alpha = np.full(NS, -np.inf, np.float32)
    alpha[0] = lp[0, ext[0]]
    alpha[1] = lp[0, ext[1]]
    path = np.full((T, NS), -1, np.int64)
    tied = np.zeros((T, NS), np.int8)               # 1: candidates (0, 1) tie at the maximum, 2: (0, 2), 3: (1, 2)
    s_idx = np.arange(NS)
    d01 = ext_a != np.roll(ext_a, 1)                # the tied candidates carry different tokens: taking the other one
    d12 = np.roll(ext_a, 1) != np.roll(ext_a, 2)    # changes the alignment (not so at s = 0, or for a label == blank_id)
    for t in range(1, T):                           # one frame at a time, every state at once
        c2 = np.roll(alpha, 2)
        c2[~three] = -np.inf                        # never chosen: argmax takes the first maximum
        cands = np.stack([alpha, np.roll(alpha, 1), c2])                        # s-1 = -1 wraps, as in Python
        k = cands.argmax(0)
        best = cands[k, s_idx]
        eq = (cands == best) & np.isfinite(best)
        tied[t] = np.where(eq[0] & eq[1] & d01, 1, np.where(eq[0] & eq[2], 2, np.where(eq[1] & eq[2] & d12, 3, 0)))
        path[t] = s_idx - k
        alpha = (best + lp[t, ext_a]).astype(np.float32)
    st = [NS - 1, NS - 2][int(np.argmax(np.array([alpha[NS - 1], alpha[NS - 2]], np.float32)))]
    seq = [0] * T
    seq[-1] = st
    for t in range(T - 2, -1, -1):
        seq[t] = int(path[t + 1, seq[t + 1]])
    ali = [ext[s] for s in seq]
    if not return_ties:
        return ali
    on_path = {}
    for t in range(1, T):
        kind = int(tied[t, seq[t]])
        if kind:
            key = [(0, 1), (0, 2), (1, 2)][kind - 1]
            on_path[key] = on_path.get(key, 0) + 1
    return ali, on_path
