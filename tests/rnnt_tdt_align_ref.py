"""Float64 reference of TDT forced alignment, written with explicit loops from the contract in include/wr_api.h ("TDT
forced alignment") and not from the kernels.

  arcs(logits, labels, T, U, durations, blank, sigma)   the arc log-probabilities of one utterance: rnnt_tdt_ref.arcs_f64,
                                         rounded to float32 and back, so that exact ties are exact
  viterbi(tb, tl, dur, T, U, durations)  -> Alignment(score, frames, durations, jumps, margin, ties, clear)
  align_utt / align_ref                  one utterance from its logits / a padded batch, padded as the device pads
  rebuild_path, is_valid_path, path_score  the arc sequence that the three output arrays determine, and its float64 score
  brute_force(...)                       every path of a tiny lattice: (best score, the arc sequences that reach it)

Candidates into a cell are ordered blank arcs by ascending d, then label arcs by ascending d, and one replaces the
best so far only if it is strictly greater: the contract's tie rule (a NaN candidate never compares greater).
"""
import collections

import numpy as np

import rnnt_tdt_ref as ref

Alignment = collections.namedtuple("Alignment", "score frames durations jumps margin ties clear")

BLANK, LABEL = 0, 1


def arcs(logits, labels, T, U, durations, blank=0, sigma=0.0):
    """(tb (T, U+1), tl (T, U), dur (T, U+1, D)) as float64 arrays of float32-representable values."""
    D = len(durations)
    x = np.asarray(logits, np.float64)[:T, :U + 1]
    tok, dur = ref.arcs_f64(x, x.shape[-1] - D, sigma)
    with np.errstate(over="ignore", invalid="ignore"):
        tok = tok.astype(np.float32).astype(np.float64)
        dur = dur.astype(np.float32).astype(np.float64)
    tb = tok[..., blank]
    tl = np.stack([tok[:, u, int(labels[u])] for u in range(U)], 1) if U else np.zeros((T, 0))
    return tb, tl, dur


def _candidates(A, tb, tl, dur, T, U, durations, t, u):
    """Incoming arcs of (t, u) -- or of the terminal, t == T, u == U -- in the tie rule's order: (value, kind, d)."""
    out = []
    for n, d in enumerate(durations):
        if d >= 1 and t - d >= 0:
            out.append(((A[t - d, u] + tb[t - d, u]) + dur[t - d, u, n], BLANK, d))
    if u >= 1 and t <= T - 1:
        for n, d in enumerate(durations):
            if t - d >= 0:
                out.append(((A[t - d, u - 1] + tl[t - d, u - 1]) + dur[t - d, u - 1, n], LABEL, d))
    return out


def _winner(cands):
    """(value, kind, d, gap to the runner-up) or None when no candidate wins"""
    best, arg = -np.inf, None
    for i, (v, _, _) in enumerate(cands):
        if v > best:
            best, arg = v, i
    if arg is None:
        return None
    rest = [v for i, (v, _, _) in enumerate(cands) if i != arg and v == v]
    second = max(rest) if rest else -np.inf
    return best, cands[arg][1], cands[arg][2], (best - second if second > -np.inf else np.inf)


def viterbi(tb, tl, dur, T, U, durations):
    A = np.full((T + 1, U + 1), -np.inf)
    back = {}
    A[0, 0] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T + 1):
            for u in range(U + 1):
                if (t == 0 and u == 0) or (t == T and u != U):
                    continue
                w = _winner(_candidates(A, tb, tl, dur, T, U, durations, t, u))
                if w is not None:
                    A[t, u] = w[0]
                    back[(t, u)] = w[1:]
    frames = np.full(U, -1, np.int64)
    durs = np.full(U, -1, np.int64)
    jumps = np.zeros(T, np.int64)
    if (T, U) not in back:
        return Alignment(-np.inf, frames, durs, jumps, np.inf, 0, np.inf)
    gaps = []
    t, u = T, U
    while (t, u) != (0, 0):
        kind, d, gap = back[(t, u)]
        gaps.append(gap)
        t -= d
        if kind == LABEL:
            u -= 1
            frames[u], durs[u] = t, d
        else:
            jumps[t] = d
    nonzero = [g for g in gaps if g > 0]
    return Alignment(A[T, U], frames, durs, jumps, min(gaps), sum(1 for g in gaps if g == 0),
                     min(nonzero) if nonzero else np.inf)


def align_utt(logits, labels, T, U, durations, blank=0, sigma=0.0):
    return viterbi(*arcs(logits, labels, T, U, durations, blank, sigma), T, U, durations)


def align_ref(logits, targets, llens, tlens, durations, blank=0, sigma=0.0):
    """A padded batch: (list of Alignment, frames (B, U) and durations (B, U) with -1 padding, jumps (B, T) with 0)."""
    B, T, U1, _ = np.shape(logits)
    frames = np.full((B, U1 - 1), -1, np.int64)
    durs = np.full((B, U1 - 1), -1, np.int64)
    jumps = np.zeros((B, T), np.int64)
    out = []
    for b in range(B):
        Tb, Ub = int(llens[b]), int(tlens[b])
        a = align_utt(np.asarray(logits)[b], np.asarray(targets)[b] if U1 > 1 else [], Tb, Ub, durations, blank, sigma)
        frames[b, :Ub], durs[b, :Ub], jumps[b, :Tb] = a.frames, a.durations, a.jumps
        out.append(a)
    return out, frames, durs, jumps


def rebuild_path(frames, durs, jumps, T, U, durations):
    """The arcs [(kind, t, u, d)] that the output rows of one utterance determine, or None if they are no path from
    (0, 0) to the terminal: at a frame, label arcs that stay (d = 0), then the one arc that leaves it."""
    frames, durs, jumps = (np.asarray(a).tolist() for a in (frames, durs, jumps))
    if any(f != -1 for f in frames[U:]) or any(d != -1 for d in durs[U:]) or any(j != 0 for j in jumps[T:]):
        return None
    path, t, u, blanks = [], 0, 0, 0
    while t < T:
        if u < U and frames[u] == t:
            d = durs[u]
            if d not in durations or t + d > T - 1 or (d > 0 and jumps[t] != 0):
                return None
            path.append((LABEL, t, u, d))
            t, u = t + d, u + 1
        else:
            d = jumps[t]
            if d < 1 or d not in durations or t + d > T or (t + d == T and u != U):
                return None
            path.append((BLANK, t, u, d))
            t, blanks = t + d, blanks + 1
    if t != T or u != U or blanks != sum(1 for j in jumps[:T] if j != 0):
        return None
    return path


def is_valid_path(frames, durs, jumps, T, U, durations):
    return rebuild_path(frames, durs, jumps, T, U, durations) is not None


def is_no_path(frames, durs, jumps):
    return bool(np.all(np.asarray(frames) == -1) and np.all(np.asarray(durs) == -1) and not np.any(jumps))


def path_score(tb, tl, dur, durations, path):
    s = 0.0
    for kind, t, u, d in path:
        s = (s + (tb[t, u] if kind == BLANK else tl[t, u])) + dur[t, u, durations.index(d)]
    return s


def brute_force(tb, tl, dur, T, U, durations):
    """Depth-first over every path: (best score, list of the arc sequences that reach it); (-inf, []) without a path."""
    best = [-np.inf, []]

    def walk(t, u, s, path):
        for n, d in enumerate(durations):
            if d >= 1:
                w = (s + tb[t, u]) + dur[t, u, n]
                arc = path + [(BLANK, t, u, d)]
                if t + d < T:
                    walk(t + d, u, w, arc)
                elif t + d == T and u == U:
                    if w > best[0]:
                        best[0], best[1] = w, [arc]
                    elif w == best[0]:
                        best[1].append(arc)
            if u < U and t + d <= T - 1:
                walk(t + d, u + 1, (s + tl[t, u]) + dur[t, u, n], path + [(LABEL, t, u, d)])

    walk(0, 0, 0.0, [])
    return best[0], best[1]
