"""Float64 reference of RNN-T forced alignment (wenet_celoss_amd.rnnt_forced_align), with the kernel's tie rule, and a
brute-force enumerator of every path of a tiny lattice.

Lattice (torchaudio's, log-softmax fused): blank(t,u) = log_softmax(logits[t,u])[blank], emit(t,u) =
log_softmax(logits[t,u])[y_{u+1}];  A(0,0) = 0,  A(t,u) = max(A(t-1,u) + blank(t-1,u), A(t,u-1) + emit(t,u-1)),
score = A(T-1,U) + blank(T-1,U).

Tie rule: the emit predecessor (t,u-1) wins only if its candidate is strictly greater than the blank predecessor's; on
equality or a NaN comparison the blank predecessor (t-1,u) wins.  On the top row (t = 0) only the emit predecessor
exists.  The value is NaN if either candidate is NaN."""
import itertools
import math

import numpy as np


def lattice_log_probs(logits, targets, blank):
    """logits (T, U+1, V) -> blank (T, U+1), emit (T, U) in float64."""
    x = np.asarray(logits, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    lp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
    U = x.shape[1] - 1
    blank_lp = lp[:, :, blank]
    emit_lp = np.stack([lp[:, u, int(targets[u])] for u in range(U)], 1) if U else np.zeros((x.shape[0], 0))
    return blank_lp, emit_lp


def viterbi(blank_lp, emit_lp, T, U):
    """Best path of the lattice restricted to T frames and U labels.  Returns (score, frames (U,) int, margin): frames[u]
    is the frame at which label u+1 is emitted; margin is the smallest |emit candidate - blank candidate| over the cells
    of the returned path where both predecessors exist (inf if there is none)."""
    A = np.full((T, U + 1), -np.inf)
    D = np.zeros((T, U + 1), dtype=bool)        # True: the emit predecessor won
    M = np.full((T, U + 1), np.inf)
    for t in range(T):
        for u in range(U + 1):
            if t == 0 and u == 0:
                A[0, 0] = 0.0
                continue
            top = A[t - 1, u] + blank_lp[t - 1, u] if t >= 1 else -np.inf
            left = A[t, u - 1] + emit_lp[t, u - 1] if u >= 1 else -np.inf
            emit = u >= 1 and (t == 0 or left > top)
            v = left if emit else top
            if u >= 1 and math.isnan(left):
                v = left
            A[t, u] = v
            D[t, u] = emit
            if t >= 1 and u >= 1:
                M[t, u] = abs(left - top)
    score = A[T - 1, U] + blank_lp[T - 1, U]
    frames = np.full(U, -1, dtype=np.int64)
    t, u = T - 1, U
    margin = np.inf
    while t > 0 or u > 0:
        margin = min(margin, M[t, u])
        if u > 0 and (t == 0 or D[t, u]):
            u -= 1
            frames[u] = t
        else:
            t -= 1
    return score, frames, margin


def path_score(blank_lp, emit_lp, T, U, frames):
    """Log-probability of the path that emits label u+1 at frame frames[u] (float64)."""
    s = 0.0
    u = 0
    for t in range(T):
        while u < U and frames[u] == t:
            s += emit_lp[t, u]
            u += 1
        s += blank_lp[t, u]
    assert u == U
    return s


def brute_force(blank_lp, emit_lp, T, U):
    """Every path of the lattice (C(T-1+U, U) of them): (best score, list of the frames of every best path)."""
    best, arg = -np.inf, []
    for frames in itertools.combinations_with_replacement(range(T), U):
        s = path_score(blank_lp, emit_lp, T, U, frames)
        if s > best:
            best, arg = s, [tuple(frames)]
        elif s == best:
            arg.append(tuple(frames))
    return best, arg


def log_num_paths(T, U):
    return math.lgamma(T + U) - math.lgamma(U + 1) - math.lgamma(T)


def is_valid_path(frames, T, U, width):
    """label_frames row of one utterance: non-decreasing frames in [0, T) for the U labels, -1 after."""
    f = np.asarray(frames)
    if f.shape != (width,):
        return False
    if U and (f[:U].min() < 0 or f[:U].max() >= T or np.any(np.diff(f[:U]) < 0)):
        return False
    return bool(np.all(f[U:] == -1))
