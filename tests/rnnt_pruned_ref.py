"""Float64 references of pruned RNN-T training (numpy / torch, CPU).

  prune_ranges_ref(px, py, boundary, s_range)   k2's get_rnnt_prune_ranges for the regular lattice, as explicit loops in
                                                the order the contract (include/wr_api.h) fixes
  band_log_probs_f64(...)                       one utterance: blank / emit log-probabilities on the (T, U+1) lattice,
                                                -inf on both arcs outside the band, log-softmax over the band's logits rows
  lattice_pruned_f64(...)                       cost, alpha, beta and the two arc occupancies of that lattice
  grad_pruned_f64(...)                          d cost / d logits (T, R, V) from the lattice: occupancy(cell) * softmax minus
                                                the blank arc's occupancy at the blank and the emit arc's at the label
  loss_pruned_torch_f64(...)                    the costs as a differentiable float64 torch expression (small lattices)
  enumerate_paths_pruned(...)                   brute force over every path that stays inside the band (tiny lattices)
"""
import itertools

import numpy as np
import torch


def prune_ranges_ref(px, py, boundary, s_range):
    """px (B, U, T+1), py (B, U+1, T) float32 arrays, boundary (B, 4) rows (0, 0, U_b, T_b) -> ranges (B, T, R) int64."""
    px, py = np.asarray(px), np.asarray(py)
    B, U1, T = py.shape
    R = min(int(s_range), U1)
    ranges = np.zeros((B, T, R), np.int64)
    for b in range(B):
        U_b, T_b = int(boundary[b][2]), int(boundary[b][3])
        s = [0] * T
        for t in range(T):
            if t >= T_b - 1:                                  # 2. padding
                s[t] = max(U_b - R + 1, 0)
                continue
            best, arg = 0.0, 0                                # 1. window score, float64, left to right
            for u0 in range(U1 - R + 1):
                sc = np.float64(py[b, u0, t])
                for r in range(1, R):
                    sc = sc + np.float64(py[b, u0 + r, t])
                if u0 > 0:
                    sc = sc - np.float64(px[b, u0 - 1, t])
                if u0 == 0 or sc > best:                      # the lowest u0 wins ties
                    best, arg = sc, u0
            s[t] = arg
        for t in range(T - 2, -1, -1):                        # 3. s = suffix_min(s)
            s[t] = min(s[t], s[t + 1])
        x = [t - s[t] for t in range(T)]
        for t in range(T - 2, -1, -1):                        #    x = suffix_min(t - s)
            x[t] = min(x[t], x[t + 1])
        for t in range(T):
            s[t] = t - max(x[t], 0)
            for r in range(R):                                # 4.
                ranges[b, t, r] = s[t] + r
    return ranges


def check_range_properties(ranges, boundary, U1):
    """The provable consequences of the padding and adjustment steps."""
    ranges = np.asarray(ranges)
    B, T, R = ranges.shape
    s = ranges[:, :, 0]
    assert (ranges == s[:, :, None] + np.arange(R)).all()
    assert (s[:, 0] == 0).all()
    d = np.diff(s, axis=1)
    assert ((d >= 0) & (d <= 1)).all()
    assert (s >= 0).all() and (s <= U1 - R).all()
    for b in range(B):
        assert (s[b] <= max(int(boundary[b][2]) - R + 1, 0)).all()


def band_log_probs_f64(logits, ranges, symbols, blank, T, U):
    """logits (>=T, R, V), ranges (>=T, R) of one utterance -> skip (T, U+1), emit (T, U+1), softmax (T, R, V) float64;
    skip = emit = -inf outside the band, emit = 0 at u == U inside it (the convention of the kernels; never used)."""
    x = np.asarray(logits)[:T].astype(np.float64)
    m = x.max(-1, keepdims=True)
    lp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
    skip = np.full((T, U + 1), -np.inf)
    emit = np.full((T, U + 1), -np.inf)
    for t in range(T):
        for r in range(x.shape[1]):
            u = int(ranges[t][r])
            if 0 <= u <= U:
                skip[t, u] = lp[t, r, blank]
                emit[t, u] = lp[t, r, int(symbols[u])] if u < U else 0.0
    return skip, emit, np.exp(lp)


def _sweeps(skip, emit, T, U):
    alpha = np.full((T, U + 1), -np.inf)
    beta = np.full((T, U + 1), -np.inf)
    alpha[0, 0] = 0.0
    for t in range(T):
        for u in range(U + 1):
            if t:
                alpha[t, u] = np.logaddexp(alpha[t, u], alpha[t - 1, u] + skip[t - 1, u])
            if u:
                alpha[t, u] = np.logaddexp(alpha[t, u], alpha[t, u - 1] + emit[t, u - 1])
    beta[T - 1, U] = skip[T - 1, U]
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            if t < T - 1:
                beta[t, u] = np.logaddexp(beta[t, u], skip[t, u] + beta[t + 1, u])
            if u < U:
                beta[t, u] = np.logaddexp(beta[t, u], emit[t, u] + beta[t, u + 1])
    return alpha, beta


def lattice_pruned_f64(logits, ranges, symbols, blank, T, U):
    """One utterance restricted to T frames and U labels: `rnnt_simple_ref.lattice_f64` with both arcs -inf outside the
    band.  Returns (cost, alpha, beta, occ_emit, occ_blank), the arrays (T, U+1); cost = +inf if no path fits."""
    skip, emit, _ = band_log_probs_f64(logits, ranges, symbols, blank, T, U)
    with np.errstate(invalid="ignore"):
        alpha, beta = _sweeps(skip, emit, T, U)
    ll = beta[0, 0]
    occ_blank = np.zeros((T, U + 1))
    occ_emit = np.zeros((T, U + 1))
    if np.isfinite(ll):
        for t in range(T):
            for u in range(U + 1):
                if not np.isfinite(alpha[t, u]) or not np.isfinite(skip[t, u]):
                    continue
                if t < T - 1:
                    occ_blank[t, u] = np.exp(alpha[t, u] + skip[t, u] + beta[t + 1, u] - ll)
                elif u == U:
                    occ_blank[t, u] = np.exp(alpha[t, u] + skip[t, u] - ll)
                if u < U:
                    occ_emit[t, u] = np.exp(alpha[t, u] + emit[t, u] + beta[t, u + 1] - ll)
    return -ll, alpha, beta, occ_emit, occ_blank


def grad_pruned_f64(logits, ranges, symbols, blank, T, U):
    """(cost, d cost / d logits) of one utterance; the gradient has the shape of `logits`, zero in rows outside the
    lattice (t >= T or ranges > U)."""
    logits = np.asarray(logits)
    cost, alpha, beta, occ_emit, occ_blank = lattice_pruned_f64(logits, ranges, symbols, blank, T, U)
    _, _, sm = band_log_probs_f64(logits, ranges, symbols, blank, T, U)
    grad = np.zeros(logits.shape, np.float64)
    for t in range(T):
        for r in range(logits.shape[1]):
            u = int(ranges[t][r])
            if not 0 <= u <= U:
                continue
            g = (occ_emit[t, u] + occ_blank[t, u]) * sm[t, r]
            g[blank] -= occ_blank[t, u]
            if u < U:
                g[int(symbols[u])] -= occ_emit[t, u]
            grad[t, r] = g
    return cost, grad


def reference_batch(logits, ranges, symbols, blank, t_lens, u_lens):
    """(costs (B,), grad (B, T, R, V)) in float64 of sum_b cost_b."""
    costs, grads = [], []
    for b in range(len(t_lens)):
        c, g = grad_pruned_f64(logits[b], ranges[b], symbols[b], blank, int(t_lens[b]), int(u_lens[b]))
        costs.append(c)
        grads.append(g)
    return np.array(costs), np.stack(grads)


def loss_pruned_torch_f64(logits, ranges, symbols, blank, t_lens, u_lens):
    """Costs (B,) as a differentiable float64 torch expression of logits (B, T, R, V).  A cell outside the band has no
    arcs: its terms are left out of the sums (a cell that no path reaches stays None).  +inf when no path fits."""
    costs = []
    for b in range(logits.shape[0]):
        T, U = int(t_lens[b]), int(u_lens[b])
        lp = torch.log_softmax(logits[b, :T].double(), -1)
        row = {}
        for t in range(T):
            for r in range(logits.shape[2]):
                u = int(ranges[b][t][r])
                if 0 <= u <= U:
                    row[(t, u)] = lp[t, r]
        alpha = {(0, 0): lp.new_zeros(())}
        for t in range(T):
            for u in range(U + 1):
                terms = []
                if t and (t - 1, u) in alpha and (t - 1, u) in row:
                    terms.append(alpha[(t - 1, u)] + row[(t - 1, u)][blank])
                if u and (t, u - 1) in alpha and (t, u - 1) in row:
                    terms.append(alpha[(t, u - 1)] + row[(t, u - 1)][int(symbols[b][u - 1])])
                if terms:
                    alpha[(t, u)] = torch.logsumexp(torch.stack(terms), 0)
        if (T - 1, U) in alpha and (T - 1, U) in row:
            costs.append(-(alpha[(T - 1, U)] + row[(T - 1, U)][blank]))
        else:
            costs.append(lp.new_full((), float("inf")))
    return torch.stack(costs)


def enumerate_paths_pruned(logits, ranges, symbols, blank, T, U):
    """Every monotone path of the T x (U+1) lattice whose every arc leaves a cell inside the band: (total probability,
    occ_emit (T, U+1), occ_blank (T, U+1)), the occupancies normalised by the total (zeros if the total is 0)."""
    skip, emit, _ = band_log_probs_f64(logits, ranges, symbols, blank, T, U)
    total = 0.0
    oe, ob = np.zeros((T, U + 1)), np.zeros((T, U + 1))
    for emits_at in itertools.combinations(range(T - 1 + U), U):
        t = u = 0
        logp = 0.0
        arcs = []
        for step in range(T - 1 + U):
            if step in emits_at:
                logp += emit[t, u]; arcs.append((1, t, u)); u += 1
            else:
                logp += skip[t, u]; arcs.append((0, t, u)); t += 1
        logp += skip[t, u]; arcs.append((0, t, u))
        p = np.exp(logp)
        total += p
        for kind, tt, uu in arcs:
            (oe if kind else ob)[tt, uu] += p
    if total > 0:
        oe, ob = oe / total, ob / total
    return total, oe, ob


def full_ranges(B, T, U1):
    """ranges with R = U + 1: the whole lattice."""
    return np.broadcast_to(np.arange(U1, dtype=np.int64), (B, T, U1)).copy()


def random_band(rng, B, T, U1, R, t_lens, u_lens):
    """A valid band per utterance in the shape get_rnnt_prune_ranges produces: starts begin at 0, rise by 0 or 1 per
    frame and reach max(U_b - R + 1, 0) by frame T_b - 1 whenever T_b - 1 steps suffice (then a complete path fits)."""
    s = np.zeros((B, T), np.int64)
    for b in range(B):
        top = max(int(u_lens[b]) - R + 1, 0)
        cur = 0
        for t in range(1, T):
            remaining = max(int(t_lens[b]) - 1 - t, 0)        # steps still possible after this frame
            if cur < top and (top - cur > remaining or rng.random() < 0.5):
                cur += 1
            s[b, t] = cur
    return s[:, :, None] + np.arange(R, dtype=np.int64)
