"""Float64 reference of the token-and-duration transducer (TDT) loss, written with explicit loops from the contract in
include/wr_api.h ("Token-and-duration transducer") and not from the kernels.

  arcs_f64(row_logits, V, sigma)         (tok log-probs - sigma, duration log-probs) of (..., V + D) logits
  tdt_utt_f64(...)                       one utterance: (cost, grad (T, U+1, V+D), alpha (T, U+1), beta (T, U+1))
  tdt_ref(...)                           a padded batch: (costs (B,), grad, alpha, beta), zeros outside the lattices; an
                                         utterance without a path costs +inf and its gradient is NaN (not defined)
  enumerate_paths(...)                   brute force: log of the summed probability of every path of a tiny lattice
  cost_torch(...)                        the cost as a differentiable float64 torch expression (NEG_BIG for "no arc")
"""
import numpy as np
import torch

NEG_BIG = -1.0e30


def _lse(x, axis=-1):
    m = np.max(x, axis=axis, keepdims=True)
    return np.squeeze(m, axis) + np.log(np.sum(np.exp(x - m), axis=axis))


def arcs_f64(logits, V, sigma):
    logits = np.asarray(logits, np.float64)
    tok = logits[..., :V] - _lse(logits[..., :V])[..., None] - sigma
    dur = logits[..., V:] - _lse(logits[..., V:])[..., None]
    return tok, dur


def tdt_utt_f64(logits, labels, T, U, durations, blank, sigma):
    """logits (>= T, >= U+1, V + D); labels (>= U,).  Nodes (t, u), t < T, and one terminal behind (T, U)."""
    D = len(durations)
    V = logits.shape[-1] - D
    logits = np.asarray(logits, np.float64)[:T, :U + 1]
    tok, dur = arcs_f64(logits, V, sigma)
    alpha = np.full((T + 1, U + 1), -np.inf)
    beta = np.full((T + 1, U + 1), -np.inf)
    if T == 0:
        return 0.0, np.zeros((0, U + 1, V + D)), alpha[:0], beta[:0]
    alpha[0, 0] = 0.0
    beta[T, U] = 0.0
    # alpha row T: only the terminal (T, U) means anything, reached by blank arcs alone
    for t in range(T + 1):
        for u in range(U + 1):
            if t == 0 and u == 0:
                continue
            if t == T and u != U:
                continue
            acc = -np.inf
            for n, d in enumerate(durations):
                if d >= 1 and t - d >= 0:                                  # blank from (t-d, u)
                    acc = np.logaddexp(acc, alpha[t - d, u] + tok[t - d, u, blank] + dur[t - d, u, n])
                if u >= 1 and t - d >= 0 and t <= T - 1:                   # label from (t-d, u-1)
                    acc = np.logaddexp(acc, alpha[t - d, u - 1] + tok[t - d, u - 1, labels[u - 1]] + dur[t - d, u - 1, n])
            alpha[t, u] = acc
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            acc = -np.inf
            for n, d in enumerate(durations):
                if d >= 1 and (t + d < T or (t + d == T and u == U)):
                    acc = np.logaddexp(acc, tok[t, u, blank] + dur[t, u, n] + beta[t + d, u])
                if u < U and t + d <= T - 1:
                    acc = np.logaddexp(acc, tok[t, u, labels[u]] + dur[t, u, n] + beta[t + d, u + 1])
            beta[t, u] = acc
    ll = alpha[T, U]
    grad = np.zeros((T, U + 1, V + D))
    if not np.isfinite(ll):
        grad[:] = np.nan
        return np.inf, grad, alpha[:T], beta[:T]
    sm_tok = np.exp(tok + sigma)
    sm_dur = np.exp(dur)
    for t in range(T):
        for u in range(U + 1):
            a = alpha[t, u]
            if not np.isfinite(a) or not np.isfinite(beta[t, u]):
                continue
            Ob = Ol = 0.0
            occ = np.zeros(D)
            for n, d in enumerate(durations):
                if d >= 1 and (t + d < T or (t + d == T and u == U)) and np.isfinite(beta[t + d, u]):
                    ob = np.exp(a + tok[t, u, blank] + dur[t, u, n] + beta[t + d, u] - ll)
                    Ob += ob
                    occ[n] += ob
                if u < U and t + d <= T - 1 and np.isfinite(beta[t + d, u + 1]):
                    ol = np.exp(a + tok[t, u, labels[u]] + dur[t, u, n] + beta[t + d, u + 1] - ll)
                    Ol += ol
                    occ[n] += ol
            O = np.exp(a + beta[t, u] - ll)
            g = sm_tok[t, u] * O
            g[blank] -= Ob
            if u < U:
                g[labels[u]] -= Ol
            grad[t, u, :V] = g
            grad[t, u, V:] = sm_dur[t, u] * O - occ
    return -ll, grad, alpha[:T], beta[:T]


def tdt_ref(logits, targets, llens, tlens, durations, blank=0, sigma=0.0):
    logits = np.asarray(logits, np.float64)
    B, T, U1, W = logits.shape
    costs = np.zeros(B)
    grad = np.zeros_like(logits)
    alpha = np.zeros((B, T, U1))
    beta = np.zeros((B, T, U1))
    for b in range(B):
        Tb, Ub = int(llens[b]), int(tlens[b])
        c, g, a, be = tdt_utt_f64(logits[b], np.asarray(targets)[b] if U1 > 1 else [], Tb, Ub, durations, blank, sigma)
        costs[b] = c
        grad[b, :Tb, :Ub + 1] = g
        alpha[b, :Tb, :Ub + 1] = a
        beta[b, :Tb, :Ub + 1] = be
    return costs, grad, alpha, beta


def enumerate_paths(logits, labels, T, U, durations, blank, sigma):
    """log of the summed probability of every path (0,0) -> terminal, by depth-first enumeration; -inf without a path."""
    D = len(durations)
    V = logits.shape[-1] - D
    tok, dur = arcs_f64(np.asarray(logits, np.float64)[:T, :U + 1], V, sigma)
    total = [0.0]

    def walk(t, u, logp):
        for n, d in enumerate(durations):
            if d >= 1:
                w = logp + tok[t, u, blank] + dur[t, u, n]
                if t + d < T:
                    walk(t + d, u, w)
                elif t + d == T and u == U:
                    total[0] += np.exp(w)
            if u < U and t + d <= T - 1:
                walk(t + d, u + 1, logp + tok[t, u, labels[u]] + dur[t, u, n])

    walk(0, 0, 0.0)
    return np.log(total[0]) if total[0] > 0.0 else -np.inf


def cost_torch(logits, labels, T, U, durations, blank, sigma):
    """The cost of one utterance as a float64 torch expression of `logits` (T.., U+1.., V + D), for autograd.  Nodes
    without an incoming arc carry NEG_BIG; a result above -NEG_BIG / 2 means "no path"."""
    D = len(durations)
    V = logits.shape[-1] - D
    x = logits[:T, :U + 1].to(torch.float64)
    tok = torch.log_softmax(x[..., :V], -1) - sigma
    dur = torch.log_softmax(x[..., V:], -1)
    neg = torch.tensor(NEG_BIG, dtype=torch.float64)
    alpha = {(0, 0): torch.zeros((), dtype=torch.float64)}
    for t in range(T + 1):
        for u in range(U + 1):
            if (t == 0 and u == 0) or (t == T and u != U):
                continue
            terms = []
            for n, d in enumerate(durations):
                if d >= 1 and t - d >= 0:
                    terms.append(alpha[(t - d, u)] + tok[t - d, u, blank] + dur[t - d, u, n])
                if u >= 1 and t - d >= 0 and t <= T - 1:
                    terms.append(alpha[(t - d, u - 1)] + tok[t - d, u - 1, labels[u - 1]] + dur[t - d, u - 1, n])
            alpha[(t, u)] = torch.logsumexp(torch.stack(terms), 0) if terms else neg
    return -alpha[(T, U)]
