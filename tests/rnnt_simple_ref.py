"""Float64 references of the additive-joiner ("simple") RNN-T loss, logits(t,u,v) = am[t,v] + lm[u,v].

  materialised(lm, am)         the (B, T, U+1, V) float32 sum the loss is defined on (what `oracle.rnnt_loss_f64` takes)
  oracle_reference(...)        cost, d_am, d_lm from `oracle.rnnt_loss_f64` on that sum: the logits gradient summed over u
                               (for am) and over t (for lm), in float64
  lattice_f64(...)             one utterance: cost, alpha, beta and the two arc occupancies, float64 numpy
                                   occ_blank(t,u) = exp(alpha(t,u) + blank(t,u) + beta(t+1,u) - ll)   (final cell: beta := 0)
                                   occ_emit(t,u)  = exp(alpha(t,u) + emit(t,u)  + beta(t,u+1) - ll)
  loss_torch_f64(...)          the costs as a differentiable float64 torch expression (small lattices only)
  enumerate_paths(...)         brute force over every path of a tiny lattice: total probability and arc occupancies
"""
import itertools

import numpy as np
import torch


def materialised(lm, am):
    lm, am = np.asarray(lm, np.float32), np.asarray(am, np.float32)
    return np.ascontiguousarray(am[:, :, None, :] + lm[:, None, :, :])


def oracle_reference(lm, am, symbols, blank, t_lens, u_lens):
    """(costs (B,) f64, d_am (B,T,V) f64, d_lm (B,U+1,V) f64) of sum_b cost_b, through the float64 oracle."""
    import oracle
    logits = materialised(lm, am)
    costs, grad = oracle.rnnt_loss_f64(logits, np.asarray(symbols, np.int32).reshape(logits.shape[0], -1),
                                       np.asarray(t_lens, np.int32), np.asarray(u_lens, np.int32), blank=blank)
    return costs, grad.sum(2, dtype=np.float64), grad.sum(1, dtype=np.float64)


def log_probs_f64(lm, am, symbols, blank):
    """One utterance: lm (U+1, V), am (T, V) -> blank (T, U+1), emit (T, U+1) (last column 0) in float64.  The sum am + lm
    is taken in the inputs' own precision (float32 inputs: the materialised float32 logits the oracle sees)."""
    x = (np.asarray(am)[:, None, :] + np.asarray(lm)[None, :, :]).astype(np.float64)
    m = x.max(-1, keepdims=True)
    lp = x - (m + np.log(np.exp(x - m).sum(-1, keepdims=True)))
    U = x.shape[1] - 1
    emit = np.zeros(lp.shape[:2])
    for u in range(U):
        emit[:, u] = lp[:, u, int(symbols[u])]
    return lp[:, :, blank], emit


def lattice_f64(lm, am, symbols, blank, T, U):
    """One utterance restricted to T frames and U labels.  Returns (cost, alpha, beta, occ_emit, occ_blank), the arrays
    (T, U+1)."""
    skip, emit = log_probs_f64(np.asarray(lm)[:U + 1], np.asarray(am)[:T], symbols, blank)
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
    ll = beta[0, 0]
    occ_blank = np.zeros((T, U + 1))
    occ_emit = np.zeros((T, U + 1))
    for t in range(T):
        for u in range(U + 1):
            if t < T - 1:
                occ_blank[t, u] = np.exp(alpha[t, u] + skip[t, u] + beta[t + 1, u] - ll)
            elif u == U:
                occ_blank[t, u] = np.exp(alpha[t, u] + skip[t, u] - ll)
            if u < U:
                occ_emit[t, u] = np.exp(alpha[t, u] + emit[t, u] + beta[t, u + 1] - ll)
    return -ll, alpha, beta, occ_emit, occ_blank


def loss_torch_f64(lm, am, symbols, blank, t_lens, u_lens):
    """Costs (B,) as a differentiable float64 torch expression of lm (B, U+1, V) and am (B, T, V)."""
    costs = []
    for b in range(lm.shape[0]):
        T, U = int(t_lens[b]), int(u_lens[b])
        x = am[b, :T, None, :].double() + lm[b, None, :U + 1, :].double()
        lp = torch.log_softmax(x, -1)
        alpha = [[None] * (U + 1) for _ in range(T)]
        alpha[0][0] = lp.new_zeros(())
        for t in range(T):
            for u in range(U + 1):
                terms = []
                if t:
                    terms.append(alpha[t - 1][u] + lp[t - 1, u, blank])
                if u:
                    terms.append(alpha[t][u - 1] + lp[t, u - 1, int(symbols[b][u - 1])])
                if terms:
                    alpha[t][u] = torch.logsumexp(torch.stack(terms), 0)
        costs.append(-(alpha[T - 1][U] + lp[T - 1, U, blank]))
    return torch.stack(costs)


def enumerate_paths(lm, am, symbols, blank, T, U):
    """Every monotone path of the T x (U+1) lattice (U emits and T blanks, the last arc the blank out of (T-1, U)):
    (total probability, occ_emit (T, U+1), occ_blank (T, U+1)) with the occupancies normalised by the total."""
    skip, emit = log_probs_f64(np.asarray(lm)[:U + 1], np.asarray(am)[:T], symbols, blank)
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
        assert (t, u) == (T - 1, U)
        logp += skip[t, u]; arcs.append((0, t, u))
        p = np.exp(logp)
        total += p
        for kind, tt, uu in arcs:
            (oe if kind else ob)[tt, uu] += p
    return total, oe / total, ob / total
