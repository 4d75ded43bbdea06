"""Float64 references of the smoothed additive-joiner RNN-T loss (k2's rnnt_loss_smoothed), written from the contract in
include/wr_api.h and not from the kernels.  With ll = lm_only_scale, la = am_only_scale, c = 1 - ll - la:

    Zl[b,u] = logsumexp_v lm[b,u,v]
    pbar[v] = mean over ALL B * (U+1) rows of softmax(lm[b,u,:])[v]  +  TINY (the smallest normal float32)
    N[b,t]  = log sum_v exp(am[b,t,v]) pbar[v]
    arc(t,u,v) = c (am[t,v] + lm[u,v] - denom(t,u)) + ll (lm[u,v] - Zl[u]) + la (am[t,v] + log pbar[v] - N[t])

A scale that is exactly 0 drops its branch.

  loss_torch_f64(...)      (a) the costs as a differentiable float64 torch expression: the arcs above in the recursion of
                           rnnt_simple_ref.loss_torch_f64
  pbar_f64(lm)             the unigram of a batch
  arcs_f64(...)            (b) one utterance, explicit loops: blank (T, U+1) and emit (T, U+1) (last column 0) given pbar
  lattice_f64(...)         (b) cost, alpha, beta and the two arc occupancies of rnnt_simple_ref.lattice_f64's recursion on
                           those arcs
  enumerate_paths(...)     brute force over every path of a tiny lattice on those arcs
  gradient_formula(...)    d_am, d_lm of sum_b g_b cost_b from the occupancies, by the formula of include/wr_api.h
"""
import itertools

import numpy as np
import torch

TINY = float(np.finfo(np.float32).tiny)


def _check(ll, la):
    assert ll >= 0 and la >= 0 and ll + la <= 1


# ------------------------------------------------------------------------------------------------- (a) torch --
def loss_torch_f64(lm, am, symbols, blank, t_lens, u_lens, ll, la):
    """Costs (B,) as a differentiable float64 torch expression of lm (B, U+1, V) and am (B, T, V)."""
    _check(ll, la)
    c = 1.0 - ll - la
    lm, am = lm.double(), am.double()
    B, U1, V = lm.shape
    zl = torch.logsumexp(lm, -1)                                              # (B, U1)
    if la != 0:
        pbar = torch.softmax(lm, -1).reshape(B * U1, V).mean(0) + TINY        # every row, padded ones included
        n = torch.logsumexp(am + pbar.log(), -1)                              # (B, T)
    costs = []
    for b in range(B):
        T, U = int(t_lens[b]), int(u_lens[b])
        x = am[b, :T, None, :] + lm[b, None, :U + 1, :]
        lp = c * torch.log_softmax(x, -1)
        if ll != 0:
            lp = lp + ll * (lm[b, None, :U + 1, :] - zl[b, None, :U + 1, None])
        if la != 0:
            lp = lp + la * (am[b, :T, None, :] + pbar.log() - n[b, :T, None, None])
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


# ------------------------------------------------------------------------------------------------- (b) numpy --
def _lse(x):
    m = max(x)
    return m + np.log(sum(np.exp(v - m) for v in x))


def pbar_f64(lm):
    """lm (B, U+1, V) -> pbar (V,): the mean row softmax over all B * (U+1) rows, plus TINY."""
    lm = np.asarray(lm, np.float64)
    rows = lm.reshape(-1, lm.shape[-1])
    acc = np.zeros(rows.shape[1])
    for r in rows:
        z = _lse(r)
        acc += np.exp(r - z)
    return acc / rows.shape[0] + TINY


def arcs_f64(lm, am, symbols, blank, T, U, pbar, ll, la):
    """One utterance, explicit loops.  lm (>= U+1, V), am (>= T, V) -> blank (T, U+1), emit (T, U+1) (last column 0)."""
    _check(ll, la)
    c = 1.0 - ll - la
    lm, am = np.asarray(lm, np.float64), np.asarray(am, np.float64)
    V = lm.shape[1]
    skip, emit = np.zeros((T, U + 1)), np.zeros((T, U + 1))
    for t in range(T):
        n = _lse([am[t, v] + np.log(pbar[v]) for v in range(V)]) if la != 0 else 0.0
        for u in range(U + 1):
            denom = _lse([am[t, v] + lm[u, v] for v in range(V)])
            zl = _lse([lm[u, v] for v in range(V)])

            def arc(v):
                a = c * (am[t, v] + lm[u, v] - denom)
                if ll != 0:
                    a += ll * (lm[u, v] - zl)
                if la != 0:
                    a += la * (am[t, v] + np.log(pbar[v]) - n)
                return a
            skip[t, u] = arc(blank)
            if u < U:
                emit[t, u] = arc(int(symbols[u]))
    return skip, emit


def lattice_from_arcs(skip, emit):
    """The recursion of rnnt_simple_ref.lattice_f64 on given arcs: (cost, alpha, beta, occ_emit, occ_blank)."""
    T, U = skip.shape[0], skip.shape[1] - 1
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


def lattice_f64(lm, am, symbols, blank, T, U, pbar, ll, la):
    return lattice_from_arcs(*arcs_f64(lm, am, symbols, blank, T, U, pbar, ll, la))


def enumerate_paths(skip, emit):
    """Every monotone path of the lattice: (total probability, occ_emit, occ_blank normalised by the total)."""
    T, U = skip.shape[0], skip.shape[1] - 1
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


def gradient_formula(lm, am, symbols, blank, t_lens, u_lens, ll, la, g):
    """(d_am (B,T,V), d_lm (B,U+1,V)) of sum_b g[b] cost_b in float64 numpy: the formula of include/wr_api.h evaluated
    from the occupancies of lattice_f64."""
    _check(ll, la)
    c = 1.0 - ll - la
    lm, am = np.asarray(lm, np.float64), np.asarray(am, np.float64)
    B, U1, V = lm.shape
    T_max = am.shape[1]
    pbar = pbar_f64(lm)
    d_am, d_lm = np.zeros((B, T_max, V)), np.zeros((B, U1, V))
    h = np.zeros(V)
    for b in range(B):
        T, U = int(t_lens[b]), int(u_lens[b])
        _, _, _, oe, ob = lattice_f64(lm[b], am[b], symbols[b], blank, T, U, pbar, ll, la)
        occ = oe + ob
        sub_am, sub_lm = np.zeros((T, V)), np.zeros((U + 1, V))      # sum oe [v = y_u] + sum ob [v = blank]
        for t in range(T):
            for u in range(U + 1):
                sub_am[t, blank] += ob[t, u]; sub_lm[u, blank] += ob[t, u]
                if u < U:
                    y = int(symbols[b][u])
                    sub_am[t, y] += oe[t, u]; sub_lm[u, y] += oe[t, u]
        x = am[b, :T, None, :] + lm[b, None, :U + 1, :]
        sig = np.exp(x - x.max(-1, keepdims=True))
        sig /= sig.sum(-1, keepdims=True)
        main = occ[:, :, None] * sig
        d_am[b, :T] = c * main.sum(1) - (c + la) * sub_am
        d_lm[b, :U + 1] = c * main.sum(0) - (c + ll) * sub_lm
        if ll != 0:
            s = np.exp(lm[b, :U + 1] - lm[b, :U + 1].max(-1, keepdims=True))
            s /= s.sum(-1, keepdims=True)
            d_lm[b, :U + 1] += ll * occ.sum(0)[:, None] * s
        if la != 0:
            n = np.log((np.exp(am[b, :T]) * pbar).sum(-1))
            e = np.exp(am[b, :T] - n[:, None])                        # exp(am - N)
            C = occ.sum(1)
            d_am[b, :T] += la * C[:, None] * e * pbar
            h += la * g[b] * ((C[:, None] * e).sum(0) - sub_am.sum(0) / pbar)
        d_am[b] *= g[b]
        d_lm[b] *= g[b]
    if la != 0:
        s = np.exp(lm - lm.max(-1, keepdims=True))
        s /= s.sum(-1, keepdims=True)
        d_lm += s * (h - (s * h).sum(-1, keepdims=True)) / (B * U1)
    return d_am, d_lm
