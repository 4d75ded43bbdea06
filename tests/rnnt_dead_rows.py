"""Host restatement of the dead-cell test of rnnt_grad_kernel (wenet-celoss_amd/csrc/rnnt_loss.hip, kDeadThr).

A valid cell (t, u) of utterance b is dead when the row log-sum-exp `denom` is finite and below 2^16 in magnitude and
every bound on an exponent of its gradient lies below -110 nats:
    alpha + beta + cost                       (main term)
    alpha + cost + beta(t+1, u)               (blank term, t < T-1; alpha + cost at the final cell)
    alpha + cost + beta(t, u+1)               (label term, u < U, unless the label is the blank of a blank-term cell)
A NaN anywhere makes the cell live.  Plain helper module (not a conftest): tests import it.
"""
import numpy as np

DEAD_THR = -110.0
DENOM_MAX = 65536.0


def lattice_f64(logits, targets, llens, tlens, blank=0):
    """float64 (denom, alpha, beta, cost) of a batch: denom/alpha/beta [B,T,U+1] (-inf outside the lattice), cost [B]."""
    x = np.asarray(logits, np.float64)
    B, T, U1, V = x.shape
    m = x.max(axis=-1, keepdims=True)
    denom = (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))[..., 0]
    alpha = np.full((B, T, U1), -np.inf)
    beta = np.full((B, T, U1), -np.inf)
    cost = np.zeros(B)
    for b in range(B):
        Tb, Ub = int(llens[b]), int(tlens[b])
        if Tb == 0:
            continue
        sk = x[b, :Tb, :Ub + 1, blank] - denom[b, :Tb, :Ub + 1]
        em = np.zeros((Tb, Ub + 1))
        if Ub > 0:
            lab = np.asarray(targets[b][:Ub], np.int64)
            em[:, :Ub] = np.take_along_axis(x[b, :Tb, :Ub, :], lab[None, :, None], axis=-1)[..., 0] - denom[b, :Tb, :Ub]
        a = alpha[b]
        for t in range(Tb):
            for u in range(Ub + 1):
                if t == 0 and u == 0:
                    a[t, u] = 0.0
                    continue
                top = a[t - 1, u] + sk[t - 1, u] if t > 0 else -np.inf
                left = a[t, u - 1] + em[t, u - 1] if u > 0 else -np.inf
                a[t, u] = np.logaddexp(top, left)
        be = beta[b]
        for t in range(Tb - 1, -1, -1):
            for u in range(Ub, -1, -1):
                if t == Tb - 1 and u == Ub:
                    be[t, u] = sk[t, u]
                    continue
                down = be[t + 1, u] + sk[t, u] if t < Tb - 1 else -np.inf
                right = be[t, u + 1] + em[t, u] if u < Ub else -np.inf
                be[t, u] = np.logaddexp(down, right)
        cost[b] = -be[0, 0]
    return denom, alpha, beta, cost


def dead_mask(alpha, beta, cost, targets, llens, tlens, blank=0, denom=None, thr=DEAD_THR):
    """Boolean [B,T,U+1]: the cells the gradient pass writes without reading (float64 arithmetic; denom=None skips the
    denom test, for callers that only have the exported lattice)."""
    alpha = np.asarray(alpha, np.float64)
    beta = np.asarray(beta, np.float64)
    B, T, U1 = alpha.shape
    t = np.arange(T)[:, None]
    u = np.arange(U1)[None, :]
    out = np.zeros((B, T, U1), bool)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            Tb, Ub = int(llens[b]), int(tlens[b])
            valid = (t < Tb) & (u <= Ub)
            final = (t == Tb - 1) & (u == Ub)
            has_b1 = t < Tb - 1
            blank_special = final | has_b1
            lab = np.full(U1, -1, np.int64)
            lab[:Ub] = np.asarray(targets[b][:Ub], np.int64)
            has_lab = (u < Ub) & ~((lab[None, :] == blank) & blank_special)
            ac = alpha[b] + float(cost[b])
            b1 = np.full((T, U1), -np.inf)
            b1[:-1] = beta[b, 1:]
            b2 = np.full((T, U1), -np.inf)
            b2[:, :-1] = beta[b, :, 1:]
            dead = valid & (ac + beta[b] < thr)
            dead &= ~blank_special | (np.where(has_b1, ac + b1, ac) < thr)
            dead &= ~has_lab | (ac + b2 < thr)
            if denom is not None:
                dead &= np.abs(np.asarray(denom[b], np.float64)) < DENOM_MAX
            out[b] = dead
    return out


def dead_share(mask, llens, tlens):
    """Dead cells over valid cells."""
    valid = sum(int(a) * (int(c) + 1) for a, c in zip(llens, tlens))
    return float(mask.sum()) / max(valid, 1)
