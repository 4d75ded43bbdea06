"""Float64 references of the modified lattice and the delay penalty of the k2 RNN-T losses, written from the contract in
include/wr_api.h ("Lattice types and the delay penalty") and not from the kernels.

Arcs are (T, U+1) arrays `skip` (blank) and `emit` (label; column U is never used) as the references of the three
losses produce them: rnnt_simple_ref.log_probs_f64, rnnt_smoothed_ref.arcs_f64, rnnt_pruned_ref.band_log_probs_f64.

  penalty_f64(dp, T)                    pen[t] = dp * ((T - 1) / 2 - t)
  penalised(emit, dp)                   emit + pen[:, None]
  lattice_modified_f64(skip, emit)      explicit loops: (cost, alpha, beta, occ_emit, occ_blank), arrays (T, U+1)
  lattice_regular_f64(skip, emit)       the regular recursion on the same arcs (rnnt_smoothed_ref.lattice_from_arcs)
  enumerate_paths_modified(skip, emit)  brute force over every path of a tiny modified lattice
  cost_torch(skip, emit, rnnt_type)     the cost as a differentiable float64 torch expression of torch arcs
  simple_costs_torch / pruned_costs_torch   the three losses (simple = smoothed with both scales 0) for either lattice
  prune_ranges_ref(px, py, boundary, s_range)   get_rnnt_prune_ranges for px of (B, U, T) or (B, U, T+1)

In the torch expressions an arc or a node that does not exist carries NEG_BIG, a large finite negative, instead of -inf:
a logsumexp whose terms are all -inf has NaN gradients.
"""
import itertools

import numpy as np
import torch

import rnnt_pruned_ref
import rnnt_smoothed_ref

NEG_BIG = -1.0e30
TINY = rnnt_smoothed_ref.TINY


def penalty_f64(dp, T):
    return np.float64(dp) * ((T - 1) / 2.0 - np.arange(T, dtype=np.float64))


def penalised(emit, dp):
    emit = np.asarray(emit, np.float64)
    return emit + penalty_f64(dp, emit.shape[0])[:, None] if dp > 0 else emit.copy()


def lattice_modified_f64(skip, emit):
    """Nodes (t, u), 0 <= t <= T; blank (t,u) -> (t+1,u), label (t,u) -> (t+1,u+1).  Returns (cost, alpha, beta, occ_emit,
    occ_blank) with rows 0 .. T-1 of alpha / beta; cost = +inf (and zero occupancies) when no path exists."""
    skip, emit = np.asarray(skip, np.float64), np.asarray(emit, np.float64)
    T, U = skip.shape[0], skip.shape[1] - 1
    alpha = np.full((T + 1, U + 1), -np.inf)
    beta = np.full((T + 1, U + 1), -np.inf)
    alpha[0, 0] = 0.0
    beta[T, U] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(1, T + 1):
            for u in range(U + 1):
                a = alpha[t - 1, u] + skip[t - 1, u]
                if u:
                    a = np.logaddexp(a, alpha[t - 1, u - 1] + emit[t - 1, u - 1])
                alpha[t, u] = a
        for t in range(T - 1, -1, -1):
            for u in range(U, -1, -1):
                b = skip[t, u] + beta[t + 1, u]
                if u < U:
                    b = np.logaddexp(b, emit[t, u] + beta[t + 1, u + 1])
                beta[t, u] = b
    ll = alpha[T, U]
    occ_blank, occ_emit = np.zeros((T, U + 1)), np.zeros((T, U + 1))
    if np.isfinite(ll):
        for t in range(T):
            for u in range(U + 1):
                if not np.isfinite(alpha[t, u]):
                    continue
                if np.isfinite(skip[t, u]) and np.isfinite(beta[t + 1, u]):
                    occ_blank[t, u] = np.exp(alpha[t, u] + skip[t, u] + beta[t + 1, u] - ll)
                if u < U and np.isfinite(emit[t, u]) and np.isfinite(beta[t + 1, u + 1]):
                    occ_emit[t, u] = np.exp(alpha[t, u] + emit[t, u] + beta[t + 1, u + 1] - ll)
    return -ll, alpha[:T], beta[:T], occ_emit, occ_blank


def lattice_regular_f64(skip, emit):
    return rnnt_smoothed_ref.lattice_from_arcs(np.asarray(skip, np.float64), np.asarray(emit, np.float64))


def enumerate_paths_modified(skip, emit):
    """Every path of the modified lattice (one arc per frame, U of the T frames carry a label): (total probability,
    occ_emit, occ_blank normalised by the total; zeros when there is no path)."""
    T, U = skip.shape[0], skip.shape[1] - 1
    total = 0.0
    oe, ob = np.zeros((T, U + 1)), np.zeros((T, U + 1))
    for label_frames in itertools.combinations(range(T), U):
        u, logp, arcs = 0, 0.0, []
        for t in range(T):
            if t in label_frames:
                logp += emit[t, u]; arcs.append((1, t, u)); u += 1
            else:
                logp += skip[t, u]; arcs.append((0, t, u))
        assert u == U
        p = np.exp(logp)
        total += p
        for kind, tt, uu in arcs:
            (oe if kind else ob)[tt, uu] += p
    if total > 0:
        oe, ob = oe / total, ob / total
    return total, oe, ob


# ------------------------------------------------------------------------------------------------- torch --
def cost_torch(skip, emit, rnnt_type):
    """skip, emit (T, U+1) float64 torch (emit already penalised; absent arcs NEG_BIG; column U of emit unused) -> cost."""
    T, U1 = skip.shape
    U = U1 - 1
    neg = skip.new_full((1,), NEG_BIG)
    if rnnt_type == "modified":
        if T < U:
            return skip.new_full((), float("inf"))
        alpha = torch.cat([skip.new_zeros(1), neg.expand(U)])
        for t in range(T):
            stay = alpha + skip[t]
            move = torch.cat([neg, (alpha + emit[t])[:U]])
            alpha = torch.logaddexp(stay, move)
        ll = alpha[U]
    else:
        assert rnnt_type == "regular"
        # anti-diagonals: entry u of `prev` is alpha(s - 1 - u, u), NEG_BIG where that is no cell
        us = torch.arange(U1)
        prev = torch.cat([skip.new_zeros(1), neg.expand(U)])           # s = 0
        for s in range(1, T + U):
            ts = s - us                                                # t of the cell (t, u) on diagonal s
            valid = (ts >= 0) & (ts < T)
            t_up = (ts - 1).clamp(0, T - 1)                            # from (t-1, u) by its blank
            up = torch.where((ts >= 1) & valid, prev + skip[t_up, us], neg)
            t_cur = ts.clamp(0, T - 1)                                 # from (t, u-1) by its label
            left = torch.cat([neg, (prev[:-1] + emit[t_cur[1:], us[:-1]])]) if U else neg
            left = torch.where(valid & (us >= 1), left, neg)
            prev = torch.where(valid, torch.logaddexp(up, left), neg)
        ll = prev[U] + skip[T - 1, U]
    if float(ll.detach()) < 0.5 * NEG_BIG:
        return skip.new_full((), float("inf"))
    return -ll


def _pen_torch(dp, T):
    return torch.as_tensor(penalty_f64(dp, T))[:, None]


def simple_costs_torch(lm, am, symbols, blank, t_lens, u_lens, ll=0.0, la=0.0, rnnt_type="regular", delay_penalty=0.0,
                       arcs=None):
    """rnnt_loss_smoothed (both scales 0: rnnt_loss_simple) on either lattice: costs (B,), differentiable in lm
    (B, U+1, V) and am (B, T, V).  The arcs are those of rnnt_smoothed_ref.loss_torch_f64; the penalty is added after
    the interpolation.  `arcs` (a list) receives every utterance's (skip, emit) with their gradients retained: after
    costs.sum().backward() they hold minus the arc occupancies (checked in test_rnnt_lattice_ref.py)."""
    c = 1.0 - ll - la
    lm, am = lm.double(), am.double()
    B, U1, V = lm.shape
    zl = torch.logsumexp(lm, -1)
    if la != 0:
        pbar = torch.softmax(lm, -1).reshape(B * U1, V).mean(0) + TINY
        n = torch.logsumexp(am + pbar.log(), -1)
    costs = []
    for b in range(B):
        T, U = int(t_lens[b]), int(u_lens[b])
        if T == 0:
            costs.append(lm.new_zeros(()))
            if arcs is not None:
                arcs.append((lm.new_zeros((0, U + 1)), lm.new_zeros((0, U + 1))))
            continue
        x = am[b, :T, None, :] + lm[b, None, :U + 1, :]
        lp = c * torch.log_softmax(x, -1)
        if ll != 0:
            lp = lp + ll * (lm[b, None, :U + 1, :] - zl[b, None, :U + 1, None])
        if la != 0:
            lp = lp + la * (am[b, :T, None, :] + pbar.log() - n[b, :T, None, None])
        skip = lp[:, :, blank]
        emit = lp.new_full((T, U + 1), NEG_BIG)
        if U:
            idx = torch.as_tensor(np.asarray(symbols[b][:U], np.int64))[None, :, None].expand(T, U, 1)
            emit = torch.cat([lp[:, :U].gather(-1, idx)[..., 0], emit[:, U:]], 1)
        if delay_penalty > 0:
            emit = emit + _pen_torch(delay_penalty, T)
        if arcs is not None:
            for x in (skip, emit):
                if x.requires_grad:
                    x.retain_grad()
            arcs.append((skip, emit))
        costs.append(cost_torch(skip, emit, rnnt_type))
    return torch.stack(costs)


def occupancies_from_arcs(arcs, B, T, U1):
    """(occ_emit, occ_blank) (B, T, U1) float64 numpy from the arcs list of simple_costs_torch after a unit backward."""
    oe, ob = np.zeros((B, T, U1)), np.zeros((B, T, U1))
    for b, (skip, emit) in enumerate(arcs):
        t, u1 = skip.shape
        if skip.grad is not None:
            ob[b, :t, :u1] = -skip.grad.numpy()
        if emit.grad is not None:
            oe[b, :t, :u1 - 1] = -emit.grad.numpy()[:, :u1 - 1]
    return oe, ob


def pruned_costs_torch(logits, ranges, symbols, blank, t_lens, u_lens, rnnt_type="regular", delay_penalty=0.0):
    """rnnt_loss_pruned on either lattice: costs (B,), differentiable in logits (B, T, R, V); +inf when no path fits."""
    costs = []
    ranges = np.asarray(ranges)
    for b in range(logits.shape[0]):
        T, U = int(t_lens[b]), int(u_lens[b])
        lp = torch.log_softmax(logits[b, :T].double(), -1)                     # (T, R, V)
        skip_rows, emit_rows = [], []
        for t in range(T):
            sk = [lp.new_full((), NEG_BIG)] * (U + 1)
            em = [lp.new_full((), NEG_BIG)] * (U + 1)
            for r in range(ranges.shape[2]):
                u = int(ranges[b, t, r])
                if 0 <= u <= U:
                    sk[u] = lp[t, r, blank]
                    if u < U:
                        em[u] = lp[t, r, int(symbols[b][u])]
            skip_rows.append(torch.stack(sk))
            emit_rows.append(torch.stack(em))
        skip, emit = torch.stack(skip_rows), torch.stack(emit_rows)
        if delay_penalty > 0:
            emit = emit + _pen_torch(delay_penalty, T)
        costs.append(cost_torch(skip, emit, rnnt_type))
    return torch.stack(costs)


def costs_and_grads(fn, inputs, grad_costs=None):
    """fn(*leaves) -> costs (B,): (costs numpy with +inf kept, [gradient numpy per input]) of sum_b g_b cost_b over the
    finite costs."""
    leaves = [torch.tensor(np.asarray(x), dtype=torch.float64, requires_grad=True) for x in inputs]
    costs = fn(*leaves)
    g = torch.ones_like(costs) if grad_costs is None else torch.as_tensor(np.asarray(grad_costs), dtype=torch.float64)
    finite = torch.isfinite(costs)
    (costs[finite] * g[finite]).sum().backward()
    return costs.detach().numpy(), [x.grad.numpy() if x.grad is not None else np.zeros(x.shape) for x in leaves]


# ------------------------------------------------------------------------------------------------ ranges --
def prune_ranges_ref(px, py, boundary, s_range):
    """get_rnnt_prune_ranges for px (B, U, T) (the modified lattice's layout; s_range >= 1) or (B, U, T+1) (s_range >= 2).
    The window score reads only columns t < T, so the rule of rnnt_pruned_ref.prune_ranges_ref applies to both."""
    px, py = np.asarray(px), np.asarray(py)
    B, U1, T = py.shape
    assert px.shape in ((B, U1 - 1, T), (B, U1 - 1, T + 1))
    assert int(s_range) >= (1 if px.shape[2] == T else 2)
    return rnnt_pruned_ref.prune_ranges_ref(px, py, boundary, s_range)
