"""Float64 reference of FastEmit and the delay penalty for the full-lattice RNN-T loss, written from the contract in
include/wr_api.h ("FastEmit and the delay penalty for the full-lattice loss") and not from the kernels.

  arcs_f64(logits, targets, T, U, blank)        (skip, emit, log-softmax) of one utterance
  loss_f64(logits, targets, llens, tlens, ...)  costs (B,), the logits gradient (B, T, U+1, V) by the formula, and the
                                                lattice of every utterance (for the checks below)
  classify(lattices, targets, llens, tlens, ...) the three row bounds with be_eff, pen and log1p(lambda): LIVE / FAINT /
                                                DEAD per cell, modelled on rnnt_faint_rows.classify

Case chain (the contract): the blank term exists at the final cell and wherever t < T_b - 1; the label term (and with it
the FastEmit term) exists for u < U_b unless the label equals the blank at a cell that has a blank term.
Plain helper module (not a conftest): tests import it.
"""
import math

import numpy as np

import rnnt_lattice_ref
from rnnt_faint_rows import DEAD, DEAD_THR, FAINT, LIVE, PADDED


def arcs_f64(logits_b, targets_b, T, U, blank):
    """logits_b (Tmax, U1max, V) -> skip (T, U+1), emit (T, U+1) (column U zero, never used), lsm (T, U+1, V)."""
    x = np.asarray(logits_b, np.float64)[:T, :U + 1]
    m = x.max(axis=-1, keepdims=True)
    lsm = x - (m + np.log(np.exp(x - m).sum(axis=-1, keepdims=True)))
    skip = lsm[:, :, blank].copy()
    emit = np.zeros((T, U + 1))
    if U:
        lab = np.asarray(targets_b[:U], np.int64)
        emit[:, :U] = np.take_along_axis(lsm[:, :U], lab[None, :, None], axis=-1)[..., 0]
    return skip, emit, lsm


def loss_f64(logits, targets, llens, tlens, blank=0, fastemit_lambda=0.0, delay_penalty=0.0, clamp=-1.0,
             grad_costs=None):
    """(costs (B,), grad (B, T, U+1, V) float64, lattices): grad = clamp(g) * grad_costs[b] with
    g = softmax (occ_blank + (1 + lambda) occ_emit) - [v = blank] occ_blank - [v = label] (1 + lambda) occ_emit,
    exact zeros outside the lattice.  lattices[b] = dict(alpha, beta, cost, emit (penalised), occ_emit, occ_blank) or None
    for an utterance without a frame."""
    logits = np.asarray(logits)
    B, Tm, U1m, V = logits.shape
    lam = float(fastemit_lambda)
    costs = np.zeros(B)
    grad = np.zeros((B, Tm, U1m, V))
    lattices = []
    for b in range(B):
        T, U = int(llens[b]), int(tlens[b])
        if T == 0:
            lattices.append(None)
            continue
        skip, emit, lsm = arcs_f64(logits[b], targets[b], T, U, blank)
        emit_p = rnnt_lattice_ref.penalised(emit, delay_penalty)
        emit_p[:, U] = 0.0
        cost, alpha, beta, occ_e, occ_b = rnnt_lattice_ref.lattice_regular_f64(skip, emit_p)
        costs[b] = cost
        go = 1.0 if grad_costs is None else float(grad_costs[b])
        sm = np.exp(lsm)
        for t in range(T):
            for u in range(U + 1):
                blank_special = t < T - 1 or u == U
                lab = int(targets[b][u]) if u < U else -1
                has_lab = u < U and not (lab == blank and blank_special)
                tot = math.exp(alpha[t, u] + beta[t, u] + cost)
                if has_lab:
                    tot += lam * occ_e[t, u]
                g = sm[t, u] * tot
                if blank_special:
                    g[blank] -= occ_b[t, u]
                if has_lab and 0 <= lab < V:
                    g[lab] -= (1.0 + lam) * occ_e[t, u]
                if clamp > 0:
                    g = np.clip(g, -clamp, clamp)
                grad[b, t, u] = g * go
        lattices.append(dict(alpha=alpha, beta=beta, cost=cost, emit=emit_p, skip=skip, occ_emit=occ_e, occ_blank=occ_b))
    return costs, grad, lattices


def classify(lattices, targets, llens, tlens, Tmax, U1max, blank=0, fastemit_lambda=0.0, delay_penalty=0.0, thr=DEAD_THR):
    """int8 (B, Tmax, U1max) of LIVE / FAINT / DEAD (PADDED outside the lattice) from the reference lattices, with the
    bounds of the contract:
        main   alpha + cost + be_eff,  be_eff = logadd(beta, log lambda + emit' + beta(t,u+1)) where the label term
               exists and lambda > 0, else beta
        blank  alpha + cost + beta(t+1,u)  (alpha + cost at the final cell)
        label  alpha + cost + beta(t,u+1) + pen(b,t) + log1p(lambda)
    and the masks (needs_blank, needs_label) of the faint rows' elements that are read.  (The kernel's |denom| < 2^16
    test is the caller's to respect: these inputs have small logits.)"""
    B = len(lattices)
    lam = float(fastemit_lambda)
    out = np.full((B, Tmax, U1max), PADDED, np.int8)
    need_b = np.zeros((B, Tmax, U1max), bool)
    need_l = np.zeros((B, Tmax, U1max), bool)
    for b, lat in enumerate(lattices):
        T, U = int(llens[b]), int(tlens[b])
        if lat is None:
            continue
        alpha, beta, cost, emit = lat["alpha"], lat["beta"], lat["cost"], lat["emit"]
        pen = rnnt_lattice_ref.penalty_f64(delay_penalty, T) if delay_penalty > 0 else np.zeros(T)
        for t in range(T):
            for u in range(U + 1):
                final = t == T - 1 and u == U
                has_b1 = t < T - 1
                blank_special = final or has_b1
                lab = int(targets[b][u]) if u < U else -1
                has_lab = u < U and not (lab == blank and blank_special)
                ac = alpha[t, u] + cost
                be_eff = beta[t, u]
                if has_lab and lam > 0:
                    be_eff = np.logaddexp(be_eff, math.log(lam) + emit[t, u] + beta[t, u + 1])
                main_dead = ac + be_eff < thr
                blank_dead = (not blank_special) or (ac + beta[t + 1, u] if has_b1 else ac) < thr
                label_dead = (not has_lab) or ac + beta[t, u + 1] + pen[t] + math.log1p(lam) < thr
                if not main_dead:
                    out[b, t, u] = LIVE
                elif blank_dead and label_dead:
                    out[b, t, u] = DEAD
                else:
                    out[b, t, u] = FAINT
                    need_b[b, t, u] = not blank_dead
                    need_l[b, t, u] = not label_dead
    return out, need_b, need_l
