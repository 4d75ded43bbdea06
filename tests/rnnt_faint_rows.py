"""Host restatement of the three-way row classification of rnnt_grad_kernel (wenet-celoss_amd/csrc/rnnt_loss.hip).

A valid cell (t, u) of utterance b has three bounds on the exponents of its gradient (rnnt_dead_rows.py):
    main   alpha + beta + cost
    blank  alpha + cost + beta(t+1, u)    (t < T-1; alpha + cost at the final cell)
    label  alpha + cost + beta(t, u+1)    (u < U, unless the label is the blank of a blank-term cell)
With `denom` finite and below 2^16 in magnitude:
    DEAD   every bound that applies is below DEAD_THR: the row is finish(0), nothing is read;
    FAINT  the main bound is below DEAD_THR, the blank or the label bound is not: the row is finish(0) except its blank /
           label element, only those (at most two) logits are read;
    LIVE   otherwise: the row is streamed.
A NaN anywhere makes the part it enters "not below".  Plain helper module (not a conftest): tests import it.

DEAD_THR restates kDeadThr: (X0 - 8.6) / log2(e) rounded toward -inf to one decimal, where X0 is the largest float such
that __builtin_amdgcn_exp2f gives +0 for it and for every float below it (measured on gfx950 by
tests/test_rnnt_faint_rows_gpu.py::test_exp2_cutoff: v_exp_f32 flushes denormal results) and 8.6 log2 units is the
margin the kernel's rounding analysis keeps.
"""
import math

import numpy as np

from rnnt_dead_rows import DENOM_MAX

X0 = -126.00000762939453             # 0xC2FC0001, the float just below -126
MARGIN_LOG2 = 8.6
LOG2E = 1.4426950408889634
DEAD_THR = -93.3
CUTOFF = 2.0 ** -126                 # what a non-zero result of the instruction is at least

LIVE, FAINT, DEAD, PADDED = 0, 1, 2, -1


def thr_from_cutoff(x0=X0):
    """(x0 - 8.6) / log2(e), rounded toward -inf to one decimal."""
    return math.floor((x0 - MARGIN_LOG2) / LOG2E * 10.0) / 10.0


def classify(alpha, beta, cost, targets, llens, tlens, blank=0, denom=None, thr=DEAD_THR):
    """int8 [B,T,U+1] of LIVE / FAINT / DEAD (PADDED outside the lattice), float64 arithmetic; denom=None skips the denom
    test, for callers that only have the exported lattice.  Also returns the boolean masks (needs_blank, needs_label)
    of the faint rows' elements that are read."""
    alpha = np.asarray(alpha, np.float64)
    beta = np.asarray(beta, np.float64)
    B, T, U1 = alpha.shape
    t = np.arange(T)[:, None]
    u = np.arange(U1)[None, :]
    out = np.full((B, T, U1), PADDED, np.int8)
    need_b = np.zeros((B, T, U1), bool)
    need_l = np.zeros((B, T, U1), bool)
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
            main_dead = ac + beta[b] < thr
            if denom is not None:
                main_dead &= np.abs(np.asarray(denom[b], np.float64)) < DENOM_MAX
            blank_dead = ~blank_special | (np.where(has_b1, ac + b1, ac) < thr)
            label_dead = ~has_lab | (ac + b2 < thr)
            cls = np.where(main_dead, np.where(blank_dead & label_dead, DEAD, FAINT), LIVE)
            out[b] = np.where(valid, cls, PADDED)
            need_b[b] = valid & main_dead & ~blank_dead
            need_l[b] = valid & main_dead & ~label_dead
    return out, need_b, need_l


def share(cls, kind, llens, tlens):
    """Cells of `kind` over valid cells."""
    valid = sum(int(a) * (int(c) + 1) for a, c in zip(llens, tlens))
    return float((cls == kind).sum()) / max(valid, 1)
