"""Guided float64 walk of a transducer search, frame by frame, along the trajectory the search itself took.

Plain module (not a conftest): the CPU self-tests in test_decode_follow_ref.py and the GPU tests in
test_decode_follow_gpu.py import it.

The state of both searches at a frame boundary is a function of what they export (oracle/decode_oracle.py, "float64
single steps"), so decoding an utterance truncated to f frames gives the search's own state after frame f.  Given those
states for every f, each frame is checked on its own: a float64 step starts from the search's state at f and must reach
its state at f + 1.  Where a near-tie let an fp32 implementation decide either way, the walk accepts the search's
choice and goes on from its state, so it never stops early; a near-tie is a pair of values whose float64 difference is
within the sum of their fp32 bounds (oracle/decode_oracle.py: gamma(K) contractions, log-softmax / mixture propagation,
one ulp per fp32 add), a bound derived from the arithmetic and not fitted to a run.  The checks report frames walked,
near-ties followed and the largest observed |error| / bound.

Beam frame f -> f + 1 (prefix_beam_search.py:77-146):
  * every survivor at f + 1 is a fused candidate of the float64 step from the survivors at f;
  * a parent's top-`beam` may differ from the float64 one only among tokens whose values lie within their bounds of
    the rank-`beam` boundary; a survivor's score then lies (within its bound) between the fusion of the certain
    members of its class and that of every possible one;
  * the survivors are the float64 top-n classes, except swaps with classes whose scores are within their bounds;
  * each survivor's score is within its class's bound of the float64 fused score, and the survivors are best first.
Greedy frame f ('greedy_search copy.py':27-58): every decision of the frame is the float64 argmax or within the bounds
of it, a frame ends at a blank or after `n_steps` emissions.
"""
from __future__ import annotations

import numpy as np

from oracle import decode_oracle as do

MAX_TIE_FRACTION = 0.05        # followed near-ties per walked frame: a bound too wide to see a systematic error trips it


class WalkError(AssertionError):
    pass


class Stats:
    def __init__(self, name):
        self.name, self.frames, self.ties, self.worst, self.where = name, 0, 0, 0.0, None

    def ratio(self, err, bound, where):
        r = float(err) / float(bound)
        if r > self.worst:
            self.worst, self.where = r, where

    def merge(self, other: "Stats"):
        self.frames += other.frames
        self.ties += other.ties
        if other.worst > self.worst:
            self.worst, self.where = other.worst, other.where

    def report(self, total=None):
        tot = f" / {total}" if total is not None else ""
        return (f"{self.name}: frames walked {self.frames}{tot}, near-ties followed {self.ties}, "
                f"worst |error| / bound {self.worst:.3g} at {self.where}")

    def check_ties(self):
        if self.ties > MAX_TIE_FRACTION * max(self.frames, 1):
            raise WalkError(f"{self.report()}: more than {MAX_TIE_FRACTION:.0%} of the frames needed a near-tie")


# ---------------------------------------------------------------------------------------------------- beam --
def _maybe_members(mix, err, beam_size):
    """Tokens of one parent's row whose top-`beam_size` membership an fp32 evaluation may decide either way: those
    whose value lies within the bounds of the rank-`beam_size` boundary (empty when the boundary is clear)."""
    order = do.topk_order(mix, beam_size + 64)
    if order.size <= beam_size:
        return set()
    inside, outside = order[:beam_size], order[beam_size:]
    lo_in = float(np.min(mix[inside] - err[inside]))
    hi_out = float(np.max(mix[outside] + err[outside]))
    if lo_in > hi_out:
        return set()
    if order.size < mix.size and mix[order[-1]] + err[order[-1]] >= lo_in:
        raise WalkError(f"more than 64 tokens within the bounds of a rank-{beam_size} boundary")
    return {int(v) for v in order if mix[v] + err[v] >= lo_in and mix[v] - err[v] <= hi_out}


def _check_beam_frame(fused, nxt, beam_size, where, st: Stats):
    """Survivors `nxt` [(hyp, score)] against the fused float64 classes -> (reason for rejecting or None, whether a
    near-tie was followed: a top-k membership or a pruned class other than the float64 one)."""
    top = [c for c in fused if c["first"] is not None]
    n_lo = min(beam_size, sum(c["lo"] > -np.inf for c in fused))
    n_hi = min(beam_size, len(fused))
    if not n_lo <= len(nxt) <= n_hi:
        return f"{len(nxt)} survivors, float64 step keeps {min(beam_size, len(top))}", False
    by_hyp = {c["hyp"]: c for c in fused}
    sel, ratios, tie = set(), [], False
    for e, (hyp, score) in enumerate(nxt):
        c = by_hyp.get(tuple(hyp))
        if c is None:
            return f"survivor {e} {tuple(hyp)[-4:]} (len {len(hyp)}) is not a candidate of the float64 step", False
        if c["hyp"] in sel:
            return f"survivor {e} repeats a hypothesis", False
        sel.add(c["hyp"])
        d = abs(score - c["score"])
        if d <= c["err"]:
            ratios.append((d, c["err"], where + (e,)))
        elif c["lo"] - c["err"] <= score <= c["hi"] + c["err"]:
            tie = True                                   # a possible member of a top-k made the difference
        else:
            return (f"survivor {e} (len {len(hyp)}): score {score!r}, float64 {c['score']!r} (possible members: "
                    f"{c['lo']!r} .. {c['hi']!r}), |diff| {d:.3g} > bound {c['err']:.3g}"), False
        if e and score > nxt[e - 1][1]:
            return f"survivors not best first at {e}: {nxt[e - 1][1]!r} < {score!r}", False
    lo_sel = min((c["hi"] + c["err"] for c in fused if c["hyp"] in sel), default=np.inf)
    hi_out = max((c["lo"] - c["err"] for c in fused if c["hyp"] not in sel), default=-np.inf)
    if lo_sel < hi_out:
        return f"pruned a class clearly better than a survivor: {lo_sel!r} < {hi_out!r}", False
    for d, b, w in ratios:
        st.ratio(d, b, w)
    return None, tie or sel != {c["hyp"] for c in top[:len(nxt)]}


def walk_beam(trie, joint, ctc_lp, ctc_err, enc, states, beam_size, tw, cw, blank=0, name="beam", frame0=0):
    """states[f] = the search's beam after f frames, [(hyp incl. the seed blank, score)] best first, for f = frame0 ..
    frame0 + len(states) - 1 (states[0] == [((blank,), 0.0)] when frame0 == 0).  Checks every transition; raises
    WalkError with frame, survivor, expected and observed values at the first one no fp32 rounding explains."""
    st = Stats(name)
    for q in range(len(states) - 1):
        f = frame0 + q
        cur, nxt = states[q], states[q + 1]
        hyps = [tuple(h) for h, _ in cur]
        mix, err = do.prefix_beam_rows_f64(trie, joint, enc[f], ctc_lp[f], ctc_err[f], hyps, tw, cw)
        maybe = [_maybe_members(mix[j], err[j], beam_size) for j in range(len(cur))]
        fused, _ = do.prefix_beam_step_f64([(h, s) for h, s in cur], mix, err, beam_size, blank, maybe)
        reason, tie = _check_beam_frame(fused, nxt, beam_size, (name, f), st)
        if reason is not None:
            n_maybe = sum(len(m) for m in maybe)
            raise WalkError(f"{name} frame {f} ({len(cur)} parents, {n_maybe} tokens near a top-k boundary): {reason}")
        st.ties += int(tie)
        st.frames += 1
    return st


# -------------------------------------------------------------------------------------------------- greedy --
def walk_greedy(trie, joint, enc, token_states, n_steps, blank=0, name="greedy", frame0=0):
    """token_states[f] = the stream's tokens after f frames (f = frame0 .. frame0 + len - 1).  Every decision of every
    frame is checked against the float64 log-probs of the same state."""
    st = Stats(name)
    for q in range(len(token_states) - 1):
        f = frame0 + q
        cur, nxt = list(token_states[q]), list(token_states[q + 1])
        if nxt[:len(cur)] != cur:
            raise WalkError(f"{name} frame {f}: tokens after frame {f + 1} do not extend those after frame {f}")
        em = nxt[len(cur):]
        if len(em) > n_steps:
            raise WalkError(f"{name} frame {f}: {len(em)} emissions, n_steps = {n_steps}")
        rows = do.greedy_frame_f64(trie, joint, enc[f], cur, em, blank)
        want = em + ([blank] if len(em) < n_steps else [])
        for i, k in enumerate(want):
            lp, err = rows[i]
            best = int(lp.argmax())
            if k == best:
                continue
            d = lp[best] - lp[k]
            b = err[best] + err[k]
            if not d <= b:
                raise WalkError(f"{name} frame {f} decision {i}: took {k} (log-prob {lp[k]!r}), float64 argmax {best} "
                                f"({lp[best]!r}), gap {d:.3g} > bound {b:.3g}")
            st.ratio(d, b, (name, f, i))
            st.ties += 1
        st.frames += 1
    return st
