"""The float64 TDT prefix beam reference (tests/tdt_beam_ref.py) on scripted joiner rows with hand-worked answers, against
the numpy oracle of the plain prefix beam search for durations = (1,), and the case generator of tests/test_tdt_beam_gpu.py
with the condition every GPU case has to meet in float64 before a GPU is involved.  No GPU."""
import functools
import math
from collections import namedtuple

import numpy as np
import pytest
import torch

import tdt_beam_ref as ref
from oracle import decode_oracle as do


def row(p_tok, p_dur):
    """Logits that ARE log-probabilities: each part sums to one, so both log-softmaxes return them."""
    assert abs(sum(p_tok) - 1) < 1e-12 and abs(sum(p_dur) - 1) < 1e-12
    return np.log(np.array(list(p_tok) + list(p_dur), dtype=np.float64))


def approx(beam, want):
    """[(tokens, t, probability)] against the beam; scores carry one fp32 rounding per arc."""
    assert [(h, t) for h, t, _ in beam] == [(h, t) for h, t, _ in want]
    np.testing.assert_allclose([s for _, _, s in beam], [math.log(p) for _, _, p in want], rtol=0, atol=2e-6)


# --------------------------------------------------------------------------------------------- hand-worked cases --
def test_waiting_entry_survives_untouched_and_clamping_fuses_finished_entries():
    # V = 2 (blank 0, label 1), durations (1, 2), beam 2, T = 3.
    # step 0, f = 0: tokens (.9, .1), durations (.6, .4): pairs blank/1 .54, blank/2 .36, label/1 .06, label/2 .04
    #   -> ((0), t1, .54), ((0), t2, .36): equal tokens at different frames are two classes.
    # step 1, f = 1: ((0), t2) waits.  ((0), t1): tokens (.2, .8), durations (.3, .7): label/2 .56, label/1 .24, blank/2
    #   .14, blank/1 .06 -> ((0,1), t3, .54 * .56 = .3024), ((0,1), t2, .54 * .24 = .1296).  Pool: .3024, .1296, the waiting
    #   .36; nothing fuses; sorted .36, .3024 | .1296 pruned.  The waiting entry is the step-0 tuple itself.
    # step 2, f = 2: ((0,1), t3) is finished and waits.  ((0), t2): tokens (.9, .1), durations (.6, .4): blank/1 .54 ->
    #   t3, blank/2 .36 -> t4 clamped to T = 3: the same class, .36 * (.54 + .36) = .324.  Sorted .324, .3024.
    table = {(0, (0,)): row((.9, .1), (.6, .4)), (1, (0,)): row((.2, .8), (.3, .7)), (2, (0,)): row((.9, .1), (.6, .4))}
    trace = []
    got = ref.search(ref.Scripted(table), 3, 2, (1, 2), 2, trace=trace)
    approx(trace[0], [((0,), 1, .54), ((0,), 2, .36)])
    approx(trace[1], [((0,), 2, .36), ((0, 1), 3, .3024)])
    assert trace[1][0] == trace[0][1]                       # bit for bit
    approx(got.beam, [((0,), 3, .324), ((0, 1), 3, .3024)])
    assert (got.steps, got.expanded) == (3, 3)
    # the smallest gap: step 2's classes, log .324 - log .3024
    np.testing.assert_allclose(got.margin, math.log(.324 / .3024), rtol=1e-5)


def test_blank_jump_fuses_with_a_waiting_entry():
    # as above up to step 1, where ((0), t1) sees tokens (.9, .1), durations (.2, .8): blank/2 .72 -> ((0), t3, .54 * .72 =
    #   .3888), blank/1 .18 -> ((0), t2, .0972), which meets the waiting ((0), t2, .36): one lattice state, .4572, in the
    #   expansion's place of the pool.  Sorted ((0), t2, .4572), ((0), t3, .3888).
    # step 2, f = 2: tokens (.9, .1), durations (.6, .4): both blank arcs end at T = 3 and meet the finished ((0), t3):
    #   .4572 * .54 + .4572 * .36 + .3888 = .80028, one entry.
    table = {(0, (0,)): row((.9, .1), (.6, .4)), (1, (0,)): row((.9, .1), (.2, .8)), (2, (0,)): row((.9, .1), (.6, .4))}
    trace = []
    got = ref.search(ref.Scripted(table), 3, 2, (1, 2), 2, trace=trace)
    approx(trace[1], [((0,), 2, .4572), ((0,), 3, .3888)])
    approx(got.beam, [((0,), 3, .80028)])


def test_label_arcs_of_duration_0_and_1_fuse_and_T_1():
    # durations (0, 1), T = 1, beam 2: tokens (.3, .7), durations (.4, .6): label/1 .42, label/0 .28, blank/1 .18, blank/0
    #   .12.  The label's d = 0 arc advances one frame like its d = 1 arc: one class, .7.
    got = ref.search(ref.Scripted({(0, (0,)): row((.3, .7), (.4, .6))}), 1, 2, (0, 1), 2)
    approx(got.beam, [((0, 1), 1, .7)])
    assert got.steps == 1
    # T = 0: nothing is consulted
    assert ref.search(ref.Scripted({}), 0, 2, (0, 1), 2).beam == [((0,), 0, 0.0)]


def test_stable_order_on_an_exact_tie():
    # durations (1,): ld = 0.  tokens (.4, .4, .2), beam 2: the tie of columns 0 and 1 goes to the lower index, and the two
    #   classes with equal scores keep the pool's order.
    got = ref.search(ref.Scripted({(0, (0,)): row((.4, .4, .2), (1.0,))}), 1, 3, (1,), 2)
    approx(got.beam, [((0,), 1, .4), ((0, 1), 1, .4)])
    assert got.beam[0][2] == got.beam[1][2]
    got = ref.search(ref.Scripted({(0, (0,)): row((.2, .4, .4), (1.0,))}), 1, 3, (1,), 2)
    approx(got.beam, [((0, 1), 1, .4), ((0, 2), 1, .4)])
    # a pair tie: tokens (.5, .5), durations (.5, .5), beam 3 of the 4 equal pairs: rank 0 with j = 0, 1, then rank 1, j = 0
    #   (T = 2, so that t' = 1 and t' = 2 stay apart; the rows of frame 1 only let the search end)
    tie = row((.5, .5), (.5, .5))
    trace = []
    ref.search(ref.Scripted({(0, (0,)): tie, (1, (0,)): tie, (1, (0, 1)): tie}), 2, 2, (1, 2), 3, trace=trace)
    approx(trace[0], [((0,), 1, .25), ((0,), 2, .25), ((0, 1), 1, .25)])


# ---------------------------------------------------------- durations = (1,): the plain prefix beam search --
class OracleRows:
    """Rows of the numpy oracle's predictor and joiner (fp32), per token sequence."""

    def __init__(self, pred, joint, enc):
        self.pred, self.joint, self.enc, self.memo = pred, joint, enc, {}

    def _step(self, toks):
        if toks not in self.memo:
            cache = self.pred.init_state(1) if len(toks) == 1 else self._step(toks[:-1])[1]
            self.memo[toks] = self.pred.forward_step(np.array([toks[-1]]), np.zeros((1, 1), np.float32), cache)
        return self.memo[toks]

    def row(self, t, toks):
        return self.joint(self.enc[t][None], self._step(toks)[0]).reshape(-1)


@pytest.mark.parametrize("ctc_weight, transducer_weight", [(0.0, 1.0), (0.3, 0.7)], ids=["transducer", "mixture"])
def test_durations_1_is_the_plain_prefix_beam_search(ctc_weight, transducer_weight):
    rng = np.random.default_rng(7)
    V, E, P, J, H, L, T, beam = 12, 6, 6, 8, 7, 2, 14, 4
    f = lambda *s: rng.normal(size=s).astype(np.float32)      # noqa: E731
    pw = {"embed.weight": f(V, P), "projection.weight": f(P, H), "projection.bias": f(P)}
    for l in range(L):
        pw.update({f"rnn.weight_ih_l{l}": f(4 * H, P if l == 0 else H), f"rnn.weight_hh_l{l}": f(4 * H, H),
                   f"rnn.bias_ih_l{l}": f(4 * H), f"rnn.bias_hh_l{l}": f(4 * H)})
    jw = {"enc_ffn.weight": f(J, E), "enc_ffn.bias": f(J), "pred_ffn.weight": f(J, P), "pred_ffn.bias": f(J),
          "ffn_out.weight": 2 * f(V + 1, J), "ffn_out.bias": f(V + 1)}
    jw["ffn_out.bias"][0] += 3.0
    cw = {"ctc_lo.weight": f(V, E), "ctc_lo.bias": f(V)}
    enc = f(T, E)
    pred = do.Predictor(pw, L)
    plain = do.Joint({**jw, "ffn_out.weight": jw["ffn_out.weight"][:V], "ffn_out.bias": jw["ffn_out.bias"][:V]})
    want, margin = do.prefix_beam_search(pred, plain, cw, enc, T, beam_size=beam, ctc_weight=ctc_weight,
                                         transducer_weight=transducer_weight, return_margin=True)
    got = ref.search(OracleRows(pred, do.Joint(jw), enc), T, V, (1,), beam, ctc_logp=do.ctc_log_softmax(cw, enc),
                     ctc_weight=ctc_weight, transducer_weight=transducer_weight)
    print("margins", margin, got.margin)
    assert margin > 1e-4 and got.margin > 1e-4
    assert got.steps == T                                   # every entry is expanded at every frame
    assert [list(h) for h, _, _ in got.beam] == [s["hyp"] for s in want]
    assert all(t == T for _, t, _ in got.beam)
    np.testing.assert_allclose([s for _, _, s in got.beam], [s["score"] for s in want], rtol=1e-5)


# ------------------------------------------------------------------- the cases of tests/test_tdt_beam_gpu.py --
E, P, J, H, L = 16, 16, 32, 32, 2
LENS = (40, 33, 17, 7, 1)          # ragged; 33 and 40 cross the 16-step replay boundary twice
MARGIN = 1e-4                      # the convention of tests/test_decode_gpu.py: compared where the reference is this clear
MIN_QUALIFY = 4
CTC_MIX = (0.3, 0.7)

Spec = namedtuple("Spec", "name kind width durations beam ctc blank seed")
Case = namedtuple("Case", "spec pred joint enc lens V ctc_logp weights")

# every seed was chosen on the CPU so that the float64 reference alone meets `case_conditions`
SPECS = (
    Spec("beam1", "lstm", 305, (1, 2, 4), 1, False, 0, 0),
    Spec("beam3", "lstm", 305, (0, 1, 2, 3, 4), 3, False, 0, 0),
    Spec("beam8-ctc", "lstm", 305, (0, 1, 2, 3, 4), 8, True, 0, 0),
    Spec("beam16-124", "lstm", 305, (1, 2, 4), 16, False, 0, 3),
    Spec("beam3-08-ctc-blank2", "lstm", 305, (0, 8), 3, True, 2, 0),
    Spec("width2054", "lstm", 2054, (0, 1, 2, 3, 4), 8, False, 0, 2),
    Spec("width5130-ctc", "lstm", 5130, (0, 1, 2, 3, 4), 8, True, 0, 0),
    Spec("embedding", "embedding", 305, (1, 2, 4), 3, False, 0, 0),
    Spec("conv-blank5", "conv", 305, (0, 1, 2, 3, 4), 3, False, 5, 0),
    Spec("dur1-ctc", "lstm", 301, (1,), 8, True, 0, 1),
    # beam 16 (beam^2 = 256 candidates: the all-pairs steps of the update kernels take more than one pass) over 40 tokens,
    # where equal prefixes meet at every frame; the durations-(1,) cases are also run through the plain search
    # (the list's shape, five utterances of up to 40 frames, is kept: MIN_QUALIFY asks for four utterances with a clear
    # margin, and a case still runs in under 3 s on the device)
    Spec("dur1-beam16-ctc", "lstm", 41, (1,), 16, True, 0, 2),
    Spec("dur1-beam16-embedding-ctc", "embedding", 41, (1,), 16, True, 0, 4),
    Spec("beam16-embedding", "embedding", 43, (0, 1, 2), 16, True, 0, 5),
)
DUR1_SPECS = tuple(s for s in SPECS if s.durations == (1,))
TIE_SPEC = Spec("ties", "lstm", 305, (0, 1, 2, 3, 4), 3, False, 0, 1)
SPEC = {s.name: s for s in SPECS}


def modules(seed, kind, width, V, blank):
    import wenet_celoss_amd as w
    torch.manual_seed(seed)
    if kind == "lstm":
        pred = w.RNNPredictor(V, P, P, 0.0, H, L, dropout=0.0)
    elif kind == "embedding":
        pred = w.EmbeddingPredictor(V, P, 0.0, n_head=2, history_size=2)
    else:
        pred = w.ConvPredictor(V, P, 0.0, history_size=2)
    joint = w.TransducerJoint(width, E, P, J)
    ctc = w.CTC(V, E)
    with torch.no_grad():                        # spread the logits (clear margins) and favour blank
        joint.ffn_out.weight *= 10
        joint.ffn_out.bias[blank] += 13
        ctc.ctc_lo.weight *= 10
        ctc.ctc_lo.bias[blank] += 13
    return pred.eval(), joint.eval(), ctc.eval()


@functools.lru_cache(maxsize=None)
def make_case(spec):
    V = spec.width - len(spec.durations)
    pred, joint, ctc = modules(spec.seed, spec.kind, spec.width, V, spec.blank)
    enc = torch.randn(len(LENS), max(LENS), E, generator=torch.Generator().manual_seed(spec.seed + 1000))
    with torch.no_grad():
        ctc_logp = ctc.log_softmax(enc) if spec.ctc else None       # fp32: the posterior the device is handed
    return Case(spec, pred, joint, enc, list(LENS), V, ctc_logp, CTC_MIX if spec.ctc else (0.0, 1.0))


@functools.lru_cache(maxsize=None)
def reference(spec):
    """The float64 beams of a case, computed once per process and shared."""
    c = make_case(spec)
    return ref.decode(c.pred, c.joint, c.enc, c.lens, c.V, spec.durations, spec.beam, spec.blank,
                      None if c.ctc_logp is None else c.ctc_logp.numpy(), *c.weights)


def case_conditions(spec, want):
    """What the reference of a GPU case has to show; a list of the conditions that fail."""
    bad = []
    if sum(r.margin > MARGIN for r in want) < MIN_QUALIFY:
        bad.append(f"fewer than {MIN_QUALIFY} utterances with a margin above {MARGIN}: {[r.margin for r in want]}")
    if not any(len(h) > 1 for r in want for h, _, _ in r.beam):
        bad.append("no label in any hypothesis")
    if spec.beam == 16 and not all(r.fused for r, n in zip(want, LENS) if n > 1):
        bad.append(f"an utterance without a fused duplicate at beam 16: {[r.fused for r in want]}")
    if spec.beam > 1 and not any(r.expanded < r.steps * min(spec.beam, len(r.beam)) for r in want):
        bad.append("no hypothesis ever waited")
    jumps = max(spec.durations) > 1
    if any(r.steps > n for r, n in zip(want, LENS)) or jumps != any(r.steps < n for r, n in zip(want, LENS)):
        bad.append("steps against T")
    return bad


@functools.lru_cache(maxsize=None)
def tie_case():
    """TIE_SPEC's model with the ffn_out row of the label its n-best name most often copied into the last token row, and
    the row of duration 0 copied into that of duration 1 -> (case, {copy: original column}, joiner, float64 beams).  The
    two token columns tie wherever they meet and the lower index goes first; a label's (and a blank's) d = 0 and d = 1
    arcs have equal values, end at the same frame and fuse: log_add of two equal scores."""
    import copy
    from collections import Counter
    c = make_case(TIE_SPEC)
    plain = reference(TIE_SPEC)
    label = [k for k, _ in Counter(k for r in plain for h, _, _ in r.beam for k in h[1:]).most_common() if k < c.V - 1][0]
    dup = {c.V - 1: label, c.V + 1: c.V}
    joint = copy.deepcopy(c.joint)
    with torch.no_grad():
        for hi, lo in dup.items():
            joint.ffn_out.weight[hi] = joint.ffn_out.weight[lo]
            joint.ffn_out.bias[hi] = joint.ffn_out.bias[lo]
    want = ref.decode(c.pred, joint, c.enc, c.lens, c.V, TIE_SPEC.durations, TIE_SPEC.beam, TIE_SPEC.blank, dup=dup)
    return c, dup, joint, want


def tie_conditions(want):
    c, dup, _, _ = tie_case()
    label = dup[c.V - 1]
    bad = []
    if sum(r.margin > MARGIN for r in want) < MIN_QUALIFY:
        bad.append(f"margins {[r.margin for r in want]}")
    tokens = [k for r in want for h, _, _ in r.beam for k in h[1:]]
    if label not in tokens or c.V - 1 not in tokens:
        bad.append("both tied tokens in the n-best")
    for r in want:                     # wherever both follow the same prefix, the lower index stands first
        hyps = [h for h, _, _ in r.beam]
        for i, h in enumerate(hyps):
            if h[-1] == c.V - 1 and h[:-1] + (label,) in hyps and hyps.index(h[:-1] + (label,)) > i:
                bad.append(f"order {hyps}")
    return bad


@pytest.mark.parametrize("spec", SPECS, ids=[s.name for s in SPECS])
def test_gpu_case_qualifies_in_float64(spec):
    want = reference(spec)
    print(spec.name, "margins", [r.margin for r in want], "steps", [r.steps for r in want], "expanded",
          [r.expanded for r in want], "best", [r.beam[0][0] for r in want])
    assert case_conditions(spec, want) == []
    for r, n in zip(want, LENS):
        assert all(t == n and h[0] == spec.blank for h, t, _ in r.beam)
        assert [s for _, _, s in r.beam] == sorted((s for _, _, s in r.beam), reverse=True)
        assert len(r.beam) <= spec.beam


def test_tie_case_qualifies_in_float64():
    c, dup, joint, want = tie_case()
    print("dup", dup, "margins", [r.margin for r in want], "n-best", [[h for h, _, _ in r.beam] for r in want])
    assert tie_conditions(want) == []
    # T = 1: the seed's blank arcs of d = 0 and d = 1 have equal values and both end at frame 1 (with every other arc of
    # that utterance, which is clamped there)
    assert all(t == 1 for _, t, _ in want[-1].beam)
