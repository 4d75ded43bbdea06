"""The float64 reference of the streaming transducer prefix beam search (tests/beam_stream_ref.py) on scripted joiner rows
with hand-worked answers, its invariance under chunking, its agreement with tests/tdt_beam_ref.py, and the cases of
tests/test_beam_stream_gpu.py with the condition each has to meet in float64 before a GPU is involved.  No GPU."""
import functools
import itertools
import math

import numpy as np
import pytest

import beam_stream_ref as ref
import tdt_beam_ref
import test_tdt_beam_ref as cases
from test_tdt_beam_ref import LENS, MARGIN, MIN_QUALIFY, SPEC, row


def prow(*p_tok):
    """A plain model's row: token logits that are log-probabilities."""
    assert abs(sum(p_tok) - 1) < 1e-12
    return np.log(np.array(p_tok, dtype=np.float64))


def approx(beam, want):
    """[(tokens, t, probability, Viterbi probability, times)] against the beam; scores carry one fp32 rounding per arc."""
    assert [(h, t, tm) for h, t, _, _, tm in beam] == [(h, t, tm) for h, t, _, _, tm in want]
    np.testing.assert_allclose([s for _, _, s, _, _ in beam], [math.log(p) for _, _, p, _, _ in want], rtol=0, atol=2e-6)
    np.testing.assert_allclose([v for _, _, _, v, _ in beam], [math.log(p) for _, _, _, p, _ in want], rtol=0, atol=2e-6)


# --------------------------------------------------------------------------------------------- hand-worked cases --
def test_times_come_from_the_viterbi_best_member_not_from_the_representative():
    # plain model, V = 2 (blank 0, label 1), beam 2, T = 2.
    # frame 0: (.6, .4) -> ((0), .6, times ()), ((0,1), .4, times (0,)): the label records the frame it was emitted at.
    # frame 1, pool in beam order: (0) sees (.55, .45): blank -> (0) .33; label -> (0,1) .27 with times (1,) -- the first
    #   (0,1) of the pool, the representative.  (0,1) sees (.9, .1): blank -> (0,1) .36 with times (0,); label -> (0,1,1) .04.
    #   Class (0,1): score .27 + .36 = .63; Viterbi max(.27, .36) = .36, held by the second member: times (0,).
    #   Sorted .63, .33 | .04 pruned.
    table = {(0, (0,)): prow(.6, .4), (1, (0,)): prow(.55, .45), (1, (0, 1)): prow(.9, .1)}
    trace = []
    got = ref.search(ref.Scripted(table), [2], 2, None, 2, trace=trace)
    approx(trace[1], [((0,), 1, .6, .6, ()), ((0, 1), 1, .4, .4, (0,))])
    approx(got.beam, [((0, 1), 2, .63, .36, (0,)), ((0,), 2, .33, .33, ())])
    # the new gap: log .36 - log .27 between the members' Viterbi scores; smaller than every score gap here
    np.testing.assert_allclose(got.margin, math.log(.36 / .27), rtol=1e-5)
    # the other way round the representative keeps its own times: (0,1) sees (.5, .5) -> blank .2 < .27
    table[(1, (0, 1))] = prow(.5, .5)
    got = ref.search(ref.Scripted(table), [2], 2, None, 2)
    approx(got.beam, [((0, 1), 2, .47, .27, (1,)), ((0,), 2, .33, .33, ())])


def test_an_exact_viterbi_tie_goes_to_the_first_member_in_pool_order():
    # every row (.5, .5): frame 0 -> ((0), .5), ((0,1), .5, times (0,)), in that order (equal scores keep the pool's order).
    # frame 1: (0) -> (0) .25, (0,1) .25 with times (1,); (0,1) -> (0,1) .25 with times (0,), (0,1,1) .25.  The two members of
    #   class (0,1) have the same Viterbi score bit for bit (the same two fp32 adds): the first in pool order keeps its times.
    tie = prow(.5, .5)
    got = ref.search(ref.Scripted({(0, (0,)): tie, (1, (0,)): tie, (1, (0, 1)): tie}), [2], 2, None, 2)
    approx(got.beam, [((0, 1), 2, .5, .25, (1,)), ((0,), 2, .25, .25, ())])
    assert got.beam[0][3] == got.beam[1][3]


def test_a_label_records_the_frame_it_was_emitted_at_not_the_frame_its_arc_ends_at():
    # durations (1, 3), beam 1, T = 4: frame 0: tokens (.1, .9), durations (.2, .8): label / 3 -> ((0,1), t' = 3, times (0,));
    # frame 3: tokens (.3, .7), durations (.9, .1): label / 1 -> ((0,1,1), t' = 4, times (0, 3)).
    table = {(0, (0,)): row((.1, .9), (.2, .8)), (3, (0, 1)): row((.3, .7), (.9, .1))}
    got = ref.search(ref.Scripted(table), [4], 2, (1, 3), 1)
    approx(got.beam, [((0, 1, 1), 4, .72 * .63, .72 * .63, (0, 3))])
    assert got.steps == 2


JUMP = {(0, (0,)): row((.9, .1), (.2, .8)), (1, (0,)): row((.7, .3), (.6, .4)), (2, (0,)): row((.9, .1), (.7, .3)),
        (3, (0,)): row((.2, .8), (.9, .1))}


def test_a_jump_across_a_chunk_boundary_waits():
    # V = 2, durations (1, 3), beam 2, chunks of 2 + 2 frames.
    # chunk 1 (F = 2, not final: nothing is clamped).
    #   f = 0: tokens (.9, .1), durations (.2, .8): blank/3 .72 -> ((0), t3), blank/1 .18 -> ((0), t1) | label/3 .08 pruned.
    #   f = 1: ((0), t3) waits.  ((0), t1): tokens (.7, .3), durations (.6, .4): blank/1 .42 -> t2, .18 * .42 = .0756;
    #     blank/3 .28 -> t4 (beyond F, kept as it is), .0504.  Pool .72, .0756, .0504: the last is pruned.
    #   Every entry has t >= 2: the chunk ends with ((0), t3, .72) waiting across the boundary.
    # chunk 2 (F = T = 4, final): nothing to clamp; fuse and sort change nothing.
    #   f = 2: ((0), t2): tokens (.9, .1), durations (.7, .3): blank/1 .63 -> t3, .0756 * .63 = .047628, which meets the waiting
    #     ((0), t3, .72) -- first in pool order, the representative: .767628, Viterbi max(.72, .047628) = .72; blank/3 .27 -> t5
    #     clamped to 4, .020412.
    #   f = 3: ((0), t3): tokens (.2, .8), durations (.9, .1): label/1 .72 -> ((0,1), t4, times (3,)), .767628 * .72, Viterbi
    #     .72 * .72; blank/1 .18 -> ((0), t4), .767628 * .18 = .13817304, Viterbi .1296, the representative of the class the
    #     waiting ((0), t4, .020412) joins: .15858504.
    trace = []
    got = ref.search(ref.Scripted(JUMP), [2, 2], 2, (1, 3), 2, trace=trace)
    approx(got.after[0], [((0,), 3, .72, .72, ()), ((0,), 2, .0756, .0756, ())])
    assert got.after[0][0] == trace[0][0]                    # the waiting entry is the step-0 tuple itself
    assert trace[2] == got.after[0]                          # the final chunk's begin changes nothing here
    approx(trace[3], [((0,), 3, .767628, .72, ()), ((0,), 4, .020412, .020412, ())])
    approx(got.beam, [((0, 1), 4, .767628 * .72, .5184, (3,)), ((0,), 4, .15858504, .1296, ())])
    assert got.steps == 4


SHORT = {(0, (0,)): row((.9, .1), (.4, .35, .25)), (2, (0,)): row((.8, .2), (.5, .3, .2))}


def test_a_final_chunk_shorter_than_the_longest_duration_clamps_fuses_and_sorts_before_it_steps():
    # V = 2, durations (2, 3, 4), beam 3, chunks of 2 + 1 frames (the final chunk is shorter than 4).
    # chunk 1 (F = 2): f = 0: tokens (.9, .1), durations (.4, .35, .25): blank/2 .36 -> t2, blank/3 .315 -> t3, blank/4 .225 -> t4
    #   (not clamped: the end is not known yet) | label/2 .04 pruned.  Every entry has t >= 2.
    # chunk 2 (F = T = 3, final).  Begin: t4 is clamped to 3; pool in beam order (t2 .36), (t3 .315), (t3 .225): the last two
    #   are one class, .54, Viterbi max = .315; sorted: ((0), t3, .54), ((0), t2, .36) -- the order has changed.
    #   f = 2: ((0), t3) waits and, first in the pool, represents; ((0), t2): tokens (.8, .2), durations (.5, .3, .2): blank/2
    #   .4, blank/3 .24, blank/4 .16 all end at t3 (clamped): .36 * (.4 + .24 + .16) = .288 joins it: .828, Viterbi
    #   max(.315, .144) = .315.
    trace = []
    got = ref.search(ref.Scripted(SHORT), [2, 1], 2, (2, 3, 4), 3, trace=trace)
    approx(got.after[0], [((0,), 2, .36, .36, ()), ((0,), 3, .315, .315, ()), ((0,), 4, .225, .225, ())])
    approx(trace[1], [((0,), 3, .54, .315, ()), ((0,), 2, .36, .36, ())])
    approx(got.beam, [((0,), 3, .828, .315, ())])
    assert got.steps == 2


def test_a_final_call_with_zero_frames_only_clamps_fuses_and_sorts():
    # as above, then a final chunk of no frames: T = 2; t3 and t4 are clamped to 2 and everything is one class: .9, Viterbi
    # .36.  No row is consulted (the table has none for it).
    got = ref.search(ref.Scripted({(0, (0,)): SHORT[(0, (0,))]}), [2, 0], 2, (2, 3, 4), 3)
    approx(got.beam, [((0,), 2, .9, .36, ())])
    assert got.steps == 1
    # and a stream that ends before its first frame
    assert ref.search(ref.Scripted({}), [0], 2, (2, 3, 4), 3).beam == [((0,), 0, 0.0, 0.0, ())]


# ------------------------------------------------------------------------------------------- chunking invariance --
class Rows:
    """A scripted utterance with a row for every (frame, tokens): logits drawn from a generator seeded by the key, favouring
    blank a little so that hypotheses of different lengths meet."""

    def __init__(self, width, seed):
        self.width, self.seed, self.memo = width, seed, {}

    def row(self, t, toks):
        key = (t, toks)
        if key not in self.memo:
            rng = np.random.default_rng([self.seed, t, len(toks)] + list(toks))
            r = 2.0 * rng.normal(size=self.width)
            r[0] += 1.0
            self.memo[key] = r
        return self.memo[key]


def splits(T):
    """every way to cut T frames into chunks of one frame or more"""
    for n in range(T):
        for cuts in itertools.combinations(range(1, T), n):
            edges = (0,) + cuts + (T,)
            yield [b - a for a, b in zip(edges, edges[1:])]


@pytest.mark.parametrize("durations, beam", [(None, 3), (None, 4), ((1, 2), 3), ((0, 1, 2, 3), 4)],
                         ids=["plain-beam3", "plain-beam4", "tdt-12", "tdt-0123"])
def test_every_chunking_of_six_frames_equals_the_one_chunk_run(durations, beam):
    T, V = 6, 4
    width = V + (len(durations) if durations else 0)
    whole = ref.search(Rows(width, 3), [T], V, durations, beam)
    assert any(len(h) > 1 for h, _, _, _, _ in whole.beam) and len(whole.beam) >= 3
    ways = [w for w in splits(T) if durations is None or w[-1] >= max(durations)]
    assert len(ways) == (32 if durations is None else 16 if max(durations) == 2 else 8)
    for w in ways:
        got = ref.search(Rows(width, 3), w, V, durations, beam)
        assert got.beam == whole.beam, w                     # tokens, frames, scores, Viterbi scores, times: all exact
        assert got.steps == whole.steps
    # zero-width chunks in between and a zero-frame final call after the last frame change nothing either
    assert ref.search(Rows(width, 3), [2, 0, 4], V, durations, beam).beam == whole.beam
    if durations is None:
        assert ref.search(Rows(width, 3), [2, 4, 0], V, durations, beam).beam == whole.beam


@pytest.mark.parametrize("durations", [(1,), (1, 2), (0, 1, 2, 3)], ids=["dur1", "12", "0123"])
def test_the_one_chunk_run_is_the_whole_utterance_reference(durations):
    T, V, beam = 6, 4, 4
    width = V + len(durations)
    want = tdt_beam_ref.search(Rows(width, 5), T, V, durations, beam)
    got = ref.search(Rows(width, 5), [T], V, durations, beam)
    assert [(h, t, s) for h, t, s, _, _ in got.beam] == list(want.beam)         # exactly
    assert got.steps == want.steps and got.margin <= want.margin
    for h, _, s, v, tm in got.beam:
        assert len(tm) == len(h) - 1 and list(tm) == sorted(tm) and v <= s + 1e-12
    if durations == (1,):                                    # the plain form: the same rows without the duration column
        class Cut:
            def row(self, t, toks):
                return Rows(width, 5).row(t, toks)[:V]
        plain = ref.search(Cut(), [T], V, None, beam)
        assert plain.beam == got.beam


# ------------------------------------------------------------------ the cases of tests/test_beam_stream_gpu.py --
# (the case generator, lengths, margin and quota are those of tests/test_tdt_beam_ref.py; a seed differs from the one there
# only where the Viterbi gap, which is new here, would disqualify the case)
STREAM_SPECS = tuple(SPEC[n] for n in ("dur1-ctc", "dur1-beam16-embedding-ctc", "beam8-ctc", "beam16-124", "beam3-08-ctc-blank2",
                                       "embedding", "conv-blank5"))
STREAM_SPEC = {s.name: s for s in STREAM_SPECS}


def cut(widths, n):
    """what an utterance of n frames takes from each of the chunks"""
    out = []
    for w in widths:
        out.append(min(w, n))
        n -= out[-1]
    assert n == 0
    return out


@functools.lru_cache(maxsize=None)
def reference(spec, widths=None):
    """The float64 beams of a case for a chunking (None: one chunk), computed once per process and shared."""
    c = cases.make_case(spec)
    return ref.decode(c.pred, c.joint, c.enc, c.lens, c.V, spec.durations, spec.beam, spec.blank,
                      None if c.ctc_logp is None else c.ctc_logp.numpy(), *c.weights, widths=widths)


def stream_conditions(want):
    bad = []
    if sum(r.margin > MARGIN for r in want) < MIN_QUALIFY:
        bad.append(f"fewer than {MIN_QUALIFY} utterances with a margin above {MARGIN}: {[r.margin for r in want]}")
    if not any(len(tm) > 0 for r in want for _, _, _, _, tm in r.beam):
        bad.append("no label in any hypothesis")
    return bad


@pytest.mark.parametrize("spec", STREAM_SPECS, ids=[s.name for s in STREAM_SPECS])
def test_gpu_case_qualifies_in_float64(spec):
    want = reference(spec)
    old = cases.reference(spec)
    print(spec.name, "margins", [r.margin for r in want], "against", [r.margin for r in old])
    assert stream_conditions(want) == []
    for r, o, n in zip(want, old, LENS):
        assert [(h, t, s) for h, t, s, _, _ in r.beam] == list(o.beam)          # the whole-utterance reference, exactly
        assert r.margin <= o.margin
        for h, t, s, v, tm in r.beam:
            assert t == n and len(tm) == len(h) - 1 and all(0 <= a <= b < n for a, b in zip(tm, tm[1:] or tm))
            assert v <= s + 1e-9


SHORT_FINAL = (5, 16, 16, 3)           # a final chunk of 3 frames against durations (0, 8)


def test_the_short_final_chunk_case_qualifies_in_float64():
    spec = STREAM_SPEC["beam3-08-ctc-blank2"]
    want = reference(spec, SHORT_FINAL)
    whole = reference(spec)
    print("margins", [r.margin for r in want], "equal to the one-chunk run", [r.beam == w.beam for r, w in zip(want, whole)])
    assert stream_conditions(want) == []
    # utterances that end in an earlier chunk get a zero-frame final call; the rule makes that equal to the one-chunk run
    # only if nothing stood beyond the end
    assert want[-1].beam == whole[-1].beam
