"""CTC decode modes on the GPU: identical hypotheses to the reference's
ASRModel.ctc_greedy_search / _ctc_prefix_beam_search outputs (tests/golden/ctc_decode_*.npz) and to the
reference's own known-answer test (runtime/core/test/ctc_prefix_beam_search_test.cc:30-73)."""
import glob
import math
import os

import numpy as np
import pytest
import torch

import ctc_decode_ref as cref
from conftest import GOLDEN
from oracle import decode_oracle as do

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "ctc_decode_*.npz"))))
def test_matches_reference(path):
    import wenet_celoss_amd as w
    d = np.load(path)
    logits = torch.tensor(d["logits"], device=DEV)
    lens = torch.tensor(d["lens"], device=DEV)
    hyps, scores = w.ctc_greedy_search(logits, lens)
    for b, h in enumerate(hyps):
        assert h == list(d["greedy"][b][: d["greedy_lens"][b]])
    np.testing.assert_allclose(scores.cpu().numpy(), d["greedy_scores"], rtol=1e-5, atol=1e-6)
    nbest = w.ctc_prefix_beam_search(logits, lens, int(d["beam"]))          # all utterances in one call
    for b, hb in enumerate(nbest):
        assert len(hb) == int(d["nbest_n"][b])
        for k, (pref, sc) in enumerate(hb):
            assert list(pref) == list(d["nbest"][b, k][: d["nbest_lens"][b, k]]), (b, k)
            assert sc == pytest.approx(d["nbest_scores"][b, k], rel=1e-5)


def test_known_answer_from_reference_gtest():
    import wenet_celoss_amd as w
    d = np.load(os.path.join(GOLDEN, "ctc_prefix_kat.npz"))
    # the kernel applies log-softmax; log of a probability row is a fixed point of it
    logits = torch.tensor(np.log(d["probs"]), device=DEV)[None]
    nb = w.ctc_prefix_beam_search(logits, torch.tensor([3]), int(d["beam"]))[0]
    for k, (pref, sc) in enumerate(nb):
        assert list(pref) == list(d["nbest"][k][: d["nbest_lens"][k]])
        assert math.exp(sc) == pytest.approx(float(d["likelihood"][k]), rel=1e-4)


def test_config_scale_against_oracle():
    import wenet_celoss_amd as w
    torch.manual_seed(9)
    B, T, V, beam = 4, 300, 5000, 10
    logits = torch.randn(B, T, V, device=DEV) * 3
    logits[:, :, 0] += 6
    lens = torch.tensor([300, 211, 150, 299], device=DEV)
    nb = w.ctc_prefix_beam_search(logits, lens, beam)
    lp = do.log_softmax(logits.cpu().numpy())
    for b in (1, 2):
        ref = do.ctc_prefix_beam_search(lp[b], int(lens[b]), beam)
        assert [p for p, _ in ref] == [p for p, _ in nb[b]]
        np.testing.assert_allclose([s for _, s in ref], [s for _, s in nb[b]], rtol=1e-6)
    gh, gs = w.ctc_greedy_search(logits, lens)
    rh, rs = do.ctc_greedy_search(logits.cpu().numpy(), lens.cpu().numpy(), V - 1)
    assert gh == rh
    np.testing.assert_allclose(gs.cpu().numpy(), rs, rtol=1e-5, atol=2e-6)


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(GOLDEN, "ctc_align_*.npz"))))
def test_forced_align_matches_reference(path):
    import wenet_celoss_amd as w
    d = np.load(path)
    ali = w.forced_align(torch.tensor(d["ctc_probs"], device=DEV), torch.tensor(d["y"], device=DEV))
    assert ali == list(d["alignment"])


def test_forced_align_batch_and_scale():
    import wenet_celoss_amd as w
    rng = np.random.default_rng(3)
    B, T, S, V = 3, 400, 120, 500
    logits = (rng.normal(size=(B, T, V)) * 2).astype(np.float32)
    y = rng.integers(1, V, size=(B, S))
    il = np.array([400, 333, 260]); tl = np.array([120, 50, 77])
    got = w.forced_align_batch(torch.tensor(logits, device=DEV), torch.tensor(y, device=DEV), torch.tensor(il),
                               torch.tensor(tl))
    lp = do.log_softmax(logits)
    for b in range(B):
        ref = do.forced_align(lp[b, :il[b]], y[b, :tl[b]])
        assert got[b] == ref
        assert len(got[b]) == il[b] and set(got[b]) <= set(y[b, :tl[b]].tolist()) | {0}
    # NOTE: with random posteriors and T >> 2S+1 the reference's s-1 = -1 wrap (state 0 <- last state) lets the
    # best path run through the labels more than once; the kernel reproduces that (got == ref above), so
    # "the alignment collapses to the label sequence" is deliberately not asserted here.


# ------------------------------------------------------------------------------------------------------------------
# The decode kernels at the edges of their parameter ranges, against the float64 references of tests/ctc_decode_ref.py
# (checked on the CPU by tests/test_ctc_decode_ref.py).
#
# Prefix search: hypotheses exact, scores at this file's bar rel=1e-5.  Exactness needs inputs on which no decision of
# the search is closer than the device's own rounding: its fp32 log-softmax differs from float64 by a few ulp of values
# up to ~20, at most ~1e-5 per frame, and T <= 40 frames accumulate at most 4e-4; every seed below was picked on the CPU
# for a smallest reference decision gap >= MIN_GAP = 1e-3 and no exact tie, and each test asserts that, together with
# the statistic (ncur, slots, merges) the case exists for.
MIN_GAP = 1e-3


def _search(x, lens, beam, blank=0):
    import wenet_celoss_amd as w
    return w.ctc_prefix_beam_search(torch.tensor(np.asarray(x), device=DEV), torch.tensor(lens), beam, blank=blank)


def _reference(x, T, beam, blank=0):
    nb, st = cref.prefix_beam_search(x, T, beam, blank)
    print(f"reference: T={T} V={x.shape[1]} beam={beam} blank={blank}: {st}")
    assert st.min_gap >= MIN_GAP and st.ties == 0, st
    return nb, st


def _same_nbest(got, want):
    assert [p for p, _ in got] == [p for p, _ in want]
    for (_, g), (_, r) in zip(got, want):
        assert g == pytest.approx(r, rel=1e-5)


@pytest.mark.parametrize("beam,T,V,seed", [(1, 30, 17, 0), (2, 31, 18, 0), (9, 33, 19, 4), (12, 35, 20, 4),
                                           (13, 37, 19, 6), (16, 40, 20, 0)])
def test_prefix_beam_range(beam, T, V, seed):
    """kMaxCtcBeam = 16: waves 2 and 3 of the slot compaction take part from beam * ncur > 128 on (beam >= 12), and the
    all-pairs steps run at up to 2 * 16 * 16 slots."""
    x = cref.peaky_logits(seed, T, V, 0)
    want, st = _reference(x, T, beam)
    assert st.max_ncur == beam
    if beam >= 2:
        assert st.merges > 0 and st.pairs > 0
    if beam >= 12:
        assert beam * st.max_ncur > 128
    if beam == 16:
        assert st.max_slots > 256
    _same_nbest(_search(x[None], [T], beam)[0], want)


@pytest.mark.parametrize("beam,blank,seed", [(16, 0, 6), (16, 5, 6), (16, 18, 1), (3, 0, 0), (3, 5, 0), (3, 18, 0)])
def test_prefix_beam_blank_position(beam, blank, seed):
    T, V = 32, 19
    x = cref.peaky_logits(seed, T, V, blank)
    want, st = _reference(x, T, beam, blank)
    assert st.max_ncur == beam and st.merges > 0 and st.pairs > 0
    if blank and beam == 16:
        assert any(0 in p for p, _ in want)             # label 0 is an ordinary token once the blank has moved
    _same_nbest(_search(x[None], [T], beam, blank)[0], want)


@pytest.mark.parametrize("V,beam,blank,T,seed", [(16, 16, 0, 30, 0), (2, 1, 0, 12, 0), (2, 2, 0, 12, 0), (2, 2, 1, 12, 0)])
def test_prefix_beam_equal_to_vocabulary_and_two_symbols(V, beam, blank, T, seed):
    """beam = V: no top-k cut, every symbol is visited.  V = 2: the smallest vocabulary the entry point takes."""
    x = cref.peaky_logits(seed, T, V, blank)
    want, st = _reference(x, T, beam, blank)
    assert st.max_ncur == beam
    if V == 16:
        assert st.max_slots > 256
    _same_nbest(_search(x[None], [T], beam, blank)[0], want)


def _length_batch():
    T, V = 30, 18
    x = np.stack([cref.peaky_logits(s, T, V, 0) for s in (10, 3, 4, 12, 5)])
    return x, [T, 0, 1, T + 5, T // 2], T, V


def test_prefix_beam_lengths_and_batch_against_alone():
    """One batch with a full, an empty, a one-frame, an over-long (lens > T behaves as T) and a half-length utterance:
    each against the reference, and bit for bit against the same utterance called alone with its own T (the sequence
    buffers are strided by the batch's T)."""
    beam = 7
    x, lens, T, V = _length_batch()
    got = _search(x, lens, beam)
    assert got[1] == [((), 0.0)]
    for b, n in enumerate(lens):
        n = min(n, T)
        if n:
            want, _ = _reference(x[b], n, beam)
            _same_nbest(got[b], want)
        alone = _search(x[b:b + 1, :max(n, 1)], [n], beam)[0]
        assert alone == got[b], b                       # hypotheses and float64 scores, bit for bit


def test_greedy_lengths_blank_and_eos():
    import wenet_celoss_amd as w
    x, lens, T, V = _length_batch()
    xd, ld = torch.tensor(x, device=DEV), torch.tensor(lens)
    for blank, eos in [(0, -1), (5, -1), (V - 1, -1), (V - 1, 4), (0, 0)]:
        gh, gs = w.ctc_greedy_search(xd, ld, blank=blank, eos=eos)
        rh, rs = cref.greedy_search(x, lens, blank, eos)
        assert gh == rh, (blank, eos)
        np.testing.assert_allclose(gs.cpu().numpy(), rs, rtol=1e-5, atol=2e-6)
        e = V - 1 if eos < 0 else eos
        assert gh[1] == ([] if e == blank else [e])     # length 0: every frame is eos
        if e != blank:
            assert gh[2][-1] == e and gh[4][-1] == e    # short utterances end in the eos of their padding frames


def test_prefix_beam_small_beam_after_large_on_reused_workspace():
    """beam 16, then beam 3 at the same B and T (the caching allocator hands the second call the blocks of the first:
    stale top-k rows and sequence buffers of a wider beam), then beam 16 again."""
    T, V = 32, 19
    x = np.stack([cref.peaky_logits(s, T, V, 0) for s in (6, 30)])
    lens = [T, T]
    first = _search(x, lens, 16)
    small = _search(x, lens, 3)
    third = _search(x, lens, 16)
    assert first == third
    for b in range(2):
        w16, st = _reference(x[b], T, 16)
        assert st.max_ncur == 16
        _same_nbest(first[b], w16)
        w3, _ = _reference(x[b], T, 3)
        _same_nbest(small[b], w3)


def test_vocabulary_limit():
    """V = 16320 is the widest row the top-k kernel's LDS takes; one more is rejected by both searches, as are a beam
    above 16 or above V and a blank outside the vocabulary -- all before anything is launched."""
    import wenet_celoss_amd as w
    T, V, beam = 4, 16320, 16
    x = np.stack([cref.peaky_logits(s, T, V, 0, scale=3.0, bonus=4.0, blank_bonus=8.0) for s in (1, 3)])
    got = _search(x, [T, T - 1], beam)
    for b, n in enumerate([T, T - 1]):
        want, st = _reference(x[b], n, beam)
        assert st.max_ncur == 16
        _same_nbest(got[b], want)
    gh, gs = w.ctc_greedy_search(torch.tensor(x, device=DEV), torch.tensor([T, T - 1]))
    rh, rs = cref.greedy_search(x, [T, T - 1], 0, -1)
    assert gh == rh
    np.testing.assert_allclose(gs.cpu().numpy(), rs, rtol=1e-5, atol=2e-6)
    wide = torch.zeros(1, 2, V + 1, device=DEV)
    one = torch.tensor([2])
    with pytest.raises(RuntimeError, match="16320"):
        w.ctc_prefix_beam_search(wide, one, 4)
    with pytest.raises(RuntimeError, match="16320"):
        w.ctc_greedy_search(wide, one)
    small = torch.zeros(1, 2, 8, device=DEV)
    with pytest.raises(RuntimeError, match="beam=17"):
        w.ctc_prefix_beam_search(torch.zeros(1, 2, 40, device=DEV), one, 17)
    with pytest.raises(RuntimeError, match="beam=9"):
        w.ctc_prefix_beam_search(small, one, 9)
    with pytest.raises(RuntimeError, match="blank 8"):
        w.ctc_prefix_beam_search(small, one, 4, blank=8)
    with pytest.raises(RuntimeError, match="blank 8"):
        w.ctc_greedy_search(small, one, blank=8)


@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("beam", [1, 2, 3])
@pytest.mark.parametrize("T", [1, 2])
def test_prefix_beam_exact_ties(T, beam, blank):
    """Uniform rows, V = 3: every score is k * log(1/3), or that plus log 2 or log 3 for the two prefixes that two or
    three routes reach -- equal scores come out of identical operation sequences, so they tie on any implementation, and
    the order is the reference's: top-k by index, prune by insertion order.  (No longer chains: log_add is not
    associative to the last bit, and the test would pin rounding, not the kernel.)"""
    x = np.zeros((T, 3), np.float32)
    want, st = cref.prefix_beam_search(x, T, beam, blank)
    assert st.ties > 0
    _same_nbest(_search(x[None], [T], beam, blank)[0], want)


@pytest.mark.parametrize("V", [2, 63, 64, 65, 130])
def test_greedy_first_index_on_tied_maxima(V):
    """Logits on a 1/4 grid with the row maximum at two or three positions: the argmax is taken on the raw logits and
    must be the first index -- within a lane's strided walk (v, v + 64), across the lanes of the reduce, at the wave's
    edge (V = 63, 64, 65)."""
    import wenet_celoss_amd as w
    rng = np.random.default_rng(V)
    B, T = 2, 48
    x = (rng.integers(-8, 8, size=(B, T, V)) / 4).astype(np.float32)
    top = x.max(-1) + 0.25
    for b in range(B):
        for t in range(T):
            x[b, t, rng.choice(V, size=min(V, 2 + t % 2), replace=False)] = top[b, t]
    x[0, 0, [0, V - 1]] = top[0, 0] + 1                 # first against last index
    assert ((x == x.max(-1, keepdims=True)).sum(-1) >= 2).all()
    lens = [T, T - 7]
    blank = int(x[0, 1].argmax())                       # a blank that does occur
    gh, gs = w.ctc_greedy_search(torch.tensor(x, device=DEV), torch.tensor(lens), blank=blank)
    rh, rs = cref.greedy_search(x, lens, blank, -1)
    assert gh == rh
    np.testing.assert_allclose(gs.cpu().numpy(), rs, rtol=1e-5, atol=2e-6)


def _long_ragged(rng):
    B, T, V = 3, 2800, 8                                # 8400 rows: more than 2048 workgroups of four one-row waves
    x = (rng.normal(size=(B, T, V)) * 2).astype(np.float32)
    return x, [1500, 2799, 2800]


def test_greedy_grid_stride_second_trip():
    import wenet_celoss_amd as w
    x, lens = _long_ragged(np.random.default_rng(41))
    x[2, 2795] += 30.0 * (np.arange(8) == 3)            # the batch-wide best frame of utterance 2 lies in the second trip
    gh, gs = w.ctc_greedy_search(torch.tensor(x, device=DEV), torch.tensor(lens), blank=2)
    rh, rs = cref.greedy_search(x, lens, 2, -1)
    assert gh == rh
    np.testing.assert_allclose(gs.cpu().numpy(), rs, rtol=1e-5, atol=2e-6)


# ------------------------------------------------------------------------------------------------ forced alignment --
# With normalized=True the kernel adds the given fp32 log-posteriors in the oracle's order: results are compared
# exactly, ties included.
def _align(lp, y, blank_id):
    import wenet_celoss_amd as w
    return w.forced_align(torch.tensor(lp, device=DEV), torch.tensor(y, device=DEV), blank_id=blank_id)


@pytest.mark.parametrize("blank_id,seed", [(0, 50), (3, 195), (8, 59)])
def test_forced_align_tied_candidates_and_blank_id(blank_id, seed):
    """Log-posteriors on a 1/8 grid (sums exact, ties frequent), a label equal to blank_id and repeated neighbours.  The
    seeds were picked so that the backtraced path itself crosses cells whose candidates [s, s-1, s-2] tie in each of
    the three ways -- s with s-1, s with s-2, s-1 with s-2 -- between candidates that carry different tokens, so that
    any other preference than the first of [s, s-1, s-2] changes the result."""
    rng = np.random.default_rng(seed)
    T, V = 26, 9
    lp = (rng.integers(-12, 0, size=(T, V)) / 8).astype(np.float32)
    y = [1, 1, blank_id, 4, 5, 5, 2]
    want, ties = cref.forced_align(lp, y, blank_id, return_ties=True)
    assert want == do.forced_align(lp, y, blank_id)
    assert {(0, 1), (0, 2), (1, 2)} <= set(ties), ties
    assert _align(lp, y, blank_id) == want


def test_forced_align_short_utterances():
    """T_b = 1, T_b < S_b and S_b <= T_b < 2 S_b + 1 in one batch; the oracle defines the result."""
    import wenet_celoss_amd as w
    rng = np.random.default_rng(12)
    B, T, S, V = 4, 9, 6, 10
    lp = do.log_softmax((rng.normal(size=(B, T, V)) * 2).astype(np.float32))
    y = rng.integers(0, V, size=(B, S))
    y[y == 3] = 4
    il, tl = [1, 4, 9, 1], [3, 6, 6, 1]
    got = w.forced_align_batch(torch.tensor(lp, device=DEV), torch.tensor(y, device=DEV), torch.tensor(il), torch.tensor(tl),
                               blank_id=3, normalized=True)
    for b in range(B):
        assert got[b] == do.forced_align(lp[b, :il[b]], y[b, :tl[b]], 3), b
    assert got[0] == [3] and got[3] == [int(y[3, 0])]   # one frame: three labels do not fit, one label does


def test_forced_align_largest_label_count():
    """S = 511: 1023 states, the block's and the int16 back-pointers' maximum; S = 512 is rejected."""
    import wenet_celoss_amd as w
    rng = np.random.default_rng(13)
    T, S, V = 1030, 511, 12
    lp = do.log_softmax((rng.normal(size=(T, V)) * 2).astype(np.float32))
    y = rng.integers(1, V, size=S)
    y[5:9] = y[5]                                       # repeated neighbours need their blank
    want = cref.forced_align(lp, y, 0)
    got = _align(lp, y, 0)
    assert got == want
    assert [v for i, v in enumerate(got) if v and (i == 0 or got[i - 1] != v)] == list(y)   # feasible: collapses to y
    with pytest.raises(RuntimeError, match="limit"):
        _align(lp, np.concatenate([y, [1]]), 0)


def test_forced_align_grid_stride_second_trip():
    import wenet_celoss_amd as w
    rng = np.random.default_rng(14)
    x, il = _long_ragged(rng)
    lp = do.log_softmax(x)
    B, S = 3, 6
    y = rng.integers(0, 8, size=(B, S))
    y[y == 2] = 5
    tl = [6, 3, 5]
    got = w.forced_align_batch(torch.tensor(lp, device=DEV), torch.tensor(y, device=DEV), torch.tensor(il), torch.tensor(tl),
                               blank_id=2, normalized=True)
    for b in range(B):
        assert got[b] == cref.forced_align(lp[b, :il[b]], y[b, :tl[b]], 2), b


def _stable_alignment(xb, yb, blank_id, rng):
    """The oracle's alignment of pre-softmax rows xb, asserted to be the same for the fp32 log-softmax, the float64 one
    rounded to fp32, and that with a uniform +-1e-5 perturbation of either sign."""
    l64 = cref.log_softmax_f64(xb).astype(np.float32)
    noise = rng.uniform(-1e-5, 1e-5, size=l64.shape)
    variants = [do.log_softmax(xb), l64, (l64 + noise).astype(np.float32), (l64 - noise).astype(np.float32)]
    alis = [do.forced_align(v, yb, blank_id) for v in variants]
    assert all(a == alis[0] for a in alis)
    return alis[0]


@pytest.mark.parametrize("seed", [0, 1])
def test_forced_align_from_logits(seed):
    """normalized=False: the device takes the log-softmax itself, so equality needs inputs whose alignment does not hang
    on its last bits (_stable_alignment asserts that)."""
    import wenet_celoss_amd as w
    rng = np.random.default_rng(seed)
    B, T, S, V = 2, 40, 8, 12
    x = (rng.normal(size=(B, T, V)) * 2).astype(np.float32)
    y = rng.integers(0, V, size=(B, S))
    y[y == 3] = 7
    il, tl = [T, 33], [S, 5]
    want = [_stable_alignment(x[b, :il[b]], y[b, :tl[b]], 3, rng) for b in range(B)]
    got = w.forced_align_batch(torch.tensor(x, device=DEV), torch.tensor(y, device=DEV), torch.tensor(il), torch.tensor(tl),
                               blank_id=3)
    assert got == want


@pytest.mark.parametrize("normalized", [True, False])
@pytest.mark.parametrize("pad", [-1, 7])
def test_forced_align_empty_transcript_in_a_batch(pad, normalized):
    """An utterance without labels has one CTC path: blank_id at every frame, whatever the padding holds."""
    import wenet_celoss_amd as w
    rng = np.random.default_rng(15)
    B, T, S, V, blank_id = 3, 21, 4, 9, 3
    x = (rng.normal(size=(B, T, V)) * 2).astype(np.float32)
    x[1, :, 7] += 6.0                                   # the padding value, and label 0, would win every frame
    x[1, :, 0] += 6.0
    lp = do.log_softmax(x)
    y = np.array([[1, 2, 2, 5], [pad] * 4, [6, 1, pad, pad]])
    il, tl = [T, 17, 12], [4, 0, 2]
    got = w.forced_align_batch(torch.tensor(lp if normalized else x, device=DEV), torch.tensor(y, device=DEV),
                               torch.tensor(il), torch.tensor(tl), blank_id=blank_id, normalized=normalized)
    assert got[1] == [blank_id] * 17
    for b in (0, 2):
        if normalized:
            want = do.forced_align(lp[b, :il[b]], y[b, :tl[b]], blank_id)
        else:
            want = _stable_alignment(x[b, :il[b]], y[b, :tl[b]], blank_id, rng)
        assert got[b] == want, b
    with pytest.raises(RuntimeError, match="empty label"):
        w.forced_align_batch(torch.tensor(lp, device=DEV), torch.zeros(B, 0, dtype=torch.int64, device=DEV),
                             torch.tensor(il), torch.zeros(B, dtype=torch.int64), blank_id=blank_id, normalized=True)
