"""TDT forced alignment on the GPU (rnnt_tdt_forced_align: tdt_stats_kernel, then tdt_viterbi_kernel and its backtrace)
against the float64 reference written from the contract (tests/rnnt_tdt_align_ref.py, itself checked against path
enumeration in tests/test_rnnt_tdt_align_ref.py).

Tolerances are those of tests/test_rnnt_align_gpu.py.  Against the reference on the same (rounded) logits: the score
within 1e-5 * max(1, |opt|), the returned path rescored in float64 within the same bound of the optimum, and the path
exactly the reference's wherever the reference's smallest decision margin along its path exceeds 1e-3.  A planted path
must come back exactly; its score is near 0 while every row's log-sum-exp is near BOOST, so there the score's bound is
that file's 2e-6 * BOOST per fp32 log-probability summed (two per arc here: token and duration) + 1e-5."""
import functools

import numpy as np
import pytest
import torch

import rnnt_tdt_align_ref as aref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BOOST = 12.0
STAGE_DIAGONALS = 256          # kTdtStageDiags of csrc/rnnt_lattice.hip: anti-diagonals per staged backtrace block
D04, D08 = (0, 1, 2, 3, 4), tuple(range(9))


def random_path(rng, T, U, durs, first=None):
    """A random arc sequence [(kind, t, u, d)] from (0, 0) to the terminal, or None if the lattice has none."""
    ok = np.zeros((T + 1, U + 1), bool)              # the terminal can be reached from (t, u)
    ok[T, U] = True
    for t in range(T - 1, -1, -1):
        for u in range(U, -1, -1):
            ok[t, u] = any((d >= 1 and t + d <= T and ok[t + d, u]) or (u < U and t + d <= T - 1 and ok[t + d, u + 1])
                           for d in durs)
    if not ok[0, 0]:
        return None
    path, t, u = [], 0, 0
    while t < T:
        arcs = [(aref.BLANK, t, u, d) for d in durs if d >= 1 and t + d <= T and ok[t + d, u]]
        arcs += [(aref.LABEL, t, u, d) for d in durs if u < U and t + d <= T - 1 and ok[t + d, u + 1]]
        if not path and first is not None and any(a[0] == first for a in arcs):
            arcs = [a for a in arcs if a[0] == first]
        arc = arcs[int(rng.integers(len(arcs)))]
        path.append(arc)
        t, u = t + arc[3], u + (arc[0] == aref.LABEL)
    return path


def planted_case(B, T, U1, V, durs, llens, tlens, seed, blank=0, label_is_blank=False, first=None):
    """Unit-normal logits with the token and the duration logit of every arc of one random path per utterance raised by
    BOOST -> (logits, targets, planted frames / durations / jumps, arcs per utterance)."""
    rng = np.random.default_rng(seed)
    D = len(durs)
    logits = rng.normal(size=(B, T, U1, V + D)).astype(np.float32)
    targets = rng.integers(0, V - 1, size=(B, U1 - 1)).astype(np.int32)
    targets += targets >= blank                       # any token but the blank ...
    if label_is_blank:
        targets[:, ::2] = blank                       # ... or every other label the blank
    frames = np.full((B, U1 - 1), -1, np.int64)
    pdurs = np.full((B, U1 - 1), -1, np.int64)
    jumps = np.zeros((B, T), np.int64)
    narcs = []
    for b in range(B):
        path = random_path(rng, int(llens[b]), int(tlens[b]), durs, first)
        narcs.append(len(path) if path else 0)
        for kind, t, u, d in path or []:
            logits[b, t, u, blank if kind == aref.BLANK else targets[b, u]] += BOOST
            logits[b, t, u, V + durs.index(d)] += BOOST
            if kind == aref.LABEL:
                frames[b, u], pdurs[b, u] = t, d
            else:
                jumps[b, t] = d
    return logits, targets, frames, pdurs, jumps, narcs


def align(logits, targets, llens, tlens, durs, blank=0, sigma=0.0, dtype=torch.float32, jumps=True):
    import wenet_celoss_amd as w
    out = w.rnnt_tdt_forced_align(torch.as_tensor(np.asarray(logits)).to(DEV).to(dtype),
                                  torch.as_tensor(np.asarray(targets), dtype=torch.int32).to(DEV),
                                  torch.as_tensor(np.asarray(llens), dtype=torch.int32).to(DEV),
                                  torch.as_tensor(np.asarray(tlens), dtype=torch.int32).to(DEV), durs, blank=blank,
                                  sigma=sigma, return_blank_jumps=jumps)
    assert len(out) == (4 if jumps else 3) and all(o.is_cuda for o in out)
    assert out[0].dtype == out[1].dtype == torch.int32 and out[2].dtype == torch.float64
    return [o.cpu().numpy() for o in out]


def rounded(logits, dtype):
    return torch.as_tensor(np.asarray(logits)).to(dtype).float().numpy()


def check_against_reference(logits, targets, llens, tlens, durs, out, blank=0, sigma=0.0, score_tol=None):
    """The three assertions of the module docstring per utterance; no path: -inf and the no-path outputs on both sides.
    Returns the reference's Alignments."""
    fr, du, sc, bj = out
    refs, rf, rd, rj = aref.align_ref(logits, targets, llens, tlens, durs, blank, sigma)
    for b, a in enumerate(refs):
        T, U = int(llens[b]), int(tlens[b])
        print(f"utterance {b}: T {T} U {U} score {sc[b]:.6f} reference {a.score:.6f} margin {a.margin:.3e} ties {a.ties}")
        if a.score == -np.inf:
            assert sc[b] == -np.inf and aref.is_no_path(fr[b], du[b], bj[b]), b
            continue
        tol = 1e-5 * max(1.0, abs(a.score))
        assert abs(sc[b] - a.score) <= (tol if score_tol is None else score_tol[b]), (b, sc[b], a.score)
        path = aref.rebuild_path(fr[b], du[b], bj[b], T, U, durs)
        assert path is not None, b
        tb, tl, dur = aref.arcs(logits[b], targets[b] if len(targets[b]) else [], T, U, durs, blank, sigma)
        assert abs(aref.path_score(tb, tl, dur, durs, path) - a.score) <= tol, b
        if a.margin > 1e-3:
            assert np.array_equal(fr[b], rf[b]) and np.array_equal(du[b], rd[b]) and np.array_equal(bj[b], rj[b]), b
    return refs


def check_planted(case, llens, tlens, durs, blank=0, dtype=torch.float32, planted_is_best=True):
    """planted_is_best=False: where a label is the blank token, a label arc can stand in for a planted blank arc and the
    planted path need not be the best one; the comparison with the reference stays."""
    logits, targets, pf, pd, pj, narcs = case
    out = align(logits, targets, llens, tlens, durs, blank=blank, dtype=dtype)
    x = rounded(logits, dtype)
    tol = [2e-6 * BOOST * 2 * n + 1e-5 for n in narcs]
    refs = check_against_reference(x, targets, llens, tlens, durs, out, blank=blank, score_tol=tol)
    for b, a in enumerate(refs):
        if narcs[b] and planted_is_best:               # a condition on the reference: the planted path is its path, clearly
            assert a.margin > 1e-3 and np.array_equal(a.frames, pf[b, :int(tlens[b])]), b
            assert np.array_equal(out[0][b], pf[b]) and np.array_equal(out[1][b], pd[b]), b
            assert np.array_equal(out[3][b], pj[b]), b
    return refs


@pytest.mark.parametrize("U1", [1, 2, 64, 65, 129, 1024])
def test_planted_paths_across_column_counts(U1):
    """U + 1 across the wave boundary (64), the LDS exchange between waves and the 1024-column limit."""
    T, V = (12, 12) if U1 == 1024 else (40, 24)
    U = U1 - 1
    llens, tlens = [T, max(T // 2, 1)], [U, max(U - 3, 0)]
    case = planted_case(2, T, U1, V, D04, llens, tlens, seed=U1)
    refs = check_planted(case, llens, tlens, D04)
    assert all(np.isfinite(a.score) for a in refs)


@pytest.mark.parametrize("durs,llens", [(D04, [30, 1, 3, 30, 17]), ((1,), [30, 1, 3, 30, 17]),
                                        ((1, 2, 4), [30, 1, 3, 30, 17]), ((0, 8), [32, 8, 16, 24, 8]),
                                        (D08, [30, 1, 5, 30, 17])])
def test_planted_paths_across_duration_sets(durs, llens):
    """A ragged batch with U_b = 0, T_b = 1 and T_b below the largest duration; utterances the lattice has no path for
    (labels that do not fit the frames) come back as no-path on both sides."""
    tlens = [9, 0, 2, 0, 9]
    case = planted_case(5, max(llens), 10, 24, durs, llens, tlens, seed=100 + len(durs))
    refs = check_planted(case, llens, tlens, durs)
    assert sum(np.isfinite(a.score) for a in refs) >= 3


@pytest.mark.parametrize("first", [aref.BLANK, aref.LABEL])
@pytest.mark.parametrize("blank", ["first", "last"])
@pytest.mark.parametrize("label_is_blank", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_planted_paths_blank_and_dtypes(first, blank, label_is_blank, dtype):
    B, T, U1, V = 4, 30, 12, 33
    blank = 0 if blank == "first" else V - 1
    llens, tlens = [30, 17, 25, 9], [11, 4, 0, 11]
    case = planted_case(B, T, U1, V, D04, llens, tlens, 11, blank=blank, label_is_blank=label_is_blank, first=first)
    check_planted(case, llens, tlens, D04, blank=blank, dtype=dtype, planted_is_best=not label_is_blank)


@functools.lru_cache(maxsize=None)
def random_case(D, seed):
    rng = np.random.default_rng(seed)
    B, T, U1, V = 8, 60, 25, 40
    logits = (rng.normal(size=(B, T, U1, V + D)) * 2.0).astype(np.float32)
    targets = rng.integers(1, V, size=(B, U1 - 1)).astype(np.int32)
    return logits, targets, [60, 60, 41, 7, 1, 33, 60, 52], [24, 10, 24, 24, 3, 0, 17, 24]


@pytest.mark.parametrize("durs", [D04, (1, 2, 4)])
def test_random_logits_against_float64_reference(durs):
    logits, targets, llens, tlens = random_case(len(durs), 5)
    out = align(logits, targets, llens, tlens, durs, sigma=0.05)
    refs = check_against_reference(logits, targets, llens, tlens, durs, out, sigma=0.05)
    ambiguous = sum(1 for a in refs if np.isfinite(a.score) and a.margin <= 1e-3)
    print(f"random logits: {ambiguous} of {len(refs)} utterances ambiguous (margin <= 1e-3)")
    assert ambiguous <= len(refs) // 8                 # so that the exact comparison cannot be skipped wholesale
    assert sum(np.isfinite(a.score) for a in refs) >= 6


def tie_case(T, U, B, dur_logits, tok_logits, label):
    row = np.concatenate([tok_logits, dur_logits]).astype(np.float32)
    assert row.size == 16                               # every row starts on the same 64-byte alignment
    logits = np.ascontiguousarray(np.broadcast_to(row, (B, T, U + 1, 16)))
    return logits, np.full((B, U), label, np.int32)


def test_exact_ties_smaller_duration_wins():
    """Every cell holds the same row and every label is the same token: paths that differ only in where their d = 0 and
    d = 2 label arcs stand (equal duration logits) tie exactly, on the device as in the reference, since sums of so few
    float32 values are exact in float64.  Every other gap is far above the fp32 difference of the two sides' constants."""
    durs, T, U, B = (0, 1, 2, 3), 9, 4, 3
    logits, targets = tie_case(T, U, B, [0.0, 0.5, 0.0, -1.0], np.linspace(-1.0, 1.0, 12), 3)
    llens, tlens = [9, 7, 6], [4, 4, 3]
    out = align(logits, targets, llens, tlens, durs)
    refs = check_against_reference(logits, targets, llens, tlens, durs, out)
    _, rf, rd, rj = aref.align_ref(logits, targets, llens, tlens, durs)
    for a in refs:
        assert a.ties >= 1 and a.clear > 1e-3
    assert np.array_equal(out[0], rf) and np.array_equal(out[1], rd) and np.array_equal(out[3], rj)


def test_exact_ties_blank_beats_label():
    """The label is the blank token, so a blank arc and a label arc out of one cell weigh the same: with durations (1,)
    every path of an utterance ties with every other, and the rule (blank first) decides each cell."""
    durs, T, U, B = (1,), 9, 4, 2
    logits, targets = tie_case(T, U, B, [0.0], np.linspace(-1.0, 1.0, 15), 0)
    llens, tlens = [9, 6], [4, 2]
    out = align(logits, targets, llens, tlens, durs)
    refs = check_against_reference(logits, targets, llens, tlens, durs, out)
    _, rf, rd, rj = aref.align_ref(logits, targets, llens, tlens, durs)
    for b, a in enumerate(refs):
        assert a.ties >= 1 and a.clear > 1e-3
        assert np.array_equal(rf[b, :tlens[b]], np.arange(tlens[b]))     # labels first: walking back, blanks won
    assert np.array_equal(out[0], rf) and np.array_equal(out[1], rd) and np.array_equal(out[3], rj)


def test_backtrace_crosses_staged_blocks():
    """T_b + U_b = 607 anti-diagonals: more than twice the STAGE_DIAGONALS = 256 that one backtrace block stages."""
    T, U1, V, durs = 600, 8, 12, (0, 1, 2, 3)
    assert T + U1 - 1 >= 2 * STAGE_DIAGONALS and V + len(durs) == 16
    rng = np.random.default_rng(77)
    logits = (rng.normal(size=(2, T, U1, 16)) * 2.0).astype(np.float32)
    targets = rng.integers(1, V, size=(2, U1 - 1)).astype(np.int32)
    llens, tlens = [600, 300], [7, 5]
    out = align(logits, targets, llens, tlens, durs)
    refs = check_against_reference(logits, targets, llens, tlens, durs, out)
    assert all(np.isfinite(a.score) for a in refs)
    planted = planted_case(1, T, U1, V, durs, [600], [7], seed=78)
    check_planted(planted, [600], [7], durs)


def test_infeasible_utterance_among_feasible_ones():
    durs = (2,)
    llens, tlens = [6, 3, 8], [2, 0, 3]
    logits, targets, _, _ = random_case(1, 9)
    logits, targets = logits[:3, :8, :4], targets[:3, :3]
    out = align(logits, targets, llens, tlens, durs)
    refs = check_against_reference(logits, targets, llens, tlens, durs, out)
    assert [np.isfinite(a.score) for a in refs] == [True, False, True]
    assert out[2][1] == -np.inf and aref.is_no_path(out[0][1], out[1][1], out[3][1])
    keep = [0, 2]
    alone = align(logits[keep], targets[keep], [6, 8], [2, 3], durs)
    for got, want in zip(alone, out):
        assert np.array_equal(got, want[keep])


@pytest.mark.parametrize("value", [np.nan, np.inf, -np.inf])
def test_non_finite_logits_stay_in_their_utterance(value):
    durs = D04
    logits, targets, llens, tlens = random_case(len(durs), 5)
    logits, targets, llens, tlens = logits[:4, :20, :8], targets[:4, :7], [20, 20, 12, 20], [7, 7, 3, 5]
    clean = align(logits, targets, llens, tlens, durs)
    dirty = logits.copy()
    dirty[1, 3, 2, 5] = value                          # a token logit
    dirty[1, 7, 1, 40 + 2] = value                     # a duration logit
    dirty[1, 0, 0, :] = value if value != -np.inf else dirty[1, 0, 0, :]      # every path leaves through this row
    out = align(dirty, targets, llens, tlens, durs)
    for got, want in zip(out, clean):
        assert np.array_equal(got[[0, 2, 3]], want[[0, 2, 3]])
    fr, du, sc, bj = (o[1] for o in out)
    assert np.all((fr >= -1) & (fr < llens[1])) and np.all(np.isin(du, durs + (-1,))) and not np.isnan(sc)
    assert aref.is_valid_path(fr, du, bj, llens[1], tlens[1], durs) or (aref.is_no_path(fr, du, bj) and sc == -np.inf)


def test_two_calls_are_bit_identical():
    durs = (1, 2, 4)
    logits, targets, llens, tlens = random_case(len(durs), 5)
    a = align(logits, targets, llens, tlens, durs)
    b = align(logits, targets, llens, tlens, durs)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_scores_against_the_loss():
    """score <= -cost: a max over paths is at most their log-sum."""
    import wenet_celoss_amd as w
    durs = D04
    logits, targets, llens, tlens = random_case(len(durs), 5)
    sc = align(logits, targets, llens, tlens, durs, sigma=0.05)[2]
    cost = w.rnnt_tdt_loss(torch.as_tensor(logits).to(DEV), torch.as_tensor(targets).to(DEV),
                           torch.tensor(llens, dtype=torch.int32, device=DEV),
                           torch.tensor(tlens, dtype=torch.int32, device=DEV), durs, sigma=0.05,
                           reduction="none").double().cpu().numpy()
    for b in range(len(llens)):
        if np.isinf(cost[b]):
            assert sc[b] == -np.inf
        else:
            assert np.isfinite(sc[b]) and sc[b] <= -cost[b] + 1e-5 * abs(cost[b]) + 1e-4


def test_null_blank_jumps():
    durs = D04
    logits, targets, llens, tlens = random_case(len(durs), 5)
    with_jumps = align(logits, targets, llens, tlens, durs)
    without = align(logits, targets, llens, tlens, durs, jumps=False)
    for x, y in zip(without, with_jumps):
        assert np.array_equal(x, y)


def test_frame_tokens_read_the_label_frames():
    import wenet_celoss_amd as w
    durs = D04
    llens, tlens = [30, 17], [9, 4]
    logits, targets, pf, _, _, _ = planted_case(2, 30, 10, 24, durs, llens, tlens, seed=3)
    fr = align(logits, targets, llens, tlens, durs)[0]
    per = w.rnnt_frame_tokens(torch.as_tensor(fr), torch.as_tensor(targets), torch.tensor(llens), torch.tensor(tlens))
    for b in range(2):
        assert len(per[b]) == llens[b] and [k for f in per[b] for k in f] == targets[b, :tlens[b]].tolist()
        assert all(targets[b, u] in per[b][pf[b, u]] for u in range(tlens[b]))
