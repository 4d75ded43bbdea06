"""Host logic of the memory-bounded joiner + RNN-T loss node (joint_rnnt_loss(..., logits_budget=n)): the slicer
`plan_slices` on ragged length sets, and the argument checks that run before any launch.  No GPU needed."""
import numpy as np
import pytest
import torch

from wenet_celoss_amd.fused import Slice, plan_slices

V = 5000


def covered(slices, t_lens, T, U1):
    """(b, t) -> how many slices hold it as a valid frame, plus every frame a slice holds past its utterance's end."""
    count = np.zeros((len(t_lens), T), np.int64)
    padded = []
    for s in slices:
        assert 0 <= s.b0 < s.b1 <= len(t_lens) and 0 <= s.t0 < s.t1 <= T
        if s.b1 - s.b0 > 1 or (s.t0, s.t1) == (0, T):
            assert (s.t0, s.t1) == (0, T), s            # a run of whole utterances spans every frame of them
        for b in range(s.b0, s.b1):
            for t in range(s.t0, s.t1):
                if t < t_lens[b]:
                    count[b, t] += 1
                else:
                    padded.append((s, b, t))
    return count, padded


CASES = [  # t_lens, T, U1, budget in frame rows
    ([1000, 700, 1000, 3, 0, 512], 1000, 151, 355.4),     # BASELINE-like with 1 GiB at V = 5000: frame slices
    ([10, 7, 10, 3, 0, 5, 10, 10], 10, 6, 25),            # two whole utterances per run
    ([10, 7, 10, 3, 0, 5, 10, 10], 10, 6, 10),            # exactly one utterance per run
    ([10, 7, 10, 3, 0, 5, 10, 10], 10, 6, 9.99),          # one frame short of a whole utterance: frame slices
    ([10, 7, 10, 3, 0, 5, 10, 10], 10, 6, 1),             # the one-row minimum
    ([10, 7, 10, 3, 0, 5, 10, 10], 10, 6, 3.7),           # not a multiple of a row
    ([0, 0, 4], 4, 1, 2),                                 # U = 0, empty utterances
    ([4, 4, 4, 4], 4, 3, 1000),                           # everything in one slice
]


@pytest.mark.parametrize("t_lens,T,U1,rows", CASES)
def test_every_valid_cell_once_within_budget(t_lens, T, U1, rows):
    budget = int(rows * U1 * V * 4)
    slices = plan_slices(t_lens, [U1 - 1] * len(t_lens), T, U1, V, budget)
    assert all(isinstance(s, Slice) for s in slices)
    count, padded = covered(slices, t_lens, T, U1)
    for b, tb in enumerate(t_lens):
        assert (count[b, :tb] == 1).all(), (b, count[b])
    for s, b, t in padded:                                  # padded frames only ever sit inside whole-utterance runs
        assert (s.t0, s.t1) == (0, T) and s.cells(U1) <= budget // (4 * V)
    for s in slices:
        assert s.cells(U1) * V * 4 <= budget, s
        if s.b1 - s.b0 == 1 and (s.t0, s.t1) != (0, T):     # a frame range never reaches past its utterance
            assert s.t1 <= t_lens[s.b0]
    # the order is fixed: utterances ascending, frames ascending
    keys = [(s.b0, s.t0) for s in slices]
    assert keys == sorted(keys)


def test_whole_utterances_packed_while_they_fit():
    t_lens, T, U1 = [10, 9, 10, 8, 10], 10, 6
    whole = T * U1 * V * 4
    assert plan_slices(t_lens, [5] * 5, T, U1, V, 2 * whole + 17) == [Slice(0, 2, 0, T), Slice(2, 4, 0, T), Slice(4, 5, 0, T)]
    assert plan_slices(t_lens, [5] * 5, T, U1, V, 5 * whole) == [Slice(0, 5, 0, T)]
    assert plan_slices(t_lens, [5] * 5, T, U1, V, whole) == [Slice(b, b + 1, 0, T) for b in range(5)]
    # an empty utterance closes the run and gets no slice
    assert plan_slices([10, 0, 10], [5] * 3, T, U1, V, 3 * whole) == [Slice(0, 1, 0, T), Slice(2, 3, 0, T)]


def test_over_budget_utterance_split_by_frames():
    T, U1 = 1000, 151
    budget = 1 << 30                                      # 355 frame rows at V = 5000
    slices = plan_slices([1000, 290], [150, 150], T, U1, V, budget)
    assert slices == [Slice(0, 1, 0, 355), Slice(0, 1, 355, 710), Slice(0, 1, 710, 1000), Slice(1, 2, 0, 290)]
    # the last range stops at the utterance's length, not at T
    assert plan_slices([400], [150], T, U1, V, budget) == [Slice(0, 1, 0, 355), Slice(0, 1, 355, 400)]


def test_budget_below_one_row_is_refused():
    U1 = 151
    row = U1 * V * 4
    assert plan_slices([3], [150], 3, U1, V, row) == [Slice(0, 1, 0, 1), Slice(0, 1, 1, 2), Slice(0, 1, 2, 3)]
    with pytest.raises(ValueError, match=str(row)):
        plan_slices([3], [150], 3, U1, V, row - 1)
    with pytest.raises(ValueError, match="frame row"):
        plan_slices([3], [150], 3, U1, V, 0)


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_sixteen_bit_modes_refused_with_a_budget(precision):
    import wenet_celoss_amd as w_
    B, T, U, J, Vs = 2, 5, 3, 8, 16
    args = (torch.zeros(B, T, J), torch.zeros(B, U + 1, J), torch.zeros(Vs, J), torch.zeros(Vs),
            torch.ones(B, U, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32), torch.full((B,), U, dtype=torch.int32))
    with pytest.raises(ValueError, match="AMP single-term mode"):
        w_.joint_rnnt_loss(*args, precision=precision, logits_budget=1 << 30)


def test_bad_budget_fails_before_any_launch():
    """The budget is checked on the host, right after the node's length sync: a CPU tensor never reaches a kernel."""
    import wenet_celoss_amd as w_
    B, T, U, J, Vs = 2, 5, 3, 8, 16
    args = (torch.zeros(B, T, J), torch.zeros(B, U + 1, J), torch.zeros(Vs, J), torch.zeros(Vs),
            torch.ones(B, U, dtype=torch.int32), torch.full((B,), T, dtype=torch.int32), torch.full((B,), U, dtype=torch.int32))
    with pytest.raises(ValueError, match=str((U + 1) * Vs * 4)):
        w_.joint_rnnt_loss(*args, logits_budget=(U + 1) * Vs * 4 - 1)
