"""The float64 TDT greedy reference (tests/tdt_greedy_ref.py) on scripted joiner rows with hand-worked answers.  No GPU."""
import numpy as np
import pytest

import tdt_greedy_ref as ref

V, DUR = 4, (0, 1, 2)


def row(k, j, second=-1.0):
    """Logits with token k and duration index j on top by 1.0 (every other column at `second`)."""
    r = np.full(V + len(DUR), second)
    r[k], r[V + j] = second + 1.0, second + 1.0
    return r


def run(table, T, n_steps=2):
    return ref.walk(ref.Scripted(table), T, V, DUR, blank=0, n_steps=n_steps)


def test_a_blank_with_duration_zero_advances_one_frame():
    r = run({(0, 0): row(0, 0), (1, 0): row(0, 1)}, T=2)
    assert r.tokens == [] and r.frames == []
    assert r.trace == [(0, 0, 0), (1, 0, 1)] and r.end == 2


def test_a_blank_with_duration_two_skips_a_frame():
    # the row of frame 1 is not in the table: consulting it would raise
    r = run({(0, 0): row(0, 2), (2, 0): row(3, 1), (3, 1): row(0, 1)}, T=4)
    assert r.tokens == [3] and r.frames == [2]
    assert r.trace == [(0, 0, 2), (2, 3, 1), (3, 0, 1)]


def test_labels_with_duration_zero_repeat_until_the_n_steps_rule_moves_on():
    r = run({(0, 0): row(1, 0), (0, 1): row(2, 0), (1, 2): row(0, 1)}, T=2, n_steps=2)
    assert r.tokens == [1, 2] and r.frames == [0, 0]
    assert r.trace == [(0, 1, 0), (0, 2, 0), (1, 0, 1)]
    # with n_steps = 3 the third decision is still taken on frame 0
    r3 = run({(0, 0): row(1, 0), (0, 1): row(2, 0), (0, 2): row(3, 0), (1, 3): row(0, 1)}, T=2, n_steps=3)
    assert r3.tokens == [1, 2, 3] and r3.frames == [0, 0, 0]


def test_a_label_with_a_positive_duration_resets_the_counter():
    # label d=0 (counter 1), label d=1 (counter 0, frame 1), label d=0 (counter 1), label d=0 (counter 2 -> frame 2).
    # A counter that the second label did not reset would leave frame 1 after the third label and drop the fourth.
    table = {(0, 0): row(1, 0), (0, 1): row(2, 1), (1, 2): row(3, 0), (1, 3): row(1, 0)}
    r = run(table, T=2, n_steps=2)
    assert r.tokens == [1, 2, 3, 1] and r.frames == [0, 0, 1, 1] and r.end == 2


def test_a_blank_resets_the_counter_too():
    table = {(0, 0): row(1, 0), (0, 1): row(0, 0), (1, 1): row(2, 0), (1, 2): row(3, 0)}
    r = run(table, T=2, n_steps=2)
    assert r.tokens == [1, 2, 3] and r.frames == [0, 1, 1] and r.end == 2


def test_a_jump_past_the_end_ends_the_utterance():
    r = run({(0, 0): row(0, 1), (1, 0): row(0, 2)}, T=2)
    assert r.tokens == [] and r.end == 3
    # a label decided on the last frame is emitted whatever its jump
    r = run({(0, 0): row(0, 1), (1, 0): row(2, 2)}, T=2)
    assert r.tokens == [2] and r.frames == [1] and r.end == 3
    r = run({}, T=0)
    assert r.tokens == [] and r.trace == [] and r.gap == float("inf")


def test_frames_are_those_of_the_decisions():
    table = {(0, 0): row(0, 2), (2, 0): row(1, 0), (2, 1): row(2, 2), (4, 2): row(0, 0), (5, 2): row(3, 1)}
    r = run(table, T=6, n_steps=3)
    assert r.tokens == [1, 2, 3] and r.frames == [2, 2, 5]
    assert [t for t, k, _ in r.trace if k != 0] == r.frames


def test_exact_ties_go_to_the_lowest_index_and_the_gap_is_the_smallest_margin():
    a = row(2, 1)
    a[3] = a[2]                                    # token 3 ties token 2
    a[V + 2] = a[V + 1]                            # duration index 2 ties index 1
    r = run({(0, 0): a, (1, 1): row(0, 1)}, T=2)
    assert r.tokens == [2] and r.trace[0] == (0, 2, 1) and r.gap == 0.0
    r = ref.walk(ref.Scripted({(0, 0): a, (1, 1): row(0, 1)}), 2, V, DUR, n_steps=2, dup={3: 2, V + 2: V + 1})
    assert r.tokens == [2] and r.gap == 1.0
    b = row(0, 1)
    b[1] = b[0] - 0.25                             # the token margin of this row
    assert run({(0, 0): b}, T=1).gap == 0.25


def test_the_plain_rule_reads_the_whole_row_as_tokens():
    def hot(k):
        r = np.full(V + len(DUR), -1.0)
        r[k] = 0.0
        return r

    rows = {(0, 0): hot(V + 1), (0, 1): hot(0), (1, 1): hot(2), (1, 2): hot(3)}
    r = ref.walk(ref.Scripted(rows), 2, V, None, blank=0, n_steps=2)
    assert r.tokens == [V + 1, 2, 3] and r.frames == [0, 1, 1] and r.end == 2


def test_a_row_of_the_wrong_width_is_refused():
    with pytest.raises(AssertionError):
        run({(0, 0): np.zeros(V + 1)}, T=1)
