"""RNN-T forced alignment without a GPU: the float64 reference against brute force (random and exactly tied lattices),
the per-frame token helper on hand-written cases, and the argument checks of the two C entry points and of the Python
functions, which all refuse before anything is launched."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_align_ref as ref


@pytest.mark.parametrize("T,U", [(1, 0), (1, 3), (4, 0), (3, 2), (5, 3), (6, 4), (4, 6)])
def test_reference_matches_brute_force(T, U):
    rng = np.random.default_rng(T * 10 + U)
    for _ in range(5):
        blank_lp = -rng.exponential(size=(T, U + 1))
        emit_lp = -rng.exponential(size=(T, U))
        score, frames, _ = ref.viterbi(blank_lp, emit_lp, T, U)
        best, arg = ref.brute_force(blank_lp, emit_lp, T, U)
        assert score == pytest.approx(best, abs=1e-12)
        assert len(arg) == 1 and tuple(frames) == arg[0]
        assert ref.path_score(blank_lp, emit_lp, T, U, frames) == pytest.approx(best, abs=1e-12)


@pytest.mark.parametrize("T,U", [(3, 2), (5, 3), (4, 4), (6, 2)])
def test_reference_with_exact_ties(T, U):
    """Small integers make many paths tie exactly: the reference's path is one of brute force's best paths and its
    score is exact; with every log-probability equal the tie rule emits every label at the first frame."""
    rng = np.random.default_rng(7 + T + U)
    for _ in range(8):
        blank_lp = -rng.integers(0, 3, size=(T, U + 1)).astype(np.float64)
        emit_lp = -rng.integers(0, 3, size=(T, U)).astype(np.float64)
        score, frames, margin = ref.viterbi(blank_lp, emit_lp, T, U)
        best, arg = ref.brute_force(blank_lp, emit_lp, T, U)
        assert score == best
        assert tuple(frames) in arg
        if len(arg) > 1:
            assert margin == 0.0
    score, frames, _ = ref.viterbi(np.zeros((T, U + 1)), np.zeros((T, U)), T, U)
    assert score == 0.0 and list(frames) == [0] * U


def test_reference_nan_gives_nan_score_and_a_valid_path():
    T, U = 5, 3
    rng = np.random.default_rng(3)
    blank_lp = -rng.exponential(size=(T, U + 1))
    emit_lp = -rng.exponential(size=(T, U))
    blank_lp[1, 1] = np.nan
    score, frames, _ = ref.viterbi(blank_lp, emit_lp, T, U)
    assert np.isnan(score)
    assert ref.is_valid_path(np.concatenate([frames, [-1]]), T, U, U + 1)


def test_lattice_log_probs_follow_log_softmax():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(3, 3, 6))
    y = [4, 1]
    b, e = ref.lattice_log_probs(x, y, blank=5)
    lp = torch.log_softmax(torch.tensor(x), -1).numpy()
    np.testing.assert_allclose(b, lp[:, :, 5], rtol=1e-12)
    np.testing.assert_allclose(e[:, 0], lp[:, 0, 4], rtol=1e-12)
    np.testing.assert_allclose(e[:, 1], lp[:, 1, 1], rtol=1e-12)


def test_frame_tokens_hand_written():
    from wenet_celoss_amd import rnnt_frame_tokens
    frames = torch.tensor([[-1, -1, -1], [0, 0, 2], [1, 3, 3]], dtype=torch.int32)
    targets = torch.tensor([[0, 0, 0], [7, 8, 9], [4, 5, 6]])
    out = rnnt_frame_tokens(frames, targets, torch.tensor([2, 3, 4]), torch.tensor([0, 3, 3]))
    assert out == [
        [[], []],                       # U = 0: blanks only
        [[7, 8], [], [9]],              # two labels in one frame, one in the last frame
        [[], [4], [], [5, 6]],          # two labels in the last frame
    ]


def _null():
    return ctypes.c_void_p(None)


def _dummy():
    return ctypes.c_void_p(256)        # never dereferenced: every case below is refused before a launch


@pytest.fixture(scope="module")
def lib():
    from wenet_celoss_amd import _lib
    return _lib.load()


def test_align_entry_point_rejects_bad_arguments(lib):
    d, n = _dummy(), _null()
    big = 1 << 40
    args = lambda **k: [k.get("logits", d), 0, k.get("targets", d), k.get("ll", d), k.get("tl", d), k.get("B", 2), 4,
                        k.get("U1", 3), 8, k.get("blank", 0), k.get("frames", d), k.get("scores", d), k.get("ws", d),
                        big, n]
    for k in ("logits", "targets", "ll", "tl", "frames", "scores", "ws"):
        assert lib.wr_rnnt_align(*args(**{k: n})) == -1, k
        assert b"null" in lib.wr_last_error()
    assert lib.wr_rnnt_align(*args(U1=1025)) == -2 and b"1024" in lib.wr_last_error()
    assert lib.wr_rnnt_align(*args(blank=8)) == -1 and b"blank" in lib.wr_last_error()
    assert lib.wr_rnnt_align(*args(blank=-1)) == -1 and b"blank" in lib.wr_last_error()
    assert lib.wr_rnnt_align(*args(B=0)) == -1
    assert lib.wr_rnnt_align(*args(B=-3)) == -1
    a = args()
    a[1] = 7
    assert lib.wr_rnnt_align(*a) == -1 and b"dtype" in lib.wr_last_error()
    a = args()
    a[13] = 16
    assert lib.wr_rnnt_align(*a) == -3


def test_align_from_stats_entry_point_rejects_bad_arguments(lib):
    d, n = _dummy(), _null()
    big = 1 << 40
    args = lambda **k: [k.get("targets", d), k.get("ll", d), k.get("tl", d), k.get("B", 2), 4, k.get("U1", 3),
                        k.get("frames", d), k.get("scores", d), k.get("ws", d), k.get("wsb", big), n]
    for k in ("targets", "ll", "tl", "frames", "scores", "ws"):
        assert lib.wr_rnnt_align_from_stats(*args(**{k: n})) == -1, k
        assert b"null" in lib.wr_last_error()
    assert lib.wr_rnnt_align_from_stats(*args(U1=1025)) == -2 and b"1024" in lib.wr_last_error()
    assert lib.wr_rnnt_align_from_stats(*args(B=0)) == -1
    assert lib.wr_rnnt_align_from_stats(*args(wsb=16)) == -3 and b"workspace" in lib.wr_last_error()
    # blank is not an argument of this entry point: the statistics were taken with it (wr_joint_rnnt_stats checks it)
    from wenet_celoss_amd import _lib
    assert len(_lib.SIGNATURES["wr_rnnt_align_from_stats"][1]) == 11


def _small():
    B, T, U, V = 2, 5, 3, 7
    logits = torch.randn(B, T, U + 1, V)
    targets = torch.randint(1, V, (B, U), dtype=torch.int32)
    return logits, targets, torch.tensor([5, 3], dtype=torch.int32), torch.tensor([3, 1], dtype=torch.int32)


def test_python_functions_refuse_cpu_tensors():
    import wenet_celoss_amd as w
    logits, targets, ll, tl = _small()
    with pytest.raises(RuntimeError, match="HIP device"):
        w.rnnt_forced_align(logits, targets, ll, tl)
    ep, pp = torch.randn(2, 5, 8), torch.randn(2, 4, 8)
    with pytest.raises(RuntimeError, match="HIP device"):
        w.joint_rnnt_forced_align(ep, pp, torch.randn(7, 8), torch.randn(7), targets, ll, tl, precision="fp32")


def test_python_functions_refuse_bad_lengths_and_blank():
    import wenet_celoss_amd as w
    logits, targets, ll, tl = _small()
    with pytest.raises(ValueError, match="logit_lengths"):
        w.rnnt_forced_align(logits, targets, torch.tensor([5, 0], dtype=torch.int32), tl)
    with pytest.raises(ValueError, match="logit_lengths"):
        w.rnnt_forced_align(logits, targets, torch.tensor([6, 3], dtype=torch.int32), tl)
    with pytest.raises(ValueError, match="target_lengths"):
        w.rnnt_forced_align(logits, targets, ll, torch.tensor([4, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="blank"):
        w.rnnt_forced_align(logits, targets, ll, tl, blank=7)
    bad = targets.clone()
    bad[0, 1] = -1                                   # inside target_lengths[0] = 3
    with pytest.raises(ValueError, match="label"):
        w.rnnt_forced_align(logits, bad, ll, tl)
    ep, pp = torch.randn(2, 5, 8), torch.randn(2, 4, 8)
    with pytest.raises(ValueError, match="logit_lengths"):
        w.joint_rnnt_forced_align(ep, pp, torch.randn(7, 8), torch.randn(7), targets,
                                  torch.tensor([0, 3], dtype=torch.int32), tl)


@pytest.mark.parametrize("precision", ["bf16", "f16"])
def test_joint_form_refuses_16bit_precisions(precision):
    import wenet_celoss_amd as w
    logits, targets, ll, tl = _small()
    ep, pp = torch.randn(2, 5, 8), torch.randn(2, 4, 8)
    with pytest.raises(ValueError, match="logits form"):
        w.joint_rnnt_forced_align(ep, pp, torch.randn(7, 8), torch.randn(7), targets, ll, tl, precision=precision)
