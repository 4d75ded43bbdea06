"""CPU self-tests of the float64 step functions (oracle/decode_oracle.py) and of the guided walker
(tests/decode_follow.py) that test_decode_follow_gpu.py runs against the HIP decoders: the unguided float64 steps
reproduce the reference's fixtures, the walker accepts the fp32 oracle's own trajectory and rejects corrupted ones for
the reason that was planted."""
import glob
import math
import os

import numpy as np
import pytest

from oracle import decode_oracle as do
from conftest import GOLDEN
import decode_follow as fw


def names(pattern):
    return sorted(glob.glob(os.path.join(GOLDEN, pattern)))


def sub(d, prefix):
    return {k[len(prefix):]: d[k] for k in d.files if k.startswith(prefix)}


@pytest.mark.parametrize("path", names("prefix_beam_*.npz"), ids=os.path.basename)
def test_prefix_beam_step_f64_chained_reproduces_reference(path):
    d = np.load(path)
    trie, joint = do.PredictorTrie64(sub(d, "pred_"), int(d["n_layers"])), do.Joint64(sub(d, "joint_"))
    T, B = int(d["T"]), int(d["beam"])
    enc = d["enc"][0]
    lp, le = do.ctc_log_softmax_f64(sub(d, "ctc_"), enc[:T])
    beam = [((0,), 0.0)]
    for i in range(T):
        mix, err = do.prefix_beam_rows_f64(trie, joint, enc[i], lp[i], le[i], [h for h, _ in beam],
                                           float(d["transducer_weight"]), float(d["ctc_weight"]))
        fused, gaps = do.prefix_beam_step_f64(beam, mix, err, B)
        assert gaps.shape == (len(beam),) and np.all(gaps >= 0)
        beam = [(c["hyp"], c["score"]) for c in fused[:B]]
    assert [list(h) for h, _ in beam] == [list(d["hyps"][k][:d["hyp_lens"][k]]) for k in range(len(d["scores"]))]
    np.testing.assert_allclose([s for _, s in beam], d["scores"], rtol=1e-5)


@pytest.mark.parametrize("path", names("greedy_core_*.npz"), ids=os.path.basename)
def test_greedy_frame_f64_reproduces_reference(path):
    d = np.load(path)
    trie, joint = do.PredictorTrie64(sub(d, "pred_"), int(d["n_layers"])), do.Joint64(sub(d, "joint_"))
    T, n_steps = int(d["T"]), int(d["n_steps"])
    hyp = []
    for t in range(T):                     # follow the float64 argmax frame by frame
        em = []
        while len(em) < n_steps:
            lp, _ = do.greedy_frame_f64(trie, joint, d["enc"][0][t], hyp, em)[-1]
            k = int(lp.argmax())
            if k == 0:
                break
            em.append(k)
        hyp += em
    assert hyp == list(d["hyp"])


# ----------------------------------------------------------------------------------------- the walker itself --
def small_model(seed, V=40, E=12, D=10, H=16, P=12, J=24, L=2):
    rng = np.random.default_rng(seed)
    u = lambda *s, a=0.25: rng.uniform(-a, a, s).astype(np.float32)
    pw = {"embed.weight": u(V, D, a=1.0), "projection.weight": u(P, H), "projection.bias": u(P)}
    for l in range(L):
        pw[f"rnn.weight_ih_l{l}"] = u(4 * H, D if l == 0 else H)
        pw[f"rnn.weight_hh_l{l}"] = u(4 * H, H)
        pw[f"rnn.bias_ih_l{l}"], pw[f"rnn.bias_hh_l{l}"] = u(4 * H), u(4 * H)
    jw = {"enc_ffn.weight": u(J, E), "enc_ffn.bias": u(J), "pred_ffn.weight": u(J, P), "pred_ffn.bias": u(J),
          "ffn_out.weight": u(V, J, a=1.0), "ffn_out.bias": u(V)}
    jw["ffn_out.bias"][0] += 2.0
    cw = {"ctc_lo.weight": u(V, E, a=1.0), "ctc_lo.bias": u(V)}
    cw["ctc_lo.bias"][0] += 2.0
    enc = rng.normal(size=(64, E)).astype(np.float32)
    return pw, jw, cw, enc, L


BEAM_T, BEAM_SIZE = 60, 4


@pytest.fixture(scope="module")
def beam_case():
    pw, jw, cw, enc, L = small_model(1)
    p, j = do.Predictor(pw, L), do.Joint(jw)
    states = [[((0,), 0.0)]]
    for f in range(1, BEAM_T + 1):       # the fp32 oracle's trajectory: its beam after f frames, for every f
        res = do.prefix_beam_search(p, j, cw, enc, f, beam_size=BEAM_SIZE)
        states.append([(tuple(s["hyp"]), s["score"]) for s in res])
    lp, le = do.ctc_log_softmax_f64(cw, enc[:BEAM_T])
    return dict(pw=pw, jw=jw, L=L, enc=enc, lp=lp, le=le, states=states)


def walk(case, states):
    trie, joint = do.PredictorTrie64(case["pw"], case["L"]), do.Joint64(case["jw"])
    return fw.walk_beam(trie, joint, case["lp"], case["le"], case["enc"], states, BEAM_SIZE, 0.7, 0.3, name="small")


def test_walker_accepts_the_fp32_oracle_trajectory(beam_case):
    st = walk(beam_case, beam_case["states"])
    print(st.report(BEAM_T))
    assert st.frames == BEAM_T
    assert st.worst < 0.5
    st.check_ties()
    assert len(beam_case["states"][-1][0][0]) > 5          # the trajectory emits


def corrupt(states, f, fn):
    out = [list(s) for s in states]
    out[f] = fn(list(out[f]))
    return out


def test_walker_rejects_a_moved_score(beam_case):
    f = BEAM_T // 2
    bad = corrupt(beam_case["states"], f, lambda s: [(s[0][0], s[0][1])] + [(s[1][0], s[1][1] + 1e-3)] + s[2:])
    with pytest.raises(fw.WalkError, match=rf"frame {f - 1} \(.*\): .*survivor 1 .*\|diff\| 0\.001"):
        walk(beam_case, bad)


def test_walker_rejects_a_survivor_that_is_not_a_candidate(beam_case):
    f = BEAM_T // 3
    bad = corrupt(beam_case["states"], f, lambda s: s[:2] + [(s[2][0] + (7, 7), s[2][1])] + s[3:])
    with pytest.raises(fw.WalkError, match=rf"frame {f - 1} \(.*\): .*survivor 2 .*not a candidate"):
        walk(beam_case, bad)


def test_walker_rejects_two_survivors_fused_that_are_not_the_same_hypothesis(beam_case):
    f = 2 * BEAM_T // 3
    s = beam_case["states"][f]

    def fuse(s):
        # survivors 0 and 1 merged into one class (score log_add of both), the beam refilled from the next frame's
        # runner-up so that only the fusion is wrong
        merged = (s[0][0], do.log_add([s[0][1], s[1][1]]))
        rest = s[2:]
        return [merged] + rest + [(s[-1][0] + (3,), s[-1][1] - 5.0)][:BEAM_SIZE - 1 - len(rest)]
    bad = corrupt(beam_case["states"], f, fuse)
    with pytest.raises(fw.WalkError, match=rf"frame {f - 1} \(.*\): "):
        walk(beam_case, bad)
    with pytest.raises(fw.WalkError, match=r"survivor 0 .*score"):
        walk(beam_case, bad[:f + 1])


GREEDY_T, N_STEPS = 60, 3


@pytest.fixture(scope="module")
def greedy_case():
    pw, jw, _, enc, L = small_model(2)
    jw = dict(jw)
    jw["ffn_out.bias"] = jw["ffn_out.bias"].copy()
    jw["ffn_out.bias"][0] -= 1.0                           # emit often, hit the cap on some frames
    p, j = do.Predictor(pw, L), do.Joint(jw)
    states = [do.greedy_search(p, j, enc, f, n_steps=N_STEPS) for f in range(GREEDY_T + 1)]
    return dict(pw=pw, jw=jw, L=L, enc=enc, states=states)


def gwalk(case, states):
    trie, joint = do.PredictorTrie64(case["pw"], case["L"]), do.Joint64(case["jw"])
    return fw.walk_greedy(trie, joint, case["enc"], states, N_STEPS, name="small greedy")


def test_greedy_walker_accepts_the_fp32_oracle_trajectory(greedy_case):
    st = gwalk(greedy_case, greedy_case["states"])
    print(st.report(GREEDY_T))
    assert st.frames == GREEDY_T
    st.check_ties()
    per_frame = [len(b) - len(a) for a, b in zip(greedy_case["states"][:-1], greedy_case["states"][1:])]
    assert max(per_frame) == N_STEPS and min(per_frame) == 0          # the cap and blank frames are both walked


def test_greedy_walker_rejects_a_swapped_token_at_a_clear_decision(greedy_case):
    trie, joint = do.PredictorTrie64(greedy_case["pw"], greedy_case["L"]), do.Joint64(greedy_case["jw"])
    states = greedy_case["states"]
    for f in range(GREEDY_T // 2, GREEDY_T):               # the first frame past the middle that emits clearly
        cur, nxt = states[f], states[f + 1]
        if len(nxt) > len(cur):
            lp, err = do.greedy_frame_f64(trie, joint, greedy_case["enc"][f], cur, [])[0]
            top2 = np.sort(lp)[-2:]
            if top2[1] - top2[0] > 100 * (err.max() * 2):
                break
    else:
        pytest.fail("no clear emitting frame")
    k = states[f + 1][len(cur)]
    other = int(np.argsort(lp)[-2])
    swapped = [s if g <= f else s[:len(cur)] + [other] + s[len(cur) + 1:] for g, s in enumerate(states)]
    assert swapped[f + 1][len(cur)] != k
    with pytest.raises(fw.WalkError, match=rf"frame {f} decision 0: took {other} .*float64 argmax {k}"):
        gwalk(greedy_case, swapped)


def test_greedy_walker_rejects_more_emissions_than_n_steps(greedy_case):
    states = [list(s) for s in greedy_case["states"]]
    f = next(q for q in range(GREEDY_T) if len(states[q + 1]) - len(states[q]) == N_STEPS)
    bad = [s if g <= f else s[:len(states[f + 1])] + [5] + s[len(states[f + 1]):] for g, s in enumerate(states)]
    with pytest.raises(fw.WalkError, match=rf"frame {f}: {N_STEPS + 1} emissions"):
        gwalk(greedy_case, bad)
