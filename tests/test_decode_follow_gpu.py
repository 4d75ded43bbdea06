"""Transducer decoding checked at every frame against a float64 step (tests/decode_follow.py).

Decoding an utterance truncated to f frames gives the HIP search's own state after frame f (a beam survivor is its
(hyp, score), a greedy stream its token list), so one call per group of lengths yields every frame boundary of an
utterance; the walker starts a float64 step from the search's state at f and checks that it reaches the search's state
at f + 1, following the search through near-ties instead of stopping at the first one.  Each copy of an utterance is
one set of lanes of a DeviceDecoder call (at most 1024 lanes); consecutive groups of lengths overlap by one, so lengths
f and f + 1 always come from the same call."""
import time

import numpy as np
import pytest
import torch

from oracle import decode_oracle as do
import decode_follow as fw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CTC_BYTES = 2 << 30           # the (copies, T, V) CTC log-probs of one call (expanded views are copied by the decoder)


def np_state(m):
    return {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}


def length_groups(L, per_call, T_bytes):
    """[a, b] ranges of lengths 1..L; consecutive ranges share their end point."""
    out, a = [], 1
    while True:
        n = per_call
        while n > 2 and (a + n - 1) * T_bytes * n > CTC_BYTES:
            n -= 1
        b = min(L, a + n - 1)
        out.append((a, b))
        if b == L:
            return out
        a = b


def beam_truncations(dec, enc_d, ctc_d, L, beam, tw, cw, blank=0):
    """Per call, the search's beams after f frames for every f of the call's group: [(a, [state_a .. state_b])]."""
    V = ctc_d.shape[-1]
    calls = []
    for a, b in length_groups(L, 1024 // beam, V * 4):
        n = b - a + 1
        lens = torch.arange(a, b + 1, dtype=torch.int32)
        e = enc_d[None, :b].expand(n, b, enc_d.shape[-1])
        c = ctc_d[None, :b].expand(n, b, V)
        res = dec.prefix_beam(e, lens, c, beam, cw, tw, blank)
        calls.append((a, [[(tuple(h), s) for h, s in r] for r in res]))
    return calls


def walk_utterance(trie, joint, cwn, enc, calls, beam, tw, cw, blank, name):
    lp, le = do.ctc_log_softmax_f64(cwn, enc)
    st = fw.Stats(name)
    init = [((blank,), 0.0)]
    for a, states in calls:
        seq = ([init] + states) if a == 1 else states
        st.merge(fw.walk_beam(trie, joint, lp, le, enc, seq, beam, tw, cw, blank, name, frame0=0 if a == 1 else a))
    return st


def beam_model(seed, V, E, P, J, H, L, blank=0, scale=True):
    import wenet_celoss_amd as w
    torch.manual_seed(seed)
    pred = w.RNNPredictor(V, P, P, 0.1, H, L).eval()
    joint = w.TransducerJoint(V, E, P, J).eval()
    ctc = w.CTC(V, E).eval()
    if scale:
        with torch.no_grad():
            joint.ffn_out.weight *= 10
            joint.ffn_out.bias[blank] += 13
            ctc.ctc_lo.weight *= 10
            ctc.ctc_lo.bias[blank] += 13
    return pred, joint, ctc


# --------------------------------------------------------------------------------------------- config 5 --
C5_LENS = [1500, 1500, 1000, 700, 400, 250, 150, 120, 100, 90, 80, 70, 60, 50, 40, 30]


@pytest.fixture(scope="module")
def config5():
    """The model, encoder output and full-call result of test_decode_gpu.py::test_config5_full_shape_prefix_beam_
    matches_oracle (same seed, same order of draws), and every truncation of every utterance."""
    from wenet_celoss_amd.decoder import DeviceDecoder
    t0 = time.time()
    V, E, P, J, H, L, B, T, beam = 5000, 256, 256, 512, 256, 2, 16, 1500, 8
    pred, joint, ctc = beam_model(0, V, E, P, J, H, L)
    enc = torch.randn(B, T, E)
    pw, jw, cwn = np_state(pred), np_state(joint), np_state(ctc)
    pred, joint, ctc = pred.to(DEV), joint.to(DEV), ctc.to(DEV)
    enc_d = enc.to(DEV)
    dec = DeviceDecoder(pred, joint, max_lanes=1024, max_utt=1024 // beam, tmax=T, max_hyp=0, max_beam=16)
    with torch.no_grad():
        ctc_d = ctc.log_softmax(enc_d)
    full = dec.prefix_beam(enc_d, torch.tensor(C5_LENS, dtype=torch.int32), ctc_d, beam, 0.3, 0.7, 0)
    trunc = [beam_truncations(dec, enc_d[i], ctc_d[i], C5_LENS[i], beam, 0.7, 0.3) for i in range(B)]
    torch.cuda.synchronize()
    print(f"config 5 truncation runs: {time.time() - t0:.1f} s")
    return dict(pw=pw, jw=jw, cwn=cwn, L=L, enc=enc.numpy(), dec=dec, enc_d=enc_d, ctc_d=ctc_d, full=full,
                trunc=trunc, beam=beam)


def test_truncation_premise_copies_identical_and_last_equals_full(config5):
    """Inside one call two copies of the same (utterance, length) in different slots give bit-identical hyps and
    scores, and the truncation to an utterance's whole length is the utterance's result in the full batch."""
    c = config5
    beam = c["beam"]
    lens = [37, 300, 1, 37, 300, 1, 299, 5]
    order = torch.tensor([0, 1, 2, 0, 1, 2, 1, 0])
    enc = c["enc_d"][order, :300].contiguous()
    ctc = c["ctc_d"][order, :300].contiguous()
    res = c["dec"].prefix_beam(enc, torch.tensor(lens, dtype=torch.int32), ctc, beam, 0.3, 0.7, 0)
    for p, q in [(0, 3), (1, 4), (2, 5)]:
        assert order[p] == order[q] and lens[p] == lens[q]
        assert [h for h, _ in res[p]] == [h for h, _ in res[q]], (p, q)
        assert [s for _, s in res[p]] == [s for _, s in res[q]], (p, q)       # bit-identical float64
    for i in range(len(C5_LENS)):
        a, states = c["trunc"][i][-1]
        last = states[-1]
        assert [list(h) for h, _ in last] == [h for h, _ in c["full"][i]], i
        np.testing.assert_allclose([s for _, s in last], [s for _, s in c["full"][i]], rtol=1e-6)
        # the length shared by two consecutive calls decodes to the same beam in both
        for (a0, s0), (a1, s1) in zip(c["trunc"][i][:-1], c["trunc"][i][1:]):
            assert [h for h, _ in s0[-1]] == [h for h, _ in s1[0]], (i, a1)
            np.testing.assert_allclose([s for _, s in s0[-1]], [s for _, s in s1[0]], rtol=1e-6)


def test_config5_prefix_beam_every_frame(config5):
    """BASELINE config 5 (B = 16, beam 8, V = 5000, weights (0.3, 0.7)): every frame of every utterance walked."""
    c = config5
    t0 = time.time()
    tot = fw.Stats("config 5")
    for i in range(len(C5_LENS)):
        trie, joint = do.PredictorTrie64(c["pw"], c["L"]), do.Joint64(c["jw"])
        st = walk_utterance(trie, joint, c["cwn"], c["enc"][i, :C5_LENS[i]], c["trunc"][i], c["beam"], 0.7, 0.3, 0,
                            f"config 5 utt {i}")
        assert st.frames == C5_LENS[i], st.report(C5_LENS[i])
        tot.merge(st)
    print(tot.report(sum(C5_LENS)), f"({time.time() - t0:.1f} s of float64 work)")
    assert tot.frames == sum(C5_LENS) == 6140
    assert tot.worst < 0.5, tot.report()
    tot.check_ties()


# ------------------------------------------------------------------------------------------ medium shapes --
MEDIUM = {                    # name: (beam, blank, transducer weight, ctc weight)
    "beam1": (1, 0, 0.7, 0.3),
    "beam3": (3, 0, 0.7, 0.3),
    "beam16": (16, 0, 0.7, 0.3),
    "blank_last": (8, -1, 0.7, 0.3),
    "ctc_only": (8, 0, 0.0, 1.0),
    "transducer_only": (8, 0, 1.0, 0.0),
}


@pytest.mark.parametrize("case", list(MEDIUM))
def test_prefix_beam_every_frame_medium(case):
    """T ~ 300, 3 utterances: beam 1, 3 and 16 (C = 256 candidates, every one of the utterance's 32 LSTM slots in
    use), blank = V - 1, and each weight alone."""
    from wenet_celoss_amd.decoder import DeviceDecoder
    beam, blank, tw, cw = MEDIUM[case]
    V, E, P, J, H, L = 1000, 128, 128, 256, 128, 2
    blank = blank % V
    pred, joint, ctc = beam_model(31 + len(case), V, E, P, J, H, L, blank=blank)
    lens = [300, 260, 170]
    enc = torch.randn(len(lens), max(lens), E)
    pw, jw, cwn = np_state(pred), np_state(joint), np_state(ctc)
    pred, joint, ctc = pred.to(DEV), joint.to(DEV), ctc.to(DEV)
    enc_d = enc.to(DEV)
    dec = DeviceDecoder(pred, joint, max_lanes=1024, max_utt=1024 // beam, tmax=max(lens), max_hyp=0, max_beam=16)
    with torch.no_grad():
        ctc_d = ctc.log_softmax(enc_d)
    tot = fw.Stats(case)
    emitted = 0
    for i, Lu in enumerate(lens):
        calls = beam_truncations(dec, enc_d[i], ctc_d[i], Lu, beam, tw, cw, blank)
        trie, j64 = do.PredictorTrie64(pw, L), do.Joint64(jw)
        st = walk_utterance(trie, j64, cwn, enc[i, :Lu].numpy(), calls, beam, tw, cw, blank, f"{case} utt {i}")
        assert st.frames == Lu
        tot.merge(st)
        emitted += len(calls[-1][1][-1][0][0]) - 1
    print(tot.report(sum(lens)), "tokens in the best hypotheses", emitted)
    assert tot.worst < 0.5, tot.report()
    tot.check_ties()
    assert emitted > 0


# ------------------------------------------------------------------------------------------ config 3 greedy --
def greedy_truncations(dec, enc_d, lens, n_steps, blank=0):
    """token lists after f frames for every stream and f = 0 .. len: states[i][f].  Groups of lengths overlap by one."""
    N, T, E = enc_d.shape
    per_call = max(2, 1024 // N)
    got = [{0: []} for _ in range(N)]
    f0 = 1
    while f0 <= T:
        fs = list(range(f0, min(T, f0 + per_call - 1) + 1))
        e = enc_d.repeat(len(fs), 1, 1)
        ln = torch.tensor([min(f, int(lens[i])) for f in fs for i in range(N)], dtype=torch.int32)
        res = dec.greedy(e, ln, n_steps=n_steps, blank=blank)
        for q, f in enumerate(fs):
            for i in range(N):
                if f <= int(lens[i]):
                    assert got[i].setdefault(f, res[q * N + i]) == res[q * N + i], (i, f)
        if fs[-1] == T:
            break
        f0 = fs[-1]
    return [[got[i][f] for f in range(int(lens[i]) + 1)] for i in range(N)]


def config3_model(weights):
    import wenet_celoss_amd as w
    V, E, P, J, H, L, N = 5000, 256, 256, 512, 256, 2, 64
    if weights == "engineered":          # test_decode_gpu.py::test_config3_shape_streams_match_oracle
        torch.manual_seed(5)
        pred = w.RNNPredictor(V, P, P, 0.1, H, L).eval()
        joint = w.TransducerJoint(V, E, P, J).eval()
        with torch.no_grad():
            joint.ffn_out.weight *= 10
            joint.ffn_out.bias[0] += 13.0
        enc = torch.randn(N, 32, E)
        lens = torch.randint(8, 33, (N,)); lens[0] = 32
        return pred, joint, enc, lens, 64, L
    torch.manual_seed(17)                # ..._chunked_streams_unscaled_weights_prefix_rule, decoded offline, n_steps 4
    pred = w.RNNPredictor(V, P, P, 0.1, H, L).eval()
    joint = w.TransducerJoint(V, E, P, J).eval()
    enc = torch.randn(N, 48, E)
    lens = torch.randint(5, 49, (N,)); lens[0] = 48
    return pred, joint, enc, lens, 4, L


@pytest.mark.parametrize("weights,look,graph", [("engineered", 0, True), ("engineered", 4, True),
                                                ("unscaled", 0, True), ("unscaled", 4, True),
                                                ("unscaled", 0, False)])
def test_config3_greedy_every_decision(weights, look, graph):
    """BASELINE config 3 (64 streams, V = 5000, LSTM 2 x 256): every decision of every frame of all 64 streams."""
    from wenet_celoss_amd.decoder import DeviceDecoder
    pred, joint, enc, lens, n_steps, L = config3_model(weights)
    pw, jw = np_state(pred), np_state(joint)
    pred, joint = pred.to(DEV), joint.to(DEV)
    N, T, _ = enc.shape
    dec = DeviceDecoder(pred, joint, max_lanes=1024, max_utt=1024, tmax=T, max_hyp=T * n_steps, max_beam=1)
    dec.set_lookahead(look)
    dec.set_graph(graph)
    enc_d = enc.to(DEV)
    states = greedy_truncations(dec, enc_d, lens, n_steps)
    full = dec.greedy(enc_d, lens.to(torch.int32), n_steps=n_steps)
    tot = fw.Stats(f"config 3 {weights} look {look} graph {graph}")
    capped = 0
    trie, j64 = do.PredictorTrie64(pw, L), do.Joint64(jw)
    for i in range(N):
        assert states[i][-1] == full[i], i
        st = fw.walk_greedy(trie, j64, enc[i].numpy(), states[i], n_steps, 0, f"stream {i}")
        assert st.frames == int(lens[i])
        tot.merge(st)
        capped += sum(len(b) - len(a) == n_steps for a, b in zip(states[i][:-1], states[i][1:]))
    print(tot.report(int(lens.sum())), "frames at the n_steps cap", capped, "tokens", sum(len(h) for h in full))
    tot.check_ties()
    assert sum(len(h) for h in full) > N
    if weights == "unscaled":
        assert capped > 0.9 * int(lens.sum())
