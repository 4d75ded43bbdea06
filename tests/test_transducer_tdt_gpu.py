"""wenet_celoss_amd.Transducer as a token-and-duration (TDT) model on the GPU, with the tiny stand-in encoder of
tests/test_transducer_gpu.py: the training step's loss against the float64 TDT reference on the joiner's own logits, and
greedy_search against a float64 torch loop over the same modules."""
import copy

import numpy as np
import pytest
import torch

import rnnt_tdt_ref as ref

pytestmark = pytest.mark.gpu


class TinySubsampling(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.subsampling_rate: int = 4
        self.right_context: int = 6


class TinyEncoder(torch.nn.Module):
    """Linear + frame mask; returns (encoder_out, mask) like wenet encoders (the stand-in of test_transducer_gpu.py)."""

    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)
        self.embed = TinySubsampling()

    def forward(self, xs, xs_lens, decoding_chunk_size=0, num_decoding_left_chunks=-1):
        T = xs.size(1)
        mask = (torch.arange(T, device=xs.device)[None, :] < xs_lens[:, None].to(xs.device)).unsqueeze(1)
        return torch.tanh(self.proj(xs)), mask


DEV = "cuda:0"
V, E, P, J, H = 11, 8, 8, 16, 12
DURATIONS = (0, 1, 2)
SEED, N_STEPS, FRAMES = 38, 3, 12         # chosen on the CPU: the float64 loop's smallest decision gap is 1.7e-2, and the
                                          # n_steps rule fires (n_steps = 2 gives other tokens)


def build(seed=SEED):
    import wenet_celoss_amd as w
    torch.manual_seed(seed)
    return w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, H, 2, dropout=0.0),
                        w.TransducerJoint(V + len(DURATIONS), E, P, J), transducer_weight=1.0, hw_weight=0.0,
                        tdt_durations=DURATIONS, tdt_sigma=0.05)


def test_training_step_loss_equals_the_reference_on_the_joiners_logits():
    m = build().to(DEV)
    B, Tin = 3, 9
    g = torch.Generator().manual_seed(5)
    speech = torch.randn(B, Tin, 8, generator=g).to(DEV)
    slen = torch.tensor([9, 6, 4], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9], [4, 4, -1, -1], [7, 1, 6, -1]], device=DEV)
    tlen = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    assert not m._can_fuse_loss()
    out = m(speech, slen, text, tlen)
    out["loss"].backward()
    with torch.no_grad():
        _, enc, _, enc_lens, _, pred, _ = m._loss_inputs(speech, slen, text, torch.IntTensor([0]), torch.IntTensor([0]))
        logits = m.joint(enc, pred)
    assert logits.shape == (B, Tin, 5, V + len(DURATIONS))
    ytxt = np.where(text.cpu().numpy() < 0, 0, text.cpu().numpy()).astype(np.int32)
    costs, _, _, _ = ref.tdt_ref(logits.float().cpu().numpy(), ytxt, enc_lens.cpu().numpy(), tlen.cpu().numpy(), DURATIONS,
                                 0, 0.05)
    assert np.isfinite(costs).all()
    print("loss_rnnt", out["loss_rnnt"].item(), "reference", costs.mean())
    assert out["loss_rnnt"].item() == pytest.approx(costs.mean(), rel=1e-5)
    assert out["loss"].item() == pytest.approx(costs.mean(), rel=1e-5)
    for name, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    assert float(m.joint.ffn_out.weight.grad[V:].abs().max()) > 0          # the duration rows train


def float64_greedy(m, speech, n_steps):
    """The greedy rule of the TDT model in float64 on the CPU over copies of the model's own modules -> (tokens, the
    smallest top-1 / top-2 gap over every token and duration decision)."""
    m = copy.deepcopy(m).cpu().double()
    x = speech.cpu().double()
    enc = torch.tanh(m.encoder.proj(x))
    T = x.size(1)
    pr, jt = m.predictor, m.joint
    state = (torch.zeros(2, 1, H, dtype=torch.double), torch.zeros(2, 1, H, dtype=torch.double))
    tok, hyps, gap = 0, [], float("inf")
    t, emitted, step = 0, 0, True
    with torch.no_grad():
        while t < T:
            if step:
                o, new_state = pr.rnn(pr.embed(torch.tensor([[tok]])), state)
                pred = pr.projection(o)
                step = False
            row = jt.ffn_out(torch.tanh(jt.enc_ffn(enc[:, t:t + 1]) + jt.pred_ffn(pred))).reshape(-1)
            for part in (row[:V], row[V:]):
                top = part.topk(2).values
                gap = min(gap, float(top[0] - top[1]))
            k, d = int(row[:V].argmax()), DURATIONS[int(row[V:].argmax())]
            if k == 0:
                t += max(d, 1)
                emitted = 0
                continue
            hyps.append(k)
            tok, state, step = k, new_state, True
            emitted = 0 if d > 0 else emitted + 1
            t += d
            if emitted >= n_steps:
                t += 1
                emitted = 0
    return hyps, gap


def test_greedy_search_matches_a_float64_loop():
    m = build()
    speech = torch.randn(1, FRAMES, 8, generator=torch.Generator().manual_seed(SEED + 100))
    want, gap = float64_greedy(m, speech, N_STEPS)
    # a condition on the reference, not a measurement: fp32 joiner rows cannot flip a decision this far apart
    assert gap >= 1e-3, gap
    assert len(want) >= 2
    m = m.to(DEV).eval()
    hyps, dist = m.greedy_search(speech.to(DEV), torch.tensor([FRAMES], dtype=torch.int32, device=DEV), n_steps=N_STEPS)
    print("tokens", hyps, "reference", want, "smallest gap", gap)
    assert dist == 0
    assert hyps == [want]
