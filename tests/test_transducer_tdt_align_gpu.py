"""Transducer.tdt_forced_align and forced_align on the GPU, with the tiny stand-in encoder of
tests/test_transducer_tdt_gpu.py: a token-and-duration model aligns on its own lattice, through either method; a model
without durations takes exactly the path it took before."""
import numpy as np
import pytest
import torch

import rnnt_tdt_align_ref as aref
from test_transducer_tdt_gpu import DEV, DURATIONS, TinyEncoder, V, E, P, J, H, build

pytestmark = pytest.mark.gpu

B, TIN = 3, 9
NONE = torch.IntTensor([0])


def batch():
    g = torch.Generator().manual_seed(5)
    speech = torch.randn(B, TIN, 8, generator=g).to(DEV)
    slen = torch.tensor([9, 6, 4], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9], [4, 4, -1, -1], [7, 1, 6, -1]], device=DEV)
    tlen = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    return speech, slen, text, tlen


def joiner_logits(m, speech, slen, text):
    with torch.no_grad():
        _, enc, _, enc_lens, _, pred, _ = m._loss_inputs(speech, slen, text, NONE, NONE)
        return m.joint(enc, pred), enc_lens.to(torch.int32)


def test_tdt_forced_align_is_the_function_on_the_joiners_logits():
    import wenet_celoss_amd as w
    m = build().to(DEV).eval()
    speech, slen, text, tlen = batch()
    logits, enc_lens = joiner_logits(m, speech, slen, text)
    assert logits.shape == (B, TIN, 5, V + len(DURATIONS))
    ytxt = torch.where(text < 0, 0, text).to(torch.int32)
    want = w.rnnt_tdt_forced_align(logits, ytxt, enc_lens, tlen, DURATIONS, blank=0, sigma=0.05, return_blank_jumps=True)
    got = m.tdt_forced_align(speech, slen, text, tlen, return_blank_jumps=True)
    assert len(got) == 4 and all(torch.equal(a, b) for a, b in zip(got, want))
    short = m.tdt_forced_align(speech, slen, text, tlen)
    assert len(short) == 3 and all(torch.equal(a, b) for a, b in zip(short, want[:3]))
    # and that is the best path of the model's TDT lattice, sigma included
    refs, rf, rd, rj = aref.align_ref(logits.cpu().numpy(), ytxt.cpu().numpy(), enc_lens.tolist(), tlen.tolist(), DURATIONS,
                                      0, 0.05)
    for b, a in enumerate(refs):
        print(f"utterance {b}: score {float(got[2][b]):.6f} reference {a.score:.6f} margin {a.margin:.3e}")
        assert np.isfinite(a.score) and abs(float(got[2][b]) - a.score) <= 1e-5 * max(1.0, abs(a.score))
        assert aref.is_valid_path(got[0][b].cpu().numpy(), got[1][b].cpu().numpy(), got[3][b].cpu().numpy(),
                                  int(enc_lens[b]), int(tlen[b]), DURATIONS)
        if a.margin > 1e-3:
            assert np.array_equal(got[0][b].cpu().numpy(), rf[b]) and np.array_equal(got[1][b].cpu().numpy(), rd[b])


def test_forced_align_on_a_tdt_model_aligns_on_the_tdt_lattice():
    """head="joint" used to hand all V + D joiner columns to the regular-lattice alignment: one softmax over tokens and
    durations, no jumps.  Its scores then differ from the TDT lattice's by far more than rounding."""
    import wenet_celoss_amd as w
    m = build().to(DEV).eval()
    speech, slen, text, tlen = batch()
    frames, durs, scores = m.tdt_forced_align(speech, slen, text, tlen)
    fr, sc = m.forced_align(speech, slen, text, tlen)
    assert torch.equal(fr, frames) and torch.equal(sc, scores)
    assert fr.dtype == torch.int32 and sc.dtype == torch.float64 and fr.shape == (B, 4)
    logits, enc_lens = joiner_logits(m, speech, slen, text)
    ytxt = torch.where(text < 0, 0, text).to(torch.int32)
    _, regular = w.rnnt_forced_align(logits, ytxt, enc_lens, tlen, blank=0)
    assert float((regular - sc).abs().min()) > 1e-2


def test_a_model_without_durations_takes_the_path_it_took():
    import wenet_celoss_amd as w
    torch.manual_seed(3)
    m = w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, H, 2, dropout=0.0),
                     w.TransducerJoint(V, E, P, J), transducer_weight=1.0, hw_weight=0.0).to(DEV).eval()
    speech, slen, text, tlen = batch()
    fr, sc = m.forced_align(speech, slen, text, tlen)
    with torch.no_grad():
        _, enc, _, enc_lens, _, pred, _ = m._loss_inputs(speech, slen, text, NONE, NONE)
        ep, pp = m.joint.pre_activation(enc, pred)
        ytxt = torch.where(text < 0, 0, text).to(torch.int32)
        want = w.joint_rnnt_forced_align(ep, pp, m.joint.ffn_out.weight, m.joint.ffn_out.bias, ytxt,
                                         enc_lens.to(torch.int32), tlen, blank=0, precision=m.joint.precision,
                                         activation=m.joint.activation)
    assert torch.equal(fr, want[0]) and torch.equal(sc, want[1])
    with pytest.raises(ValueError, match="no tdt_durations"):
        m.tdt_forced_align(speech, slen, text, tlen)
