"""Streaming CTC prefix beam search on the GPU (include/wr_api.h, "Streaming CTC prefix beam search").

Bars, taken from tests/test_ctc_decode_gpu.py: hypotheses and times exact, scores and Viterbi scores against the float64
reference of tests/ctc_stream_ref.py at rel = 1e-5 -- on inputs whose smallest reference decision gap, the Viterbi
decisions included, is at least MIN_GAP = 1e-3 with no exact tie (the device's fp32 log-softmax differs from float64 by
at most ~1e-5 per frame, 4e-4 over the 40 frames used here); every test asserts that on the reference before it
compares.  The two equalities of the contract -- a one-chunk call against wr_ctc_prefix_beam_search, any chunking
against the one-chunk call -- are bit for bit: tuples of ints and Python floats compared with ==."""
import json
import math
import os

import numpy as np
import pytest
import torch

import ctc_decode_ref as cref
import ctc_stream_ref as sref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MIN_GAP = 1e-3
PAD = 7.0           # value of the frames of a chunk past a stream's lens: never consumed


def _reference(x, T, beam, blank=0):
    nb, st = sref.search(x, T, beam, blank)
    print(f"reference: T={T} V={x.shape[1]} beam={beam} blank={blank}: {st}")
    assert st.min_gap >= MIN_GAP and st.ties == 0, st
    sref.check_times(nb, T)
    return nb, st


def _same(got, want):
    assert [(t, tm) for t, _, _, tm in got] == [(t, tm) for t, _, _, tm in want]
    for (_, gs, gv, _), (_, rs, rv, _) in zip(got, want):
        print(f"score {gs!r} reference {rs!r}; viterbi {gv!r} reference {rv!r}")
        assert gs == pytest.approx(rs, rel=1e-5) and gv == pytest.approx(rv, rel=1e-5)


def _feed(stream, xs, plan):
    """Feed per-stream inputs xs[b] (T_b, V) through `stream`: plan is a list of per-chunk lens tuples; a chunk is as
    wide as its longest part (one frame when every part is empty) and stream b's part holds its next lens[b] frames."""
    import wenet_celoss_amd as w  # noqa: F401
    pos = [0] * len(xs)
    out = None
    for lens in plan:
        width = max(max(lens), 1)
        chunk = np.full((len(xs), width, xs[0].shape[1]), PAD, np.float32)
        for b, n in enumerate(lens):
            chunk[b, :n] = xs[b][pos[b]:pos[b] + n]
            pos[b] += n
        out = stream.search(torch.tensor(chunk, device=DEV), torch.tensor(lens))
        assert stream.frames == pos
        for b in range(len(xs)):
            sref.check_times(out[b], pos[b])                       # partial results too: one frame per token, increasing
    return out


def _whole(x, T, beam, blank=0):
    import wenet_celoss_amd as w
    return w.ctc_prefix_beam_search_times(torch.tensor(x[None, :T], device=DEV), torch.tensor([T]), beam, blank=blank)[0]


def _chunked(x, widths, beam, blank=0):
    import wenet_celoss_amd as w
    s = w.CtcPrefixBeamStream(1, beam, sum(max(n, 1) for n in widths), blank=blank)
    return _feed(s, [x], [(n,) for n in widths])[0]


@pytest.mark.parametrize("widths", [[3], [1, 2], [2, 1], [1, 1, 1]])
def test_known_answers_of_the_reference_test(widths):
    """runtime/core/test/ctc_prefix_beam_search_test.cc:30-73: hypotheses, likelihoods, Viterbi likelihoods, times."""
    d = np.load(os.path.join(GOLDEN, "ctc_prefix_kat.npz"))
    with open(os.path.join(GOLDEN, "ctc_prefix_times_kat.json")) as f:
        k = json.load(f)
    x = np.log(d["probs"]).astype(np.float32)          # a probability row's log is a fixed point of the log-softmax
    nb = _chunked(x, widths, k["beam"])
    assert [list(t) for t, _, _, _ in nb] == k["nbest"]
    assert [list(tm) for _, _, _, tm in nb] == k["times"]
    for (_, s, v, _), like, vit in zip(nb, k["likelihood"], k["viterbi_likelihood"]):
        assert math.exp(s) == pytest.approx(like, rel=1e-5) and math.exp(v) == pytest.approx(vit, rel=1e-5)


@pytest.mark.parametrize("beam,T,V,seed", [(1, 30, 17, 0), (2, 31, 18, 0), (9, 33, 19, 4), (12, 35, 20, 4),
                                           (13, 37, 19, 6), (16, 40, 20, 0)])
def test_range_whole_against_reference_and_existing_search(beam, T, V, seed):
    import wenet_celoss_amd as w
    x = cref.peaky_logits(seed, T, V, 0)
    want, st = _reference(x, T, beam)
    assert st.max_ncur == beam
    if beam >= 9:
        assert st.kept > 0 and st.merges > 0 and st.pairs > 0
    got = _whole(x, T, beam)
    _same(got, want)
    old = w.ctc_prefix_beam_search(torch.tensor(x[None], device=DEV), torch.tensor([T]), beam)[0]
    assert [(t, s) for t, s, _, _ in got] == old          # hyps / hyp_lens / scores / n_hyps, bit for bit


@pytest.fixture(scope="module")
def case16():
    x = cref.peaky_logits(0, 40, 20, 0)
    want, _ = _reference(x, 40, 16)
    whole = _whole(x, 40, 16)
    _same(whole, want)
    return x, whole


@pytest.mark.parametrize("widths", [[1] * 40, [7, 16, 16, 1], [16, 0, 24]], ids=["40x1", "7+16+16+1", "16+0+24"])
def test_chunking_is_bit_identical(case16, widths):
    x, whole = case16
    assert _chunked(x, widths, 16) == whole


def test_three_streams_ragged_equal_each_alone():
    """Lengths (40, 23, 1) in one stream set; the short streams sit out chunks with lens = 0, and one chunk is ragged."""
    import wenet_celoss_amd as w
    beam, V = 16, 20
    xs = [cref.peaky_logits(0, 40, V, 0), cref.peaky_logits(5, 23, V, 0), cref.peaky_logits(0, 1, V, 0)]
    plan = [(8, 8, 0), (8, 7, 1), (8, 0, 0), (8, 8, 0), (8, 0, 0)]
    assert [sum(p[b] for p in plan) for b in range(3)] == [40, 23, 1]
    got = _feed(w.CtcPrefixBeamStream(3, beam, 40), xs, plan)
    for b, x in enumerate(xs):
        want, _ = _reference(x, len(x), beam)
        _same(got[b], want)
        assert got[b] == _whole(x, len(x), beam), b


@pytest.mark.parametrize("beam,T,V,seed,blank", [(16, 32, 19, 3, 5), (3, 32, 19, 0, 18), (1, 12, 2, 0, 0), (2, 12, 2, 0, 0),
                                                 (2, 12, 2, 0, 1), (16, 30, 16, 0, 0)],
                         ids=["blank5", "blank_last", "V2_beam1", "V2_beam2", "V2_blank1", "beam_eq_V"])
def test_blank_position_two_symbols_and_beam_equal_to_vocabulary(beam, T, V, seed, blank):
    import wenet_celoss_amd as w
    x = cref.peaky_logits(seed, T, V, blank)
    want, _ = _reference(x, T, beam, blank)
    got = _whole(x, T, beam, blank)
    _same(got, want)
    assert _chunked(x, [5, 1, T - 6], beam, blank) == got
    old = w.ctc_prefix_beam_search(torch.tensor(x[None], device=DEV), torch.tensor([T]), beam, blank=blank)[0]
    assert [(t, s) for t, s, _, _ in got] == old


def test_state_reuse_after_reset_with_a_smaller_beam():
    import wenet_celoss_amd as w
    from wenet_celoss_amd import _lib
    x = cref.peaky_logits(0, 40, 20, 0)
    state = torch.empty(_lib.load().wr_ctc_stream_state_bytes(1, 16, 40), dtype=torch.uint8, device=DEV)
    _feed(w.CtcPrefixBeamStream(1, 16, 40, state=state), [x], [(16,), (24,)])
    want, _ = _reference(x, 40, 3)
    reused = _feed(w.CtcPrefixBeamStream(1, 3, 40, state=state), [x], [(16,), (24,)])[0]
    _same(reused, want)
    assert reused == _chunked(x, [16, 24], 3)
    # and reset() on one object
    s = w.CtcPrefixBeamStream(1, 3, 40)
    _feed(s, [x], [(9,)])
    s.reset()
    assert s.frames == [0]
    assert _feed(s, [x], [(40,)])[0] == reused


def test_capacity():
    import wenet_celoss_amd as w
    x = cref.peaky_logits(0, 40, 20, 0)[:8]
    whole = _whole(x, 8, 16)
    s = w.CtcPrefixBeamStream(1, 16, 8)
    assert _feed(s, [x], [(5,), (3,)])[0] == whole                # reaching max_frames exactly passes
    s.reset()
    _feed(s, [x], [(5,)])
    with pytest.raises(RuntimeError, match=r"5 frames done \+ a chunk of 4 exceeds max_frames=8"):
        s.search(torch.zeros(1, 4, 20, device=DEV), torch.tensor([4]))
    assert s.frames == [5]
    out = s.search(torch.tensor(x[None, 5:], device=DEV), torch.tensor([3]))[0]
    assert out == whole and s.frames == [8]                       # the refused call left the stream as it was
    with pytest.raises(RuntimeError, match="vocabulary changed from 20 to 21"):
        s.search(torch.zeros(1, 1, 21, device=DEV), torch.tensor([1]))


class TinyEncoder(torch.nn.Module):
    """Linear + frame mask; returns (encoder_out, mask) like wenet encoders."""

    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)

    def forward(self, xs, xs_lens, decoding_chunk_size=0, num_decoding_left_chunks=-1):
        T = xs.size(1)
        mask = (torch.arange(T, device=xs.device)[None, :] < xs_lens[:, None].to(xs.device)).unsqueeze(1)
        return torch.tanh(self.proj(xs)), mask


def test_transducer_methods():
    """Transducer.ctc_prefix_beam_search_times against the existing n-best, and the streaming pair over 4-frame chunks
    of the encoder output against the one-shot call.  The projections run as library GEMMs whose rounding may depend
    on the number of rows, so scores are compared at the file's bar and hypotheses exactly, after the gap condition has
    been asserted on the float64 reference of the device's own logits."""
    import wenet_celoss_amd as w
    V, E, P, beam = 23, 12, 10, 4
    torch.manual_seed(1)
    m = w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, 14, 2, dropout=0.0), w.TransducerJoint(V, E, P, 16),
                     ctc=w.CTC(V, E), ctc_weight=0.3, transducer_weight=0.7, hw_weight=0.0)
    with torch.no_grad():
        m.ctc.ctc_lo.weight.mul_(12.0)                           # peaky posteriors: decisions well apart
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(5)
    speech = torch.randn(2, 20, 8, generator=g).to(DEV)
    slen = torch.tensor([20, 13], dtype=torch.int32, device=DEV)
    with torch.no_grad():
        enc, _ = m.encoder(speech, slen)
        logits = m.ctc.ctc_lo(enc).cpu().numpy()
        refs = [_reference(logits[b], int(slen[b]), beam)[0] for b in range(2)]
        got = m.ctc_prefix_beam_search_times(speech, slen, beam)
        for b in range(2):
            n = int(slen[b])
            _same(got[b], refs[b])
            old, _ = m._ctc_prefix_beam_search(speech[b:b + 1, :n], slen[b:b + 1], beam)
            assert [t for t, _, _, _ in got[b]] == [t for t, _ in old]
            for (_, s, _, _), (_, so) in zip(got[b], old):
                assert s == pytest.approx(so, rel=1e-5)
        m.reset_ctc_stream(n_streams=2, beam_size=beam, max_frames=20)
        for t0 in range(0, 20, 4):
            part = m.forward_ctc_prefix_beam_search(enc[:, t0:t0 + 4], (slen - t0).clamp(0, 4))
        assert m._ctc_stream.frames == [20, 13]
        for b in range(2):
            _same(part[b], refs[b])
            assert [(t, tm) for t, _, _, tm in part[b]] == [(t, tm) for t, _, _, tm in got[b]]
