"""TDT prefix beam search on the device (wr_prefix_beam_search_tdt, DeviceDecoder.prefix_beam_tdt, the Transducer methods)
against the float64 rule of tests/tdt_beam_ref.py over copies of the same modules.

The cases, their seeds and the float64 beams come from tests/test_tdt_beam_ref.py, which has shown on the CPU that at least
four of the five utterances of every case have a reference margin above 1e-4.  An utterance is compared where its margin
exceeds 1e-4 (the convention of tests/test_decode_gpu.py): hypotheses, order and n_hyps equal, scores at rtol 1e-5."""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

import test_tdt_beam_ref as cases
from test_tdt_beam_ref import DUR1_SPECS, LENS, MARGIN, MIN_QUALIFY, SPEC, SPECS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def decoder(pred, joint, beam, B=len(LENS), T=max(LENS), max_hyp=0):
    from wenet_celoss_amd.decoder import DeviceDecoder
    return DeviceDecoder(copy.deepcopy(pred).to(DEV), copy.deepcopy(joint).to(DEV), B * beam, B, T, max_hyp, beam)


def run(dec, c, durations=None, beam=None, rows=slice(None), with_ctc=True):
    ctc = c.ctc_logp[rows].to(DEV) if (with_ctc and c.ctc_logp is not None) else None
    weights = c.weights if ctc is not None else (0.0, 1.0)
    return dec.prefix_beam_tdt(c.enc[rows].to(DEV), torch.tensor(c.lens[rows], dtype=torch.int32),
                               durations or c.spec.durations, beam or c.spec.beam, c.spec.blank, ctc_logp=ctc,
                               ctc_weight=weights[0], transducer_weight=weights[1])


def check(got, want, what=""):
    """Device n-best against the float64 beams: every utterance whose margin is clear, and enough of them."""
    print(what, "margins", [r.margin for r in want])
    for b, (g, r) in enumerate(zip(got, want)):
        print(" utt", b, "device", [(h, round(s, 5)) for h, s in g][:3], "reference",
              [(list(h), round(s, 5)) for h, _, s in r.beam][:3])
    qualify = 0
    for b, (g, r) in enumerate(zip(got, want)):
        if r.margin <= MARGIN:
            continue
        qualify += 1
        assert [h for h, _ in g] == [list(h) for h, _, _ in r.beam], (what, b, r.margin)       # hypotheses, order, n_hyps
        np.testing.assert_allclose([s for _, s in g], [s for _, _, s in r.beam], rtol=1e-5, err_msg=f"{what} utt {b}")
    assert qualify >= MIN_QUALIFY, (what, [r.margin for r in want])


# ------------------------------------------------------------------------------------------------------- parity --
@pytest.mark.parametrize("spec", SPECS, ids=[s.name for s in SPECS])
def test_device_equals_the_float64_rule(spec):
    c, want = cases.make_case(spec), cases.reference(spec)
    assert cases.case_conditions(spec, want) == []
    got = run(decoder(c.pred, c.joint, spec.beam), c)
    assert len(got) == len(LENS) and all(1 <= len(g) <= spec.beam for g in got)
    for g in got:
        assert all(h[0] == spec.blank for h, _ in g) and [s for _, s in g] == sorted((s for _, s in g), reverse=True)
    check(got, want, spec.name)


# ---------------------------------------------------------------------------------------------- constructed ties --
def test_exact_ties_go_to_the_lower_index_and_equal_duration_arcs_fuse():
    c, dup, joint, want = cases.tie_case()
    assert cases.tie_conditions(want) == []
    check(run(decoder(c.pred, joint, c.spec.beam), c), want, "ties")


# ------------------------------------------------------------------------------------------------ cross-checks --
@pytest.mark.parametrize("spec", DUR1_SPECS, ids=[s.name for s in DUR1_SPECS])
def test_durations_1_equals_the_plain_prefix_beam_search(spec):
    """durations = (1,): the plain search over the joiner's first V outputs gives the same hypotheses and scores, and
    they are those of the float64 rule."""
    import wenet_celoss_amd as w
    c, want = cases.make_case(spec), cases.reference(spec)
    assert cases.case_conditions(spec, want) == []
    tdt = run(decoder(c.pred, c.joint, spec.beam), c)
    plain_joint = w.TransducerJoint(c.V, cases.E, cases.P, cases.J).eval()
    state = {k: (v[:c.V] if k.startswith("ffn_out.") else v) for k, v in c.joint.state_dict().items()}
    plain_joint.load_state_dict(state)
    plain = decoder(c.pred, plain_joint, spec.beam).prefix_beam(
        c.enc.to(DEV), torch.tensor(c.lens, dtype=torch.int32), c.ctc_logp.to(DEV), spec.beam, *c.weights, spec.blank)
    compared = 0
    for b, r in enumerate(want):
        print("utt", b, "margin", r.margin, "tdt", tdt[b][:2], "plain", plain[b][:2])
        if r.margin > MARGIN:
            compared += 1
            assert [h for h, _ in tdt[b]] == [h for h, _ in plain[b]], b
            np.testing.assert_allclose([s for _, s in tdt[b]], [s for _, s in plain[b]], rtol=1e-5)
    assert compared >= MIN_QUALIFY
    check(plain, want, spec.name + " plain")


def test_beam_1_gives_the_tokens_of_the_greedy_search():
    """Beam 1, durations (1, 2, 4), no CTC: every arc advances under both rules, so the one hypothesis is greedy's."""
    spec = SPEC["beam1"]
    c, want = cases.make_case(spec), cases.reference(spec)
    assert min(r.margin for r in want) > MARGIN
    dec = decoder(c.pred, c.joint, 1, max_hyp=max(LENS))
    beam = run(dec, c)
    greedy = dec.greedy_tdt(c.enc.to(DEV), torch.tensor(c.lens, dtype=torch.int32), spec.durations, n_steps=4,
                            blank=spec.blank)
    print("beam", beam, "greedy", greedy)
    assert [g[0][0][1:] for g in beam] == greedy
    assert any(greedy)


# -------------------------------------------------------------------------------------------------- invariance --
def test_graphs_on_and_off_give_identical_outputs():
    spec = SPEC["beam8-ctc"]
    c = cases.make_case(spec)
    dec = decoder(c.pred, c.joint, spec.beam)
    dec.set_graph(True)
    on = run(dec, c)
    dec.set_graph(False)
    off = run(dec, c)
    dec.set_graph(True)
    assert on == off == run(dec, c)
    check(on, cases.reference(spec), "graph")


def test_batch_equals_single_utterance():
    spec = SPEC["beam8-ctc"]
    c, want = cases.make_case(spec), cases.reference(spec)
    dec = decoder(c.pred, c.joint, spec.beam)
    batch = run(dec, c)
    for b, r in enumerate(want):
        single = run(dec, c, rows=slice(b, b + 1))[0]
        if r.margin > MARGIN:
            assert [h for h, _ in single] == [h for h, _ in batch[b]], b
            np.testing.assert_allclose([s for _, s in single], [s for _, s in batch[b]], rtol=1e-6)


def test_one_handle_serves_interleaved_calls():
    """Plain beam search, TDT beam search with two duration sets and TDT greedy search on ONE handle give what each gives
    on a handle of its own.  The embedding table and the plain search's CTC posterior have a row / column for every joiner
    output, so that the plain search may emit any of them."""
    import wenet_celoss_amd as w
    width, beam, T, B = 305, 4, max(LENS), len(LENS)
    torch.manual_seed(11)
    pred = w.RNNPredictor(width, cases.P, cases.P, 0.0, cases.H, cases.L, dropout=0.0).eval()
    joint = w.TransducerJoint(width, cases.E, cases.P, cases.J).eval()
    ctc = w.CTC(width, cases.E).eval()
    with torch.no_grad():
        joint.ffn_out.weight *= 10
        joint.ffn_out.bias[0] += 13
    enc = torch.randn(B, T, cases.E, generator=torch.Generator().manual_seed(12)).to(DEV)
    lens = torch.tensor(LENS, dtype=torch.int32)
    with torch.no_grad():
        ctc_logp = ctc.log_softmax(enc.cpu()).to(DEV)
    calls = {
        "plain": lambda d: d.prefix_beam(enc, lens, ctc_logp, beam, 0.3, 0.7, 0),
        "tdt 0-4": lambda d: d.prefix_beam_tdt(enc, lens, (0, 1, 2, 3, 4), beam, 0),
        "tdt 1-2-4": lambda d: d.prefix_beam_tdt(enc, lens, (1, 2, 4), beam, 0),
        "greedy": lambda d: d.greedy_tdt(enc, lens, (0, 1, 2, 3, 4), n_steps=4, blank=0),
    }
    alone = {k: f(decoder(pred, joint, beam, max_hyp=4 * T)) for k, f in calls.items()}
    assert alone["tdt 0-4"] != alone["tdt 1-2-4"]
    shared = decoder(pred, joint, beam, max_hyp=4 * T)
    shared.set_graph(True)
    for k in ("plain", "tdt 0-4", "greedy", "tdt 1-2-4", "plain", "tdt 0-4", "tdt 1-2-4", "greedy"):
        assert calls[k](shared) == alone[k], k


# --------------------------------------------------------------------- refusals that need a handle, in order --
def test_the_handle_checks_refuse_in_the_documented_order():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    spec = SPEC["beam3"]
    c = cases.make_case(spec)
    B, T = 2, 8
    dec = decoder(c.pred, c.joint, 4, B=B, T=T)
    enc = torch.zeros(B, T, cases.E, device=DEV)
    lens = torch.full((B,), T, dtype=torch.int32, device=DEV)
    hyps = torch.empty(B, 4, T + 1, dtype=torch.int32, device=DEV)
    hl = torch.empty(B, 4, dtype=torch.int32, device=DEV)
    sc = torch.empty(B, 4, dtype=torch.float64, device=DEV)
    nh = torch.empty(B, dtype=torch.int32, device=DEV)

    def call(B_=B, T_=T, beam=4, cw=0.0, tw=1.0, blank=0, d=(0, 1, 2, 3, 4)):
        arr = (ctypes.c_int32 * len(d))(*d)
        rc = lib.wr_prefix_beam_search_tdt(dec._h, enc.data_ptr(), lens.data_ptr(), None, B_, T_, beam, cw, tw, blank, arr,
                                           len(d), hyps.data_ptr(), hl.data_ptr(), sc.data_ptr(), nh.data_ptr(), None)
        return rc, lib.wr_last_error()

    # each call breaks one rule more, from the last to the first: the first broken rule in the documented order answers
    order = [(dict(cw=0.3, tw=0.7), b"no CTC posterior"),
             (dict(cw=0.3, tw=0.7, blank=c.V), b"blank"),
             (dict(cw=0.3, tw=0.7, blank=c.V, T_=T + 1), b"T=9 exceeds"),
             (dict(cw=0.3, tw=0.7, blank=c.V, T_=T + 1, B_=B + 1), b"B*beam"),
             (dict(cw=0.3, tw=0.7, blank=c.V, T_=T + 1, B_=B + 1, beam=5), b"beam=5"),
             (dict(cw=0.3, tw=0.7, blank=c.V, T_=T + 1, B_=B + 1, beam=0), b"beam=0"),
             (dict(cw=0.3, tw=0.7, blank=c.V, beam=0, d=(0, 9)), b"lies outside [0, 8]")]
    for kw, text in order:
        rc, err = call(**kw)
        assert rc == -1 and err.startswith(b"prefix_beam_search_tdt: ") and text in err, (kw, err)
    # the token vocabulary follows D: 9 durations leave 305 - 9 = 296 token columns, and blank = 296 is then out of range
    rc, err = call(d=tuple(range(9)), blank=296)
    assert rc == -1 and b"blank 296 out of range [0,296)" in err, err
    assert call()[0] == 0                                   # and the handle still serves a good call


def test_too_few_token_columns_or_embedding_rows_are_refused():
    import wenet_celoss_amd as w
    from wenet_celoss_amd import _lib
    torch.manual_seed(0)
    pred = w.RNNPredictor(8, cases.P, cases.P, 0.0, cases.H, cases.L, dropout=0.0).eval()
    dec = decoder(pred, w.TransducerJoint(10, cases.E, cases.P, cases.J).eval(), 2, B=1, T=4)
    enc, lens = torch.zeros(1, 4, cases.E, device=DEV), torch.tensor([4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match=r"D=9 durations leave 1 token columns"):
        dec.prefix_beam_tdt(enc, lens, tuple(range(9)), 2, 0)
    dec = decoder(pred, w.TransducerJoint(10, cases.E, cases.P, cases.J).eval(), 2, B=1, T=4)
    with pytest.raises(RuntimeError, match=r"the embedding table has 8 rows, the token vocabulary 9"):
        dec.prefix_beam_tdt(enc, lens, (1,), 2, 0)
    assert _lib.load().wr_api_version() == 3


# ------------------------------------------------------------------------------------- the Transducer methods --
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


class TinyAttnDecoder(torch.nn.Module):
    """The stand-in attention decoder of test_transducer_gpu.py: logits = out(tanh(embed(ys) + mean_t(memory)))."""

    def __init__(self, V, E):
        super().__init__()
        self.embed = torch.nn.Embedding(V, E)
        self.out = torch.nn.Linear(E, V)
        self.right_decoder = torch.nn.Linear(E, V)

    def forward(self, memory, memory_mask, ys_in_pad, ys_in_lens, r_ys_in_pad, reverse_weight: float = 0.0):
        ctx = memory.mean(1, keepdim=True)
        return (self.out(torch.tanh(self.embed(ys_in_pad) + ctx)),
                self.right_decoder(torch.tanh(self.embed(r_ys_in_pad) + ctx)), ys_in_lens)


@functools.lru_cache(maxsize=None)
def model():
    import wenet_celoss_amd as w
    V, E, P, J, H = 23, 12, 10, 16, 14
    torch.manual_seed(21)
    m = w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, H, 2, dropout=0.0),
                     w.TransducerJoint(V + 3, E, P, J), ctc=w.CTC(V, E), ctc_weight=0.3, transducer_weight=0.7,
                     hw_weight=0.0, tdt_durations=(0, 1, 2), tdt_sigma=0.05)
    m.decoder = TinyAttnDecoder(V, E)
    m.reverse_weight = 0.0
    with torch.no_grad():
        m.joint.ffn_out.weight *= 5
        m.joint.ffn_out.bias[0] += 1.5
        m.ctc.ctc_lo.weight *= 5
        m.ctc.ctc_lo.bias[0] += 1.0
    return m.to(DEV).eval()


def test_transducer_beam_methods_run_and_agree():
    m = model()
    lens = [26, 15, 20]
    speech = torch.randn(3, 26, 8, generator=torch.Generator().manual_seed(5)).to(DEV)
    slen = torch.tensor(lens, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        nbest = m.tdt_beam_search_batch(speech, slen, beam_size=4)
        mixed = m.tdt_beam_search_batch(speech, slen, beam_size=4, ctc_weight=0.3, transducer_weight=0.7)
        hyp, score = m.tdt_beam_search(speech[:1], slen[:1], beam_size=4)
    print("n-best", nbest, "best", hyp, score)
    assert len(nbest) == 3 and all(1 <= len(u) <= 4 for u in nbest)
    assert any(len(h) >= 2 for u in nbest for h, _ in u)
    assert all([s for _, s in u] == sorted((s for _, s in u), reverse=True) for u in nbest)
    assert (hyp, score) == nbest[0][0]                     # utterance 0 has the full length: alone as in the batch
    assert [[s for _, s in u] for u in mixed] != [[s for _, s in u] for u in nbest]


def test_cal_tdt_score_and_attention_rescoring():
    import wenet_celoss_amd as w
    from torch.nn.utils.rnn import pad_sequence
    m = model()
    Tin, beam = 26, 4
    speech = torch.randn(1, Tin, 8, generator=torch.Generator().manual_seed(6)).to(DEV)
    slen = torch.tensor([Tin], dtype=torch.int32, device=DEV)
    wts = dict(ctc_weight=0.2, attn_weight=0.3, transducer_weight=0.5)
    with torch.no_grad():
        got_hyp, got_score = m.tdt_attention_rescoring(speech, slen, beam, search_ctc_weight=0.3,
                                                       search_transducer_weight=0.7, **wts)
        enc_out, mask = m.encoder(speech, slen)
        nbest = w.tdt_prefix_beam_search(m, enc_out, mask.squeeze(1).sum(1), beam, 0.3, 0.7)[0]
        hyps, beam_score = [s.hyp[1:] for s in nbest], [s.score for s in nbest]
        n = len(hyps)
        assert n >= 2 and all(s.cache is None for s in nbest)
        hyps_pad = pad_sequence([torch.tensor(h, device=DEV, dtype=torch.long) for h in hyps], True, m.ignore_id)
        hyps_lens = torch.tensor([len(h) for h in hyps], device=DEV, dtype=torch.long)
        enc_n, mask_n = enc_out.repeat(n, 1, 1), torch.ones(n, 1, enc_out.size(1), dtype=torch.bool, device=DEV)
        td = m._cal_tdt_score(enc_n, mask_n, hyps_lens, hyps_pad)
        # -rnnt_tdt_loss of each hypothesis on its own
        # (beside a filler row of its own length, or of one label for the empty hypothesis: the loss wants the longest
        # label row to fill the lattice)
        T = enc_out.size(1)
        for i, h in enumerate(hyps):
            U = max(len(h), 1)
            rows = [h + [0] * (U - len(h)), [1] * U]
            ys = torch.tensor([[m.blank] + r for r in rows], device=DEV)
            logits = m.joint(enc_out.repeat(2, 1, 1), m.predictor(ys))
            loss = w.rnnt_tdt_loss(logits, torch.tensor(rows, dtype=torch.int32, device=DEV),
                                   torch.tensor([T, T], dtype=torch.int32, device=DEV),
                                   torch.tensor([len(h), U], dtype=torch.int32, device=DEV), m.tdt_durations, blank=m.blank,
                                   sigma=m.tdt_sigma, reduction="none")
            assert td[i].item() == pytest.approx(-loss[0].item(), rel=1e-5), (i, h)
        dec_out, r_dec_out = m._cal_attn_score(enc_n, mask_n, hyps_pad, hyps_lens)
        att = m._attention_scores(hyps, dec_out, r_dec_out, 0.0)
    totals = [att[i] * wts["attn_weight"] + beam_score[i] * wts["ctc_weight"] + td[i].item() * wts["transducer_weight"]
              for i in range(n)]
    best = int(np.argmax(totals))
    print("totals", totals, "returned", got_hyp, float(got_score))
    assert got_hyp == hyps[best]
    assert float(got_score) == pytest.approx(totals[best], rel=1e-6)
