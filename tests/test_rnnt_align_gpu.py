"""RNN-T forced alignment on the GPU (wr_rnnt_align / wr_rnnt_align_from_stats) against planted paths, the float64
reference (tests/rnnt_align_ref.py), the RNN-T loss, the logits form of the joiner and the Transducer loss block.

Tolerances: scores are the fp64 sweep over the fp32 log-probabilities of pass 1, so against the float64 reference they
agree to 1e-5 * max(1, |score|); the paths agree exactly wherever the reference's smallest decision margin along its
path exceeds 1e-3 (far above the fp32 rounding of the log-probabilities summed over a path)."""
import math

import numpy as np
import pytest
import torch

import rnnt_align_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BOOST = 12.0


def random_frames(g, T, U):
    return sorted(torch.randint(0, T, (U,), generator=g).tolist())


def plant(logits, targets, t_lens, u_lens, blank, g):
    """Raise the logits of one chosen path of every utterance by BOOST; returns the planted frames (B, U) with -1 pad."""
    B, _, U1, _ = logits.shape
    planted = torch.full((B, U1 - 1), -1, dtype=torch.int32)
    for b in range(B):
        T_b, U_b = int(t_lens[b]), int(u_lens[b])
        fr = random_frames(g, T_b, U_b)
        planted[b, :U_b] = torch.tensor(fr, dtype=torch.int32)
        u = 0
        for t in range(T_b):
            while u < U_b and fr[u] == t:
                logits[b, t, u, int(targets[b, u])] += BOOST
                u += 1
            logits[b, t, u, blank] += BOOST
    return planted


def make(B, T, U1, V, t_lens, u_lens, blank, seed, label_is_blank=False):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, T, U1, V, generator=g)
    targets = torch.randint(0, V, (B, U1 - 1), generator=g, dtype=torch.int32)
    if label_is_blank and U1 > 1:
        targets[:, ::2] = blank
    for b in range(B):
        targets[b, int(u_lens[b]):] = -1                    # IGNORE_ID padding beyond a length
    planted = plant(logits, targets, t_lens, u_lens, blank, g)
    return logits, targets, torch.tensor(t_lens, dtype=torch.int32), torch.tensor(u_lens, dtype=torch.int32), planted


def align(logits, targets, t_lens, u_lens, blank=0):
    import wenet_celoss_amd as w
    fr, sc = w.rnnt_forced_align(logits.to(DEV), targets.to(DEV), t_lens.to(DEV), u_lens.to(DEV), blank=blank)
    assert fr.dtype == torch.int32 and sc.dtype == torch.float64 and fr.is_cuda and sc.is_cuda
    return fr.cpu(), sc.cpu()


def ref_one(logits_b, targets_b, T_b, U_b, blank):
    lg = logits_b[:T_b, :U_b + 1].double().cpu().numpy()
    bl, em = ref.lattice_log_probs(lg, targets_b[:U_b].tolist(), blank)
    return bl, em


@pytest.mark.parametrize("U1", [1, 63, 64, 65, 129, 1024])
def test_planted_paths_across_column_counts(U1):
    """U+1 across the wave boundary (64), the multi-wave LDS exchange and the 1024-column limit; a ragged batch with
    U_b = 0 and T_b = 1 rows."""
    T, V = (12, 12) if U1 == 1024 else (40, 24)
    U = U1 - 1
    t_lens = [T, 1, max(T // 2, 1), T]
    u_lens = [U, min(U, 5), 0, max(U - 3, 0)]
    logits, targets, tl, ul, planted = make(4, T, U1, V, t_lens, u_lens, blank=0, seed=U1)
    fr, sc = align(logits, targets, tl, ul)
    assert torch.equal(fr, planted)
    assert torch.isfinite(sc).all()


@pytest.mark.parametrize("blank", ["first", "last"])
@pytest.mark.parametrize("label_is_blank", [False, True])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_planted_paths_blank_and_dtypes(blank, label_is_blank, dtype):
    B, T, U1, V = 5, 30, 20, 33
    blank = 0 if blank == "first" else V - 1
    t_lens, u_lens = [30, 17, 1, 25, 9], [19, 4, 3, 0, 19]
    logits, targets, tl, ul, planted = make(B, T, U1, V, t_lens, u_lens, blank, seed=11, label_is_blank=label_is_blank)
    fr, sc = align(logits.to(dtype), targets, tl, ul, blank=blank)
    assert torch.equal(fr, planted)
    for b in range(B):
        bl, em = ref_one(logits.to(dtype).float()[b], targets[b], t_lens[b], u_lens[b], blank)
        opt = ref.path_score(bl, em, t_lens[b], u_lens[b], planted[b, :u_lens[b]].tolist())
        # fp32 log-probabilities of rows whose log-sum-exp is near BOOST: about one ulp of BOOST per step
        assert abs(float(sc[b]) - opt) <= 2e-6 * BOOST * (t_lens[b] + u_lens[b]) + 1e-5


def same_path_where_clear(logits, targets, t_lens, u_lens, fr_a, fr_b, blank=0):
    """fr_a and fr_b are valid paths, equal wherever the float64 reference's margin along its path exceeds 1e-3."""
    lc, tc = logits.float().cpu(), targets.cpu()
    for b in range(lc.shape[0]):
        T_b, U_b = int(t_lens[b]), int(u_lens[b])
        bl, em = ref_one(lc[b], tc[b], T_b, U_b, blank)
        _, frames, margin = ref.viterbi(bl, em, T_b, U_b)
        for fr in (fr_a, fr_b):
            assert ref.is_valid_path(fr[b].cpu().numpy(), T_b, U_b, lc.shape[2] - 1)
        if margin > 1e-3:
            assert fr_a[b, :U_b].tolist() == frames.tolist() == fr_b[b, :U_b].tolist(), b


def check_against_reference(logits, targets, t_lens, u_lens, fr, sc, blank=0):
    """Scores within 1e-5 * max(1, |opt|), the returned path rescored in float64 within the same bound of the optimum,
    exact path equality where the reference's smallest margin along its path exceeds 1e-3.  Returns the ambiguous count."""
    ambiguous = 0
    for b in range(logits.shape[0]):
        T_b, U_b = int(t_lens[b]), int(u_lens[b])
        bl, em = ref_one(logits[b], targets[b], T_b, U_b, blank)
        opt, frames, margin = ref.viterbi(bl, em, T_b, U_b)
        tol = 1e-5 * max(1.0, abs(opt))
        assert abs(float(sc[b]) - opt) <= tol, (b, float(sc[b]), opt)
        assert ref.is_valid_path(fr[b].numpy(), T_b, U_b, logits.shape[2] - 1)
        assert abs(ref.path_score(bl, em, T_b, U_b, fr[b, :U_b].tolist()) - opt) <= tol
        if margin > 1e-3:
            assert fr[b, :U_b].tolist() == frames.tolist(), b
        else:
            ambiguous += 1
    return ambiguous


def test_random_logits_against_float64_reference():
    g = torch.Generator().manual_seed(5)
    B, T, U1, V = 8, 60, 25, 40
    logits = torch.randn(B, T, U1, V, generator=g) * 2.0
    targets = torch.randint(1, V, (B, U1 - 1), generator=g, dtype=torch.int32)
    tl = torch.tensor([60, 60, 41, 7, 1, 33, 60, 52], dtype=torch.int32)
    ul = torch.tensor([24, 10, 24, 24, 3, 0, 17, 24], dtype=torch.int32)
    fr, sc = align(logits, targets, tl, ul)
    amb = check_against_reference(logits, targets, tl, ul, fr, sc)
    print(f"random logits: {amb} of {B} utterances ambiguous (margin <= 1e-3)")


def test_scores_against_the_loss():
    """score <= -cost (a max is at most the log-sum-exp), score >= -cost - log(#paths)."""
    import wenet_celoss_amd as w
    g = torch.Generator().manual_seed(9)
    B, T, U1, V = 6, 50, 16, 30
    logits = torch.randn(B, T, U1, V, generator=g).to(DEV)
    targets = torch.randint(1, V, (B, U1 - 1), generator=g, dtype=torch.int32).to(DEV)
    tl = torch.tensor([50, 44, 50, 3, 20, 12], dtype=torch.int32, device=DEV)
    ul = torch.tensor([15, 15, 0, 9, 15, 2], dtype=torch.int32, device=DEV)
    cost = w.rnnt_loss(logits, targets, tl, ul, blank=0, reduction="none").double().cpu()
    _, sc = w.rnnt_forced_align(logits, targets, tl, ul)
    sc = sc.cpu()
    for b in range(B):
        c = float(cost[b])
        assert float(sc[b]) <= -c + 1e-5 * abs(c) + 1e-4
        assert float(sc[b]) >= -c - ref.log_num_paths(int(tl[b]), int(ul[b])) - 1e-5 * abs(c) - 1e-4


def test_baseline_lattice():
    """Full-length utterances at the BASELINE lattice (T=1000, U=150, V=5000, fp32): one against the float64 reference
    (log-probabilities computed on the device in float64), every one valid and bounded by the loss."""
    import wenet_celoss_amd as w
    B, T, U, V = 3, 1000, 150, 5000
    g = torch.Generator(device=DEV).manual_seed(1)
    logits = torch.randn(B, T, U + 1, V, generator=g, device=DEV)
    targets = torch.randint(1, V, (B, U), generator=g, device=DEV, dtype=torch.int32)
    tl = torch.full((B,), T, dtype=torch.int32, device=DEV)
    ul = torch.full((B,), U, dtype=torch.int32, device=DEV)
    fr, sc = w.rnnt_forced_align(logits, targets, tl, ul)
    cost = w.rnnt_loss(logits, targets, tl, ul, blank=0, reduction="none").double().cpu()
    fr, sc = fr.cpu(), sc.cpu()
    for b in range(B):
        assert ref.is_valid_path(fr[b].numpy(), T, U, U)
        c = float(cost[b])
        assert -c - ref.log_num_paths(T, U) - 1e-5 * abs(c) <= float(sc[b]) <= -c + 1e-5 * abs(c)
    lp = torch.log_softmax(logits[0].double(), -1)
    bl = lp[:, :, 0].cpu().numpy()
    em = torch.gather(lp[:, :U], 2, targets[0].long()[None, :, None].expand(T, U, 1))[..., 0].cpu().numpy()
    del lp
    opt, frames, margin = ref.viterbi(bl, em, T, U)
    assert abs(float(sc[0]) - opt) <= 1e-5 * max(1.0, abs(opt))
    assert abs(ref.path_score(bl, em, T, U, fr[0].tolist()) - opt) <= 1e-5 * max(1.0, abs(opt))
    if margin > 1e-3:
        assert fr[0].tolist() == frames.tolist()
    print(f"BASELINE utterance 0: score {float(sc[0]):.4f}, float64 optimum {opt:.4f}, path margin {margin:.2e}")


def test_nan_logit_stays_in_its_utterance():
    B, T, U1, V = 4, 20, 8, 16
    t_lens, u_lens = [20, 20, 13, 20], [7, 5, 7, 0]
    logits, targets, tl, ul, _ = make(B, T, U1, V, t_lens, u_lens, 0, seed=4)
    clean_fr, clean_sc = align(logits, targets, tl, ul)
    bad = logits.clone()
    bad[1, 3, 2, 5] = float("nan")
    fr, sc = align(bad, targets, tl, ul)
    assert math.isnan(float(sc[1]))
    assert ref.is_valid_path(fr[1].numpy(), t_lens[1], u_lens[1], U1 - 1)
    keep = [0, 2, 3]
    assert torch.equal(fr[keep], clean_fr[keep])
    assert torch.equal(sc[keep], clean_sc[keep])


def test_two_calls_are_bit_identical():
    import wenet_celoss_amd as w
    g = torch.Generator().manual_seed(8)
    logits = torch.randn(5, 70, 90, 50, generator=g).to(DEV)
    targets = torch.randint(1, 50, (5, 89), generator=g, dtype=torch.int32).to(DEV)
    tl = torch.tensor([70, 60, 70, 2, 33], dtype=torch.int32, device=DEV)
    ul = torch.tensor([89, 89, 40, 89, 0], dtype=torch.int32, device=DEV)
    a = w.rnnt_forced_align(logits, targets, tl, ul)
    b = w.rnnt_forced_align(logits, targets, tl, ul)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------- logits-free form --
def path_cells(frames, T):
    """The lattice cells (t, u) a path visits."""
    cells, u = [(0, 0)], 0
    for t in range(T):
        while u < len(frames) and frames[u] == t:
            u += 1
            cells.append((t, u))
        if t + 1 < T:
            cells.append((t + 1, u))
    return set(cells)


def one_hot_joiner(cell_logits, t_lens, u_lens, activation):
    """ep, pp, w, b whose joiner logits equal `cell_logits` (T, U1, V) exactly in every utterance: feature k = (t', u')
    is 1 only in cell (t', u') -- relu(ep + pp) with ep = 1 / -1 on a frame match and pp = 0 / -2 on a label match
    (hardtanh gives 2 * one-hot - 1, undone by the bias) -- and column k of w holds that cell's logits."""
    T, U1, V = cell_logits.shape
    B = len(t_lens)
    J = (T * U1 + 3) // 4 * 4                                  # the joiner takes J in multiples of 4: zero columns pad
    k = torch.arange(J)
    ep = torch.where((k // U1)[None, :] == torch.arange(T)[:, None], 1.0, -1.0)
    pp = torch.where((k % U1)[None, :] == torch.arange(U1)[:, None], 0.0, -2.0)
    w = torch.zeros(V, J)
    w[:, :T * U1] = cell_logits.reshape(T * U1, V).T
    if activation == "relu":
        b = torch.zeros(V)
    else:                                                      # hardtanh: logits = 2 w[:, k] - w.sum(1) + b
        w = w / 2
        b = w.sum(1)
    return (ep[None].expand(B, T, J).contiguous(), pp[None].expand(B, U1, J).contiguous(), w, b)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("activation", ["relu", "hardtanh"])
@pytest.mark.parametrize("spread", [False, True])
def test_logits_free_form_planted(precision, activation, spread):
    """Planted paths through the joiner: same path as the planted one and as the logits form, scores within 1e-5
    relative.  `spread`: one row spreads over more than 88 nats, so the statistics epilogue overflows and the repair
    launch runs."""
    import wenet_celoss_amd as w_
    T, U1, V = 10, 7, 40
    g = torch.Generator().manual_seed(21)
    cell = torch.randn(T, U1, V, generator=g)
    t_lens, u_lens = [10, 6, 10], [6, 3, 0]
    targets = torch.randint(1, V, (3, U1 - 1), generator=g, dtype=torch.int32)
    # one planted path shared by the batch (the joiner's logits do not depend on b): plant utterance 0's, the others
    # are prefixes of the same lattice
    planted = plant(cell[None].clone(), targets[:1], [T], [U1 - 1], 0, g)
    fr0 = planted[0].tolist()
    u = 0
    for t in range(T):
        while u < U1 - 1 and fr0[u] == t:
            cell[t, u, int(targets[0, u])] += BOOST
            u += 1
        cell[t, u, 0] += BOOST
    if spread:                                   # a cell off the planted path (it is never worth passing through)
        on = path_cells(fr0, T)
        off = next((t, u) for t in range(T) for u in range(U1) if (t, u) not in on)
        cell[off[0], off[1], :] = torch.linspace(-60.0, 60.0, V)
    targets[1:] = targets[0]
    ep, pp, wt, bt = [x.to(DEV) for x in one_hot_joiner(cell, t_lens, u_lens, activation)]
    tg, tl, ul = targets.to(DEV), torch.tensor(t_lens, dtype=torch.int32, device=DEV), torch.tensor(u_lens, dtype=torch.int32, device=DEV)
    logits = w_.joint_logits(ep, pp, wt, bt, precision=precision, activation=activation)
    if precision == "fp32":
        assert torch.allclose(logits[0].cpu(), cell, atol=1e-3)
    f_ref, s_ref = w_.rnnt_forced_align(logits, tg, tl, ul)
    f_jf, s_jf = w_.joint_rnnt_forced_align(ep, pp, wt, bt, tg, tl, ul, precision=precision, activation=activation)
    assert f_jf[0].tolist() == fr0 == f_ref[0].tolist()
    assert f_jf[2].tolist() == [-1] * (U1 - 1)
    same_path_where_clear(logits, tg, tl, ul, f_jf, f_ref)
    # 1e-5 relative, plus two fp32 ulps of a row log-sum-exp near BOOST per step: the planted path's score is near 0, and
    # the two forms merge each row's statistics in another order
    atol = 2 * float(np.spacing(np.float32(BOOST))) * (T + U1 - 1)
    assert torch.allclose(s_jf.cpu(), s_ref.cpu(), rtol=1e-5, atol=atol)
    assert torch.isfinite(s_jf).all()


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("activation", ["tanh", "swish"])
def test_logits_free_form_random(precision, activation):
    """A random joiner: the logits-free form against the logits form of the same precision -- scores within 1e-5
    relative, the same path wherever the float64 reference's margin along its path exceeds 1e-3."""
    import wenet_celoss_amd as w_
    g = torch.Generator().manual_seed(3)
    B, T, U, J, V = 4, 40, 12, 32, 97
    ep = torch.randn(B, T, J, generator=g).to(DEV)
    pp = torch.randn(B, U + 1, J, generator=g).to(DEV)
    wt = (torch.randn(V, J, generator=g) * (4.0 / J ** 0.5)).to(DEV)
    bt = torch.randn(V, generator=g).to(DEV)
    tg = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(DEV)
    tl = torch.tensor([40, 31, 40, 5], dtype=torch.int32, device=DEV)
    ul = torch.tensor([12, 12, 4, 12], dtype=torch.int32, device=DEV)
    logits = w_.joint_logits(ep, pp, wt, bt, precision=precision, activation=activation)
    f_ref, s_ref = w_.rnnt_forced_align(logits, tg, tl, ul)
    f_jf, s_jf = w_.joint_rnnt_forced_align(ep, pp, wt, bt, tg, tl, ul, precision=precision, activation=activation)
    assert torch.allclose(s_jf.cpu(), s_ref.cpu(), rtol=1e-5, atol=0)
    same_path_where_clear(logits, tg, tl, ul, f_jf, f_ref)


def test_logits_free_form_refuses_16bit_under_autocast():
    import wenet_celoss_amd as w_
    ep, pp = torch.randn(1, 4, 8, device=DEV), torch.randn(1, 3, 8, device=DEV)
    args = (torch.randn(9, 8, device=DEV), torch.randn(9, device=DEV), torch.ones(1, 2, dtype=torch.int32, device=DEV),
            torch.tensor([4], dtype=torch.int32, device=DEV), torch.tensor([2], dtype=torch.int32, device=DEV))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        with pytest.raises(ValueError, match="logits form"):
            w_.joint_rnnt_forced_align(ep, pp, *args, precision="autocast")


# ---------------------------------------------------------------- Transducer --
class TinyEncoder(torch.nn.Module):
    """Linear + frame mask; returns (encoder_out, mask) like wenet encoders."""

    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)

    def forward(self, xs, xs_lens, decoding_chunk_size=0, num_decoding_left_chunks=-1):
        T = xs.size(1)
        mask = (torch.arange(T, device=xs.device)[None, :] < xs_lens[:, None].to(xs.device)).unsqueeze(1)
        return torch.tanh(self.proj(xs)), mask


def tiny_model(precision=None, with_bias=False):
    import wenet_celoss_amd as w
    torch.manual_seed(1)
    V, E, P, J = 23, 12, 10, 16
    cb = None
    if with_bias:
        from bias_stub import TinyBias
        cb = TinyBias(V, E, P)
    m = w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, 14, 2, dropout=0.0),
                     w.TransducerJoint(V, E, P, J, precision=precision), ctc=w.CTC(V, E), ctc_weight=0.3,
                     transducer_weight=0.7, context_bias=cb, hw_weight=0.0).to(DEV)
    return m.eval()


def tiny_batch():
    g = torch.Generator().manual_seed(2)
    speech = torch.randn(3, 11, 8, generator=g).to(DEV)
    slen = torch.tensor([11, 7, 9], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9], [4, 4, -1, -1], [7, 1, 6, -1]], device=DEV)
    tlen = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    return speech, slen, text, tlen


def hand_composed(m, enc, enc_lens, pred, text, tlen):
    """encoder / predictor outputs -> joiner logits -> rnnt_forced_align; also returns the logits and labels."""
    import wenet_celoss_amd as w
    tg = torch.where(text == -1, 0, text).to(torch.int32)
    logits = m.joint(enc, pred)
    fr, sc = w.rnnt_forced_align(logits, tg, enc_lens.to(torch.int32), tlen, blank=0)
    return fr, sc, logits, tg


@pytest.mark.parametrize("mode", ["fp32", "autocast_bf16"])
def test_transducer_forced_align_matches_hand_composition(mode):
    import wenet_celoss_amd as w
    m = tiny_model(precision="autocast" if mode == "autocast_bf16" else "fp32")
    speech, slen, text, tlen = tiny_batch()
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if mode == "autocast_bf16" else torch.autocast("cuda", enabled=False)
    with ctx, torch.no_grad():
        fr, sc = m.forced_align(speech, slen, text, tlen)
        enc, mask = m.encoder(speech, slen)
        pred = m.predictor(w.add_blank(text, 0, -1))
        f_h, s_h, logits, tg = hand_composed(m, enc, mask.squeeze(1).sum(1), pred, text, tlen)
    if mode == "fp32":        # the logits-free path against the logits form: statistics merged in another order
        assert torch.allclose(sc, s_h, rtol=1e-5, atol=1e-6)
        same_path_where_clear(logits, tg, mask.squeeze(1).sum(1), tlen, fr, f_h)
    else:                     # the same 16-bit logits through the same kernels
        assert logits.dtype == torch.bfloat16
        assert torch.equal(fr, f_h) and torch.equal(sc, s_h)


def test_transducer_forced_align_sees_the_loss_inputs_with_context_bias():
    """With a ContextBias module attached, forced_align aligns exactly the encoder / predictor outputs that forward's
    loss block received (captured from compute_loss)."""
    import wenet_celoss_amd as w
    m = tiny_model(precision="fp32", with_bias=True)
    speech, slen, text, tlen = tiny_batch()
    ctx_list = torch.tensor([[5, 6, 7], [8, 9, 0]], dtype=torch.int32, device=DEV)
    ctx_lens = torch.tensor([3, 2], dtype=torch.int32, device=DEV)
    seen = {}
    orig = m.compute_loss

    def spy(encoder_out, encoder_out_lens, predictor_out, text_, text_lengths, skip_padding=False):
        seen.update(enc=encoder_out.detach().clone(), lens=encoder_out_lens.detach().clone(),
                    pred=predictor_out.detach().clone())
        return orig(encoder_out, encoder_out_lens, predictor_out, text_, text_lengths, skip_padding)

    m.compute_loss = spy
    with torch.no_grad():
        m(speech, slen, text, tlen, ctx_list, ctx_lens)
        fr, sc = m.forced_align(speech, slen, text, tlen, ctx_list, ctx_lens)
        f_h, s_h, logits, tg = hand_composed(m, seen["enc"], seen["lens"], seen["pred"], text, tlen)
        ep, pp = m.joint.pre_activation(seen["enc"], seen["pred"])
        f_jf, s_jf = w.joint_rnnt_forced_align(ep, pp, m.joint.ffn_out.weight, m.joint.ffn_out.bias, tg,
                                               seen["lens"].to(torch.int32), tlen, precision="fp32")
    assert torch.equal(fr, f_jf) and torch.equal(sc, s_jf)      # the same launches on the same inputs
    assert torch.allclose(sc, s_h, rtol=1e-5, atol=1e-6)
    same_path_where_clear(logits, tg, seen["lens"], tlen, fr, f_h)
