"""The additive-joiner ("simple") RNN-T loss on the GPU against float64.

The checker is not the code under test: the simple loss is the ordinary RNN-T loss on the materialised sum
am[:, :, None, :] + lm[:, None, :, :], so `oracle.rnnt_loss_f64` on that tensor is the reference for the cost and -- its
logits gradient summed over u and over t -- for d_am and d_lm; the arc occupancies come from the float64 lattice of
tests/rnnt_simple_ref.py.  Tolerances are the project's bar for this lattice against float64 (test_rnnt_gpu.py check():
cost rtol 1e-5 / atol 1e-5, gradient rtol 1e-4 / atol 1e-5)."""
import numpy as np
import pytest
import torch

import oracle  # noqa: F401  (the float64 checker behind rnnt_simple_ref.oracle_reference)
import rnnt_align_ref as aref
import rnnt_simple_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COST_TOL = dict(rtol=1e-5, atol=1e-5)
GRAD_TOL = dict(rtol=1e-4, atol=1e-5)


def make_case(rng, B, T, U, V, scale=1.0, full=False, blank=0):
    lm = (rng.normal(size=(B, U + 1, V)) * scale).astype(np.float32)
    am = (rng.normal(size=(B, T, V)) * scale).astype(np.float32)
    labels = [v for v in range(V) if v != blank]
    symbols = rng.choice(labels, size=(B, U)).astype(np.int64) if U > 0 else np.zeros((B, 0), np.int64)
    if full:
        t_lens = np.full(B, T, np.int64); u_lens = np.full(B, U, np.int64)
    else:
        t_lens = np.concatenate([[T], rng.integers(1, T + 1, size=B - 1)]).astype(np.int64)
        u_lens = rng.integers(0, U + 1, size=B).astype(np.int64)
        u_lens[rng.integers(0, B)] = U
    return lm, am, symbols, t_lens, u_lens


def boundary_of(t_lens, u_lens):
    bd = torch.zeros(len(t_lens), 4, dtype=torch.int64)
    bd[:, 2] = torch.as_tensor(np.asarray(u_lens))
    bd[:, 3] = torch.as_tensor(np.asarray(t_lens))
    return bd.to(DEV)


def run_hip(lm, am, symbols, t_lens, u_lens, blank=0, reduction="none", grad_out=None, return_grad=False):
    import wenet_celoss_amd as w
    l = torch.tensor(lm, device=DEV, requires_grad=True)
    a = torch.tensor(am, device=DEV, requires_grad=True)
    out = w.rnnt_loss_simple(l, a, torch.tensor(symbols, device=DEV), blank, boundary=boundary_of(t_lens, u_lens),
                             reduction=reduction, return_grad=return_grad)
    loss = out[0] if return_grad else out
    if grad_out is None:
        loss.sum().backward()
    else:
        loss.backward(torch.tensor(grad_out, device=DEV, dtype=torch.float32))
    res = (loss.detach().cpu().numpy(), a.grad.cpu().numpy(), l.grad.cpu().numpy())
    return res + ((out[1][0].cpu().numpy(), out[1][1].cpu().numpy()),) if return_grad else res


def flag_of(lm, am, symbols, t_lens, u_lens, blank=0):
    from wenet_celoss_amd.rnnt_simple import rnnt_simple_lattice
    return int(rnnt_simple_lattice(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV),
                                   torch.tensor(symbols, device=DEV), blank, boundary_of(t_lens, u_lens))[3].item())


def check(lm, am, symbols, t_lens, u_lens, blank=0, expect_flag=0):
    costs, d_am, d_lm = run_hip(lm, am, symbols, t_lens, u_lens, blank=blank)
    oc, o_am, o_lm = ref.oracle_reference(lm, am, symbols, blank, t_lens, u_lens)
    print("cost err", np.abs(costs - oc).max(), "d_am err", np.abs(d_am - o_am).max(), "d_lm err", np.abs(d_lm - o_lm).max())
    assert np.isfinite(costs).all() and np.isfinite(d_am).all() and np.isfinite(d_lm).all()
    np.testing.assert_allclose(costs, oc, **COST_TOL)
    np.testing.assert_allclose(d_am, o_am, **GRAD_TOL)
    np.testing.assert_allclose(d_lm, o_lm, **GRAD_TOL)
    for b in range(lm.shape[0]):                          # padding is exactly zero
        assert not d_am[b, t_lens[b]:].any()
        assert not d_lm[b, u_lens[b] + 1:].any()
    assert flag_of(lm, am, symbols, t_lens, u_lens, blank) == expect_flag
    return costs, d_am, d_lm


# ---------------------------------------------------------------------------------------------- 1. parity --
@pytest.mark.parametrize("B,T,U,V", [          # the ragged table of test_rnnt_gpu.py
    (1, 1, 0, 2), (2, 5, 0, 7), (3, 7, 3, 5), (4, 20, 9, 33), (3, 33, 17, 128), (2, 70, 64, 40), (2, 40, 150, 36),
    (2, 12, 200, 20), (1, 9, 300, 12), (1, 6, 511, 8), (2, 9, 700, 12), (1, 5, 1023, 6), (5, 130, 30, 64),
])
def test_parity_ragged(B, T, U, V):
    rng = np.random.default_rng(B * 1000 + T * 10 + U + V)
    check(*make_case(rng, B, T, U, V, scale=1.5))


@pytest.mark.parametrize("V", [2, 31, 500, 1024, 5000])
def test_parity_vocabularies(V):
    rng = np.random.default_rng(V)
    check(*make_case(rng, 2, 37, 11, V))


def test_parity_blank_nonzero_label_equal_blank_and_single_frame():
    rng = np.random.default_rng(5)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 25, 11, 48, full=True, blank=47)
    check(lm, am, symbols, t_lens, u_lens, blank=47)
    symbols[:, 3] = 47                                    # a label equal to the blank, and a repeated label
    symbols[:, 7] = symbols[:, 2]
    check(lm, am, symbols, t_lens, u_lens, blank=47)
    symbols[:, 5] = 0
    check(lm, am, symbols, t_lens, u_lens, blank=0)
    check(*make_case(rng, 2, 1, 6, 19, full=True))        # T = 1: every label is emitted at the only frame
    check(*make_case(rng, 2, 9, 0, 19, full=True))        # U = 0: the blank-only path


def test_grad_costs_and_reductions():
    rng = np.random.default_rng(6)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 4, 21, 8, 40)
    oc, o_am, o_lm = [], [], []
    for b in range(4):                                    # per utterance, to weight the gradients
        c, ga, gl = ref.oracle_reference(lm[b:b + 1], am[b:b + 1], symbols[b:b + 1], 0, t_lens[b:b + 1], u_lens[b:b + 1])
        oc.append(c[0]); o_am.append(ga[0]); o_lm.append(gl[0])
    oc, o_am, o_lm = np.array(oc), np.stack(o_am), np.stack(o_lm)
    gw = np.array([0.5, -2.0, 1.25, 3.0], np.float32)
    costs, d_am, d_lm = run_hip(lm, am, symbols, t_lens, u_lens, grad_out=gw)
    np.testing.assert_allclose(costs, oc, **COST_TOL)
    np.testing.assert_allclose(d_am, o_am * gw[:, None, None], **GRAD_TOL)
    np.testing.assert_allclose(d_lm, o_lm * gw[:, None, None], **GRAD_TOL)
    for reduction, scale in (("none", 1.0), ("sum", 1.0), ("mean", 0.25)):
        loss, d_am, d_lm = run_hip(lm, am, symbols, t_lens, u_lens, reduction=reduction)
        want = oc if reduction == "none" else (oc.sum() if reduction == "sum" else oc.mean())
        np.testing.assert_allclose(loss, want, **COST_TOL)
        np.testing.assert_allclose(d_am, o_am * scale, **GRAD_TOL)
        np.testing.assert_allclose(d_lm, o_lm * scale, **GRAD_TOL)


def test_half_precision_inputs_get_half_gradients():
    import wenet_celoss_amd as w
    rng = np.random.default_rng(8)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 2, 10, 4, 16, full=True)
    l = torch.tensor(lm, device=DEV).half().requires_grad_(True)
    a = torch.tensor(am, device=DEV).bfloat16().requires_grad_(True)
    w.rnnt_loss_simple(l, a, torch.tensor(symbols, device=DEV), 0).backward()
    assert l.grad.dtype == torch.float16 and a.grad.dtype == torch.bfloat16


# ----------------------------------------------------------------------------------------- 2. opposed peaks --
def test_opposed_peaks_take_the_direct_path():
    """am's peak on symbol 3 and lm's on symbol 7, both 120 tall: the factored sum e^{am-ma} e^{lm-ml} is below e^{-87}
    in every term, exactly 0 in fp32, so the fast kernel raises the flag and the direct kernels redo statistics and
    gradient.  The float64 reference handles the input without comment."""
    rng = np.random.default_rng(11)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 40, 8, 5000)
    peak_am, peak_lm = am.copy(), lm.copy()
    peak_am[..., 3] += 120
    peak_lm[..., 7] += 120
    check(lm, am, symbols, t_lens, u_lens, expect_flag=0)
    check(peak_lm, peak_am, symbols, t_lens, u_lens, expect_flag=1)
    mixed_am, mixed_lm = am.copy(), lm.copy()             # only utterance 1 has opposed peaks
    mixed_am[1], mixed_lm[1] = peak_am[1], peak_lm[1]
    check(mixed_lm, mixed_am, symbols, t_lens, u_lens, expect_flag=1)


# ------------------------------------------------------------------------------------------ 3. padded region --
def test_padded_region_is_zero_and_nan_there_does_not_leak():
    rng = np.random.default_rng(12)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 4, 70, 66, 37)
    t_lens[1], u_lens[1] = 33, 20
    clean = run_hip(lm, am, symbols, t_lens, u_lens)
    dirty_lm, dirty_am = lm.copy(), am.copy()
    for b in range(4):
        dirty_am[b, t_lens[b]:] = np.nan
        dirty_lm[b, u_lens[b] + 1:] = np.nan
    got = run_hip(dirty_lm, dirty_am, symbols, t_lens, u_lens)
    for x, y in zip(clean, got):
        np.testing.assert_array_equal(x, y)
    for b in range(4):
        assert not got[1][b, t_lens[b]:].any() and not got[2][b, u_lens[b] + 1:].any()
    assert flag_of(dirty_lm, dirty_am, symbols, t_lens, u_lens) == 0


# ----------------------------------------------------------------------------------- 4. workspace interchange --
def test_export_lattice_matches_float64():
    from wenet_celoss_amd.rnnt_simple import rnnt_simple_lattice
    rng = np.random.default_rng(13)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 14, 6, 50)
    costs, alpha, beta, _ = rnnt_simple_lattice(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV),
                                                torch.tensor(symbols, device=DEV), 0, boundary_of(t_lens, u_lens))
    alpha, beta, costs = alpha.cpu().numpy(), beta.cpu().numpy(), costs.cpu().numpy()
    for b in range(3):
        T, U = int(t_lens[b]), int(u_lens[b])
        c, a, be, _, _ = ref.lattice_f64(lm[b], am[b], symbols[b], 0, T, U)
        np.testing.assert_allclose(alpha[b, :T, :U + 1], a, rtol=1e-5, atol=1e-4)     # test_rnnt_gpu.py's lattice bar
        np.testing.assert_allclose(beta[b, :T, :U + 1], be, rtol=1e-5, atol=1e-4)
        assert abs(c - costs[b]) < 1e-4 * max(1.0, abs(c))


ALIGN_CASES = [(21, 3, 30, 7, 40), (22, 2, 64, 20, 129), (23, 4, 17, 5, 5000)]      # (seed, B, T, U, V)


def align_case(seed, B, T, U, V):
    return make_case(np.random.default_rng(seed), B, T, U, V, scale=2.0)


def align_margins(lm, am, symbols, t_lens, u_lens):
    """Float64 Viterbi of every utterance: (frames, margin) lists."""
    out = []
    for b in range(lm.shape[0]):
        T, U = int(t_lens[b]), int(u_lens[b])
        bl, em = aref.lattice_log_probs(ref.materialised(lm[b:b + 1, :U + 1], am[b:b + 1, :T])[0], symbols[b, :U], 0)
        _, frames, margin = aref.viterbi(bl, em, T, U)
        out.append((frames, margin))
    return out


@pytest.mark.parametrize("seed,B,T,U,V", ALIGN_CASES)
def test_forced_align_matches_the_logits_form(seed, B, T, U, V):
    """Same frames as rnnt_forced_align on the materialised sum.  Every case's float64 best / second-best margin exceeds
    1e-3 (checked on the CPU in test_rnnt_simple_host.py too), so none is dropped."""
    import wenet_celoss_amd as w
    lm, am, symbols, t_lens, u_lens = align_case(seed, B, T, U, V)
    want = align_margins(lm, am, symbols, t_lens, u_lens)
    assert all(m > 1e-3 for _, m in want)
    sy = torch.tensor(symbols, device=DEV)
    frames, scores = w.rnnt_simple_forced_align(torch.tensor(lm, device=DEV), torch.tensor(am, device=DEV), sy, 0,
                                                boundary_of(t_lens, u_lens))
    ll = torch.tensor(t_lens, dtype=torch.int32, device=DEV)
    tl = torch.tensor(u_lens, dtype=torch.int32, device=DEV)
    f2, s2 = w.rnnt_forced_align(torch.tensor(ref.materialised(lm, am), device=DEV), sy.to(torch.int32), ll, tl, blank=0)
    assert torch.equal(frames, f2)
    np.testing.assert_allclose(scores.cpu().numpy(), s2.cpu().numpy(), rtol=1e-5, atol=1e-4)
    for b, (fr, _) in enumerate(want):
        U_b = int(u_lens[b])
        np.testing.assert_array_equal(frames[b, :U_b].cpu().numpy(), fr)
        assert (frames[b, U_b:] == -1).all()
    tokens = w.rnnt_frame_tokens(frames, sy, ll, tl)
    assert [sum(len(f) for f in per) for per in tokens] == [int(u) for u in u_lens]


# -------------------------------------------------------------------------------------------- 5. return_grad --
def test_return_grad_occupancies():
    rng = np.random.default_rng(14)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 3, 23, 9, 60)
    symbols[:, 4] = symbols[:, 1]
    costs, d_am, d_lm, (px, py) = run_hip(lm, am, symbols, t_lens, u_lens, return_grad=True)
    plain = run_hip(lm, am, symbols, t_lens, u_lens)
    np.testing.assert_array_equal(costs, plain[0])
    np.testing.assert_array_equal(d_am, plain[1])
    np.testing.assert_array_equal(d_lm, plain[2])
    B, T, U = 3, 23, 9
    assert px.shape == (B, U, T + 1) and py.shape == (B, U + 1, T)
    assert not px[:, :, T].any()
    for b in range(B):
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        _, _, _, oe, ob = ref.lattice_f64(lm[b], am[b], symbols[b], 0, Tb, Ub)
        want_px, want_py = np.zeros((U, T + 1)), np.zeros((U + 1, T))
        want_px[:Ub, :Tb] = oe[:, :Ub].T
        want_py[:Ub + 1, :Tb] = ob.T
        np.testing.assert_allclose(px[b], want_px, **GRAD_TOL)
        np.testing.assert_allclose(py[b], want_py, **GRAD_TOL)
        assert not px[b, Ub:].any() and not px[b, :, Tb:].any() and not py[b, Ub + 1:].any() and not py[b, :, Tb:].any()
        assert abs(py[b].sum() - Tb) <= 1e-4 * Tb                  # every path takes T_b blank arcs
        assert abs(px[b].sum() - Ub) <= 1e-4 * max(Ub, 1)          # and U_b emit arcs


# -------------------------------------------------------------------------------------------- 6. determinism --
def test_backward_is_bit_identical_run_to_run():
    rng = np.random.default_rng(15)
    lm, am, symbols, t_lens, u_lens = make_case(rng, 4, 150, 40, 700)
    symbols[:, 10:20] = symbols[:, :10]                             # repeated labels: the chained scatter terms
    first = run_hip(lm, am, symbols, t_lens, u_lens)
    second = run_hip(lm, am, symbols, t_lens, u_lens)
    for x, y in zip(first, second):
        assert np.array_equal(x, y)


# ------------------------------------------------------------------------------------------------ 7. memory --
def test_memory_stays_far_below_logits_size():
    """Forward + backward at B=4, T=1000, U=150, V=5000: the logits tensor alone would be 12 GB."""
    import wenet_celoss_amd as w
    from wenet_celoss_amd import _lib
    B, T, U, V = 4, 1000, 150, 5000
    gen = torch.Generator(device=DEV).manual_seed(16)
    am = torch.randn(B, T, V, device=DEV, generator=gen).requires_grad_(True)
    lm = torch.randn(B, U + 1, V, device=DEV, generator=gen).requires_grad_(True)
    sy = torch.randint(1, V, (B, U), device=DEV, generator=gen)
    lib = _lib.load()
    bound = (3 * (am.numel() + lm.numel()) * 4 + lib.wr_rnnt_workspace_bytes(B, T, U + 1)
             + lib.wr_rnnt_simple_workspace_bytes(B, T, U + 1, V) + (64 << 20))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    w.rnnt_loss_simple(lm, am, sy, 0).backward()
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - base
    print(f"peak above baseline {used / 2**20:.1f} MiB, bound {bound / 2**20:.1f} MiB")
    assert used <= bound
    assert torch.isfinite(am.grad).all() and torch.isfinite(lm.grad).all()


# --------------------------------------------------------------------------------------------- 8. full size --
def test_full_size_utterance_against_float64():
    """One BASELINE utterance (T=1000, U=150, V=5000) and one short one against the float64 oracle on the materialised
    sum (3 GB of logits on the host for the long one), as test_rnnt_gpu.py does for the ordinary loss."""
    B, T, U, V = 2, 1000, 150, 5000
    rng = np.random.default_rng(17)
    lm = rng.normal(size=(B, U + 1, V)).astype(np.float32)
    am = rng.normal(size=(B, T, V)).astype(np.float32)
    symbols = rng.integers(1, V, size=(B, U)).astype(np.int64)
    t_lens, u_lens = np.array([T, 311]), np.array([U, 47])
    costs, d_am, d_lm = run_hip(lm, am, symbols, t_lens, u_lens)
    assert flag_of(lm, am, symbols, t_lens, u_lens) == 0
    worst = {}
    for b in range(B):
        Tb, Ub = int(t_lens[b]), int(u_lens[b])
        oc, o_am, o_lm = ref.oracle_reference(lm[b:b + 1, :Ub + 1], am[b:b + 1, :Tb], symbols[b:b + 1, :Ub], 0, [Tb], [Ub])
        worst[b] = (abs(oc[0] - costs[b]) / abs(oc[0]),
                    float((np.abs(d_am[b, :Tb] - o_am[0]) / (1e-5 + 1e-4 * np.abs(o_am[0]))).max()),
                    float((np.abs(d_lm[b, :Ub + 1] - o_lm[0]) / (1e-5 + 1e-4 * np.abs(o_lm[0]))).max()))
        print("full-size utterance", b, "cost rel err, worst d_am and d_lm |err| / (1e-5 + 1e-4 |ref|):", worst[b])
        np.testing.assert_allclose(costs[b], oc[0], **COST_TOL)
        np.testing.assert_allclose(d_am[b, :Tb], o_am[0], **GRAD_TOL)
        np.testing.assert_allclose(d_lm[b, :Ub + 1], o_lm[0], **GRAD_TOL)
        assert not d_am[b, Tb:].any() and not d_lm[b, Ub + 1:].any()


# -------------------------------------------------------------------------------------------- 9. Transducer --
class TinyEncoder(torch.nn.Module):
    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)

    def forward(self, xs, xs_lens, decoding_chunk_size=0, num_decoding_left_chunks=-1):
        T = xs.size(1)
        mask = (torch.arange(T, device=xs.device)[None, :] < xs_lens[:, None].to(xs.device)).unsqueeze(1)
        return torch.tanh(self.proj(xs)), mask


def test_transducer_simple_loss_and_head_gradients():
    import wenet_celoss_amd as w
    V, E, P = 23, 12, 10
    torch.manual_seed(3)
    m = w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, 14, 2, dropout=0.0),
                     w.TransducerJoint(V, E, P, 16), ctc_weight=0.0, transducer_weight=1.0, hw_weight=0.0,
                     simple_loss_weight=0.5).to(DEV)
    assert m.simple_am_proj.in_features == E and m.simple_lm_proj.in_features == P
    g = torch.Generator().manual_seed(2)
    speech = torch.randn(3, 11, 8, generator=g).to(DEV)
    slen = torch.tensor([11, 7, 9], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9], [4, 4, -1, -1], [7, 1, 6, -1]], device=DEV)
    tlen = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    out = m(speech, slen, text, tlen)
    assert set(out.keys()) == {"loss", "loss_att", "loss_ctc", "loss_rnnt", "hw_loss", "loss_simple"}
    torch.testing.assert_close(out["loss"], out["loss_rnnt"] + 0.5 * out["loss_simple"])
    out["loss"].backward()

    with torch.no_grad():                                  # the tensors the joiner (and the two heads) see
        _, enc, _, enc_lens, _, pred, _ = m._loss_inputs(speech, slen, text, torch.IntTensor([0]), torch.IntTensor([0]))
    prm = {n: getattr(m, h).get_parameter(k).detach().double().cpu().requires_grad_(True)
           for h in ("simple_am_proj", "simple_lm_proj") for k in ("weight", "bias") for n in [f"{h}.{k}"]}
    am = enc.double().cpu() @ prm["simple_am_proj.weight"].T + prm["simple_am_proj.bias"]
    lm = pred.double().cpu() @ prm["simple_lm_proj.weight"].T + prm["simple_lm_proj.bias"]
    symbols = torch.where(text.cpu() < 0, 0, text.cpu())
    want = ref.loss_torch_f64(lm, am, symbols, 0, enc_lens.cpu(), tlen.cpu()).mean()
    np.testing.assert_allclose(out["loss_simple"].item(), want.item(), **COST_TOL)
    (0.5 * want).backward()
    for n, p in prm.items():
        got = m.get_parameter(n).grad.cpu().numpy()
        np.testing.assert_allclose(got, p.grad.numpy(), **GRAD_TOL)

    frames, scores = m.forced_align(speech, slen, text, tlen, head="simple")
    with torch.no_grad():
        f2, s2 = w.rnnt_simple_forced_align(m.simple_lm_proj(pred), m.simple_am_proj(enc), symbols.to(DEV), 0,
                                            boundary_of(enc_lens.cpu().numpy(), tlen.cpu().numpy()))
    assert torch.equal(frames, f2)
    assert frames.shape == (3, 4) and scores.shape == (3,)
    with pytest.raises(ValueError):
        m.forced_align(speech, slen, text, tlen, head="other")
