"""FastEmit and the delay penalty through the fused joiner + RNN-T loss nodes (joint_rnnt_loss, with and without a
logits_budget) against TransducerJoint + rnnt_loss with the same options and against the float64 reference
(tests/rnnt_latency_ref.py) pushed through float64 logits.

Tolerances are the ones tests/test_fused_gpu.py and tests/test_bounded_loss_gpu.py use for the same comparisons without
the options: costs 1e-6 against the unfused pair (the row statistics are merged in another order), every parameter
gradient within 1e-5 of its largest entry; against the float64 reference costs rtol 2e-5 ("fp32" only, as there), and
the parameter gradients, which those files do not compare with float64, within 1e-4 of each one's largest entry -- the
fp32 bar of the loss gradient itself (tests/test_rnnt_gpu.py) carried through the linear joiner backward."""
import numpy as np
import pytest
import torch

import rnnt_latency_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SETTINGS = [(0.5, 0.0), (0.0, 0.5), (0.5, 0.5)]
CASES = [  # B, T, U, J, V, ragged
    (2, 9, 4, 16, 50, False),
    (3, 70, 11, 32, 257, True),      # several 64-cell tiles, odd V
    (1, 5, 0, 8, 7, False),          # U = 0: blank-only lattice
]


def make(B, T, U, J, V, ragged, seed=0):
    g = torch.Generator().manual_seed(seed)
    ep = torch.randn(B, T, J, generator=g).to(DEV)
    pp = torch.randn(B, U + 1, J, generator=g).to(DEV)
    w = (torch.randn(V, J, generator=g) * (2.0 / J ** 0.5)).to(DEV)
    b = torch.randn(V, generator=g).to(DEV)
    y = torch.randint(1, V, (B, max(U, 1)), generator=g, dtype=torch.int32)[:, :U].contiguous().to(DEV)
    if ragged:
        tl = torch.randint(max(T // 2, 1), T + 1, (B,), generator=g)
        ul = torch.randint(0, U + 1, (B,), generator=g)
        tl[0], ul[-1] = T, U
    else:
        tl, ul = torch.full((B,), T), torch.full((B,), U)
    return ep, pp, w, b, y, tl.to(torch.int32).to(DEV), ul.to(torch.int32).to(DEV)


def row_bytes(args):
    return args[1].shape[1] * args[2].shape[0] * 4


def run_fused(args, lam, dp, precision="fp32", budget=None, buckets=1, gw=None, clamp=-1.0):
    import wenet_celoss_amd as w_
    leaves = [t.clone().requires_grad_(True) for t in args[:4]]
    out = w_.joint_rnnt_loss(*leaves, *args[4:], blank=0, clamp=clamp, reduction="none", precision=precision,
                             buckets=buckets, logits_budget=budget, fastemit_lambda=lam, delay_penalty=dp)
    (out * gw).sum().backward()
    return out.detach(), [t.grad for t in leaves]


def run_unfused(args, lam, dp, precision="fp32", gw=None, clamp=-1.0):
    import wenet_celoss_amd as w_
    ep, pp, w, b, y, tl, ul = args
    leaves = [t.clone().requires_grad_(True) for t in (ep, pp, w, b)]
    logits = w_.joint_logits(*leaves, tl, ul, precision=precision)
    out = w_.rnnt_loss(logits, y, tl, ul, blank=0, clamp=clamp, reduction="none", fastemit_lambda=lam, delay_penalty=dp)
    (out * gw).sum().backward()
    return out.detach(), [t.grad for t in leaves]


def run_f64(args, lam, dp, gw, clamp=-1.0):
    """the float64 reference's costs and its logits gradient pushed through float64 logits"""
    ep, pp, w, b, y, tl, ul = args
    leaves = [t.detach().double().cpu().requires_grad_(True) for t in (ep, pp, w, b)]
    logits = torch.tanh(leaves[0][:, :, None] + leaves[1][:, None]) @ leaves[2].T + leaves[3]
    costs, grad, _ = ref.loss_f64(logits.detach().numpy(), y.cpu().numpy(), tl.cpu().numpy(), ul.cpu().numpy(), 0, lam, dp,
                                  clamp=clamp, grad_costs=gw.cpu().numpy())
    logits.backward(gradient=torch.as_tensor(grad))
    return costs, [t.grad for t in leaves]


def assert_grads_close(ga, gr, rel=1e-5):
    for name, a, r in zip(("ep", "pp", "w", "b"), ga, gr):
        assert torch.isfinite(a).all(), name
        r = r.to(a.device, a.dtype) if r.dtype != a.dtype else r
        assert float((a - r).abs().max()) <= rel * float(r.abs().max()) + 1e-9, name


@pytest.fixture(params=["epilogue", "row-pass"])
def lse_mode(request, monkeypatch):
    """the fused node's row statistics from the joiner forward's epilogue and from the loss's own row pass"""
    monkeypatch.setenv("WR_FUSED_LSE_EPILOGUE", "1" if request.param == "epilogue" else "0")
    return request.param


@pytest.mark.parametrize("lam,dp", SETTINGS)
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_both_nodes_equal_the_unfused_pair_and_the_reference(case, precision, lam, dp, lse_mode):
    args = make(*case)
    gw = torch.linspace(0.5, 1.5, case[0], device=DEV)
    c_ref, g_ref = run_unfused(args, lam, dp, precision, gw)
    c0, g0 = run_fused(args, lam, dp, precision, gw=gw)
    torch.testing.assert_close(c0, c_ref, rtol=1e-6, atol=1e-6)
    assert_grads_close(g0, g_ref)
    if lse_mode == "epilogue":          # the bounded node has one forward: once is enough
        c1, g1 = run_fused(args, lam, dp, precision, budget=3 * row_bytes(args) + 4, gw=gw)   # several frame slices
        torch.testing.assert_close(c1, c_ref, rtol=1e-6, atol=1e-6)
        assert_grads_close(g1, g_ref)
    if precision == "fp32":
        oc, og = run_f64(args, lam, dp, gw)
        np.testing.assert_allclose(c0.cpu().numpy(), oc, rtol=2e-5)
        assert_grads_close(g0, og, rel=1e-4)
    # the options are in the result: the costs move with the penalty only, the gradients with either
    cp, gp = run_fused(args, 0.0, 0.0, precision, gw=gw)
    assert torch.equal(cp, c0) == (dp == 0.0 or case[2] == 0)
    if case[2] > 0:
        assert float((gp[0] - g0[0]).abs().max()) > 1e-3 * float(gp[0].abs().max())


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_buckets_and_slices(precision):
    """>= 2 label-length buckets and a budget that cuts >= 3 slices, in both nodes: T_b is per utterance, so neither
    changes the penalty; per-utterance costs are bit-identical across buckets"""
    from wenet_celoss_amd.fused import plan_buckets, plan_slices
    B, T, U, J, V = 9, 60, 40, 32, 300
    lam, dp = 0.5, 0.5
    args = make(B, T, U, J, V, False, seed=21)
    tl = torch.tensor([60, 33, 58, 41, 60, 25, 47, 52, 39], dtype=torch.int32, device=DEV)
    ul = torch.tensor([40, 3, 17, 38, 9, 22, 40, 5, 30], dtype=torch.int32, device=DEV)
    args = args[:5] + (tl, ul)
    groups = plan_buckets(tl.tolist(), ul.tolist())
    assert groups is not None and len(groups) >= 2
    budget = 20 * row_bytes(args)
    assert len(plan_slices(tl.tolist(), ul.tolist(), T, U + 1, V, budget)) >= 3
    gw = torch.linspace(0.5, 1.5, B, device=DEV)
    c_ref, g_ref = run_unfused(args, lam, dp, precision, gw)
    base = None
    for budget_ in (None, budget):
        for nb in (1, 4):
            c, g = run_fused(args, lam, dp, precision, budget=budget_, buckets=nb, gw=gw)
            torch.testing.assert_close(c, c_ref, rtol=1e-6, atol=1e-6)
            assert_grads_close(g, g_ref)
            if nb == 1:
                base = c
            else:
                assert torch.equal(c, base)
    if precision == "fp32":
        oc, og = run_f64(args, lam, dp, gw)
        np.testing.assert_allclose(base.cpu().numpy(), oc, rtol=2e-5)


def test_clamp_and_costs_independent_of_lambda():
    args = make(3, 70, 11, 32, 257, True)
    gw = torch.ones(3, device=DEV)
    for budget in (None, 3 * row_bytes(args) + 4):
        c0, _ = run_fused(args, 0.0, 0.5, budget=budget, gw=gw)
        c1, g1 = run_fused(args, 0.5, 0.5, budget=budget, gw=gw, clamp=0.05)
        assert torch.equal(c0, c1)
        _, g_ref = run_unfused(args, 0.5, 0.5, gw=gw, clamp=0.05)
        assert_grads_close(g1, g_ref)
        # (0, 0) through the keywords is the call without them, bit for bit
        a = run_fused(args, 0.0, 0.0, budget=budget, gw=gw)
        import wenet_celoss_amd as w_
        leaves = [t.clone().requires_grad_(True) for t in args[:4]]
        out = w_.joint_rnnt_loss(*leaves, *args[4:], blank=0, reduction="none", buckets=1, logits_budget=budget)
        out.sum().backward()
        assert torch.equal(a[0], out.detach())
        for x, y in zip(a[1], leaves):
            assert torch.equal(x, y.grad)


def test_transducer_loss_equals_its_own_pieces(monkeypatch):
    """Transducer(fastemit_lambda=, rnnt_delay_penalty=): the loss of forward() is the weighted sum of compute_loss's
    full-lattice term with the options and the CTC term, on the fused, bounded and two-op routes (the AMP route hands
    the same keywords to rnnt_loss per label-length group: tests/test_rnnt_latency_host.py; 16-bit logits with the options:
    tests/test_rnnt_latency_gpu.py)"""
    import wenet_celoss_amd as w
    from test_transducer_gpu import TinyEncoder
    lam, dp = 0.25, 0.5
    V, E, P, J, H, ctc_w = 23, 12, 10, 16, 14, 0.3

    def build(**kw):
        torch.manual_seed(1)
        return w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, H, 2, dropout=0.0),
                            w.TransducerJoint(V, E, P, J), ctc=w.CTC(V, E), ctc_weight=ctc_w, transducer_weight=1.0 - ctc_w,
                            hw_weight=0.0, **kw).to(DEV)

    g = torch.Generator().manual_seed(2)
    speech = torch.randn(3, 11, 8, generator=g).to(DEV)
    slen = torch.tensor([11, 7, 9], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9], [4, 4, -1, -1], [7, 1, 6, -1]], device=DEV)
    tlen = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    m = build(fastemit_lambda=lam, rnnt_delay_penalty=dp)
    plain = build()
    routes = {}
    for name, fused, budget in (("fused", True, None), ("bounded", True, 1 << 14), ("two-op", False, None)):
        m.fused_loss, m.logits_budget = fused, budget
        m.zero_grad()
        out = m(speech, slen, text, tlen)
        out["loss"].backward()
        assert float(out["loss"]) == pytest.approx((1.0 - ctc_w) * float(out["loss_rnnt"]) + ctc_w * float(out["loss_ctc"]),
                                                   rel=1e-6)
        routes[name] = (float(out["loss_rnnt"]), {n: p.grad.clone() for n, p in m.named_parameters()})
    # the full-lattice term is rnnt_loss with the options on the model's own logits
    enc, mask = m.encoder(speech, slen)
    enc_lens = mask.squeeze(1).sum(1).to(torch.int32)
    from wenet_celoss_amd.common import add_blank
    pred = m.predictor(add_blank(text, m.blank, m.ignore_id))
    logits = m.joint(enc, pred)
    y = torch.where(text < 0, 0, text).to(torch.int32)
    want = w.rnnt_loss(logits, y, enc_lens, tlen, blank=0, reduction="mean", fastemit_lambda=lam, delay_penalty=dp)
    without = w.rnnt_loss(logits, y, enc_lens, tlen, blank=0, reduction="mean")
    assert abs(float(want) - float(without)) > 1e-3
    for name, (loss_rnnt, grads) in routes.items():
        assert loss_rnnt == pytest.approx(float(want), rel=1e-6), name
        for n, gr in routes["two-op"][1].items():
            assert float((grads[n] - gr).abs().max()) <= 1e-5 * float(gr.abs().max()) + 1e-9, (name, n)
    # and differs from the model without the options, whose loss is the plain one
    plain.fused_loss = False
    assert float(plain(speech, slen, text, tlen)["loss_rnnt"]) == pytest.approx(float(without), rel=1e-6)
