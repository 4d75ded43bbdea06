"""The memory-bounded joiner + TDT loss node (joint_rnnt_tdt_loss: wr_joint_tdt_stats -> wr_rnnt_tdt_sweeps; backward per
slice wr_joint_tdt_grad -> joiner backward) against the materialised path (joint_logits -> rnnt_tdt_loss(inplace_grad=True))
and against the float64 reference of tests/rnnt_tdt_ref.py on float64-computed joiner logits rounded to fp32.

Tolerances.  Against the materialised path: costs rtol 1e-6, atol 1e-6 -- the token log-sum-exp is merged in another order,
the tolerance tests/test_fused_gpu.py and tests/test_bounded_loss_gpu.py state for that; the four parameter gradients within
1e-5 of each tensor's largest entry (fp32 sums over u / t / slices in another order).  Against the reference: costs rtol
1e-5, atol 1e-5 and the logits gradient rtol 1e-4, atol 1e-5, the tolerances of tests/test_rnnt_tdt_gpu.py.  Across budgets
the forward is the same launch, so costs are bit-identical."""
import functools
import gc

import numpy as np
import pytest
import torch

import rnnt_tdt_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make(B, T, U, J, V, D, ragged, seed=0, scale=1.0):
    """tests/test_bounded_loss_gpu.py::make with W = V + D output rows; labels stay in the token columns"""
    W = V + D
    g = torch.Generator().manual_seed(seed)
    ep = torch.randn(B, T, J, generator=g).to(DEV)
    pp = torch.randn(B, U + 1, J, generator=g).to(DEV)
    w = (torch.randn(W, J, generator=g) * (2.0 * scale / J ** 0.5)).to(DEV)
    b = torch.randn(W, generator=g).to(DEV)
    y = torch.randint(1, V, (B, max(U, 1)), generator=g, dtype=torch.int32)[:, :U].contiguous().to(DEV)
    if ragged:
        tl = torch.randint(max(T // 2, 1), T + 1, (B,), generator=g)
        ul = torch.randint(0, U + 1, (B,), generator=g)
        tl[0], ul[-1] = T, U
    else:
        tl, ul = torch.full((B,), T), torch.full((B,), U)
    return ep, pp, w, b, y, tl.to(torch.int32).to(DEV), ul.to(torch.int32).to(DEV)


def bounded(args, durs, budget, sigma=0.0, blank=0, reduction="none", gw=None):
    import wenet_celoss_amd as w_
    leaves = [t.clone().requires_grad_(True) for t in args[:4]]
    out = w_.joint_rnnt_tdt_loss(*leaves, *args[4:], durs, blank=blank, sigma=sigma, reduction=reduction,
                                 logits_budget=budget)
    (out * gw).sum().backward() if gw is not None else out.sum().backward()
    return out.detach(), [t.grad for t in leaves]


def materialised(args, durs, sigma=0.0, blank=0, reduction="none", gw=None):
    import wenet_celoss_amd as w_
    leaves = [t.clone().requires_grad_(True) for t in args[:4]]
    logits = w_.joint_logits(*leaves, precision="fp32")
    out = w_.rnnt_tdt_loss(logits, *args[4:], durs, blank=blank, sigma=sigma, reduction=reduction, inplace_grad=True)
    (out * gw).sum().backward() if gw is not None else out.sum().backward()
    return out.detach(), [t.grad for t in leaves]


def assert_grads_close(ga, gr, rel=1e-5):
    for name, a, r in zip(("ep", "pp", "w", "b"), ga, gr):
        assert torch.isfinite(a).all(), name
        err, top = float((a - r).abs().max()), float(r.abs().max())
        print(name, "max |grad err|", err, "of", top)
        assert err <= rel * top + 1e-9, name


def row_bytes(args):
    return args[1].shape[1] * args[2].shape[0] * 4


def oracle(args, durs, sigma=0.0, blank=0):
    """(costs, logits gradient) of the float64 reference on float64 joiner logits rounded to fp32"""
    ep, pp, w, b, y, tl, ul = args
    B, U1 = ep.shape[0], pp.shape[1]
    lg = (torch.tanh(ep.double()[:, :, None] + pp.double()[:, None]) @ w.double().T + b.double()).float().cpu().numpy()
    oc, og, _, _ = ref.tdt_ref(lg, y.cpu().numpy().reshape(B, U1 - 1), tl.cpu().numpy(), ul.cpu().numpy(), durs, blank, sigma)
    return oc, og


def logits_gradient(args, durs, sigma=0.0, blank=0):
    """wr_joint_tdt_stats -> wr_rnnt_tdt_sweeps -> wr_joint_tdt_grad over the whole cell range, grad_costs = NULL"""
    from wenet_celoss_amd import _lib
    from wenet_celoss_amd.rnnt_tdt import _durations_arg
    ep, pp, w, b, y, tl, ul = args
    (B, T, J), U1, W, D = ep.shape, pp.shape[1], w.shape[0], len(durs)
    ws = _lib.workspace("wr_joint_workspace_bytes", J, W, device=DEV)
    tws = _lib.workspace("wr_rnnt_tdt_workspace_bytes", B, T, U1, D, device=DEV)
    costs = torch.empty(B, dtype=torch.float32, device=DEV)
    g = torch.full((B, T, U1, W), float("nan"), dtype=torch.float32, device=DEV)
    d = _durations_arg(durs)
    _lib.call("wr_joint_tdt_stats", ep, pp, w, b, tl, ul, y, B, T, U1, J, W, 0, blank, d, D, sigma, ws, ws.numel(), tws,
              tws.numel(), device=DEV)
    _lib.call("wr_rnnt_tdt_sweeps", tl, ul, B, T, U1, d, D, costs, tws, tws.numel(), device=DEV)
    _lib.call("wr_joint_tdt_grad", ep, pp, w, b, tl, ul, y, B, T, U1, J, W, 0, blank, d, D, sigma, None, tws, tws.numel(), 0,
              B * T * U1, g, ws, ws.numel(), 0, device=DEV)
    return costs.cpu().numpy(), g.cpu().numpy()


ALL9 = tuple(range(9))
CASES = [  # B, T, U, J, V, durations, sigma, ragged
    (2, 9, 4, 16, 50, (0, 1, 2), 0.0, False),
    (3, 70, 11, 32, 253, (0, 1, 2, 3, 4), 0.05, True),     # several 64-cell tiles; W = 258: durations across a 32-column tile
    (2, 33, 6, 64, 5000, (0, 1, 2, 3, 4), 0.0, True),      # the shipped width
    (1, 5, 0, 8, 7, (1,), 0.0, False),                     # U = 0, and {1} is the modified lattice
    (2, 40, 9, 512, 1024, (1, 2, 4, 8), 0.0, True),        # the shipped join_dim and the largest jump
    (2, 13, 5, 16, 31, ALL9, 0.05, True),                  # W = 40: the duration columns straddle tiles inside one wave
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%dT%dU%dJ%dV%dD%d" % (c[:5] + (len(c[5]),)))
def test_bounded_equals_materialised_and_reference(case):
    B, T, U, J, V, durs, sigma, ragged = case
    args = make(B, T, U, J, V, len(durs), ragged)
    gw = torch.linspace(0.5, 1.5, B, device=DEV)
    c0, g0 = materialised(args, durs, sigma, gw=gw)
    c1, g1 = bounded(args, durs, 3 * row_bytes(args) + 4, sigma, gw=gw)       # every utterance cut into frame slices
    oc, og = oracle(args, durs, sigma)
    assert np.isfinite(oc).all(), "the case must be feasible"
    print("costs", c1.tolist(), "materialised", c0.tolist(), "reference", oc.tolist())
    torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
    assert_grads_close(g1, g0)
    np.testing.assert_allclose(c1.cpu().numpy(), oc, rtol=1e-5, atol=1e-5)
    c2, g = logits_gradient(args, durs, sigma)
    assert np.array_equal(c2, c1.cpu().numpy())
    print("max |logits grad err|", np.abs(g - og).max())
    np.testing.assert_allclose(g, og, rtol=1e-4, atol=1e-5)
    tl, ul = args[5].tolist(), args[6].tolist()
    for b in range(B):                                     # padding rows: exactly zero
        assert not g[b, tl[b]:].any() and not g[b, :, ul[b] + 1:].any()


def test_budgets_change_only_the_summation_order():
    B, T, U, J, V, durs = 5, 40, 9, 64, 300, (0, 1, 2, 3, 4)
    args = make(B, T, U, J, V, len(durs), True, seed=4)
    args = args[:5] + (torch.tensor([40, 17, 40, 1, 29], dtype=torch.int32, device=DEV), args[6])
    row = row_bytes(args)
    whole = T * row
    budgets = [B * whole,          # one slice for the whole batch
               2 * whole + 123,    # two utterances per slice
               7 * row,            # every utterance cut into frame slices
               row,                # the one-row minimum
               5 * row + row // 3] # not a multiple of a row
    c_ref, g_ref = bounded(args, durs, budgets[0], 0.05)
    assert torch.isfinite(c_ref).all()
    for budget in budgets[1:]:
        c, g_ = bounded(args, durs, budget, 0.05)
        assert torch.equal(c, c_ref), budget
        assert_grads_close(g_, g_ref)
    for budget in (budgets[1], budgets[3]):                    # deterministic: same budget, same bits
        c1, g1 = bounded(args, durs, budget, 0.05)
        c2, g2 = bounded(args, durs, budget, 0.05)
        assert torch.equal(c1, c2)
        for a, r in zip(g1, g2):
            assert torch.equal(a, r)


def test_lattice_edge_cases():
    """blank != 0, a label equal to the blank, T_b = 1 and U_b = 0 in one batch."""
    B, T, U, J, V, durs = 4, 21, 7, 32, 40, (0, 1, 2)
    ep, pp, w, b, y, tl, ul = make(B, T, U, J, V, len(durs), True, seed=7)
    tl = torch.tensor([21, 5, 13, 1], dtype=torch.int32, device=DEV)
    ul = torch.tensor([7, 0, 3, 7], dtype=torch.int32, device=DEV)
    blank = 11
    y[0, 2] = blank
    y[3, 0] = blank
    args = (ep, pp, w, b, y, tl, ul)
    c0, g0 = materialised(args, durs, 0.05, blank=blank)
    c1, g1 = bounded(args, durs, 2 * row_bytes(args), 0.05, blank=blank)
    oc, og = oracle(args, durs, 0.05, blank=blank)
    assert np.isfinite(oc).all()
    torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
    assert_grads_close(g1, g0)
    np.testing.assert_allclose(c1.cpu().numpy(), oc, rtol=1e-5, atol=1e-5)
    _, g = logits_gradient(args, durs, 0.05, blank=blank)
    np.testing.assert_allclose(g, og, rtol=1e-4, atol=1e-5)


def test_infeasible_utterance_costs_inf_and_leaves_the_others_alone():
    """durations = (2,): T_b = 3, U_b = 0 has no path.  Costs only: that utterance's gradient is not defined."""
    import wenet_celoss_amd as w_
    B, T, U, J, V, durs = 3, 6, 2, 16, 20, (2,)
    ep, pp, w, b, y, _, _ = make(B, T, U, J, V, 1, False, seed=3)
    tl = torch.tensor([6, 3, 4], dtype=torch.int32, device=DEV)
    ul = torch.tensor([2, 0, 1], dtype=torch.int32, device=DEV)
    oc, _ = oracle((ep, pp, w, b, y, tl, ul), durs)
    assert np.isfinite(oc[[0, 2]]).all() and oc[1] == np.inf
    budget = 2 * row_bytes((ep, pp, w))
    with torch.no_grad():
        c = w_.joint_rnnt_tdt_loss(ep, pp, w, b, y, tl, ul, durs, reduction="none", logits_budget=budget)
        keep = torch.tensor([0, 2], device=DEV)
        c2 = w_.joint_rnnt_tdt_loss(ep[keep], pp[keep], w, b, y[keep], tl[keep], ul[keep], durs, reduction="none",
                                    logits_budget=budget)
    assert c[1] == float("inf")
    assert torch.equal(c[keep], c2)
    np.testing.assert_allclose(c[keep].cpu().numpy(), oc[[0, 2]], rtol=1e-5, atol=1e-5)


def test_empty_utterance_costs_zero():
    B, T, U, J, V, durs = 3, 5, 2, 16, 20, (0, 1, 2)
    ep, pp, w, b, y, _, _ = make(B, T, U, J, V, len(durs), False, seed=6)
    tl = torch.tensor([5, 0, 3], dtype=torch.int32, device=DEV)
    ul = torch.tensor([2, 1, 0], dtype=torch.int32, device=DEV)
    args = (ep, pp, w, b, y, tl, ul)
    c1, g1 = bounded(args, durs, 2 * row_bytes(args))
    c0, g0 = materialised(args, durs)
    assert c1[1] == 0.0 and torch.isfinite(c1).all()
    torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
    assert_grads_close(g1, g0)
    assert not g1[0][1].any()                                  # the empty utterance's frames get no gradient


def test_reductions_and_grad_costs():
    args = make(3, 70, 11, 32, 253, 5, True, seed=2)
    durs = (0, 1, 2, 3, 4)
    budget = 9 * row_bytes(args)
    for red in ("none", "mean", "sum"):
        c0, g0 = materialised(args, durs, 0.05, reduction=red)
        c1, g1 = bounded(args, durs, budget, 0.05, reduction=red)
        torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
        assert_grads_close(g1, g0)
    gw = torch.tensor([0.5, -2.0, 3.0], device=DEV)
    c0, g0 = materialised(args, durs, 0.05, gw=gw)
    c1, g1 = bounded(args, durs, budget, 0.05, gw=gw)
    assert_grads_close(g1, g0)


def test_wide_row_spread_is_repaired():
    """Weights scaled so that the token logits of a row spread over more than 88 nats: the statistics epilogue overflows,
    raises the flag, and the repair launch (running maximum) gives the materialised path's costs and finite gradients."""
    B, T, U, J, V, durs = 2, 12, 4, 32, 300, (0, 1, 2)
    ep, pp, w, b, y, tl, ul = make(B, T, U, J, V, len(durs), False, seed=5)
    w = w * 60.0
    args = (ep, pp, w, b, y, tl, ul)
    lg = (torch.tanh(ep.double()[:, :, None] + pp.double()[:, None]) @ w.double().T + b.double())[..., :V]
    assert float((lg.amax(-1) - lg.amin(-1)).max()) > 200.0
    c1, g1 = bounded(args, durs, 2 * row_bytes(args))
    assert torch.isfinite(c1).all()
    for g_ in g1:
        assert torch.isfinite(g_).all()
    c0, g0 = materialised(args, durs)
    print("costs", c1.tolist(), "materialised", c0.tolist())
    torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-4)
    # the flag -- the last 256-byte slot of the TDT workspace (csrc/rnnt_tdt.hpp) -- was raised here and is clear otherwise
    assert repair_flag(args, durs) == 1
    assert repair_flag((ep, pp, w / 60.0, b, y, tl, ul), durs) == 0


def repair_flag(args, durs):
    from wenet_celoss_amd import _lib
    from wenet_celoss_amd.rnnt_tdt import _durations_arg
    ep, pp, w, b, y, tl, ul = args
    (B, T, J), U1, W, D = ep.shape, pp.shape[1], w.shape[0], len(durs)
    ws = _lib.workspace("wr_joint_workspace_bytes", J, W, device=DEV)
    tws = _lib.workspace("wr_rnnt_tdt_workspace_bytes", B, T, U1, D, device=DEV)
    _lib.call("wr_joint_tdt_stats", ep, pp, w, b, tl, ul, y, B, T, U1, J, W, 0, 0, _durations_arg(durs), D, 0.0, ws, ws.numel(),
              tws, tws.numel(), device=DEV)
    return int(tws[-256:-252].view(torch.int32).item())


def test_second_backward_through_a_retained_graph():
    import wenet_celoss_amd as w_
    args = make(3, 70, 11, 32, 253, 5, True)
    leaves = [t.clone().requires_grad_(True) for t in args[:4]]
    costs = w_.joint_rnnt_tdt_loss(*leaves, *args[4:], (0, 1, 2, 3, 4), reduction="none", logits_budget=4 * row_bytes(args))
    first = torch.autograd.grad(costs.sum(), leaves, retain_graph=True)
    second = torch.autograd.grad(costs.sum(), leaves)
    for a, r in zip(first, second):
        assert torch.equal(a, r)


def test_peak_memory_is_below_half_the_logits_tensor():
    """B=2, T=200, U=50, J=64, W=1005: the logits would be 82 MB, the budget is 8 MB.  The TDT workspace is about 100 bytes
    per cell against the 4020 of a logits row, so forward + backward must stay below half the logits tensor."""
    import wenet_celoss_amd as w_
    B, T, U, J, V, durs = 2, 200, 50, 64, 1000, (0, 1, 2, 3, 4)
    args = make(B, T, U, J, V, len(durs), False, seed=11)
    logits_bytes = B * T * (U + 1) * (V + len(durs)) * 4
    leaves = [t.clone().requires_grad_(True) for t in args[:4]]
    gc.collect(); torch.cuda.empty_cache(); torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    costs = w_.joint_rnnt_tdt_loss(*leaves, *args[4:], durs, reduction="none", logits_budget=8 << 20)
    costs.sum().backward()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    print("peak growth", grew, "logits", logits_bytes)
    assert torch.isfinite(costs).all()
    assert grew < logits_bytes // 2, (grew, logits_bytes)


def test_transducer_with_budget_env(monkeypatch):
    """WR_FUSED_LOGITS_BUDGET_MB routes a TDT Transducer's loss block through the bounded node (here about 1 KB: three
    frames per slice): same loss and parameter gradients as without it, where the call sequence is the old one."""
    import wenet_celoss_amd.transducer as tr
    from test_transducer_tdt_gpu import build      # the tiny TDT model of the existing end-to-end test
    B, Tin = 3, 11
    g = torch.Generator().manual_seed(2)
    speech = torch.randn(B, Tin, 8, generator=g).to(DEV)
    slen = torch.tensor([11, 7, 9], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9], [4, 4, -1, -1], [7, 1, 6, -1]], device=DEV)
    tlen = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)
    calls = []
    for name in ("rnnt_tdt_loss", "joint_rnnt_tdt_loss"):
        monkeypatch.setattr(tr, name, functools.partial(lambda fn, n, *a, **k: (calls.append(n), fn(*a, **k))[1],
                                                        getattr(tr, name), name))

    def step():
        m = build().to(DEV)
        out = m(speech, slen, text, tlen)
        out["loss"].backward()
        return m, out["loss_rnnt"].detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    monkeypatch.delenv("WR_FUSED_LOGITS_BUDGET_MB", raising=False)
    m0, l0, g0 = step()
    assert m0._logits_budget() is None and calls == ["rnnt_tdt_loss"]
    del calls[:]
    monkeypatch.setenv("WR_FUSED_LOGITS_BUDGET_MB", "0.001")
    m1, l1, g1 = step()
    assert m1._logits_budget() == int(0.001 * (1 << 20)) and calls == ["joint_rnnt_tdt_loss"]
    print("loss_rnnt", l1.item(), "without the budget", l0.item())
    torch.testing.assert_close(l1, l0, rtol=1e-6, atol=0.0)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for n in g0:
        assert float((g1[n] - g0[n]).abs().max()) <= 1e-5 * float(g0[n].abs().max()) + 1e-9, n
