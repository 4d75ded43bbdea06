"""The memory-bounded joiner + RNN-T loss node (joint_rnnt_loss(..., logits_budget=n): wr_joint_rnnt_stats ->
wr_rnnt_loss_sweeps; backward per slice wr_joint_rnnt_grad -> joiner backward) against the node that keeps the logits and
against the float64 oracle.

Tolerances: costs 1e-6 relative against the other node (the row statistics are merged in another order, as in
tests/test_fused_gpu.py); gradients 1e-5 of each tensor's largest entry.  Across budgets the forward is the same launch,
so costs are bit-identical; each cell's gradient is computed row by row from the same statistics, so the four parameter
gradients differ only by the order of fp32 sums (over u / t inside the joiner backward, and over the slices): the same
1e-5 of the largest entry bounds that."""
import gc

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def make(B, T, U, J, V, ragged, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ep = torch.randn(B, T, J, generator=g).to(DEV)
    pp = torch.randn(B, U + 1, J, generator=g).to(DEV)
    w = (torch.randn(V, J, generator=g) * (2.0 * scale / J ** 0.5)).to(DEV)
    b = torch.randn(V, generator=g).to(DEV)
    y = torch.randint(1, V, (B, max(U, 1)), generator=g, dtype=torch.int32)[:, :U].contiguous().to(DEV)
    if ragged:
        tl = torch.randint(max(T // 2, 1), T + 1, (B,), generator=g)
        ul = torch.randint(0, U + 1, (B,), generator=g)
        tl[0], ul[-1] = T, U
    else:
        tl, ul = torch.full((B,), T), torch.full((B,), U)
    return ep, pp, w, b, y, tl.to(torch.int32).to(DEV), ul.to(torch.int32).to(DEV)


def run(args, budget, precision="fp32", reduction="none", blank=0, clamp=-1.0, activation="tanh", buckets=1, gw=None):
    import wenet_celoss_amd as w_
    leaves = [t.clone().requires_grad_(True) for t in args[:4]]
    out = w_.joint_rnnt_loss(*leaves, *args[4:], blank=blank, clamp=clamp, reduction=reduction, precision=precision,
                             activation=activation, buckets=buckets, logits_budget=budget)
    (out * gw).sum().backward() if gw is not None else out.sum().backward()
    return out.detach(), [t.grad for t in leaves]


def assert_grads_close(ga, gr, rel=1e-5):
    for name, a, r in zip(("ep", "pp", "w", "b"), ga, gr):
        assert torch.isfinite(a).all(), name
        assert float((a - r).abs().max()) <= rel * float(r.abs().max()) + 1e-9, name


def row_bytes(args):
    return args[1].shape[1] * args[2].shape[0] * 4


def oracle_costs(args, blank=0):
    ep, pp, w, b, y, tl, ul = args
    B, U1 = ep.shape[0], pp.shape[1]
    lg = (torch.tanh(ep.double()[:, :, None] + pp.double()[:, None]) @ w.double().T + b.double()).float().cpu().numpy()
    oc, _ = oracle.rnnt_loss_f64(lg, y.cpu().numpy().reshape(B, U1 - 1), tl.cpu().numpy(), ul.cpu().numpy(), blank=blank,
                                 want_grad=False)
    return oc


CASES = [  # B, T, U, J, V, ragged
    (2, 9, 4, 16, 50, False),
    (3, 70, 11, 32, 257, True),      # several 64-cell tiles, odd V
    (2, 33, 6, 64, 5000, True),      # the shipped vocabulary
    (1, 5, 0, 8, 7, False),          # U = 0: blank-only lattice
    (4, 130, 37, 512, 1024, True),   # the shipped join_dim
]


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_bounded_equals_unbounded_and_oracle(case, precision):
    args = make(*case)
    gw = torch.linspace(0.5, 1.5, case[0], device=DEV)
    c0, g0 = run(args, None, precision, gw=gw)
    c1, g1 = run(args, 3 * row_bytes(args) + 4, precision, gw=gw)       # several frame slices per utterance
    torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
    assert_grads_close(g1, g0)
    if precision == "fp32":
        np.testing.assert_allclose(c1.cpu().numpy(), oracle_costs(args), rtol=2e-5)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_budgets_change_only_the_summation_order(precision):
    B, T, U, J, V = 5, 40, 9, 64, 300
    args = make(B, T, U, J, V, True, seed=4)
    args = args[:5] + (torch.tensor([40, 17, 40, 1, 29], dtype=torch.int32, device=DEV), args[6])
    row = row_bytes(args)
    whole = T * row
    budgets = [B * whole,          # one slice for the whole batch
               2 * whole + 123,    # two utterances per slice
               7 * row,            # every utterance cut into frame slices
               row,                # the one-row minimum
               5 * row + row // 3] # not a multiple of a row
    c_ref, g_ref = run(args, budgets[0], precision)
    for budget in budgets[1:]:
        c, g_ = run(args, budget, precision)
        assert torch.equal(c, c_ref), budget
        assert_grads_close(g_, g_ref)
    for budget in (budgets[1], budgets[3]):                    # deterministic: same budget, same bits
        c1, g1 = run(args, budget, precision)
        c2, g2 = run(args, budget, precision)
        assert torch.equal(c1, c2)
        for a, r in zip(g1, g2):
            assert torch.equal(a, r)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_lattice_edge_cases(precision):
    """Ragged T_b < T, U_b = 0, blank != 0, a label equal to the blank."""
    B, T, U, J, V = 4, 21, 7, 32, 40
    ep, pp, w, b, y, tl, ul = make(B, T, U, J, V, True, seed=7)
    tl = torch.tensor([21, 5, 13, 1], dtype=torch.int32, device=DEV)
    ul = torch.tensor([7, 0, 3, 7], dtype=torch.int32, device=DEV)
    blank = 11
    y[0, 2] = blank
    y[3, 0] = blank
    args = (ep, pp, w, b, y, tl, ul)
    c0, g0 = run(args, None, precision, blank=blank)
    c1, g1 = run(args, 2 * row_bytes(args), precision, blank=blank)
    torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
    assert_grads_close(g1, g0)
    if precision == "fp32":
        np.testing.assert_allclose(c1.cpu().numpy(), oracle_costs(args, blank=blank), rtol=2e-5)


def test_clamp_reductions_and_activations():
    import wenet_celoss_amd as w_
    args = make(3, 70, 11, 32, 257, True, seed=2)
    budget = 9 * row_bytes(args)
    c0, g0 = run(args, None, clamp=0.05)
    c1, g1 = run(args, budget, clamp=0.05)
    torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
    assert_grads_close(g1, g0)
    for red in ("none", "mean", "sum"):
        c0, g0 = run(args, None, reduction=red)
        c1, g1 = run(args, budget, reduction=red)
        torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
        assert_grads_close(g1, g0)
    for act in sorted(w_._lib.ACTIVATIONS):
        for precision in ("fp32", "bf16x3"):
            c0, g0 = run(args, None, precision, activation=act)
            c1, g1 = run(args, budget, precision, activation=act)
            torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
            assert_grads_close(g1, g0)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_bucketed_batch(precision):
    """Length bucketing (plan_buckets) still applies outside the node: each group is a bounded node of its own."""
    args = make(8, 60, 30, 32, 129, True, seed=9)
    c0, g0 = run(args, None, precision, buckets=4)
    c1, g1 = run(args, 5 * row_bytes(args), precision, buckets=4)
    torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-6)
    assert_grads_close(g1, g0)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_wide_row_spread_is_repaired(precision):
    """Weights scaled so that rows spread over more than 88 nats: the statistics epilogue overflows, raises the flag,
    and the repair launch (running maximum) gives oracle-correct costs and finite gradients."""
    B, T, U, J, V = 2, 12, 4, 32, 300
    ep, pp, w, b, y, tl, ul = make(B, T, U, J, V, False, seed=5)
    w = w * 60.0
    args = (ep, pp, w, b, y, tl, ul)
    lg = torch.tanh(ep.double()[:, :, None] + pp.double()[:, None]) @ w.double().T + b.double()
    assert float((lg.amax(-1) - lg.amin(-1)).max()) > 200.0
    c1, g1 = run(args, 2 * row_bytes(args), precision)
    assert torch.isfinite(c1).all()
    for g_ in g1:
        assert torch.isfinite(g_).all()
    c0, g0 = run(args, None, precision)
    torch.testing.assert_close(c1, c0, rtol=1e-6, atol=1e-4)
    if precision == "fp32":
        np.testing.assert_allclose(c1.cpu().numpy(), oracle_costs(args), rtol=2e-5)


@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
def test_second_backward_through_a_retained_graph(precision):
    import wenet_celoss_amd as w_
    args = make(3, 70, 11, 32, 257, True)
    leaves = [t.clone().requires_grad_(True) for t in args[:4]]
    costs = w_.joint_rnnt_loss(*leaves, *args[4:], reduction="none", precision=precision, buckets=1,
                               logits_budget=4 * row_bytes(args))
    first = torch.autograd.grad(costs.sum(), leaves, retain_graph=True)
    second = torch.autograd.grad(costs.sum(), leaves)
    for a, r in zip(first, second):
        assert torch.equal(a, r)


def test_peak_memory_at_baseline_lattice():
    """B=8 at the BASELINE lattice (T=1000, U=150, V=5000, J=512), fp32, 1 GiB budget: the node that keeps the logits
    needs more than 24 GB here.  The growth of max_memory_allocated over forward + backward stays within what the shapes
    explain: the budget, dZ and H of the largest slice, the RNN-T workspace, the gradients of ep / pp / w / b (the
    result and one slice's contribution), the joiner's W re-layout and weight-gradient workspaces, and 64 MiB of slack."""
    import wenet_celoss_amd as w_
    from wenet_celoss_amd import _lib
    from wenet_celoss_amd.fused import plan_slices
    B, T, U, J, V = 8, 1000, 150, 512, 5000
    U1 = U + 1
    g = torch.Generator().manual_seed(17)
    ep = (torch.randn(B, T, J, generator=g) * 0.7).to(DEV)
    pp = (torch.randn(B, U1, J, generator=g) * 0.7).to(DEV)
    w = (torch.randn(V, J, generator=g) * 0.06).to(DEV)
    b = (torch.randn(V, generator=g) * 0.5).to(DEV)
    y = torch.randint(1, V, (B, U), generator=g, dtype=torch.int32).to(DEV)
    tl = torch.randint(T // 2, T + 1, (B,), generator=g); tl[0] = T
    ul = torch.randint(U // 3, U + 1, (B,), generator=g); ul[-1] = U
    tl, ul = tl.to(torch.int32).to(DEV), ul.to(torch.int32).to(DEV)
    budget = 1 << 30
    leaves = [t.clone().requires_grad_(True) for t in (ep, pp, w, b)]
    gc.collect(); torch.cuda.empty_cache(); torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    costs = w_.joint_rnnt_loss(*leaves, y, tl, ul, reduction="none", buckets=1, logits_budget=budget)
    costs.sum().backward()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    lib = _lib.load()
    slices = plan_slices(tl.tolist(), ul.tolist(), T, U1, V, budget)
    nmax = max(s.cells(U1) for s in slices)
    grads = 4 * (ep.numel() + pp.numel() + w.numel() + b.numel())
    bound = (budget + 2 * nmax * J * 4 + lib.wr_rnnt_workspace_bytes(B, T, U1) + 2 * grads
             + 2 * lib.wr_joint_workspace_bytes(J, V) + lib.wr_joint_dw_workspace_bytes(J, V) + (64 << 20))
    assert grew <= bound, (grew, bound)
    c = costs.detach().cpu().numpy()
    assert np.isfinite(c).all()
    del leaves, costs
    gc.collect(); torch.cuda.empty_cache()
    # two whole utterances against the float64 oracle (their logits built one utterance at a time)
    for bi in (0, int(torch.argmin(tl))):
        n_t, n_u = int(tl[bi]), int(ul[bi])
        lg = (torch.tanh(ep[bi, :n_t].double()[:, None] + pp[bi, :n_u + 1].double()[None]) @ w.double().T
              + b.double()).float().cpu().numpy()[None]
        oc, _ = oracle.rnnt_loss_f64(lg, y[bi:bi + 1, :n_u].cpu().numpy(), np.array([n_t], np.int32),
                                     np.array([n_u], np.int32), want_grad=False)
        del lg
        np.testing.assert_allclose(c[bi], oc[0], rtol=1e-4, atol=1e-5)


def test_transducer_with_budget_env(monkeypatch):
    """WR_FUSED_LOGITS_BUDGET_MB routes Transducer.compute_loss through the bounded node (here 1 KB: two frames per
    slice): same loss and parameter gradients as without it."""
    from test_transducer_gpu import build      # the tiny model of the existing end-to-end tests
    B, Tin = 3, 11
    g = torch.Generator().manual_seed(2)
    speech = torch.randn(B, Tin, 8, generator=g).to(DEV)
    slen = torch.tensor([11, 7, 9], dtype=torch.int32, device=DEV)
    text = torch.tensor([[3, 5, 2, 9], [4, 4, -1, -1], [7, 1, 6, -1]], device=DEV)
    tlen = torch.tensor([4, 2, 3], dtype=torch.int32, device=DEV)

    def step():
        m = build()
        out = m(speech, slen, text, tlen)
        out["loss"].backward()
        return m, out["loss_rnnt"].detach(), {n: p.grad.clone() for n, p in m.named_parameters() if p.grad is not None}

    monkeypatch.delenv("WR_FUSED_LOGITS_BUDGET_MB", raising=False)
    m0, l0, g0 = step()
    assert m0._logits_budget() is None
    monkeypatch.setenv("WR_FUSED_LOGITS_BUDGET_MB", "0.001")
    m1, l1, g1 = step()
    assert m1._logits_budget() == int(0.001 * (1 << 20))
    torch.testing.assert_close(l1, l0, rtol=1e-6, atol=1e-6)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for n in g0:
        assert float((g1[n] - g0[n]).abs().max()) <= 1e-5 * float(g0[n].abs().max()) + 1e-9, n


def test_budget_with_amp_joiner_warns(monkeypatch):
    """The 16-bit (AMP) joiner keeps its logits (two-op path): a set budget cannot apply and says so instead of being
    dropped silently."""
    import wenet_celoss_amd as w_
    B, T, U, E, V = 2, 9, 3, 32, 64
    gen = torch.Generator().manual_seed(3)
    enc = torch.randn(B, T, E, generator=gen).to(DEV)
    pred = torch.randn(B, U + 1, E, generator=gen).to(DEV)
    text = torch.randint(1, V, (B, U), generator=gen).to(DEV)
    m = w_.Transducer.__new__(w_.Transducer)
    torch.nn.Module.__init__(m)
    m.joint = w_.TransducerJoint(V, E, E, 64, precision="bf16")
    m.fused_loss, m.ignore_id, m.blank = True, -1, 0
    m = m.to(DEV)
    monkeypatch.setenv("WR_FUSED_LOGITS_BUDGET_MB", "64")
    with pytest.warns(RuntimeWarning, match="logits_budget"):
        joint_out, loss = m.compute_loss(enc, torch.tensor([T, 7], device=DEV), pred, text, torch.tensor([U, 2], device=DEV))
    assert torch.isfinite(loss)
