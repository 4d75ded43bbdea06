"""Parity of the HIP RNN-T loss (through the C-ABI) against the CPU oracle.

Tolerance (BASELINE.json north_star): loss and gradient within 1e-4 relative
in fp32.  Costs are compared with rtol 1e-5; gradients (values in [-1,1]) with
atol 1e-5 + rtol 1e-4 -- tighter than the bar.
"""
import numpy as np
import pytest
import torch

import oracle
from test_oracle_rnnt import KAT_COST, KAT_GRAD, KAT_LOGITS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run_hip(logits, targets, llens, tlens, blank=0, clamp=-1.0, reduction="none", grad_out=None, inplace=False):
    import wenet_celoss_amd as w
    x = torch.tensor(logits, device=DEV, requires_grad=True)
    xin = x.clone() if inplace else x          # a non-leaf so that in-place gradient is legal
    y = torch.tensor(targets, dtype=torch.int32, device=DEV).reshape(x.shape[0], -1)
    ll = torch.tensor(llens, dtype=torch.int32, device=DEV)
    tl = torch.tensor(tlens, dtype=torch.int32, device=DEV)
    loss = w.rnnt_loss(xin, y, ll, tl, blank=blank, clamp=clamp, reduction=reduction, inplace_grad=inplace)
    if grad_out is None:
        loss.sum().backward()
    else:
        loss.backward(torch.tensor(grad_out, device=DEV, dtype=torch.float32))
    return loss.detach().cpu().numpy(), x.grad.cpu().numpy()


def make_case(rng, B, T, U, V, scale=1.5, full=False):
    logits = (rng.normal(size=(B, T, U + 1, V)) * scale).astype(np.float32)
    targets = rng.integers(1, V, size=(B, U)).astype(np.int32) if U > 0 else np.zeros((B, 0), np.int32)
    if full:
        llens = np.full(B, T, np.int32); tlens = np.full(B, U, np.int32)
    else:
        llens = np.concatenate([[T], rng.integers(1, T + 1, size=B - 1)]).astype(np.int32)
        tlens = rng.integers(0, U + 1, size=B).astype(np.int32)
        tlens[rng.integers(0, B)] = U
    return logits, targets, llens, tlens


def check(logits, targets, llens, tlens, blank=0, clamp=-1.0):
    costs, grad = run_hip(logits, targets, llens, tlens, blank=blank, clamp=clamp)
    oc, og = oracle.rnnt_loss_f64(logits, targets, llens, tlens, blank=blank, clamp=clamp)
    np.testing.assert_allclose(costs, oc, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(grad, og, rtol=1e-4, atol=1e-5)
    for b in range(logits.shape[0]):                      # padding is exactly zero
        assert not grad[b, llens[b]:].any()
        assert not grad[b, :, tlens[b] + 1:].any()
    return costs, grad


def test_public_known_answer():
    costs, grad = run_hip(KAT_LOGITS, np.array([[1, 2]]), [2], [2])
    assert abs(costs[0] - KAT_COST) < 1e-5
    np.testing.assert_allclose(grad, KAT_GRAD, atol=1e-6)


@pytest.mark.parametrize("B,T,U,V", [
    (1, 1, 0, 2),          # single cell
    (2, 5, 0, 7),          # no labels: blank-only path
    (3, 7, 3, 5),          # V < 4: scalar head/tail only
    (4, 20, 9, 33),        # V % 4 != 0: every row has a different 16-B phase
    (3, 33, 17, 128),
    (2, 70, 64, 40),       # U1 = 65 -> K = 2 label columns per lane
    (2, 40, 150, 36),      # U1 = 151 -> K = 3 (the BASELINE shape's width)
    (2, 12, 200, 20),      # K = 4
    (1, 9, 300, 12),       # K = 5
    (1, 6, 511, 8),        # 8 waves: round 1's maximum
    (2, 9, 700, 12),       # 701 columns, 11 waves
    (1, 5, 1023, 6),       # 1024 columns: the supported maximum (16 waves)
    (5, 130, 30, 64),      # more steps than the prefetch ring several times over
])
def test_parity_ragged(B, T, U, V):
    rng = np.random.default_rng(B * 1000 + T * 10 + U + V)
    check(*make_case(rng, B, T, U, V))


def test_frameless_utterance_beside_live_ones_over_two_waves():
    """T_b = 0 between two live utterances at U1 = 65: its two workgroups leave through the sweep's early exit while the
    others run the two-wave barrier path.  The live ones against the float64 oracle (which has no T = 0 case of its own);
    the frameless one costs 0 and has no gradient."""
    rng = np.random.default_rng(65)
    B, T, U, V = 3, 9, 64, 17
    logits, targets, _, _ = make_case(rng, B, T, U, V)
    llens, tlens = np.array([T, 0, 5], np.int32), np.array([U, 7, U], np.int32)
    costs, grad = run_hip(logits, targets, llens, tlens)
    live = [0, 2]
    oc, og = oracle.rnnt_loss_f64(logits[live], targets[live], llens[live], tlens[live])
    np.testing.assert_allclose(costs[live], oc, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(grad[live], og, rtol=1e-4, atol=1e-5)
    assert costs[1] == 0 and not grad[1].any()
    for b in live:                                        # padding is exactly zero
        assert not grad[b, llens[b]:].any() and not grad[b, :, tlens[b] + 1:].any()


def test_parity_full_lengths_and_blank_nonzero():
    rng = np.random.default_rng(5)
    logits, targets, llens, tlens = make_case(rng, 3, 25, 11, 48, full=True)
    check(logits, targets, llens, tlens)
    blank = 47
    targets = rng.integers(0, 47, size=targets.shape).astype(np.int32)
    check(logits, targets, llens, tlens, blank=blank)
    # blank=-1 means "last class" (torchaudio convention)
    c1, _ = run_hip(logits, targets, llens, tlens, blank=-1)
    c2, _ = run_hip(logits, targets, llens, tlens, blank=47)
    np.testing.assert_array_equal(c1, c2)


def test_label_equal_to_blank_follows_case_chain():
    rng = np.random.default_rng(6)
    logits, targets, llens, tlens = make_case(rng, 2, 9, 5, 16, full=True)
    targets[0, 2] = 0
    targets[1, 4] = 0
    check(logits, targets, llens, tlens)


def test_clamp_and_large_logits():
    rng = np.random.default_rng(8)
    logits, targets, llens, tlens = make_case(rng, 2, 14, 6, 32, scale=6.0)
    check(logits, targets, llens, tlens, clamp=0.05)
    check(logits + 80.0, targets, llens, tlens)          # max-subtraction must hold
    check(logits - 80.0, targets, llens, tlens)


def test_reductions_and_grad_scaling():
    rng = np.random.default_rng(9)
    logits, targets, llens, tlens = make_case(rng, 4, 11, 5, 24)
    oc, og = oracle.rnnt_loss_f64(logits, targets, llens, tlens)
    for red, scale in (("mean", 1.0 / 4), ("sum", 1.0)):
        loss, grad = run_hip(logits, targets, llens, tlens, reduction=red)
        np.testing.assert_allclose(loss, oc.sum() * scale, rtol=1e-5)
        np.testing.assert_allclose(grad, og * scale, rtol=1e-4, atol=1e-6)
    go = np.array([0.5, -2.0, 0.0, 3.0], np.float32)
    _, grad = run_hip(logits, targets, llens, tlens, grad_out=go)
    np.testing.assert_allclose(grad, og * go[:, None, None, None], rtol=1e-4, atol=1e-5)


def test_launch_shape_knobs_do_not_change_results():
    """The streaming passes' launch shape (wr_tune_set keys 0-4: persistent grids of round 1, vectors in flight,
    non-temporal bits) only changes which wave visits which row: costs and gradients are bit-identical to the automatic
    grid's, on a shape large enough for several rows per wave (13 000 rows)."""
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(12)
    case = make_case(rng, 5, 130, 19, 200)
    ref = run_hip(*case)
    defaults = {0: 0, 1: 0, 2: 7, 3: 16, 4: 16}
    try:
        for knobs in ({0: 12, 1: 16}, {0: 1, 1: 1, 3: 4, 4: 4}, {2: 0, 3: 8, 4: 8}, {0: 4800, 1: 2048, 2: 6}):
            for k, v in {**defaults, **knobs}.items():
                assert lib.wr_tune_set(k, v) == 0
            got = run_hip(*case)
            assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), knobs
    finally:
        for k, v in defaults.items():
            lib.wr_tune_set(k, v)


def test_inplace_gradient_matches():
    rng = np.random.default_rng(10)
    logits, targets, llens, tlens = make_case(rng, 3, 17, 8, 40)
    c0, g0 = run_hip(logits, targets, llens, tlens)
    c1, g1 = run_hip(logits, targets, llens, tlens, inplace=True)
    np.testing.assert_array_equal(c0, c1)
    np.testing.assert_array_equal(g0, g1)


def test_lattice_alpha_beta_match_oracle_recursion():
    from wenet_celoss_amd.rnnt_loss import rnnt_lattice
    rng = np.random.default_rng(12)
    logits, targets, llens, tlens = make_case(rng, 3, 30, 70, 20)
    x = torch.tensor(logits, device=DEV)
    costs, alpha, beta = rnnt_lattice(x, torch.tensor(targets, device=DEV), torch.tensor(llens, device=DEV),
                                      torch.tensor(tlens, device=DEV))
    alpha, beta = alpha.cpu().numpy(), beta.cpu().numpy()
    lp = torch.log_softmax(torch.tensor(logits, dtype=torch.float64), -1).numpy()
    for b in range(3):
        T, U = llens[b], tlens[b]
        a = np.full((T, U + 1), -np.inf); a[0, 0] = 0
        for t in range(T):
            for u in range(U + 1):
                if t: a[t, u] = np.logaddexp(a[t, u], a[t - 1, u] + lp[b, t - 1, u, 0])
                if u: a[t, u] = np.logaddexp(a[t, u], a[t, u - 1] + lp[b, t, u - 1, targets[b, u - 1]])
        np.testing.assert_allclose(alpha[b, :T, :U + 1], a, rtol=1e-5, atol=1e-4)
        # cost from the forward variable agrees with the kernel's (beta-side) cost
        assert abs(-(a[T - 1, U] + lp[b, T - 1, U, 0]) - costs[b].item()) < 1e-4 * max(1, abs(costs[b].item()))
        assert abs(beta[b, 0, 0] + costs[b].item()) < 1e-6


def test_argument_checks_raise_like_torchaudio():
    import wenet_celoss_amd as w
    x = torch.zeros(2, 4, 3, 8, device=DEV)
    y = torch.ones(2, 2, dtype=torch.int32, device=DEV)
    ll = torch.tensor([4, 3], dtype=torch.int32, device=DEV)
    tl = torch.tensor([2, 1], dtype=torch.int32, device=DEV)
    w.rnnt_loss(x, y, ll, tl, blank=0)
    with pytest.raises(RuntimeError, match="int32"):
        w.rnnt_loss(x, y.long(), ll, tl, blank=0)
    with pytest.raises(RuntimeError, match="input length mismatch"):
        w.rnnt_loss(x, y, torch.tensor([3, 3], dtype=torch.int32, device=DEV), tl, blank=0)
    with pytest.raises(RuntimeError, match="output length mismatch"):
        w.rnnt_loss(x, y, ll, torch.tensor([1, 1], dtype=torch.int32, device=DEV), blank=0)
    with pytest.raises(RuntimeError, match="blank"):
        w.rnnt_loss(x, y, ll, tl, blank=8)
    with pytest.raises(RuntimeError, match="contiguous"):
        w.rnnt_loss(x.transpose(1, 2).contiguous().transpose(1, 2), y, ll, tl, blank=0)
    with pytest.raises(ValueError):
        w.rnnt_loss(x, y, ll, tl, blank=0, reduction="avg")


def test_medium_shape_properties():
    """Size-independent properties at a shape too large for the f64 oracle to be quick:
    every gradient row sums to zero (occupancy in = occupancy out), padding is zero,
    and the threaded f32 port agrees."""
    import wenet_celoss_amd as w
    torch.manual_seed(3)
    B, T, U, V = 4, 200, 40, 1000
    x = torch.randn(B, T, U + 1, V, device=DEV, requires_grad=True)
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=DEV)
    ll = torch.tensor([200, 180, 77, 150], dtype=torch.int32, device=DEV)
    tl = torch.tensor([40, 12, 40, 33], dtype=torch.int32, device=DEV)
    costs = w.rnnt_loss(x, y, ll, tl, blank=0, reduction="none")
    costs.sum().backward()
    g = x.grad
    assert g.sum(-1).abs().max().item() < 2e-5
    c32, g32 = oracle.rnnt_loss_f32(x.detach().cpu().numpy(), y.cpu().numpy(), ll.cpu().numpy(), tl.cpu().numpy())
    np.testing.assert_allclose(costs.detach().cpu().numpy(), c32, rtol=2e-5)
    np.testing.assert_allclose(g.cpu().numpy(), g32, rtol=1e-3, atol=2e-5)


@pytest.mark.parametrize("dtype,tol", [(torch.float16, 2e-3), (torch.bfloat16, 1.6e-2)])
@pytest.mark.parametrize("V", [64, 37])
def test_half_precision_logits(dtype, tol, V):
    """AMP path (executor.py:91 autocast): fp16/bf16 logits in, fp32 arithmetic inside, gradient returned in the
    input dtype.  Checked against the oracle evaluated on the same rounded logits; the tolerance is the output
    dtype's rounding."""
    import wenet_celoss_amd as w
    rng = np.random.default_rng(21)
    logits, targets, llens, tlens = make_case(rng, 3, 19, 7, V)
    xh = torch.tensor(logits, device=DEV).to(dtype)
    x = xh.clone().requires_grad_(True)
    loss = w.rnnt_loss(x, torch.tensor(targets, device=DEV), torch.tensor(llens, device=DEV),
                       torch.tensor(tlens, device=DEV), blank=0, reduction="none")
    assert loss.dtype == dtype and x.dtype == dtype
    loss.float().sum().backward()
    assert x.grad.dtype == dtype
    oc, og = oracle.rnnt_loss_f64(xh.float().cpu().numpy(), targets, llens, tlens)
    np.testing.assert_allclose(loss.detach().float().cpu().numpy(), oc, rtol=tol)
    np.testing.assert_allclose(x.grad.float().cpu().numpy(), og, rtol=tol, atol=tol * 1e-1)
    for b in range(3):
        assert not x.grad[b, llens[b]:].any() and not x.grad[b, :, tlens[b] + 1:].any()


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_full_length_utterance_16bit_logits_vs_f64(dt):
    """The AMP step's loss at the BASELINE lattice scale: one whole utterance (T=1000, U=150, V=5000) of 16-bit logits.
    The kernels read the 16-bit values, compute in fp32 / fp64 as for fp32 logits and round the gradient to the input
    dtype; the float64 oracle gets the same values widened.  Cost within one rounding of the 16-bit format it is returned in;
    gradient within one rounding of the 16-bit format (2^-8 relative for bfloat16, 2^-11 for float16) plus the fp32 path's own 1e-4 / 1e-5."""
    import wenet_celoss_amd as w
    T, U, V = 1000, 150, 5000
    gen = torch.Generator(device=DEV).manual_seed(99)
    x = torch.randn(1, T, U + 1, V, device=DEV, generator=gen).to(dt)
    y = torch.randint(1, V, (1, U), dtype=torch.int32, device=DEV, generator=gen)
    ll = torch.tensor([T], dtype=torch.int32, device=DEV); tl = torch.tensor([U], dtype=torch.int32, device=DEV)
    lg = x.detach().requires_grad_(True)
    cost = w.rnnt_loss(lg, y, ll, tl, blank=0, reduction="sum")
    cost.backward()
    assert lg.grad.dtype == dt
    c64, g64 = oracle.rnnt_loss_f64(x.float().cpu().numpy(), y.cpu().numpy(), np.array([T], np.int32), np.array([U], np.int32))
    ulp = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    assert cost.dtype == dt                                     # the cost comes back in the logits' dtype, as torchaudio's does
    assert abs(c64[0] - float(cost)) <= ulp * abs(c64[0]), (c64[0], float(cost))
    got = lg.grad.float().cpu().numpy()
    err = np.abs(got - g64)
    bound = 1e-5 + (1e-4 + ulp) * np.abs(g64)
    if dt == torch.float16:
        bound = bound + 6e-8                                  # float16 subnormal spacing: tiny gradient entries flush in steps
    worst = float((err / bound).max())
    at = np.unravel_index(int((err / bound).argmax()), err.shape)
    print(f"{dt}: full-length utterance gradient vs f64 oracle, worst |err| / bound = {worst:.3f} at {at}: "
          f"got {got[at]!r}, f64 {g64[at]!r}")
    assert worst <= 1.0


def test_full_baseline_shape_properties():
    """BASELINE.json configs[1] at full size (B=32, T=1000, U=150, V=5000, fp32; 96.6 GB of logits, gradient
    written in place).  north_star's bar -- loss and gradient within 1e-4 relative -- is checked AT THIS LATTICE
    SCALE (T + U = 1150 dependent steps, lattice values ~1e4) against the float64 oracle on two whole utterances:
    b = 0 is full length (T=1000, U=150: 151 000 cells x 5 000 logits, ~3 GB), b = 5 is ragged.  Cost rtol 1e-5,
    whole gradient rtol 1e-4 / atol 1e-5 -- the tolerances of check() above.  The other 30 utterances are covered by
    size-independent properties: (1) forward/backward lattice agreement, -beta(0,0) == -(alpha(T-1,U) +
    log p(blank | T-1,U)); (2) every gradient row sums to zero; (3) padded cells are exactly zero.  (4) the
    threaded fp32 CPU port (the timed cpu_baseline) is compared too, at the looser tolerance its fp32 lattice allows."""
    import wenet_celoss_amd as w
    from wenet_celoss_amd.rnnt_loss import rnnt_lattice
    free, _ = torch.cuda.mem_get_info()
    B, T, U, V = 32, 1000, 150, 5000
    if free < 110e9:
        pytest.skip("needs ~100 GB of free HBM")
    gen = torch.Generator(device=DEV).manual_seed(20260)
    x = torch.empty(B, T, U + 1, V, device=DEV)
    for b in range(B):
        x[b].normal_(generator=gen)
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=DEV, generator=gen)
    cg = torch.Generator().manual_seed(1)
    ll = torch.randint(T // 2, T + 1, (B,), generator=cg).to(torch.int32); ll[0] = T
    tl = torch.randint(U // 3, U + 1, (B,), generator=cg).to(torch.int32); tl[0] = U; tl[1] = U
    assert int(ll[5]) < T and int(tl[5]) < U                           # b = 5 is the ragged one
    ll, tl = ll.to(DEV), tl.to(DEV)
    keep = {b: x[b].cpu().numpy().copy() for b in (0, 5)}            # before the in-place gradient overwrites them
    costs, alpha, beta = rnnt_lattice(x, y, ll, tl)
    for b in range(0, B, 3):
        Tb, Ub = int(ll[b]), int(tl[b])
        lp_blank = torch.log_softmax(x[b, Tb - 1, Ub].double(), -1)[0].item()
        fwd_ll = alpha[b, Tb - 1, Ub].item() + lp_blank
        assert abs(fwd_ll + costs[b].item()) < 2e-3 * max(1.0, abs(fwd_ll) * 1e-3), (b, fwd_ll, costs[b].item())
        assert abs(beta[b, 0, 0].item() + costs[b].item()) < 1e-2
    del alpha, beta
    # in-place gradient through the C-ABI directly (an autograd leaf cannot be overwritten)
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    xd = x.detach()
    wsb = lib.wr_rnnt_workspace_bytes(B, T, U + 1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    c2 = torch.empty(B, device=DEV)
    st = _lib.current_stream(torch.device(DEV)); P = _lib.ptr
    _lib.check(lib.wr_rnnt_loss_fwd(P(xd), 0, P(y), P(ll), P(tl), B, T, U + 1, V, 0, P(c2), P(ws), wsb, st))
    _lib.check(lib.wr_rnnt_loss_bwd(P(xd), 0, P(y), P(ll), P(tl), B, T, U + 1, V, 0, -1.0, None, P(xd), P(ws), wsb, st))
    torch.cuda.synchronize()
    torch.testing.assert_close(c2, costs)
    g = xd                                                            # now holds the gradient
    for b in (0, 7, 31):
        Tb, Ub = int(ll[b]), int(tl[b])
        assert g[b, :Tb, :Ub + 1].sum(-1).abs().max().item() < 3e-5
        assert not g[b, Tb:].any() and not g[b, :, Ub + 1:].any()
    worst = {}
    for b, xb in keep.items():
        lb, ub = np.array([int(ll[b])], np.int32), np.array([int(tl[b])], np.int32)
        xs = np.ascontiguousarray(xb[None, :lb[0], :ub[0] + 1])
        ys = np.ascontiguousarray(y[b:b + 1, :max(ub[0], 1)].cpu().numpy())
        got = g[b, :lb[0], :ub[0] + 1].cpu().numpy()
        # the float64 oracle: the 1e-4 bar itself
        c64, g64 = oracle.rnnt_loss_f64(xs, ys, lb, ub)
        assert abs(c64[0] - costs[b].item()) < 1e-5 * abs(c64[0]), (b, c64[0], costs[b].item())
        err = np.abs(got - g64[0])
        worst[b] = float((err / (1e-5 + 1e-4 * np.abs(g64[0]))).max())
        np.testing.assert_allclose(got, g64[0], rtol=1e-4, atol=1e-5)
        del g64, err
        # secondary: the threaded fp32 port that bench.py times as cpu_baseline (its fp32 lattice is the noisy side)
        c32, g32 = oracle.rnnt_loss_f32(xs, ys, lb, ub, nthreads=16)
        assert abs(c32[0] - costs[b].item()) < 1e-4 * abs(c32[0])
        np.testing.assert_allclose(got, g32[0], rtol=2e-2, atol=3e-5)
        del g32
    print("full-shape gradient vs f64 oracle, worst |err| / (1e-5 + 1e-4 |ref|):", worst)


def _bench_dump(tmp_path, name, *shape_args):
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = tmp_path / name
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--cpu-sample", "0", "--extra-seconds", "0", "--dump-outputs", str(out), *shape_args],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    files = {p.name: np.load(p) for p in out.iterdir()}
    assert all(a.dtype == np.float32 for a in files.values())
    assert sum(p.stat().st_size for p in out.iterdir()) <= 64 * 10**6
    return files


def test_bench_dump_outputs_are_the_last_step_and_repeat(tmp_path):
    """bench.py --dump-outputs: a small shape is written whole and equals the float64 oracle on bench.py's own seeded
    inputs; a gradient above the size cap is written as a seeded sample that is identical from run to run."""
    B, T, U, V = 3, 12, 5, 20
    d = _bench_dump(tmp_path, "small", "--B", str(B), "--T", str(T), "--U", str(U), "--V", str(V))
    assert sorted(d) == ["costs.npy", "grads.npy"] and d["grads.npy"].shape == (B, T, U + 1, V)
    gen = torch.Generator(device=DEV)                   # bench.py's inputs: same seed, same draws, same order
    gen.manual_seed(20260)
    x = torch.empty(B, T, U + 1, V, dtype=torch.float32, device=DEV)
    for b in range(B):
        x[b].normal_(generator=gen)
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=DEV, generator=gen)
    c64, g64 = oracle.rnnt_loss_f64(x.cpu().numpy(), y.cpu().numpy(), np.full(B, T, np.int32), np.full(B, U, np.int32))
    np.testing.assert_allclose(d["costs.npy"], c64, rtol=1e-5)
    np.testing.assert_allclose(d["grads.npy"], g64 / B, rtol=1e-4, atol=1e-6)
    big = ("--B", "4", "--T", "200", "--U", "50", "--V", "500")       # 82 MB of gradient
    d1, d2 = _bench_dump(tmp_path, "big1", *big), _bench_dump(tmp_path, "big2", *big)
    assert sorted(d1) == ["costs.npy", "grads_sample.npy"] and d1["grads_sample.npy"].size > 10**6
    assert all(np.array_equal(d1[k], d2[k]) for k in d1)
    assert np.abs(d1["grads_sample.npy"]).max() > 0


def test_bench_plain_run_leaves_side_measurements_to_full(tmp_path):
    """A plain bench.py run carries the headline and the timed steps' own roofline figures only; --full adds the
    device-copy calibration, the CPU baseline and the secondary measurements, after the same timed steps with the same
    results."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    shape = ["--B", "3", "--T", "12", "--U", "5", "--V", "20", "--steps", "2", "--warmup", "1"]
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full", "--extra-seconds", "1"])):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *shape, *extra,
                            "--dump-outputs", str(tmp_path / mode)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines[mode] = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    plain, full = lines["plain"], lines["full"]
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert plain[k] == full[k], k
    assert plain["value"] > 0 and plain["ms_per_step"] > 0 and plain["roofline"]["avg_ms"] > 0
    assert "cpu_baseline" not in plain and "extra" not in plain and plain["roofline"]["device_copy_GBps"] is None
    assert full["roofline"]["device_copy_GBps"] > 0
    assert full["cpu_baseline"]["value"] > 0 and full["cpu_baseline"]["max_rel_cost_diff_vs_gpu"] < 1e-4
    assert "joiner" in full["extra"] and "error" not in full["extra"]
    for name in ("costs.npy", "grads.npy"):
        assert np.array_equal(np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)), name
