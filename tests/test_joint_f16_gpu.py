"""The float16 single-term joiner kernels (wr_joint_fwd_f16, wr_joint_bwd_dz_f16, wr_joint_bwd_dw_f16) against
f16-operand float64 references (joint_amp_ref.py), the "f16" backward dispatch, and the "autocast" precision.

As in test_joint_amp_gpu.py: exact data (dyadic operands, relu) demands bit equality; tanh data gets the per-element
bound of fp32 accumulation + one f16 ulp of the near-midpoint activations (+ half an ulp of a 16-bit output).  Forward
outputs sit inside sentinel guard bands."""
import os

import pytest
import torch

import joint_amp_ref as R
from test_joint_amp_gpu import (DEV, DZ_SHAPES, FWD_CASES, KIND, OUT, assert_guards, bwd_data, case_data, guarded,
                                knobs, run_fwd, _poison)

pytestmark = pytest.mark.gpu


def _lib():
    from wenet_celoss_amd import _lib as L
    return L, L.load()


def run_fwd16(ep, pp, W, b, act, out_dtype, lens=None):
    """wr_joint_fwd_f16 through the C ABI into a guarded output (guards checked)."""
    L, lib = _lib()
    B, T, J = ep.shape
    U1, V = pp.shape[1], W.shape[0]
    out, buf, pre = guarded((B, T, U1, V), out_dtype)
    wsb = lib.wr_joint_split_workspace_bytes(J, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    ll, tl = lens if lens is not None else (None, None)
    P = L.ptr
    L.check(lib.wr_joint_fwd_f16(P(ep), P(pp), P(W), P(b), P(ll), P(tl), B, T, U1, J, V, R.ACT[act], P(out),
                                 L.dtype_code(out_dtype), P(ws), wsb, L.current_stream(torch.device(DEV))), "wr_joint_fwd_f16")
    torch.cuda.synchronize()
    assert_guards(buf, pre, out.numel() * out.element_size(), "wr_joint_fwd_f16")
    return out


# ---- forward ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KIND)
@pytest.mark.parametrize("out_dtype", OUT, ids=["fp32", "f16", "bf16"])
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_forward_launch_forms(name, out_dtype, kind):
    """Every single-term launch form of joint_fwd_split_launch (test_joint_amp_gpu.FWD_CASES) with f16 operands."""
    c = dict(FWD_CASES[name])
    kn, lens_on = c.pop("knobs", {}), c.pop("lens", False)
    B, T, U1, J, V = c["B"], c["T"], c["U1"], c["J"], c["V"]
    act, (ep, pp, W, b) = case_data(kind, B, T, U1, J, V, seed=B * 1000 + T + J + V + 1)
    lens = R.ragged_lens(B, T, U1, seed=T, device=DEV) if lens_on else None
    with knobs(kn):
        out = run_fwd16(ep, pp, W, b, act, out_dtype, lens)
    ref = R.fwd_ref(ep, pp, W, b, act, out_dtype, lens, operand="f16")
    assert ref.exact == (kind == "exact")
    R.assert_matches(out, ref, f"{name} {out_dtype} {kind}")


def _f16_not_bf16_case(B, T, U1, J, V, seed):
    """Operands exact in f16 but not in bf16: activations relu(ep + pp), odd multiples of 2^-9 in (-1, 1) (up to 9
    significant bits); W = n 2^-12 with n odd in [257, 511] (9 bits) and a random sign; b on the 2^-21 grid."""
    gen = torch.Generator().manual_seed(seed)
    ep = (2 * torch.randint(-128, 128, (B, T, J), generator=gen) + 1).double() * 2.0 ** -9     # odd / 512 in (-1/2, 1/2)
    pp = torch.randint(-128, 129, (B, U1, J), generator=gen).double() * 2.0 ** -8                 # [-1/2, 1/2] on 2^-8
    n = 2 * torch.randint(128, 256, (V, J), generator=gen) + 1
    W = (n * (2 * torch.randint(0, 2, (V, J), generator=gen) - 1)).double() * 2.0 ** -12
    b = torch.randint(-1024, 1025, (V,), generator=gen).double() * 2.0 ** -21
    return tuple(x.float().to(DEV) for x in (ep, pp, W, b))


@pytest.mark.parametrize("out_dtype", OUT, ids=["fp32", "f16", "bf16"])
def test_forward_tells_f16_from_bf16(out_dtype):
    """Operands with 9-11 significant bits: exact in f16, not in bf16; every partial sum exact in fp32.  The f16 kernel
    must match bit for bit; the bf16 kernel on the same data must not (it rounds the operands to 8 bits)."""
    B, T, U1, J, V = 2, 9, 5, 64, 320
    ep, pp, W, b = _f16_not_bf16_case(B, T, U1, J, V, seed=11)
    assert not torch.equal(W, W.bfloat16().float())
    ref = R.fwd_ref(ep, pp, W, b, "relu", out_dtype, operand="f16")
    assert ref.exact, "the data must make every partial sum an fp32 number"
    R.assert_matches(run_fwd16(ep, pp, W, b, "relu", out_dtype), ref, "f16 kernel")
    got_bf16 = run_fwd(ep, pp, W, b, "relu", out_dtype).double().cpu()
    assert not torch.equal(got_bf16, ref.value), "the bf16 kernel should not reproduce the f16-operand result"


def _torch_fp16_mm(ep, pp, W, b):
    """torch.mm on float16 operands on the same device (the vendor GEMM), for the record when the kernel and the
    reference part on subnormals."""
    a = torch.relu(ep[:, :, None, :] + pp[:, None, :, :]).reshape(-1, ep.shape[2]).half()
    return (torch.mm(a, W.half().t(), out_dtype=torch.float32) + b).double().cpu()


@pytest.mark.parametrize("where", ["weights", "activations"])
def test_forward_f16_subnormal_operands(where):
    """f16 subnormal operands (magnitudes 2^-24 .. 2^-15), exact data: the kernel keeps them (bit-exact against the
    reference, which rounds to nearest even into the subnormal range and flushes nothing)."""
    B, T, U1, J, V = 1, 26, 5, 64, 256
    ep, pp, W, b = R.exact_case(B, T, U1, J, V, seed=5)
    gen = torch.Generator().manual_seed(6)
    if where == "weights":
        mag = torch.randint(1, 513, (V, J), generator=gen).float() * 2.0 ** -24              # 2^-24 .. 2^-15
        W = mag * (2 * torch.randint(0, 2, (V, J), generator=gen) - 1).float()
    else:
        ep, pp = ep * 2.0 ** -16, pp * 2.0 ** -16                                          # relu(z): odd * 2^-21 < 2^-15
    b = torch.zeros(V)
    ep, pp, W, b = (x.to(DEV) for x in (ep, pp, W, b))
    ref = R.fwd_ref(ep, pp, W, b, "relu", torch.float32, operand="f16")
    assert ref.exact
    a = R.round_to(torch.relu(ep[:, :, None, :] + pp[:, None, :, :]).cpu(), "f16")
    w16 = R.round_to(W.cpu(), "f16")
    sub = (a.abs() < 2.0 ** -14) & (a != 0) if where == "activations" else (w16.abs() < 2.0 ** -14) & (w16 != 0)
    assert float(sub.double().mean()) > 0.2, "most of these operands must be f16 subnormals"
    out = run_fwd16(ep, pp, W, b, "relu", torch.float32)
    g = out.double().cpu().view(-1, V)
    if not torch.equal(g, ref.value.view(-1, V)):
        tm = _torch_fp16_mm(ep, pp, W, b)
        raise AssertionError(f"f16 subnormal {where}: kernel != reference (max |diff| "
                             f"{float((g - ref.value.view(-1, V)).abs().max())!r}); torch.mm on fp16 "
                             f"{'matches the kernel' if torch.equal(tm, g) else 'does not match the kernel'}, "
                             f"{'matches' if torch.equal(tm, ref.value.view(-1, V)) else 'does not match'} the reference")


def test_forward_overflow_to_inf():
    """W entries beyond the f16 range become +-inf as W.half() makes them (65519 -> 65504, 65520 -> inf by round to
    even, 7e4 -> inf, -1e5 -> -inf); relu activations of 0 then give inf * 0 = NaN.  The pattern of +-inf / NaN must be the
    one the f16-rounded operands predict, every other column bit-exact."""
    B, T, U1, J, V = 1, 8, 4, 32, 64
    ep, pp, W, b = R.exact_case(B, T, U1, J, V, seed=9)
    big = {(3, 5): 7.0e4, (7, 9): -1.0e5, (11, 2): 65519.0, (13, 0): 65520.0, (17, 31): -65520.0}
    for (v, k), x in big.items():
        W[v, k] = x
    assert torch.equal(R.round_to(W, "f16"), W.half().double())
    ep, pp, W, b = (x.to(DEV) for x in (ep, pp, W, b))
    out = run_fwd16(ep, pp, W, b, "relu", torch.float32).double().cpu().view(-1, V)
    cols = sorted({v for v, _ in big})
    rest = [v for v in range(V) if v not in cols]
    ref = R.fwd_ref(ep, pp, W[rest], b[rest], "relu", torch.float32, operand="f16")
    assert ref.exact
    R.assert_matches(out[:, rest], R.Ref(ref.value.view(-1, len(rest)), ref.tol.view(-1, len(rest))), "finite columns")
    # the big columns: float64 elementwise over the f16-rounded operands (IEEE: inf * 0 = NaN, inf + finite = inf)
    a = R.round_to(torch.relu(ep[:, :, None, :] + pp[:, None, :, :]).cpu().reshape(-1, J), "f16")
    w16 = R.round_to(W.cpu()[cols], "f16")
    want = (a[:, None, :] * w16[None, :, :]).sum(-1) + b.cpu()[cols].double()
    got = out[:, cols]
    assert bool(torch.isinf(want).any()) and bool(torch.isnan(want).any())
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN pattern"
    assert torch.equal(torch.isinf(got), torch.isinf(want)), "inf pattern"
    inf = torch.isinf(want)
    assert torch.equal(got[inf], want[inf]), "inf signs"
    fin = torch.isfinite(want)          # the 65504 column: finite, inside the fp32 accumulation bound
    assert bool(((got[fin] - want[fin]).abs() <= R.chain(J) * (a.abs() @ w16.abs().T)[fin]).all())


# ---- backward: the f16 entry points -------------------------------------------------------------------------------
def run_dz16(g, ep, pp, W, act, lens):
    L, lib = _lib()
    B, T, U1, V = g.shape
    J = ep.shape[2]
    wsb = lib.wr_joint_dz_split_workspace_bytes(J, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dz = torch.full((B, T, U1, J), float("nan"), device=DEV)
    h = torch.full_like(dz, float("nan"))
    P = L.ptr
    L.check(lib.wr_joint_bwd_dz_f16(P(g), L.dtype_code(g.dtype), P(ep), P(pp), P(W), P(lens[0]), P(lens[1]), B, T, U1, J,
                                    V, R.ACT[act], P(dz), P(h), P(ws), wsb, L.current_stream(torch.device(DEV))),
            "wr_joint_bwd_dz_f16")
    return dz, h


def run_dw16(g, h, lens):
    L, lib = _lib()
    B, T, U1, V = g.shape
    J = h.shape[-1]
    wsb = lib.wr_joint_dw_split_workspace_bytes(B, T, U1, J, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dw = torch.full((V, J), float("nan"), device=DEV)
    db = torch.full((V,), float("nan"), device=DEV)
    P = L.ptr
    L.check(lib.wr_joint_bwd_dw_f16(P(g), L.dtype_code(g.dtype), P(h), P(lens[0]), P(lens[1]), B, T, U1, J, V, P(dw), P(db),
                                    P(ws), wsb, L.current_stream(torch.device(DEV))), "wr_joint_bwd_dw_f16")
    return dw, db


GRAD = [torch.float32, torch.float16]


@pytest.mark.parametrize("kind", KIND)
@pytest.mark.parametrize("gdt", GRAD, ids=["fp32_grad", "f16_grad"])
@pytest.mark.parametrize("B,T,U1,J,V", DZ_SHAPES)
def test_dz_f16(B, T, U1, J, V, gdt, kind):
    """wr_joint_bwd_dz_f16: dZ = (f16(dY) f16(W)) act'(z) and H against bwd_ref(g16, path="library") -- W rounded to the
    gradient's dtype, which is exactly these kernels' arithmetic; zeros in padded cells."""
    act, ep, pp, W, g = bwd_data(kind, B, T, U1, J, V, seed=T + J + V + 2)
    g = g.to(gdt)
    lens = R.ragged_lens(B, T, U1, seed=J + 1, device=DEV)
    dz, h = run_dz16(g, ep, pp, W, act, lens)
    ref = R.bwd_ref(g.half(), ep, pp, W, act, lens, "library")
    assert ref["dz"].exact == (kind == "exact")
    R.assert_matches(dz, ref["dz"], "dz")
    R.assert_matches(h, ref["h"], "h")
    pad = ~R.cell_mask(B, T, U1, lens, DEV)
    assert bool((dz[pad] == 0).all()) and bool((h[pad] == 0).all())


@pytest.mark.parametrize("kind", KIND)
@pytest.mark.parametrize("gdt", GRAD, ids=["fp32_grad", "f16_grad"])
@pytest.mark.parametrize("B,T,U1,J,V", [(2, 100, 60, 260, 296), (1, 20, 9, 512, 1000), (3, 11, 7, 36, 40)])
def test_dw_f16(B, T, U1, J, V, gdt, kind):
    """wr_joint_bwd_dw_f16: dW = f16(dY)^T f16(H) over valid cells against bwd_ref(g16, "library"); db summed in fp32 from
    the gradient as given."""
    act, ep, pp, W, g = bwd_data(kind, B, T, U1, J, V, seed=T * 3 + J + V + 2)
    g = g.to(gdt)
    lens = R.ragged_lens(B, T, U1, seed=V + 1, device=DEV)
    z = ep[:, :, None, :] + pp[:, None, :, :]
    h = torch.relu(z) if act == "relu" else torch.tanh(z)
    dw, db = run_dw16(g, h.contiguous(), lens)
    ref = R.bwd_ref(g.half(), ep, pp, W, act, lens, "library")
    assert ref["dw"].exact == (kind == "exact")
    R.assert_matches(dw, ref["dw"], "dw")
    R.assert_matches(db, R.bwd_ref(g, ep, pp, W, act, lens, "library")["db"], "db")


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_nonfinite_padding_f16_entries(value):
    """NaN / Inf in every padded cell of the gradient, lengths given: the f16 dZ and dW entries, with fp32 and f16
    gradients, select padded cells away -- results identical to zeros there."""
    B, T, U1, J, V = 3, 20, 9, 256, 520
    act, ep, pp, W, g = bwd_data("exact", B, T, U1, J, V, seed=79)
    lens = R.ragged_lens(B, T, U1, seed=9, device=DEV)
    h = torch.relu(ep[:, :, None, :] + pp[:, None, :, :]).contiguous()
    for gdt in GRAD:
        gz = g.to(gdt)
        gp = _poison(gz, lens, value)
        for a, b in zip(run_dz16(gz, ep, pp, W, act, lens), run_dz16(gp, ep, pp, W, act, lens)):
            assert torch.equal(a, b), f"dz entry {gdt}"
        for a, b in zip(run_dw16(gz, h, lens), run_dw16(gp, h, lens)):
            assert torch.equal(a, b), f"dw entry {gdt}"


# ---- backward: the "f16" dispatch of joint_backward ----------------------------------------------------------------
def _spy(monkeypatch):
    """Record which backward entry points joint_backward reaches (names, with the gradient dtype code of the f16 ones)."""
    from wenet_celoss_amd import joint as jm
    L, lib = _lib()
    calls = []
    for name in ("wr_joint_bwd_dz_f16", "wr_joint_bwd_dz_split_bf16", "wr_joint_bwd_dz_split", "wr_joint_bwd_dz"):
        fn = getattr(lib, name)

        def wrap(*a, _fn=fn, _name=name):
            calls.append((_name, a[1]) if _name.endswith("_f16") else (_name,))
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrap)
    lib_fn = jm._amp_backward_library

    def lib_wrap(*a, **k):
        calls.append(("library", a[1].dtype))
        return lib_fn(*a, **k)
    monkeypatch.setattr(jm, "_amp_backward_library", lib_wrap)
    return calls


def _joint_backward_f16(g, ep, pp, W, act, lens, amp_backward):
    from wenet_celoss_amd.joint import TERMS_F16, joint_backward
    old = os.environ.get("WR_AMP_BACKWARD")
    os.environ["WR_AMP_BACKWARD"] = amp_backward
    try:
        return joint_backward(g, ep, pp, W, lens[0], lens[1], TERMS_F16, True, True, act=R.ACT[act])
    finally:
        if old is None:
            del os.environ["WR_AMP_BACKWARD"]
        else:
            os.environ["WR_AMP_BACKWARD"] = old


def _expect(gdt, V, amp_backward):
    """(entry point reached, reference path, gradient the reference rounds) for "f16" per the dispatch table."""
    from wenet_celoss_amd.joint import _mm_takes_out_dtype
    lib_ok = amp_backward == "library" and _mm_takes_out_dtype()
    if V % 4:
        return ("wr_joint_bwd_dz",), "exact", None
    if gdt == torch.bfloat16:
        if lib_ok and V % 8 == 0:
            return ("library", torch.bfloat16), "library", None
        return ("wr_joint_bwd_dz_split_bf16",) if V % 8 == 0 else ("wr_joint_bwd_dz_split",), "kernels", None
    if gdt == torch.float16 and V % 8 == 0:
        if lib_ok:
            return ("library", torch.float16), "library", None
        return ("wr_joint_bwd_dz_f16", 1), "library", torch.float16
    return ("wr_joint_bwd_dz_f16", 0), "library", torch.float16


@pytest.mark.parametrize("V", [520, 300, 298], ids=["V%8==0", "V%8", "V%4"])
@pytest.mark.parametrize("amp_backward", ["library", "kernels"])
@pytest.mark.parametrize("gdt", [torch.float32, torch.float16, torch.bfloat16], ids=["fp32", "f16", "bf16"])
def test_f16_backward_dispatch(monkeypatch, gdt, amp_backward, V):
    """joint_backward for precision "f16": float16 gradient -> library GEMMs (default) or the f16 kernels taking it as it
    is; float32 -> the f16 kernels rounding in-kernel; bfloat16 (bf16 autocast) -> the "bf16" backward; V % 8 != 0 ->
    the f16 kernels on a widened gradient; V % 4 != 0 -> the exact kernels.  Exact data: each result bit-exact against
    the reference of the path it took; lengths given, NaN in every padded cell of the gradient."""
    B, T, U1, J = 3, 20, 9, 260                          # J = 260: a column-tile tail
    act, ep, pp, W, g = bwd_data("exact", B, T, U1, J, V, seed=V + 3)
    g = g.to(gdt)
    lens = R.ragged_lens(B, T, U1, seed=4, device=DEV)
    gp = _poison(g, lens, float("nan"))
    calls = _spy(monkeypatch)
    res = _joint_backward_f16(gp, ep, pp, W, act, lens, amp_backward)
    want_call, path, rnd = _expect(gdt, V, amp_backward)
    assert calls and calls[0] == want_call, calls
    ref = R.bwd_ref(g.to(rnd) if rnd is not None else g, ep, pp, W, act, lens, path)
    for got, key in zip(res, ("d_ep", "d_pp", "dw", "db")):
        assert torch.isfinite(got).all(), key
        R.assert_matches(got, ref[key], key)


# ---- modes ---------------------------------------------------------------------------------------------------------
def _joint_run(prec, enc, pred, dt, V=320, E=64, J=256, seed=21):
    import wenet_celoss_amd as w
    torch.manual_seed(seed)
    m = w.TransducerJoint(V, E, E, J, precision=prec).to(DEV)
    e = enc.clone().requires_grad_(True)
    p = pred.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=dt or torch.float16, enabled=dt is not None):
        out = m(e, p)
    out.float().pow(2).mean().backward()
    return out.detach(), [e.grad, p.grad] + [q.grad for q in m.parameters()]


@pytest.mark.parametrize("dt,same_as", [(None, "fp32"), (torch.bfloat16, "bf16"), (torch.float16, "f16")],
                         ids=["no_autocast", "bf16_autocast", "f16_autocast"])
def test_autocast_precision_is_bit_identical(dt, same_as):
    """precision="autocast" = "fp32" outside autocast, "bf16" under bf16 autocast, "f16" under fp16 autocast: logits and
    every gradient bit-identical."""
    B, T, U1, E = 2, 30, 7, 64
    gen = torch.Generator().manual_seed(2)
    enc = torch.randn(B, T, E, generator=gen).to(DEV)
    pred = torch.randn(B, U1, E, generator=gen).to(DEV)
    o1, g1 = _joint_run("autocast", enc, pred, dt)
    o2, g2 = _joint_run(same_as, enc, pred, dt)
    assert o1.dtype == o2.dtype == (dt or torch.float32)
    assert torch.equal(o1, o2)
    for a, b in zip(g1, g2):
        assert torch.equal(a, b)


def _transducer(prec, V, E):
    import wenet_celoss_amd as w
    m = w.Transducer.__new__(w.Transducer)
    torch.nn.Module.__init__(m)
    m.joint = w.TransducerJoint(V, E, E, 256, precision=prec)
    m.fused_loss, m.ignore_id, m.blank = True, -1, 0
    return m.to(DEV)


def test_autocast_precision_fused_loss_matches_fp32():
    """Transducer.compute_loss outside autocast with "autocast" takes the fused joiner + loss node as "fp32" does: the
    same loss and gradients, bit for bit."""
    B, T, U, E, V = 3, 25, 6, 64, 320
    gen = torch.Generator().manual_seed(8)
    enc = torch.randn(B, T, E, generator=gen).to(DEV)
    pred = torch.randn(B, U + 1, E, generator=gen).to(DEV)
    text = torch.randint(1, V, (B, U), generator=gen).to(DEV)
    el = torch.tensor([T, 20, 11], device=DEV)
    tl = torch.tensor([U, 4, 2], device=DEV)
    res = []
    for prec in ("autocast", "fp32"):
        torch.manual_seed(1)
        m = _transducer(prec, V, E)
        e = enc.clone().requires_grad_(True)
        joint_out, loss = m.compute_loss(e, el, pred, text, tl)
        assert joint_out is None                          # the fused node
        loss.backward()
        res.append([loss.detach(), e.grad] + [q.grad for q in m.joint.parameters()])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def test_f16_closer_to_reference_graph_than_bf16():
    """Under fp16 autocast the reference module graph (TransducerJoint._export_forward: fp16 Linear layers, add, tanh,
    fp16 ffn_out) is the target.  Measured in float64 against its logits, the median |error| of "f16" must be at most half
    that of "bf16": operand rounding 2^-11 against 2^-8, with the reference's own fp16 add and tanh on top."""
    import wenet_celoss_amd as w
    B, T, U1, E, J, V = 2, 40, 9, 128, 256, 512
    torch.manual_seed(13)
    m = w.TransducerJoint(V, E, E, J).to(DEV)
    enc = torch.randn(B, T, E, device=DEV)
    pred = torch.randn(B, U1, E, device=DEV)
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.float16):
        ref = m._export_forward(enc, pred).double()
        err = {}
        for prec in ("f16", "bf16"):
            m.precision = prec
            out = m(enc, pred)
            assert out.dtype == torch.float16
            err[prec] = float((out.double() - ref).abs().median())
    ratio = err["f16"] / err["bf16"]
    print(f"median |error| vs the reference graph: f16 {err['f16']:.3e}  bf16 {err['bf16']:.3e}  ratio {ratio:.3f}")
    assert ratio <= 0.5, err


def test_fp16_autocast_step_with_grad_scaler():
    """One fp16-autocast training step of the loss block with GradScaler and precision="f16", each stage against float64
    on its own actual inputs: logits (f16 operands), loss and scaled 16-bit logits gradient (float64 oracle), the joiner
    backward on that gradient (library path: W and H in f16), then unscale_ / step."""
    import numpy as np
    import oracle
    import wenet_celoss_amd as w
    B, T, U, E, P, J, V = 2, 50, 15, 64, 64, 512, 2000
    S = 1024.0
    torch.manual_seed(321)
    m = w.TransducerJoint(V, E, P, J, precision="f16").to(DEV)
    opt = torch.optim.SGD(m.parameters(), lr=0.5)
    scaler = torch.amp.GradScaler("cuda", init_scale=S, growth_interval=1000)
    enc = torch.randn(B, T, E, device=DEV)
    pred = torch.randn(B, U + 1, P, device=DEV)
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=DEV)
    ll = torch.tensor([T, 33], dtype=torch.int32, device=DEV)
    tl = torch.tensor([U, 9], dtype=torch.int32, device=DEV)
    saved = {}
    with torch.autocast("cuda", dtype=torch.float16):
        ep, pp = m.pre_activation(enc, pred)
        ep = ep.float().detach().requires_grad_(True)
        pp = pp.float().detach().requires_grad_(True)
        logits = w.joint_logits(ep, pp, m.ffn_out.weight, m.ffn_out.bias, precision=m.precision)
        assert logits.dtype == torch.float16
        logits.register_hook(lambda g: saved.setdefault("g", g))
        loss = w.rnnt_loss(logits, y, ll, tl, blank=0, reduction="sum")
    scaler.scale(loss).backward()
    W0, b0 = m.ffn_out.weight.detach().clone(), m.ffn_out.bias.detach().clone()
    # stage 1: the forward on its own inputs, f16 operands
    R.assert_matches(logits, R.fwd_ref(ep.detach(), pp.detach(), W0, b0, "tanh", torch.float16, operand="f16"), "logits")
    # stage 2: loss and the scaled 16-bit gradient on the kernel's own logits
    x = logits.detach().float().cpu().numpy()
    c64, g64 = oracle.rnnt_loss_f64(x, y.cpu().numpy(), ll.cpu().numpy(), tl.cpu().numpy())
    ulp = 2.0 ** -11
    assert abs(c64.sum() - float(loss)) <= ulp * abs(c64.sum()), (c64.sum(), float(loss))
    gk = saved["g"]
    assert gk.dtype == torch.float16 and bool(torch.isfinite(gk).all())
    got = gk.float().cpu().numpy() / S
    bound = 1e-5 + (1e-4 + ulp) * np.abs(g64) + 6e-8 / S
    assert float((np.abs(got - g64) / bound).max()) <= 1.0
    # stage 3: the joiner backward on the kernel's own (scaled) gradient -- library GEMMs or, without torch.mm(out_dtype=),
    # the f16 kernels taking it as it is: the same operand roundings (W and H in f16, dY as it is)
    ref = R.bwd_ref(gk, ep.detach(), pp.detach(), W0, "tanh", None, "library")
    R.assert_matches(m.ffn_out.weight.grad, ref["dw"], "ffn_out.weight.grad")
    # the bias gradient (wr_joint_db_f16) is two recursive fp32 sums -- rows of a part, then up to 1024 parts in order --
    # of same-signed terms where the loss is confident: the recursive-summation bound gamma(n) sum |dY|, not the MFMA chain's
    M = B * T * (U + 1)
    parts = min(M, 1024)
    n = parts + -(-M // parts)
    mag = torch.where(R.cell_mask(B, T, U + 1, (ll, tl), "cpu").reshape(-1, 1), gk.double().cpu().reshape(-1, V),
                      torch.zeros((), dtype=torch.float64)).abs().sum(0)
    R.assert_matches(m.ffn_out.bias.grad, R.Ref(ref["db"].value, n * 2.0 ** -24 / (1 - n * 2.0 ** -24) * mag),
                     "ffn_out.bias.grad")
    R.assert_matches(ep.grad, ref["d_ep"], "d_ep")
    R.assert_matches(pp.grad, ref["d_pp"], "d_pp")
    # stage 4: unscale (a power of two: exact) and the optimiser step
    gw = m.ffn_out.weight.grad.clone()
    scaler.unscale_(opt)
    assert torch.equal(m.ffn_out.weight.grad, gw / S)
    scaler.step(opt)
    scaler.update()
    assert scaler.get_scale() == S                       # no inf / NaN found: the step was taken
    assert torch.equal(m.ffn_out.weight.detach(), W0 - 0.5 * (gw / S))
