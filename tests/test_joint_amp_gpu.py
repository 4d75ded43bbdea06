"""The single-term (AMP) joiner kernels against operand-rounded float64 references (joint_amp_ref.py), at every launch
form of the forward and on every backward entry point of the --use_amp step.

Two kinds of data per case:
  * exact -- dyadic operands (relu / hardtanh) on which every partial sum is an fp32 number: the kernel must match the
    reference BIT FOR BIT, whatever its tiling, column slabs, split-K partials or reduction order;
  * tanh  -- normal draws: per-element bound = fp32 accumulation error + one operand ulp of the near-midpoint
    activations (+ half an ulp of a 16-bit output), 100-1000x tighter than an r.m.s.-relative bar.
Every forward output is allocated inside guard bands of a sentinel byte that must be intact after the call (tail stores
that escape the tensor), and every tuning knob a test sets is restored in `finally`.
"""
import contextlib
import os

import pytest
import torch

import joint_amp_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0xA5
GUARD = 512                                              # bytes of guard band on each side of an output


def _lib():
    from wenet_celoss_amd import _lib as L
    return L, L.load()


@contextlib.contextmanager
def knobs(settings):
    """wr_tune_set for the duration of a test; every key restored to its default (0 for 7, 12, 13) afterwards."""
    L, lib = _lib()
    try:
        for k, v in settings.items():
            assert lib.wr_tune_set(k, v) == 0
        yield
    finally:
        for k in settings:
            lib.wr_tune_set(k, 0)


def guarded(shape, dtype, byte_off=0):
    """(tensor, buffer, pre): an uninitialised-looking tensor of `shape` at 16-byte alignment + byte_off inside a buffer
    whose every byte is SENTINEL."""
    esz = torch.empty((), dtype=dtype).element_size()
    n = 1
    for s in shape:
        n *= s
    pre = GUARD + byte_off
    buf = torch.full((pre + n * esz + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    t = buf[pre:pre + n * esz].view(dtype).view(shape)
    assert t.data_ptr() % 16 == byte_off % 16
    return t, buf, pre


def assert_guards(buf, pre, nbytes, what=""):
    head, tail = buf[:pre], buf[pre + nbytes:]
    for name, g in (("before", head), ("after", tail)):
        bad = (g != SENTINEL).nonzero()
        assert bad.numel() == 0, f"{what}: store {name} the output at byte {int(bad[0])} of the guard band"


def case_data(kind, B, T, U1, J, V, seed):
    act = "relu" if kind == "exact" else "tanh"
    gen = R.exact_case if kind == "exact" else R.random_case
    return act, tuple(x.to(DEV) for x in gen(B, T, U1, J, V, seed=seed))


def run_fwd(ep, pp, W, b, act, out_dtype, lens=None, byte_off=0):
    """wr_joint_fwd_split(terms=1) through the C ABI into a guarded output; returns the output (guards checked)."""
    L, lib = _lib()
    B, T, J = ep.shape
    U1, V = pp.shape[1], W.shape[0]
    out, buf, pre = guarded((B, T, U1, V), out_dtype, byte_off)
    wsb = lib.wr_joint_split_workspace_bytes(J, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    ll, tl = lens if lens is not None else (None, None)
    P = L.ptr
    L.check(lib.wr_joint_fwd_split(P(ep), P(pp), P(W), P(b), P(ll), P(tl), B, T, U1, J, V, R.ACT[act], 1, P(out),
                                   L.dtype_code(out_dtype), P(ws), wsb, L.current_stream(torch.device(DEV))),
            "wr_joint_fwd_split")
    torch.cuda.synchronize()
    assert_guards(buf, pre, out.numel() * out.element_size(), "wr_joint_fwd_split")
    return out


OUT = [torch.float32, torch.float16, torch.bfloat16]
KIND = ["exact", "tanh"]

# launch forms of joint_fwd_split_launch (single-term mode); M = B * T * U1
FWD_CASES = {
    "two_per_cu_one_slab_partial_tile": dict(B=1, T=26, U1=5, J=128, V=256),       # M = 130: a partial 64-cell tile
    "two_per_cu_auto_2_slabs": dict(B=1, T=10, U1=7, J=512, V=5000),               # W image 5.2 MB
    "two_per_cu_auto_4_slabs": dict(B=1, T=10, U1=7, J=512, V=6208),               # 6.4 MB
    "two_per_cu_auto_8_slabs": dict(B=1, T=10, U1=7, J=512, V=12352),              # 12.6 MB
    "forced_2_slabs_uneven": dict(B=2, T=9, U1=5, J=128, V=320, knobs={7: 2}),     # 5 column pairs: 3 + 2
    "forced_3_slabs": dict(B=2, T=9, U1=5, J=128, V=320, knobs={7: 3}),            # 2 + 2 + 1
    "forced_8_slabs_some_empty": dict(B=2, T=9, U1=5, J=128, V=320, knobs={7: 8}),  # 5 slabs of one pair, 3 of none
    "one_per_cu_v300": dict(B=2, T=9, U1=5, J=128, V=300),                         # 16-bit rows not 16-byte multiples
    "one_per_cu_odd_v517": dict(B=3, T=11, U1=7, J=256, V=517),
    "one_per_cu_bias_slab_split": dict(B=1, T=5, U1=4, J=512, V=24322),            # bias slab > LDS: extra slabs
    "forced_one_per_cu": dict(B=1, T=26, U1=5, J=256, V=320, knobs={12: 1}),       # staged store of the one-per-CU form
    "wide_128_cells": dict(B=1, T=512, U1=130, J=128, V=320, knobs={12: 2}),       # M >= 65536
    "wide_128_cells_transposed": dict(B=1, T=512, U1=130, J=128, V=320, knobs={12: 2, 13: 1}),
    "transposed": dict(B=1, T=26, U1=5, J=256, V=320, knobs={13: 1}),
    "transposed_v300_tail": dict(B=2, T=9, U1=5, J=128, V=300, knobs={13: 1}),
    "transposed_one_per_cu": dict(B=2, T=9, U1=5, J=128, V=320, knobs={12: 1, 13: 1}),
    "j4": dict(B=2, T=5, U1=3, J=4, V=64),
    "j36": dict(B=2, T=13, U1=4, J=36, V=96),
    "j500": dict(B=1, T=20, U1=7, J=500, V=200),
    "j512": dict(B=1, T=20, U1=7, J=512, V=520),
    "lengths": dict(B=3, T=40, U1=9, J=256, V=320, lens=True),
    "lengths_one_per_cu": dict(B=3, T=40, U1=9, J=128, V=300, lens=True),
}


@pytest.mark.parametrize("kind", KIND)
@pytest.mark.parametrize("out_dtype", OUT, ids=["fp32", "f16", "bf16"])
@pytest.mark.parametrize("name", list(FWD_CASES))
def test_forward_launch_forms(name, out_dtype, kind):
    c = dict(FWD_CASES[name])
    kn, lens_on = c.pop("knobs", {}), c.pop("lens", False)
    B, T, U1, J, V = c["B"], c["T"], c["U1"], c["J"], c["V"]
    act, (ep, pp, W, b) = case_data(kind, B, T, U1, J, V, seed=B * 1000 + T + J + V)
    lens = R.ragged_lens(B, T, U1, seed=T, device=DEV) if lens_on else None
    with knobs(kn):
        out = run_fwd(ep, pp, W, b, act, out_dtype, lens)
    ref = R.fwd_ref(ep, pp, W, b, act, out_dtype, lens)
    assert ref.exact == (kind == "exact")
    R.assert_matches(out, ref, f"{name} {out_dtype} {kind}")


@pytest.mark.parametrize("kind", KIND)
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("out_dtype,byte_off", [(torch.float16, 2), (torch.float16, 4), (torch.float16, 8),
                                                (torch.bfloat16, 2), (torch.bfloat16, 8), (torch.float32, 4),
                                                (torch.float32, 8)])
def test_forward_misaligned_output(out_dtype, byte_off, transposed, kind):
    """An output view that breaks 16-byte alignment: the two-per-CU gate (staged form) and the vector stores of the
    transposed form must fall back to a path that stores exactly the tensor's elements."""
    B, T, U1, J, V = 1, 26, 5, 128, 320
    act, (ep, pp, W, b) = case_data(kind, B, T, U1, J, V, seed=byte_off)
    with knobs({13: 1} if transposed else {}):
        out = run_fwd(ep, pp, W, b, act, out_dtype, byte_off=byte_off)
    R.assert_matches(out, R.fwd_ref(ep, pp, W, b, act, out_dtype), f"offset {byte_off}")


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("act", list(R.ACT))
def test_forward_every_activation(act, out_dtype):
    B, T, U1, J, V = 2, 9, 5, 256, 320
    ep, pp, W, b = (x.to(DEV) for x in R.random_case(B, T, U1, J, V, seed=R.ACT[act]))
    out = run_fwd(ep, pp, W, b, act, out_dtype)
    R.assert_matches(out, R.fwd_ref(ep, pp, W, b, act, out_dtype), act)


# ---- backward -----------------------------------------------------------------------------------------------------
def bwd_data(kind, B, T, U1, J, V, seed):
    act, (ep, pp, W, _) = case_data(kind, B, T, U1, J, V, seed)
    if kind == "exact":
        g = R.exact_grad(B, T, U1, V, seed=seed).to(DEV)
    else:
        g = torch.randn(B, T, U1, V, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    return act, ep, pp, W, g


def run_dz(g, ep, pp, W, act, lens, g16):
    L, lib = _lib()
    B, T, U1, V = g.shape
    J = ep.shape[2]
    wsb = lib.wr_joint_dz_split_workspace_bytes(J, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dz = torch.full((B, T, U1, J), float("nan"), device=DEV)
    h = torch.full_like(dz, float("nan"))
    fn = lib.wr_joint_bwd_dz_split_bf16 if g16 else lib.wr_joint_bwd_dz_split
    P = L.ptr
    L.check(fn(P(g), P(ep), P(pp), P(W), P(lens[0]), P(lens[1]), B, T, U1, J, V, R.ACT[act], 1, P(dz), P(h), P(ws), wsb,
               L.current_stream(torch.device(DEV))), "wr_joint_bwd_dz_split")
    return dz, h


def run_dw(g, h, lens, g16):
    L, lib = _lib()
    B, T, U1, V = g.shape
    J = h.shape[-1]
    wsb = lib.wr_joint_dw_split_workspace_bytes(B, T, U1, J, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    dw = torch.full((V, J), float("nan"), device=DEV)
    db = torch.full((V,), float("nan"), device=DEV)
    fn = lib.wr_joint_bwd_dw_split_bf16 if g16 else lib.wr_joint_bwd_dw_split
    P = L.ptr
    L.check(fn(P(g), P(h), P(lens[0]), P(lens[1]), B, T, U1, J, V, 1, P(dw), P(db), P(ws), wsb,
               L.current_stream(torch.device(DEV))), "wr_joint_bwd_dw_split")
    return dw, db


def run_db16(g, lens):
    L, lib = _lib()
    B, T, U1, V = g.shape
    wsb = lib.wr_joint_db_workspace_bytes(B, T, U1, V)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    db = torch.full((V,), float("nan"), device=DEV)
    fn = lib.wr_joint_db_bf16 if g.dtype == torch.bfloat16 else lib.wr_joint_db_f16
    P = L.ptr
    L.check(fn(P(g), P(lens[0]), P(lens[1]), B, T, U1, V, P(db), P(ws), wsb, L.current_stream(torch.device(DEV))),
            "wr_joint_db_16")
    return db


DZ_SHAPES = [
    (2, 9, 5, 512, 296),       # n_jt == 16 (the FULL instantiation); V % 32 == 8
    (1, 70, 3, 480, 1000),     # FULL at J = 480; V % 32 == 8
    (2, 13, 4, 260, 520),      # non-FULL; V % 32 == 8
    (1, 33, 2, 36, 40),        # one column tile, V < 64
    (3, 20, 9, 128, 5000),     # the shipped vocabulary, ragged lengths over several 128-cell tiles
]


@pytest.mark.parametrize("kind", KIND)
@pytest.mark.parametrize("g16", [False, True], ids=["fp32_grad", "bf16_grad"])
@pytest.mark.parametrize("B,T,U1,J,V", DZ_SHAPES)
def test_dz_split_single_term(B, T, U1, J, V, g16, kind):
    """wr_joint_bwd_dz_split / _bf16, terms=1: dZ (dY and W rounded to bf16) and H against float64, with lengths --
    dZ and H exactly zero in padded cells."""
    act, ep, pp, W, g = bwd_data(kind, B, T, U1, J, V, seed=T + J + V)
    if g16:
        g = g.to(torch.bfloat16)
    lens = R.ragged_lens(B, T, U1, seed=J, device=DEV)
    dz, h = run_dz(g, ep, pp, W, act, lens, g16)
    ref = R.bwd_ref(g, ep, pp, W, act, lens, "kernels")
    assert ref["dz"].exact == (kind == "exact")
    R.assert_matches(dz, ref["dz"], "dz")
    R.assert_matches(h, ref["h"], "h")
    pad = ~R.cell_mask(B, T, U1, lens, DEV)
    assert bool((dz[pad] == 0).all()) and bool((h[pad] == 0).all())


@pytest.mark.parametrize("kind", KIND)
@pytest.mark.parametrize("g16", [False, True], ids=["fp32_grad", "bf16_grad"])
@pytest.mark.parametrize("B,T,U1,J,V", [(2, 100, 60, 260, 296),     # M = 12000: several split-K partials; partial 256-blocks
                                        (1, 20, 9, 512, 1000),
                                        (3, 11, 7, 36, 40)])
def test_dw_split_single_term(B, T, U1, J, V, g16, kind):
    """wr_joint_bwd_dw_split / _bf16, terms=1: dW = bf16(dY)^T bf16(H) and db over valid cells against float64."""
    act, ep, pp, W, g = bwd_data(kind, B, T, U1, J, V, seed=T * 3 + J + V)
    if g16:
        g = g.to(torch.bfloat16)
    lens = R.ragged_lens(B, T, U1, seed=V, device=DEV)
    z = (ep[:, :, None, :] + pp[:, None, :, :])
    h = torch.relu(z) if act == "relu" else torch.tanh(z)
    dw, db = run_dw(g, h.contiguous(), lens, g16)
    ref = R.bwd_ref(g, ep, pp, W, act, lens, "kernels")
    assert ref["dw"].exact == (kind == "exact")
    R.assert_matches(dw, ref["dw"], "dw")
    R.assert_matches(db, ref["db"], "db")


def _joint_backward(g, ep, pp, W, act, lens, amp_backward, need=(True, True), zero_pad=False):
    from wenet_celoss_amd.joint import joint_backward
    old = os.environ.get("WR_AMP_BACKWARD")
    os.environ["WR_AMP_BACKWARD"] = amp_backward
    try:
        return joint_backward(g, ep, pp, W, lens[0], lens[1], 1, need[0], need[1], gout_zero_in_padding=zero_pad,
                              act=R.ACT[act])
    finally:
        if old is None:
            del os.environ["WR_AMP_BACKWARD"]
        else:
            os.environ["WR_AMP_BACKWARD"] = old


def _check_backward(res, ref, what):
    for got, key in zip(res, ("d_ep", "d_pp", "dw", "db")):
        R.assert_matches(got, ref[key], f"{what} {key}")


@pytest.mark.parametrize("kind", KIND)
@pytest.mark.parametrize("amp_backward", ["library", "kernels"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_joint_backward_amp_paths(dt, amp_backward, kind):
    """joint_backward (terms=1) with a 16-bit logits gradient, the library GEMM path and WR_AMP_BACKWARD=kernels, each
    against bwd_ref with its own operand roundings (library: W, H in the gradient's dtype; kernels: bf16)."""
    from wenet_celoss_amd.joint import _mm_takes_out_dtype
    if amp_backward == "library" and not _mm_takes_out_dtype():
        pytest.skip("this PyTorch has no torch.mm(out_dtype=): the library form is not reachable")
    B, T, U1, J, V = 3, 20, 9, 512, 1000
    act, ep, pp, W, g = bwd_data(kind, B, T, U1, J, V, seed=41)
    g = g.to(dt)
    lens = R.ragged_lens(B, T, U1, seed=5, device=DEV)
    res = _joint_backward(g, ep, pp, W, act, lens, amp_backward)
    ref = R.bwd_ref(g, ep, pp, W, act, lens, amp_backward)
    _check_backward(res, ref, amp_backward)


@pytest.mark.parametrize("V,path", [(300, "kernels"), (298, "exact")])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_joint_backward_fallbacks(dt, V, path):
    """ok16 false: V % 8 != 0 with V % 4 == 0 runs the fp32 split entries on a widened gradient (bf16 operands);
    V % 4 != 0 runs the exact-fp32 kernels.  Exact data: bitwise against the same reference."""
    B, T, U1, J = 2, 17, 6, 256
    act, ep, pp, W, g = bwd_data("exact", B, T, U1, J, V, seed=V)
    g = g.to(dt)
    lens = R.ragged_lens(B, T, U1, seed=3, device=DEV)
    res = _joint_backward(g, ep, pp, W, act, lens, "library")
    _check_backward(res, R.bwd_ref(g, ep, pp, W, act, lens, path), f"V={V}")


# ---- non-finite values in the padded cells of the gradient --------------------------------------------------------
def _poison(g, lens, value):
    m = R.cell_mask(*g.shape[:3], lens, DEV)
    return torch.where(m[..., None], g, torch.tensor(value, dtype=g.dtype, device=DEV))


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_nonfinite_padding_split_entries(value):
    """NaN / Inf in every padded cell of the gradient, lengths given: the two dZ entries, the two dW entries and the two
    16-bit bias-gradient entries select padded cells away -- results identical to zeros there."""
    B, T, U1, J, V = 3, 20, 9, 256, 520
    act, ep, pp, W, g = bwd_data("exact", B, T, U1, J, V, seed=77)
    lens = R.ragged_lens(B, T, U1, seed=9, device=DEV)
    h = torch.relu(ep[:, :, None, :] + pp[:, None, :, :]).contiguous()
    for g16 in (False, True):
        gz = g.to(torch.bfloat16) if g16 else g
        gp = _poison(gz, lens, value)
        for a, b in zip(run_dz(gz, ep, pp, W, act, lens, g16), run_dz(gp, ep, pp, W, act, lens, g16)):
            assert torch.equal(a, b), f"dz entry g16={g16}"
        for a, b in zip(run_dw(gz, h, lens, g16), run_dw(gp, h, lens, g16)):
            assert torch.equal(a, b), f"dw entry g16={g16}"
    for dt in (torch.bfloat16, torch.float16):
        gz = g.to(dt)
        assert torch.equal(run_db16(gz, lens), run_db16(_poison(gz, lens, value), lens)), f"db entry {dt}"


@pytest.mark.parametrize("value", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("V", [520, 300, 298], ids=["ok16", "V%8", "V%4"])
@pytest.mark.parametrize("amp_backward", ["library", "kernels"])
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_nonfinite_padding_joint_backward(dt, amp_backward, V, value):
    """joint_backward with lengths and gout_zero_in_padding=False, NaN / Inf in every padded cell: every output equal to
    the zero-padding run's, and to float64.  The library path used to form d_w = dY^T H as a plain GEMM relying on
    H == 0 in padded cells; 0 * NaN poisoned every column of d_w.  _amp_backward_library now selects padded rows of the
    gradient to zero when the caller does not guarantee zeros there (no extra pass when it does)."""
    B, T, U1, J = 3, 20, 9, 256
    act, ep, pp, W, g = bwd_data("exact", B, T, U1, J, V, seed=78)
    g = g.to(dt)
    lens = R.ragged_lens(B, T, U1, seed=9, device=DEV)
    base = _joint_backward(g, ep, pp, W, act, lens, amp_backward)
    got = _joint_backward(_poison(g, lens, value), ep, pp, W, act, lens, amp_backward)
    for a, b, k in zip(base, got, ("d_ep", "d_pp", "d_w", "d_b")):
        assert torch.isfinite(b).all(), f"{k}: non-finite values from the padded cells"
        assert torch.equal(a, b), k
    path = "exact" if V % 4 else ("kernels" if V % 8 or amp_backward == "kernels" else "library")
    _check_backward(got, R.bwd_ref(g, ep, pp, W, act, lens, path), "poisoned")


# ---- one AMP step, each stage against float64 on its own actual inputs --------------------------------------------
@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16], ids=["bf16", "f16"])
def test_amp_step_stage_by_stage(dt):
    """TransducerJoint(precision="bf16") + rnnt_loss under autocast at B=3, T=60, U=20, J=512, V=5000 (the two-slab
    forward), ragged.  Logits against fwd_ref on the module's own ep / pp; loss and 16-bit logits gradient against the
    float64 oracle on the kernel's own 16-bit logits (the bars of test_full_length_utterance_16bit_logits_vs_f64);
    weight / bias / ep / pp gradients against bwd_ref on the kernel's own 16-bit gradient.  No stage inherits the
    error of the one before it."""
    import numpy as np
    import oracle
    import wenet_celoss_amd as w
    from wenet_celoss_amd.joint import _mm_takes_out_dtype
    B, T, U, E, P, J, V = 3, 60, 20, 64, 64, 512, 5000
    torch.manual_seed(123)
    m = w.TransducerJoint(V, E, P, J, precision="bf16").to(DEV)
    enc = torch.randn(B, T, E, device=DEV)
    pred = torch.randn(B, U + 1, P, device=DEV)
    y = torch.randint(1, V, (B, U), dtype=torch.int32, device=DEV)
    ll = torch.tensor([T, 41, 17], dtype=torch.int32, device=DEV)
    tl = torch.tensor([U, 13, 4], dtype=torch.int32, device=DEV)
    saved = {}
    with torch.autocast("cuda", dtype=dt):
        ep, pp = m.pre_activation(enc, pred)
        ep = ep.float().detach().requires_grad_(True)
        pp = pp.float().detach().requires_grad_(True)
        logits = w.joint_logits(ep, pp, m.ffn_out.weight, m.ffn_out.bias, precision="bf16")
        assert logits.dtype == dt
        logits.register_hook(lambda g: saved.setdefault("g", g))
        loss = w.rnnt_loss(logits, y, ll, tl, blank=0, reduction="sum")
    loss.float().backward()
    # stage 1: the forward on its own inputs
    R.assert_matches(logits, R.fwd_ref(ep.detach(), pp.detach(), m.ffn_out.weight.detach(), m.ffn_out.bias.detach(),
                                       "tanh", dt), "logits")
    # stage 2: the loss on the kernel's own 16-bit logits
    x = logits.detach().float().cpu().numpy()
    c64, g64 = oracle.rnnt_loss_f64(x, y.cpu().numpy(), ll.cpu().numpy(), tl.cpu().numpy())
    ulp = 2.0 ** -8 if dt == torch.bfloat16 else 2.0 ** -11
    assert abs(c64.sum() - float(loss)) <= ulp * abs(c64.sum()), (c64.sum(), float(loss))
    gk = saved["g"]
    assert gk.dtype == dt
    got = gk.float().cpu().numpy()
    bound = 1e-5 + (1e-4 + ulp) * np.abs(g64)
    if dt == torch.float16:
        bound = bound + 6e-8
    assert float((np.abs(got - g64) / bound).max()) <= 1.0
    # stage 3: the joiner backward on the kernel's own 16-bit gradient
    path = "library" if _mm_takes_out_dtype() and os.environ.get("WR_AMP_BACKWARD", "library") != "kernels" else "kernels"
    ref = R.bwd_ref(gk, ep.detach(), pp.detach(), m.ffn_out.weight.detach(), "tanh", None, path)
    R.assert_matches(m.ffn_out.weight.grad, ref["dw"], "ffn_out.weight.grad")
    R.assert_matches(m.ffn_out.bias.grad, ref["db"], "ffn_out.bias.grad")
    R.assert_matches(ep.grad, ref["d_ep"], "d_ep")
    R.assert_matches(pp.grad, ref["d_pp"], "d_pp")
