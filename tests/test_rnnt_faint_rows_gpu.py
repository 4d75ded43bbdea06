"""Faint rows of the RNN-T gradient pass, and the exp2 cut-off its threshold rests on.

A faint row (rnnt_faint_rows.py) has a main term that is provably +0 in every element and a blank or label term that is
not: rnnt_grad_kernel writes it as finish(0) with that one or those two elements patched in from the only logits it
reads.  Costs and gradients with wr_tune_set key 14 = 1 (the default: every no-read rule on) are compared as raw bit
patterns with key 14 = 0 (every valid cell streamed), and every case counts, from the host restatement on the exported
lattice, that it has faint rows, so that the path cannot be switched off unnoticed.

test_exp2_cutoff measures where __builtin_amdgcn_exp2f (v_exp_f32) first returns something other than +0, with the
library's compile flags: on gfx950 it flushes denormal results, so the largest float X0 with "+0 for every float <= X0"
is the float just below -126, exp2(-126) = 2^-126 is the first non-zero result, and kDeadThr = -93.3 nats keeps the
kernel's margin of 8.6 log2 units under it.
"""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from rnnt_faint_rows import DEAD, DEAD_THR, FAINT, LOG2E, MARGIN_LOG2, X0, classify, share, thr_from_cutoff

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY_SKIP = 14


def _lib():
    from wenet_celoss_amd import _lib as L
    return L, L.load()


def _alloc(shape, dtype, offset=0):
    """A contiguous tensor of `shape` whose storage starts `offset` elements into a fresh buffer (misaligned rows)."""
    n = int(np.prod(shape))
    return torch.empty(n + offset, dtype=dtype, device=DEV)[offset:].view(shape)


def _run(x, targets, ll, tl, blank=0, clamp=-1.0, gc=None, inplace=False, skip=1, offset=0):
    """fwd + bwd through the C-ABI with key 14 = skip; returns (costs, grads) with the grads in a buffer of the same
    misalignment as the logits (or a copy of the logits overwritten in place)."""
    L, lib = _lib()
    B, T, U1, V = x.shape
    if inplace:
        xin = _alloc(x.shape, x.dtype, offset)
        xin.copy_(x)
        grads = xin
    else:
        xin = x
        grads = _alloc(x.shape, x.dtype, offset)
    wsb = lib.wr_rnnt_workspace_bytes(B, T, U1)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    costs = torch.empty(B, dtype=torch.float32, device=DEV)
    st = L.current_stream(torch.device(DEV))
    P = L.ptr
    dt = L.dtype_code(x.dtype)
    assert lib.wr_tune_set(KEY_SKIP, skip) == 0
    try:
        L.check(lib.wr_rnnt_loss_fwd(P(xin), dt, P(targets), P(ll), P(tl), B, T, U1, V, blank, P(costs), P(ws), wsb, st),
                "fwd")
        L.check(lib.wr_rnnt_loss_bwd(P(xin), dt, P(targets), P(ll), P(tl), B, T, U1, V, blank, float(clamp),
                                     None if gc is None else P(gc), P(grads), P(ws), wsb, st), "bwd")
        torch.cuda.synchronize()
    finally:
        lib.wr_tune_set(KEY_SKIP, 1)
    return costs, grads


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _classes(x, targets, ll, tl, blank, thr=DEAD_THR):
    from wenet_celoss_amd.rnnt_loss import rnnt_lattice
    costs, alpha, beta = rnnt_lattice(x, targets, ll, tl, blank=blank)
    return classify(alpha.cpu().numpy(), beta.cpu().numpy(), costs.double().cpu().numpy(), targets.cpu().numpy(),
                    ll.cpu().numpy(), tl.cpu().numpy(), blank, thr=thr)


def _check(x, targets, ll, tl, **kw):
    """Key 14 = 1 against key 14 = 0, bit for bit; returns the faint share the host restatement finds and its masks."""
    c1, g1 = _run(x, targets, ll, tl, skip=1, **kw)
    c0, g0 = _run(x, targets, ll, tl, skip=0, **kw)
    assert _same(c1, c0), (c1, c0)
    assert _same(g1, g0)
    del g1, g0
    cls, need_b, need_l = _classes(x, targets, ll, tl, kw.get("blank", 0))
    lln, tln = ll.cpu().numpy(), tl.cpu().numpy()
    faint = share(cls, FAINT, lln, tln)
    print(f"faint share {faint:.4f}, dead share {share(cls, DEAD, lln, tln):.4f}, "
          f"blank reads {int(need_b.sum())}, label reads {int(need_l.sum())}")
    return faint, cls, need_b, need_l


def _case(seed, B, T, U, V, scale=1.0, ragged=False, dtype=torch.float32, blank=0, offset=0):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = _alloc((B, T, U + 1, V), torch.float32, 0)
    x.normal_(generator=g)
    x.mul_(scale)
    if dtype != torch.float32 or offset:
        y = _alloc(x.shape, dtype, offset)
        y.copy_(x)
        x = y
    targets = torch.randint(0, V, (B, U), dtype=torch.int32, device=DEV, generator=g)
    targets[targets == blank] = (blank + 1) % V
    if ragged:
        ll = torch.randint(T // 2, T + 1, (B,), dtype=torch.int32, device=DEV, generator=g)
        tl = torch.randint(U // 3, U + 1, (B,), dtype=torch.int32, device=DEV, generator=g)
        ll[0], tl[0] = T, U
    else:
        ll = torch.full((B,), T, dtype=torch.int32, device=DEV)
        tl = torch.full((B,), U, dtype=torch.int32, device=DEV)
    return x, targets, ll, tl


def test_bench_shape_bit_identical_and_faint_rows_fire():
    """B=2 at the benchmark's (T, U, V) = (1000, 150, 5000), fp32, its data model (iid N(0,1) logits).  A float64 model
    of that lattice puts the faint share at 0.02; the host restatement on the exported lattice must find >= 0.01."""
    x, targets, ll, tl = _case(20261, 2, 1000, 150, 5000)
    gc = torch.full((2,), 0.5, device=DEV)
    faint, cls, _, _ = _check(x, targets, ll, tl, gc=gc)
    assert faint >= 0.01, faint
    # what is no longer read: the rule before this one (all three bounds below -110) skipped about 0.32 of the cells
    assert faint + share(cls, DEAD, ll.cpu().numpy(), tl.cpu().numpy()) >= 0.2


@pytest.mark.parametrize("name,kw,case", [
    ("ragged", {}, dict(seed=21, B=4, T=300, U=60, V=700, scale=3.0, ragged=True)),
    ("ragged_small", {}, dict(seed=22, B=5, T=120, U=25, V=97, scale=3.0, ragged=True)),
    ("blank_last", dict(blank=699), dict(seed=23, B=3, T=200, U=40, V=700, scale=3.0, ragged=True, blank=699)),
    ("clamp", dict(clamp=0.25), dict(seed=24, B=3, T=200, U=40, V=600, scale=3.0, ragged=True)),
    ("fp16", {}, dict(seed=25, B=3, T=200, U=40, V=640, scale=3.0, ragged=True, dtype=torch.float16)),
    ("bf16", {}, dict(seed=26, B=3, T=200, U=40, V=640, scale=3.0, ragged=True, dtype=torch.bfloat16)),
])
def test_bit_identical(name, kw, case):
    x, targets, ll, tl = _case(**case)
    faint, _, _, _ = _check(x, targets, ll, tl, **kw)
    assert faint > 0, faint


def _place(row_elem_offset, v, V, N):
    """'head' / 'body' / 'tail' of element v in a row that starts row_elem_offset elements past a 16-byte boundary
    (RowSplit of row_stream.hpp)."""
    h = min((N - row_elem_offset % N) % N, V)
    nv = (V - h) // N
    return "head" if v < h else ("body" if v < h + N * nv else "tail")


@pytest.mark.parametrize("name,blank,case", [
    ("v_mod1_misaligned", 0, dict(seed=27, B=2, T=150, U=30, V=1001, scale=3.0, ragged=True, offset=1)),
    ("v_mod2", 1001, dict(seed=28, B=2, T=150, U=30, V=1002, scale=3.0, ragged=True, blank=1001)),
    ("v_mod3_misaligned", 2, dict(seed=29, B=2, T=150, U=30, V=1003, scale=3.0, ragged=True, offset=3, blank=2)),
    ("f16_v_odd_misaligned", 0, dict(seed=30, B=2, T=150, U=30, V=1003, scale=3.0, ragged=True, dtype=torch.float16,
                                    offset=5)),
    ("bf16_v_mod2_misaligned", 1001, dict(seed=31, B=2, T=150, U=30, V=1002, scale=3.0, ragged=True,
                                          dtype=torch.bfloat16, offset=3, blank=1001)),
])
def test_head_body_tail(name, blank, case):
    """V = 1, 2, 3 (mod 4) and misaligned base pointers: the split of a row into head / body / tail changes from row to
    row.  The labels walk through the first and last N + 1 elements of the row (0, h-1, h, V-tail-1, V-1 for every h and
    tail there is), so the elements a faint row reads land in all three places; that they do is counted on the host."""
    x, targets, ll, tl = _case(**case)
    B, T, U1, V = x.shape
    N = 16 // x.element_size()
    ends = [v for v in list(range(N + 1)) + list(range(V - N - 1, V)) if v != blank]
    for u in range(U1 - 1):
        targets[:, u] = ends[u % len(ends)]
    faint, _, need_b, need_l = _check(x, targets, ll, tl, blank=blank, offset=case.get("offset", 0))
    assert faint > 0, faint
    off0 = x.data_ptr() // x.element_size()
    tg = targets.cpu().numpy()
    seen = set()
    for need, elem in ((need_b, lambda b, u: blank), (need_l, lambda b, u: int(tg[b, u]))):
        for b, t, u in np.argwhere(need):
            seen.add(_place(off0 + ((int(b) * T + int(t)) * U1 + int(u)) * V, elem(b, u), V, N))
    print(name, sorted(seen))
    assert seen == {"head", "body", "tail"}, seen


def test_label_equals_blank():
    x, targets, ll, tl = _case(32, 3, 200, 40, 500, scale=3.0, ragged=True)
    targets[:, ::4] = 0
    faint, _, _, _ = _check(x, targets, ll, tl)
    assert faint > 0, faint


@pytest.mark.parametrize("inplace", [False, True])
def test_grad_costs_negative_nan_and_minus_zero(inplace):
    """finish() of a faint row's zeros and of its blank / label element keeps -0 for a negative grad_costs, NaN for a NaN
    one and the sign rules of a -0 one, exactly as the streamed row gives; also with the gradient written over the
    logits."""
    x, targets, ll, tl = _case(33, 4, 200, 40, 500, scale=3.0, ragged=True)
    gc = torch.tensor([-1.5, float("nan"), 0.25, -0.0], device=DEV)
    faint, cls, _, _ = _check(x, targets, ll, tl, gc=gc, inplace=inplace)
    assert faint > 0, faint
    assert all((cls[b] == FAINT).any() for b in range(4))


def test_neg_inf_at_the_element_a_faint_row_reads():
    """-inf at the blank / label element of faint rows: 0 - exp2(-inf) = 0 - 0 on both paths."""
    x, targets, ll, tl = _case(34, 3, 200, 40, 500, scale=3.0, ragged=True)
    _, need_b, need_l = _classes(x, targets, ll, tl, 0)
    tg = targets.cpu().numpy()
    cb, cl = np.argwhere(need_b)[::2], np.argwhere(need_l)[::2]
    assert len(cb) and len(cl)
    for b, t, u in cb:
        x[int(b), int(t), int(u), 0] = float("-inf")
    for b, t, u in cl:
        x[int(b), int(t), int(u), int(tg[b, u])] = float("-inf")
    faint, _, nb, nl = _check(x, targets, ll, tl)
    assert faint > 0, faint
    # the rows that were changed are still read at that element (their side bounds do not depend on their own logits)
    assert sum(bool(nb[tuple(c)]) for c in cb) + sum(bool(nl[tuple(c)]) for c in cl) > 0


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_inf_nan_logit_in_faint_row(bad):
    """A +inf or NaN logit in a row that would otherwise be faint: its denom is not finite, the row (and whatever the
    lattice spreads it to) keeps the streamed path and its NaN pattern."""
    x, targets, ll, tl = _case(35, 2, 200, 40, 500, scale=3.0, ragged=True)
    lo, _, _ = _classes(x, targets, ll, tl, 0, thr=DEAD_THR - 1.0)
    hi, _, _ = _classes(x, targets, ll, tl, 0, thr=DEAD_THR + 1.0)
    cells = np.argwhere((lo[1] == FAINT) & (hi[1] == FAINT))     # faint whatever the float32 export rounded
    assert len(cells)
    b, (t, u) = 1, (int(v) for v in cells[len(cells) // 2])
    x[b, t, u, 7] = bad
    c1, g1 = _run(x, targets, ll, tl, skip=1)
    c0, g0 = _run(x, targets, ll, tl, skip=0)
    assert _same(c1, c0) and _same(g1, g0)
    assert bool(torch.isnan(g1[b, t, u]).any())
    assert bool(torch.isfinite(g1[0]).all())           # the other utterance is untouched
    cls, _, _ = _classes(x[:1], targets[:1], ll[:1], tl[:1], 0)
    assert (cls == FAINT).any()


_EXP2_SRC = r"""
#include <hip/hip_runtime.h>
#include <stdint.h>
// negative floats of magnitude bits lo..hi: how many give something other than +0, and the largest such magnitude
__global__ void sweep(uint32_t lo, uint32_t hi, unsigned long long *nonzero, uint32_t *max_mag)
{
    const uint64_t n = (uint64_t)hi - lo + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t mag = (uint32_t)(lo + i);
        const float y = __builtin_amdgcn_exp2f(__uint_as_float(0x80000000u | mag));
        if (__float_as_uint(y) != 0u) { atomicAdd(nonzero, 1ull); atomicMax(max_mag, mag); }
    }
}
__global__ void eval(const float *x, float *y, int n)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = __builtin_amdgcn_exp2f(x[i]);
}
extern "C" int exp2_sweep(uint32_t lo, uint32_t hi, unsigned long long *nonzero, uint32_t *max_mag)
{
    hipLaunchKernelGGL(sweep, dim3(8192), dim3(256), 0, 0, lo, hi, nonzero, max_mag);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}
extern "C" int exp2_eval(const float *x, float *y, int n)
{
    hipLaunchKernelGGL(eval, dim3((n + 255) / 256), dim3(256), 0, 0, x, y, n);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}
"""


def _f32_bits(v):
    return int(np.array(v, np.float32).view(np.uint32))


def _f32_from_bits(b):
    return float(np.array(b, np.uint32).view(np.float32))


def build_exp2_probe(d):
    """The probe library, compiled in directory d with the library's compile flags (wenet_celoss_amd/_lib.py)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src, so = os.path.join(d, "exp2_cutoff.hip"), os.path.join(d, "exp2_cutoff.so")
    with open(src, "w") as f:
        f.write(_EXP2_SRC)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC"] + os.environ.get("WR_EXTRA_HIPCC_FLAGS", "").split()
    r = subprocess.run([hipcc] + flags + ["-shared", src, "-o", so], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return load_exp2_probe(so)


def load_exp2_probe(so):
    lib = ctypes.CDLL(so)
    lib.exp2_sweep.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
    lib.exp2_eval.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    return lib


def measure_exp2_cutoff(lib):
    """Sweep every float in [-152, -125] and every float <= X0.  Returns a dict of what was seen."""
    torch.cuda.synchronize()
    xs = torch.tensor([-1.0, -126.0, X0], dtype=torch.float32, device=DEV)
    ys = torch.full((3,), -1.0, device=DEV)
    assert lib.exp2_eval(xs.data_ptr(), ys.data_ptr(), 3) == 0
    nz = torch.zeros(1, dtype=torch.int64, device=DEV)
    mx = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.exp2_sweep(_f32_bits(125.0), _f32_bits(152.0), nz.data_ptr(), mx.data_ptr()) == 0
    out = {"exp2(-1)": ys[0].item(), "exp2(-126)": ys[1].item(), "exp2(X0)_bits": int(_bits(ys)[2].item()) & 0xFFFFFFFF,
           "nonzero_in_[-152,-125]": int(nz.item()), "n_in_[-152,-125]": _f32_bits(152.0) - _f32_bits(125.0) + 1}
    last = int(mx.item()) & 0xFFFFFFFF                       # magnitude bits of the lowest float with a non-zero result
    out["lowest_nonzero_x"] = -_f32_from_bits(last)
    out["x0"] = -_f32_from_bits(last + 1)
    xl = torch.tensor([out["lowest_nonzero_x"]], dtype=torch.float32, device=DEV)
    yl = torch.zeros(1, device=DEV)
    assert lib.exp2_eval(xl.data_ptr(), yl.data_ptr(), 1) == 0
    out["first_nonzero_result"] = yl.item()
    nz.zero_()
    mx.zero_()
    assert lib.exp2_sweep(_f32_bits(-X0), 0x7F800000, nz.data_ptr(), mx.data_ptr()) == 0      # X0 .. -FLT_MAX, -inf
    out["nonzero_at_or_below_X0"] = int(nz.item())
    return out


def test_exp2_cutoff():
    """The property kDeadThr rests on.  Measured on gfx950 (MI355X), -O3, no denormal flags, 1 966 081 floats in
    [-152, -125]: every float <= X0 = -126.00000762939453 (0xC2FC0001) gives +0 bit-exactly, exp2(-126) = 2^-126
    = 1.1754943508222875e-38 is the first non-zero result: the instruction flushes denormal results.  A compile flag
    that made it keep them would fail here."""
    with tempfile.TemporaryDirectory() as d:
        m = measure_exp2_cutoff(build_exp2_probe(d))
    print(m)
    assert m["exp2(-1)"] == 0.5                                        # the probe is live
    assert m["nonzero_in_[-152,-125]"] > 0                             # and the sweep reaches floats that do not underflow
    assert m["nonzero_at_or_below_X0"] == 0, m
    assert m["exp2(X0)_bits"] == 0, m
    assert m["x0"] >= X0, m
    # the constant, restated in the helper, keeps the kernel's margin under the cut-off and is the one the rule gives
    assert DEAD_THR * LOG2E <= X0 - MARGIN_LOG2
    assert DEAD_THR == thr_from_cutoff(X0)
