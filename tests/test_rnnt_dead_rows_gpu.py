"""The RNN-T gradient pass writes dead cells (every exponential of the cell provably +0, kDeadThr in rnnt_loss.hip)
without reading their logits.  That must not change a bit: costs and gradients with wr_tune_set key 14 = 1 (the
default) are compared as raw bit patterns with key 14 = 0 (every valid cell streamed), so -0 against +0 and NaN
payloads count.  Also: the skip fires on the benchmark's data, and __builtin_amdgcn_exp2f returns +0 for every float
the dead-cell bound allows."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from rnnt_dead_rows import dead_mask, dead_share

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
    misalignment as the logits (or the logits themselves when in place)."""
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


def _check(x, targets, ll, tl, **kw):
    """Key 14 = 1 against key 14 = 0, bit for bit; returns the dead share the host restatement finds."""
    c1, g1 = _run(x, targets, ll, tl, skip=1, **kw)
    c0, g0 = _run(x, targets, ll, tl, skip=0, **kw)
    assert _same(c1, c0), (c1, c0)
    assert _same(g1, g0)
    del g1, g0
    return _share(x, targets, ll, tl, kw.get("blank", 0))


def _share(x, targets, ll, tl, blank):
    from wenet_celoss_amd.rnnt_loss import rnnt_lattice
    costs, alpha, beta = rnnt_lattice(x, targets, ll, tl, blank=blank)
    m = dead_mask(alpha.cpu().numpy(), beta.cpu().numpy(), costs.double().cpu().numpy(), targets.cpu().numpy(),
                  ll.cpu().numpy(), tl.cpu().numpy(), blank)
    return dead_share(m, ll.cpu().numpy(), tl.cpu().numpy()), m


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


def test_bench_shape_bit_identical_and_skip_fires():
    """B=2 at the benchmark's (T, U, V) = (1000, 150, 5000), fp32, its data model (iid N(0,1) logits): about 30 % of
    the cells are dead.  The share is counted on the host from the exported lattice and must stay >= 0.2, so a change
    that switches the skip off does not go unnoticed."""
    x, targets, ll, tl = _case(20260, 2, 1000, 150, 5000)
    gc = torch.full((2,), 0.5, device=DEV)
    share, _ = _check(x, targets, ll, tl, gc=gc)
    assert share >= 0.2, share


@pytest.mark.parametrize("name,kw,case", [
    ("ragged", {}, dict(seed=1, B=4, T=300, U=60, V=700, scale=3.0, ragged=True)),
    ("blank_last", dict(blank=699), dict(seed=2, B=3, T=200, U=40, V=700, scale=3.0, ragged=True, blank=699)),
    ("clamp", dict(clamp=0.25), dict(seed=3, B=3, T=200, U=40, V=600, scale=3.0, ragged=True)),
    ("fp16", {}, dict(seed=4, B=3, T=200, U=40, V=640, scale=3.0, ragged=True, dtype=torch.float16)),
    ("bf16", {}, dict(seed=5, B=3, T=200, U=40, V=640, scale=3.0, ragged=True, dtype=torch.bfloat16)),
    ("v_mod1_misaligned", dict(offset=1), dict(seed=6, B=2, T=150, U=30, V=1001, scale=3.0, ragged=True, offset=1)),
    ("v_mod2", {}, dict(seed=7, B=2, T=150, U=30, V=1002, scale=3.0, ragged=True)),
    ("v_mod3_misaligned", dict(offset=3), dict(seed=8, B=2, T=150, U=30, V=1003, scale=3.0, ragged=True, offset=3)),
    ("f16_v_odd_misaligned", dict(offset=5), dict(seed=9, B=2, T=150, U=30, V=1003, scale=3.0, ragged=True,
                                                  dtype=torch.float16, offset=5)),
])
def test_bit_identical(name, kw, case):
    x, targets, ll, tl = _case(**case)
    share, _ = _check(x, targets, ll, tl, **kw)
    assert share > 0.05, share                       # the case has dead cells to skip


def test_label_equals_blank():
    x, targets, ll, tl = _case(10, 3, 200, 40, 500, scale=3.0, ragged=True)
    targets[:, ::4] = 0
    share, _ = _check(x, targets, ll, tl)
    assert share > 0.05, share


@pytest.mark.parametrize("inplace", [False, True])
def test_grad_costs_negative_and_nan(inplace):
    """finish(0) keeps -0 for a negative grad_costs and NaN for a NaN one, exactly as the streamed cell gives."""
    x, targets, ll, tl = _case(11, 4, 200, 40, 500, scale=3.0, ragged=True)
    gc = torch.tensor([-1.5, float("nan"), 0.25, -0.0], device=DEV)
    _check(x, targets, ll, tl, gc=gc, inplace=inplace)
    _, g = _run(x, targets, ll, tl, gc=gc, inplace=inplace)
    _, m = _share(x, targets, ll, tl, 0)
    m = torch.from_numpy(m).to(DEV)
    gb = _bits(g)
    assert m[0].any() and bool((gb[0][m[0]] == _bits(torch.tensor(-0.0, device=DEV))).all())
    assert bool(torch.isnan(g[1][m[1]]).all())


def test_neg_inf_logits():
    """-inf logits, many of them in dead cells (denom stays finite, the streamed exponentials are exactly +0)."""
    x, targets, ll, tl = _case(12, 3, 200, 40, 500, scale=3.0, ragged=True)
    g = torch.Generator(device=DEV)
    g.manual_seed(13)
    sel = torch.rand(x.shape, device=DEV, generator=g) < 0.02
    x[sel] = float("-inf")
    share, _ = _check(x, targets, ll, tl)
    assert share > 0.05, share


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_inf_nan_logit_in_dead_cell(bad):
    """A +inf or NaN logit in a cell that would otherwise be dead: its denom is not finite, the cell (and whatever the
    lattice spreads it to) keeps the streamed path and its NaN pattern."""
    x, targets, ll, tl = _case(14, 2, 200, 40, 500, scale=3.0, ragged=True)
    _, m = _share(x, targets, ll, tl, 0)
    cells = np.argwhere(m[1])
    assert len(cells)
    b, (t, u) = 1, (int(v) for v in cells[len(cells) // 2])
    x[b, t, u, 7] = bad
    _check(x, targets, ll, tl)
    _, gr = _run(x, targets, ll, tl)
    assert bool(torch.isnan(gr[b, t, u]).any())
    assert bool(torch.isfinite(gr[0]).all())           # the other utterance is untouched


_EXP2_SRC = r"""
#include <hip/hip_runtime.h>
#include <stdint.h>
__global__ void probe(uint32_t lo, uint32_t hi, unsigned long long *bad, uint32_t *first)
{
    const uint64_t n = (uint64_t)hi - lo + 1;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t bits = 0x80000000u | (uint32_t)(lo + i);           // negative floats, magnitude lo..hi
        const float y = __builtin_amdgcn_exp2f(__uint_as_float(bits));
        if (__float_as_uint(y) != 0u) { atomicAdd(bad, 1ull); atomicMin(first, (uint32_t)(lo + i)); }
    }
}
__global__ void one(float x, float *y) { *y = __builtin_amdgcn_exp2f(x); }
extern "C" int exp2_probe(uint32_t lo, uint32_t hi, unsigned long long *bad, uint32_t *first)
{
    hipLaunchKernelGGL(probe, dim3(8192), dim3(256), 0, 0, lo, hi, bad, first);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}
extern "C" int exp2_one(float x, float *y)
{
    hipLaunchKernelGGL(one, dim3(1), dim3(1), 0, 0, x, y);
    return hipDeviceSynchronize() == hipSuccess ? 0 : -1;
}
"""


def test_fast_exp2_underflows_to_plus_zero():
    """Every float <= -151 (magnitudes 151 .. FLT_MAX, then -inf) gives exactly +0 from __builtin_amdgcn_exp2f with
    the library's compile flags.  The dead-cell bound puts every exponent of a dead cell below -158.6 (log2 units)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src, so = os.path.join(d, "exp2_probe.hip"), os.path.join(d, "exp2_probe.so")
        with open(src, "w") as f:
            f.write(_EXP2_SRC)
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", src, "-o", so],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        lib = ctypes.CDLL(so)
        lib.exp2_probe.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p]
        lib.exp2_one.argtypes = [ctypes.c_float, ctypes.c_void_p]
        torch.cuda.synchronize()
        y = torch.zeros(1, device=DEV)
        assert lib.exp2_one(-1.0, y.data_ptr()) == 0
        assert y.item() == 0.5                                       # the probe is live
        lo = int(np.array(151.0, np.float32).view(np.uint32))
        hi = 0x7F800000                                              # FLT_MAX = 0x7F7FFFFF, then +inf
        bad = torch.zeros(1, dtype=torch.int64, device=DEV)
        first = torch.full((1,), -1, dtype=torch.int32, device=DEV)  # 0xFFFFFFFF
        assert lib.exp2_probe(lo, hi, bad.data_ptr(), first.data_ptr()) == 0
        fb = int(first.item()) & 0xFFFFFFFF
        assert int(bad.item()) == 0, (int(bad.item()), -float(np.array(fb, np.uint32).view(np.float32)))
