"""Workgroup order of the RNN-T streaming passes (wr_tune_set keys 15 - 17; logical_block in wr_common.hpp).

Which workgroup visits a row must not change a bit of the result: costs, the exported lattice and the whole gradient
under mode 2 (XCD runs of c, the default) are compared as raw bit patterns with mode 0 (the identity), with c = 1 and 3
forced through key 17 and with the run length the library derives from U1max; mode 0 with a forced c compares the
identity with itself and shows that mode 0 ignores c.  (Mode 1, XCD regions, was measured and removed.)  Gradient buffer and workspace start from a sentinel pattern, so
a row that no workgroup visits shows.  Grids: 3, 23, 120 and 537 workgroups (one row per wave), and 256 with the
persistent-grid knobs, where every wave walks its grid-stride loop.
"""
import pytest
import torch

from rnnt_faint_rows import DEAD, FAINT, LIVE, classify

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KEY_LSE_GRID, KEY_GRAD_GRID, KEY_SKIP, KEY_LSE_ORDER, KEY_GRAD_ORDER, KEY_RUN = 0, 1, 14, 15, 16, 17
SHAPES = [(1, 3, 2, 17), (2, 9, 4, 33), (3, 20, 7, 130), (5, 33, 12, 257)]
# (mode, forced c; 0 = derived from U1max)
VARIANTS = [(2, 1), (2, 3), (2, 0), (0, 3)]


def _lib():
    from wenet_celoss_amd import _lib as L
    return L, L.load()


def _case(seed, B, T, U, V, scale=1.0, dtype=torch.float32, blank=0):
    """Inputs as tests/test_rnnt_faint_rows_gpu.py builds them: iid N(0, scale^2) logits, ragged lengths with the
    maxima pinned on utterance 0."""
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.empty(B, T, U + 1, V, device=DEV).normal_(generator=g).mul_(scale).to(dtype)
    targets = torch.randint(0, V, (B, U), dtype=torch.int32, device=DEV, generator=g)
    targets[targets == blank] = (blank + 1) % V
    ll = torch.randint((T + 1) // 2, T + 1, (B,), dtype=torch.int32, device=DEV, generator=g)
    tl = torch.randint(U // 3, U + 1, (B,), dtype=torch.int32, device=DEV, generator=g)
    ll[0], tl[0] = T, U
    return x, targets, ll, tl


def _run(x, targets, ll, tl, tune, blank=0, inplace=False, reg=None):
    """fwd + lattice export + bwd through the C-ABI under the tune keys `tune`; every key is put back afterwards."""
    L, lib = _lib()
    B, T, U1, V = x.shape
    xin = x.clone() if inplace else x
    grads = xin if inplace else torch.full_like(x, 12345.0)
    wsb = lib.wr_rnnt_workspace_bytes(B, T, U1)
    ws = torch.full((wsb,), 0x5A, dtype=torch.uint8, device=DEV)
    costs = torch.full((B,), 12345.0, device=DEV)
    alpha = torch.full((B, T, U1), 12345.0, device=DEV)
    beta = torch.full((B, T, U1), 12345.0, device=DEV)
    gc = torch.linspace(0.5, 1.5, B, device=DEV)
    st = L.current_stream(torch.device(DEV))
    P = L.ptr
    dt = L.dtype_code(x.dtype)
    defaults = {KEY_LSE_GRID: 0, KEY_GRAD_GRID: 0, KEY_SKIP: 1, KEY_LSE_ORDER: 2, KEY_GRAD_ORDER: 2, KEY_RUN: 0}
    try:
        for k, v in tune.items():
            assert k in defaults and lib.wr_tune_set(k, v) == 0
        if reg is None:
            L.check(lib.wr_rnnt_loss_fwd(P(xin), dt, P(targets), P(ll), P(tl), B, T, U1, V, blank, P(costs), P(ws), wsb, st),
                    "fwd")
        else:
            L.check(lib.wr_rnnt_loss_fwd_lattice(P(xin), dt, P(targets), P(ll), P(tl), B, T, U1, V, blank, 0, reg[0], P(costs),
                                                 P(ws), wsb, st), "fwd_lattice")
        L.check(lib.wr_rnnt_export_lattice(P(ws), wsb, P(ll), P(tl), B, T, U1, P(alpha), P(beta), st), "export")
        if reg is None:
            L.check(lib.wr_rnnt_loss_bwd(P(xin), dt, P(targets), P(ll), P(tl), B, T, U1, V, blank, -1.0, P(gc), P(grads),
                                         P(ws), wsb, st), "bwd")
        else:
            L.check(lib.wr_rnnt_loss_bwd_lattice(P(xin), dt, P(targets), P(ll), P(tl), B, T, U1, V, blank, -1.0, 0, reg[0],
                                                 reg[1], P(gc), P(grads), P(ws), wsb, st), "bwd_lattice")
        torch.cuda.synchronize()
    finally:
        for k, v in defaults.items():
            lib.wr_tune_set(k, v)
    return costs, alpha, beta, grads


def _bits(t):
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


def _check(x, targets, ll, tl, extra=None, ref_extra=None, **kw):
    """Every variant against mode 0, bit for bit.  `extra`: further tune keys of the variants, `ref_extra` of the
    reference.  Returns the reference outputs."""
    ref_tune = dict(ref_extra or {})
    ref_tune.update({KEY_LSE_ORDER: 0, KEY_GRAD_ORDER: 0})
    ref = _run(x, targets, ll, tl, ref_tune, **kw)
    assert not bool((ref[3] == 12345.0).any()) and not bool((ref[0] == 12345.0).any())
    for mode, c in VARIANTS:
        tune = dict(extra or {})
        tune.update({KEY_LSE_ORDER: mode, KEY_GRAD_ORDER: mode, KEY_RUN: c})
        got = _run(x, targets, ll, tl, tune, **kw)
        for name, a, b in zip(("costs", "alpha", "beta", "grads"), got, ref):
            assert torch.equal(_bits(a), _bits(b)), (name, mode, c)
    return ref


@pytest.mark.parametrize("shape", SHAPES)
def test_bit_identical(shape):
    _check(*_case(41, *shape))


@pytest.mark.parametrize("shape", SHAPES[2:])
@pytest.mark.parametrize("inplace", [False, True])
def test_blank_not_zero_and_in_place(shape, inplace):
    blank = shape[3] - 1
    _check(*_case(42, *shape, blank=blank), blank=blank, inplace=inplace)


@pytest.mark.parametrize("shape", SHAPES[1:])
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_half_precision_logits(shape, dtype):
    _check(*_case(43, *shape, dtype=dtype))


@pytest.mark.parametrize("shape", SHAPES[1:])
def test_regularised_gradient(shape):
    """FastEmit plus delay penalty: the regularised instantiation of rnnt_grad_kernel takes the same map."""
    _check(*_case(44, *shape), reg=(0.25, 0.01))


def test_grid_stride_loop():
    """256 workgroups for 2 145 rows (keys 0 and 1 = 1): every wave visits two or three rows of its logical block."""
    grid = {KEY_LSE_GRID: 1, KEY_GRAD_GRID: 1}
    _check(*_case(45, *SHAPES[3]), extra=grid)


@pytest.mark.parametrize("skip", [1, 0])
def test_dead_faint_and_live_rows(skip):
    """Key 14 both ways on an input in which all three row classes of the gradient pass occur (counted on the host from
    the exported lattice): logits of scale 12 make most of a 33 x 13 lattice dead, its boundary faint."""
    x, targets, ll, tl = _case(46, *SHAPES[3], scale=12.0)
    ref = _check(x, targets, ll, tl, extra={KEY_SKIP: skip}, ref_extra={KEY_SKIP: skip})
    cls, _, _ = classify(ref[1].cpu().numpy(), ref[2].cpu().numpy(), ref[0].double().cpu().numpy(), targets.cpu().numpy(),
                         ll.cpu().numpy(), tl.cpu().numpy(), 0)
    counts = {name: int((cls == k).sum()) for name, k in (("live", LIVE), ("faint", FAINT), ("dead", DEAD))}
    print(counts)
    assert all(n > 0 for n in counts.values()), counts
