"""Float64 references for the single-term (AMP) joiner kernels, with the operand roundings of each kernel path.

Plain module (not a conftest): the CPU tests in test_joint_amp_ref.py and the GPU tests in test_joint_amp_gpu.py import
it.  Everything is torch float64 on the CPU except the contractions, which run as float64 GEMMs on the device the inputs
live on (exact sums on exact data; the elementwise rounding stays on the CPU, where test_joint_amp_ref.py checks it).

A reference is a pair (value, tol) of float64 tensors: the kernel passes when |got - value| <= tol element by element.
  * Exact data (`exact_case`): every operand is exact in bf16 / f16 and every partial sum of the contraction is exact in
    fp32, in any order -- the helper proves this from the data itself (`_fp32_exact`) and then returns tol == 0, so the
    kernel must match bit for bit whatever its tiling, split-K partials or reduction order.  For 16-bit outputs `value`
    is then the round-to-nearest-even of the exact fp32 result.
  * General data: per element
        tol = chain(K) * sum_k |a~_k b~_k|  +  ulp_rel(op) * sum_{k near} |a~_k b~_k|  (+ half an ulp of a 16-bit output)
    chain(K) = 4e-7 (fp32 accumulation: the MFMA chain's error against float64 is ~0.75-1.5e-7 * sum|a b| at K <= 1024,
    grown linearly in K / 1024 past that, as the worst case of a rounding per step does);  "near" = the k whose float64 activation lies within 2^-20 relative (plus 2^-22
    absolute: the forward's exp2 / rcp tanh is within ~1e-7 absolute) of a rounding midpoint of the operand format, where
    the device activation may round the other way -- one ulp of the operand, at most 2^-7 (bf16) / 2^-10 (f16) of it.
Padded lattice cells are excluded by selection (torch.where), never by multiplication, so a NaN or Inf there cannot
leak into a reference.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

ACT = {"tanh": 0, "relu": 1, "hardtanh": 2, "selu": 3, "swish": 4, "gelu": 5}

# (significand bits incl. the implicit one, smallest normal exponent, largest finite value)
_FMT = {
    "bf16": (8, -126, (2.0 - 2.0 ** -7) * 2.0 ** 127),
    "f16": (11, -14, 65504.0),
    "fp32": (24, -126, (2.0 - 2.0 ** -23) * 2.0 ** 127),
}
_DT = {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "fp32"}


def fmt_of(dtype) -> str:
    return dtype if isinstance(dtype, str) else _DT[dtype]


def _ulp(x64: torch.Tensor, fmt: str) -> torch.Tensor:
    """Spacing of `fmt` at |x| (the subnormal spacing below the smallest normal)."""
    p, emin, _ = _FMT[fmt]
    _, e = torch.frexp(x64)                              # |x| in [2^(e-1), 2^e)
    e = torch.clamp(e.to(torch.int64) - 1, min=emin)
    return torch.ldexp(torch.ones_like(x64), e - (p - 1))


def round_to(x: torch.Tensor, fmt) -> torch.Tensor:
    """fp32 values -> round-to-nearest-even in `fmt` ("bf16", "f16", "fp32" or a torch dtype), widened to float64.
    The rounding of v_cvt_pk_bf16_f32 and of the kernels' bf16_bits; overflow goes to +-inf, NaN stays NaN."""
    fmt = fmt_of(fmt)
    x64 = x.to(torch.float32).to(torch.float64)
    if fmt == "fp32":
        return x64
    q = _ulp(x64, fmt)
    r = torch.round(x64 / q) * q                         # torch.round: half to even
    big = r.abs() > _FMT[fmt][2]
    r = torch.where(big, torch.copysign(torch.full_like(r, math.inf), x64), r)
    return torch.where(torch.isfinite(x64), r, x64)


def _act64(z: torch.Tensor, act: str):
    """Float64 activation value and derivative (wenet/utils/common.py get_activation)."""
    if act == "tanh":
        h = torch.tanh(z)
        return h, 1 - h * h
    if act == "relu":
        return torch.clamp(z, min=0), (z > 0).to(z.dtype)
    if act == "hardtanh":
        return torch.clamp(z, -1, 1), ((z > -1) & (z < 1)).to(z.dtype)
    if act == "selu":
        a, s = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
        return s * torch.where(z > 0, z, a * torch.expm1(z)), s * torch.where(z > 0, torch.ones_like(z), a * torch.exp(z))
    if act == "swish":
        sg = torch.sigmoid(z)
        return z * sg, sg * (1 + z * (1 - sg))
    if act == "gelu":
        cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
        return z * cdf, cdf + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
    raise KeyError(act)


def _near(a64: torch.Tensor, fmt: str) -> torch.Tensor:
    """a's float64 value lies so close to a rounding midpoint of `fmt` that the device value may round the other way."""
    q = _ulp(a64, fmt)
    d = (a64 / q - torch.floor(a64 / q) - 0.5).abs() * q            # distance to the midpoint of a's ulp interval
    return d <= 2.0 ** -20 * a64.abs() + 2.0 ** -22


def _ulp_rel(fmt: str) -> float:
    return 2.0 ** -(_FMT[fmt][0] - 1)


def chain(K: int) -> float:
    """Relative error bound of an fp32 accumulation over K products, against float64 (module docstring)."""
    return 4e-7 * max(1.0, K / 1024)


def _grid_exp(x: torch.Tensor) -> Optional[int]:
    """Smallest s in [0, 40] with x * 2^s integral for every element (None: not dyadic at that depth)."""
    for s in range(41):
        y = x * 2.0 ** s
        if bool((y == torch.round(y)).all()):
            return s
    return None


def _fp32_exact(terms_abs_sum: torch.Tensor, s: Optional[int]) -> bool:
    """Every partial sum of terms on the grid 2^-s whose absolute values sum to at most `terms_abs_sum` is an fp32
    number: an integer multiple of 2^-s below 2^24 * 2^-s."""
    return s is not None and bool((terms_abs_sum * 2.0 ** s < 2.0 ** 24).all())


class Ref(NamedTuple):
    value: torch.Tensor
    tol: torch.Tensor

    @property
    def exact(self) -> bool:
        """Equality demanded wherever the reference compares (tol inf: cells not compared)."""
        return bool(((self.tol == 0) | torch.isinf(self.tol)).all())


def cell_mask(B, T, U1, lens, device) -> Optional[torch.Tensor]:
    """(B, T, U1) bool of the valid lattice cells t < llens[b], u <= tlens[b] (None without lengths)."""
    if lens is None or lens[0] is None:
        return None
    ll, tl = (x.to(device).long() for x in lens)
    tt = torch.arange(T, device=device)[None, :, None] < ll[:, None, None]
    uu = torch.arange(U1, device=device)[None, None, :] <= tl[:, None, None]
    return tt & uu


def _z32(ep, pp):
    """ep[b, t] + pp[b, u] as the kernels form it: one fp32 addition (B, T, U1, J), then widened."""
    return (ep.float()[:, :, None, :] + pp.float()[:, None, :, :]).double()


def _cpu(*xs):
    return tuple(x.detach().cpu() for x in xs)


def _mm(dev):
    """float64 matrix product on `dev`, result on the CPU."""
    return lambda x, y: (x.to(dev) @ y.to(dev)).cpu()


def _out_tol(value, tol, out_fmt):
    if out_fmt == "fp32":
        return tol
    return tol + 0.5 * _ulp(value.abs() + tol, out_fmt)


def fwd_ref(ep, pp, W, b, act: str, out_dtype, lens=None, operand="bf16") -> Ref:
    """Reference of wr_joint_fwd_split(terms=1): bias + sum_k op(W)[v,k] * op(act(ep+pp))[k], op = RNE to `operand`.
    Under both f16 and bf16 autocast the kernel's operands are bf16 (joint_split.hip, the single-term MFMA), hence the
    default.  Cells outside `lens` (a (llens, tlens) pair) get value 0, tol inf: they are not compared."""
    out_fmt, opf = fmt_of(out_dtype), fmt_of(operand)
    mm = _mm(ep.device)
    ep, pp, W, b = _cpu(ep, pp, W, b)
    B, T, J = ep.shape
    U1, V = pp.shape[1], W.shape[0]
    z = _z32(ep, pp).reshape(-1, J)
    a64, _ = _act64(z, act)
    a = round_to(a64.float(), opf)                       # the kernel rounds its fp32 activation
    w = round_to(W, opf)
    bias = b.double()
    value = mm(a, w.T) + bias
    mag = mm(a.abs(), w.abs().T)
    exact = act in ("relu", "hardtanh") and bool((a == a64).all())
    if exact:
        s_w, s_a, s_b = _grid_exp(w), _grid_exp(a), _grid_exp(bias)
        exact = None not in (s_w, s_a, s_b) and _fp32_exact(mag + bias.abs(), max(s_w + s_a, s_b))
    if exact:
        value = round_to(value.float(), out_fmt)         # the exact fp32 sum, rounded once to the output format
        tol = torch.zeros_like(value)
    else:
        near = (_near(a64, opf) & (a64 != 0)).double()
        tol = chain(J) * (mag + bias.abs()) + _ulp_rel(opf) * mm(a.abs() * near, w.abs().T)
        tol = _out_tol(value, tol, out_fmt)
    value, tol = value.view(B, T, U1, V), tol.view(B, T, U1, V)
    m = cell_mask(B, T, U1, lens, "cpu")
    if m is not None:
        value = torch.where(m[..., None], value, torch.zeros((), dtype=value.dtype, device=value.device))
        tol = torch.where(m[..., None], tol, torch.full((), math.inf, dtype=tol.dtype, device=tol.device))
    return Ref(value, tol)


def bwd_ref(gout, ep, pp, W, act: str, lens=None, path="kernels") -> dict:
    """References of the joiner backward from the logits gradient `gout` (B, T, U1, V): dict of Ref for
    "dz" (B,T,U1,J; 0 in padded cells), "h" (the activation, 0 in padded cells), "d_ep", "d_pp", "dw", "db".
    Operand roundings per path:
      "kernels" -- wr_joint_bwd_dz_split* / wr_joint_bwd_dw_split* with terms=1: dY and W to bf16 for dZ, dY and H to bf16
                   for dW (an f16 gradient is widened to fp32 first, then rounded to bf16 like any fp32 gradient);
      "library" -- _amp_backward_library: W and H to the gradient's dtype, dY as it is;
      "exact"   -- the exact-fp32 kernels (wr_joint_bwd_dz / wr_joint_bwd_dw): no operand rounding.
    db = the column sums of dY over valid cells, in fp32."""
    B, T, J = ep.shape
    U1, V = pp.shape[1], W.shape[0]
    M = B * T * U1
    mm = _mm(ep.device)
    gout, ep, pp, W = _cpu(gout, ep, pp, W)
    dev = "cpu"
    if path == "kernels":
        opf = "bf16"
    elif path == "library":
        opf = fmt_of(gout.dtype)
    elif path == "exact":
        opf = "fp32"
    else:
        raise KeyError(path)
    mask = cell_mask(B, T, U1, lens, dev)
    keep = torch.ones(M, dtype=torch.bool, device=dev) if mask is None else mask.reshape(M)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    g = round_to(gout.reshape(M, V).float(), opf)
    g = torch.where(keep[:, None], g, zero)              # selection: NaN / Inf in padded cells never enter
    w = round_to(W, opf)
    z = _z32(ep, pp).reshape(M, J)
    h64, d64 = _act64(z, act)
    h64 = torch.where(keep[:, None], h64, zero)
    d64 = torch.where(keep[:, None], d64, zero)
    h = round_to(h64.float(), opf)
    exact_act = act in ("relu", "hardtanh")

    # dZ = (dY W) * act'(z)
    pre = mm(g, w)
    pre_mag = mm(g.abs(), w.abs())
    s_g, s_w = (_grid_exp(g), _grid_exp(w)) if exact_act else (None, None)
    ex_dz = None not in (s_g, s_w) and _fp32_exact(pre_mag, s_g + s_w)
    dz = pre * d64
    if ex_dz:
        dz_tol = torch.zeros_like(dz)
    else:
        # fp32 chain over V, the product with the derivative, and the device derivative (tanhf / expf / erff: a few ulp)
        dz_tol = (chain(V) * pre_mag + 2.0 ** -21 * pre.abs()) * d64.abs().clamp(min=1.0)
    dz_tol = torch.where(keep[:, None], dz_tol, zero)    # padded cells: exactly zero
    h_tol = torch.zeros_like(h64) if exact_act else 2.0 ** -21 * h64.abs() + 2.0 ** -40

    def sums(x, tol, dim, mag_x):
        x4, t4, m4 = (y.view(B, T, U1, J) for y in (x, tol, mag_x))
        n = x4.shape[dim]
        v = x4.sum(dim)
        if ex_dz and _fp32_exact(m4.abs().sum(dim), _grid_exp(x)):
            return Ref(v, torch.zeros_like(v))
        return Ref(v, t4.sum(dim) + chain(n) * m4.abs().sum(dim))

    # dW = dY^T H over valid cells
    dw = mm(g.T, h)
    dw_mag = mm(g.abs().T, h.abs())
    s_h = _grid_exp(h) if exact_act and bool((h == h64).all()) else None
    ex_dw = None not in (s_g, s_h) and _fp32_exact(dw_mag, s_g + s_h)
    if ex_dw:
        dw_tol = torch.zeros_like(dw)
    else:
        near = (_near(h64, opf) & (h64 != 0)).double() if opf != "fp32" else torch.zeros_like(h64)
        # the library path's dW is a vendor GEMM whose reduction structure (split-K, block partial sums) is not this
        # project's: twice the chain bound (measured worst: 1.01 x chain(M) at M = 3780, bf16 operands)
        dw_tol = (2 if path == "library" else 1) * chain(M) * dw_mag + _ulp_rel(opf) * mm(g.abs().T, h.abs() * near)
        if opf == "fp32":
            dw_tol = dw_tol + 2.0 ** -21 * dw_mag     # device activation, a few ulp
    gd = torch.where(keep[:, None], gout.reshape(M, V).double(), zero)
    db = gd.sum(0)
    db_mag = gd.abs().sum(0)
    ex_db = _fp32_exact(db_mag, _grid_exp(gd))
    db_tol = torch.zeros_like(db) if ex_db else chain(M) * db_mag
    return {
        "dz": Ref(dz.view(B, T, U1, J), dz_tol.view(B, T, U1, J)),
        "h": Ref(h64.view(B, T, U1, J), h_tol.view(B, T, U1, J)),
        "d_ep": sums(dz, dz_tol, 2, dz),
        "d_pp": sums(dz, dz_tol, 1, dz),
        "dw": Ref(dw, dw_tol),
        "db": Ref(db, db_tol),
    }


def assert_matches(got: torch.Tensor, ref: Ref, what: str = "") -> None:
    """|got - ref.value| <= ref.tol everywhere (tol inf: not compared); tol == 0 demands the same number (NaN fails)."""
    g = got.detach().to(torch.float64).to(ref.value.device)
    err = (g - ref.value).abs()
    bad = ~(err <= ref.tol)
    bad &= ~torch.isinf(ref.tol)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound ({'exact' if ref.exact else 'tolerance'}); "
            f"first at {idx}: got {float(g[idx])!r}, want {float(ref.value[idx])!r} +- {float(ref.tol[idx])!r}")


# ---- exact-data generators ------------------------------------------------------------------------------------
# Dyadic grids: ep in odd multiples of 2^-5 in (-1, 1), pp in 2^-4 Z cap [-1, 1] -- their sum is an odd multiple of
# 2^-5, never 0 or +-1, so relu / hardtanh and their derivatives have no ties; W in 2^-6 Z cap [-1/8, 1/8],
# b in 2^-10 Z cap [-1, 1], dY in 2^-3 Z cap [-1, 1].  Every operand is exact in bf16 and f16.  Independent draws per
# element: distinct rows and columns, nothing i+j shaped.
def _grid(gen, shape, step_exp: int, lo: int, hi: int, odd: bool = False) -> torch.Tensor:
    n = torch.randint(lo, hi + 1, shape, generator=gen, dtype=torch.int64)
    if odd:
        n = 2 * n + 1
    return n.double().mul(2.0 ** -step_exp).float()


def exact_case(B, T, U1, J, V, seed=0, device="cpu"):
    """(ep, pp, W, b) fp32 on the dyadic grids above."""
    gen = torch.Generator().manual_seed(seed)
    ep = _grid(gen, (B, T, J), 5, -16, 15, odd=True)     # (2n+1)/32 in [-31/32, 31/32]
    pp = _grid(gen, (B, U1, J), 4, -16, 16)
    W = _grid(gen, (V, J), 6, -8, 8)
    b = _grid(gen, (V,), 10, -1024, 1024)
    return tuple(x.to(device) for x in (ep, pp, W, b))


def exact_grad(B, T, U1, V, seed=0, device="cpu", dtype=torch.float32):
    gen = torch.Generator().manual_seed(seed + 7919)
    return _grid(gen, (B, T, U1, V), 3, -8, 8).to(device=device, dtype=dtype)


def random_case(B, T, U1, J, V, seed=0, device="cpu"):
    """(ep, pp, W, b) fp32 normal draws at joiner-like scales (general data: tolerance references)."""
    gen = torch.Generator().manual_seed(seed)
    ep = torch.randn(B, T, J, generator=gen)
    pp = torch.randn(B, U1, J, generator=gen)
    W = torch.randn(V, J, generator=gen) / math.sqrt(J)
    b = torch.randn(V, generator=gen) * 0.1
    return tuple(x.to(device) for x in (ep, pp, W, b))


def ragged_lens(B, T, U1, seed=0, device="cpu"):
    """(llens, tlens) int32 with the first utterance full length and the others ragged (some tiles fully padded)."""
    gen = torch.Generator().manual_seed(seed + 17)
    ll = torch.randint(1, T + 1, (B,), generator=gen).to(torch.int32)
    tl = torch.randint(0, U1, (B,), generator=gen).to(torch.int32)
    ll[0], tl[0] = T, U1 - 1
    if B > 1:
        ll[-1], tl[-1] = max(1, T // 3), max(0, U1 // 2 - 1)
    return ll.to(device), tl.to(device)
