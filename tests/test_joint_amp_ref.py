"""CPU checks of the float64 references in joint_amp_ref.py (no GPU): the rounding helper against torch's own
conversions, the exact-data generators really exact, and exact data answered with equality rather than a tolerance."""
import math

import pytest
import torch

import joint_amp_ref as R


def _probe_values():
    """fp32 values around every rounding case of bf16 / f16: ties both ways, just off ties, subnormals of both formats,
    fp32 subnormals, the overflow edge, signed zeros, infinities."""
    vals = [0.0, -0.0, 1.0, -1.0, math.inf, -math.inf, 65504.0, 65519.0, 65520.0, -65520.0, 3.3895313892515355e38,
            2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -126, 2.0 ** -133, 2.0 ** -149,
            3 * 2.0 ** -134, 1e-40, -1e-40, 5.96e-8, 6.1e-5, 1e-5]
    x = torch.tensor(vals, dtype=torch.float32)
    # bf16 ties (low 16 bits 0x8000, even and odd kept part) and their neighbours; f16 ties (13 dropped bits)
    base = torch.randint(0, 2 ** 31 - 1, (4096,), generator=torch.Generator().manual_seed(1), dtype=torch.int64)
    bits = torch.cat([(base & ~0xFFFF) | 0x8000, (base & ~0xFFFF) | 0x7FFF, (base & ~0xFFFF) | 0x8001,
                      (base & ~0x1FFF) | 0x1000, (base & ~0x1FFF) | 0x0FFF, base])
    bits = bits & 0x7FFFFFFF
    bits = bits[((bits >> 23) & 0xFF) != 0xFF]          # finite only
    r = torch.from_numpy(bits.to(torch.int32).numpy().view("float32"))
    small = torch.randn(4096, generator=torch.Generator().manual_seed(2)) * 1e-6    # f16 subnormal range
    tiny = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 1e-39   # bf16 / fp32 subnormals
    mid = torch.randn(4096, generator=torch.Generator().manual_seed(4)) * 1e3
    return torch.cat([x, r, -r, small, tiny, mid])


@pytest.mark.parametrize("dt", [torch.bfloat16, torch.float16])
def test_round_to_matches_torch_conversion(dt):
    x = _probe_values()
    want = x.to(dt).to(torch.float64)
    got = R.round_to(x, dt)
    same = (got == want) | (torch.isnan(got) & torch.isnan(want))
    assert bool(same.all()), x[~same][:8]
    # sign of zero and of infinities kept
    assert bool((torch.signbit(got) == torch.signbit(want)).all())


def test_round_to_ties_to_even():
    one_bf = 2.0 ** -7                                   # bf16 spacing in [1, 2)
    x = torch.tensor([1 + one_bf / 2, 1 + 3 * one_bf / 2, 1 + one_bf / 2 + 2.0 ** -23, -(1 + 3 * one_bf / 2)],
                     dtype=torch.float32)
    assert R.round_to(x, "bf16").tolist() == [1.0, 1 + 2 * one_bf, 1 + one_bf, -(1 + 2 * one_bf)]
    h = torch.tensor([2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -24 * 1.5], dtype=torch.float32)   # f16 subnormal ties
    assert R.round_to(h, "f16").tolist() == [0.0, 2 * 2.0 ** -24, 2 * 2.0 ** -24]


def _fp32_sum(terms: torch.Tensor, order) -> torch.Tensor:
    acc = torch.zeros(terms.shape[:-1], dtype=torch.float32)
    for k in order:
        acc = acc + terms[..., k].float()
    return acc


@pytest.mark.parametrize("act", ["relu", "hardtanh"])
def test_exact_generators_are_exact_in_any_order(act):
    """Every product of the generated operands is an fp32 number, and the fp32 sum of a logit's (and of dZ's and dW's)
    products taken forwards and in a shuffled order equal the float64 sum."""
    B, T, U1, J, V = 2, 3, 4, 512, 96
    ep, pp, W, b = R.exact_case(B, T, U1, J, V, seed=5)
    g = R.exact_grad(B, T, U1, V, seed=5)
    for x, f in ((ep, "f16"), (pp, "f16"), (W, "f16"), (g, "f16"), (ep, "bf16"), (pp, "bf16"), (W, "bf16"), (g, "bf16")):
        assert torch.equal(R.round_to(x, f), x.double())
    z = R._z32(ep, pp).reshape(-1, J)
    a, d = R._act64(z, act)
    assert bool((z != 0).all() and (z.abs() != 1).all())            # no ties of relu / hardtanh or their derivatives
    assert torch.equal(R.round_to(a.float(), "bf16"), a)
    perm = torch.randperm(J, generator=torch.Generator().manual_seed(9)).tolist()
    fwd_terms = torch.cat([a[:, None, :] * W.double()[None], b.double()[None, :, None].expand(a.shape[0], V, 1)], -1)
    want = fwd_terms.sum(-1)
    assert torch.equal(_fp32_sum(fwd_terms, range(J + 1)).double(), want)
    assert torch.equal(_fp32_sum(fwd_terms, [J] + perm[::-1]).double(), want)
    g2 = g.reshape(-1, V).double()
    dz_terms = g2[:, None, :] * W.double().T[None]                   # (M, J, V)
    pre = dz_terms.sum(-1)
    assert torch.equal(_fp32_sum(dz_terms, range(V)).double(), pre)
    assert torch.equal(_fp32_sum(dz_terms, list(range(V))[::-1]).double(), pre)
    dw_terms = (g2.T[:, None, :] * a.T[None]).contiguous()           # (V, J, M)
    dw = dw_terms.sum(-1)
    M = g2.shape[0]
    assert torch.equal(_fp32_sum(dw_terms, range(M)).double(), dw)
    assert torch.equal(_fp32_sum(dw_terms, list(range(M))[::-1]).double(), dw)


@pytest.mark.parametrize("out", [torch.float32, torch.float16, torch.bfloat16])
@pytest.mark.parametrize("act", ["relu", "hardtanh"])
def test_exact_data_demands_equality(act, out):
    B, T, U1, J, V = 2, 5, 3, 64, 40
    ep, pp, W, b = R.exact_case(B, T, U1, J, V, seed=11)
    ref = R.fwd_ref(ep, pp, W, b, act, out)
    assert ref.exact
    # the value is an fp32 number (the exact sum) rounded once to the output format
    assert torch.equal(R.round_to(ref.value.float(), out), ref.value)
    # and a one-ulp change of any element fails the comparison
    got = ref.value.clone()
    got.view(-1)[7] += R._ulp(got.view(-1)[7:8].abs(), R.fmt_of(out))[0]
    R.assert_matches(ref.value, ref, "self")
    with pytest.raises(AssertionError, match="exact"):
        R.assert_matches(got, ref, "perturbed")
    g = R.exact_grad(B, T, U1, V, seed=11)
    lens = R.ragged_lens(B, T, U1, seed=11)
    for path in ("kernels", "library", "exact"):
        refs = R.bwd_ref(g.to(torch.bfloat16) if path == "library" else g, ep, pp, W, act, lens, path)
        for k in ("dz", "h", "d_ep", "d_pp", "dw", "db"):
            assert refs[k].exact, (path, k)


def test_general_data_gets_a_tight_tolerance():
    """tanh data: a tolerance, far below the old 3e-2 x rms, that still admits the kernel's rounding-order freedom."""
    B, T, U1, J, V = 1, 4, 3, 512, 64
    ep, pp, W, b = R.random_case(B, T, U1, J, V, seed=3)
    ref = R.fwd_ref(ep, pp, W, b, "tanh", torch.float32)
    assert not ref.exact
    rms = float(ref.value.pow(2).mean().sqrt())
    assert float(ref.tol.median()) < 1e-5 * rms          # the fp32 chain alone
    assert float(ref.tol.max()) < 3e-3 * rms             # plus one operand ulp of the few near-midpoint activations
    # an fp32 evaluation of the same rounded operands in another order passes
    z = R._z32(ep, pp).reshape(-1, J)
    a = R.round_to(torch.tanh(z).float(), "bf16").float()
    w = R.round_to(W, "bf16").float()
    alt = (a.flip(-1) @ w.flip(-1).T + b).double().view_as(ref.value)
    R.assert_matches(alt, ref, "fp32 reordered")
    # a W image truncated instead of rounded does not
    wt = torch.from_numpy((W.numpy().view("int32") & ~0xFFFF).view("float32")).double()
    bad = (a.double() @ wt.T + b.double()).view_as(ref.value)
    with pytest.raises(AssertionError):
        R.assert_matches(bad, ref, "truncated W")


def test_padded_cells_excluded_by_selection():
    B, T, U1, J, V = 2, 4, 3, 16, 32
    ep, pp, W, b = R.exact_case(B, T, U1, J, V, seed=2)
    lens = (torch.tensor([4, 2], dtype=torch.int32), torch.tensor([2, 0], dtype=torch.int32))
    g = R.exact_grad(B, T, U1, V, seed=2)
    m = R.cell_mask(B, T, U1, lens, "cpu")
    g_nan = torch.where(m[..., None], g, torch.tensor(float("nan")))
    g_inf = torch.where(m[..., None], g, torch.tensor(float("inf")))
    r0 = R.bwd_ref(g, ep, pp, W, "relu", lens)
    for gg in (g_nan, g_inf):
        r1 = R.bwd_ref(gg, ep, pp, W, "relu", lens)
        for k in r0:
            assert torch.equal(r0[k].value, r1[k].value), k
    assert bool((r0["dz"].value[~m] == 0).all())
