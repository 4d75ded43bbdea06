"""CPU-side checks of the additive-joiner ("simple") RNN-T loss: the float64 helper the GPU tests lean on is itself
checked against `oracle.rnnt_loss_f64` and against brute-force path enumeration; the new entry points reject bad
arguments before any launch; the host layer's argument handling; the Transducer's optional heads."""
import ctypes

import numpy as np
import pytest
import torch

import rnnt_align_ref as aref
import rnnt_simple_ref as ref


def small_case(seed, B=3, T=6, U=3, V=7):
    rng = np.random.default_rng(seed)
    lm = rng.normal(size=(B, U + 1, V)).astype(np.float32)
    am = rng.normal(size=(B, T, V)).astype(np.float32)
    symbols = rng.integers(1, V, size=(B, U))
    return lm, am, symbols, np.array([T, 4, 2][:B]), np.array([U, 1, 0][:B])


def test_helper_lattice_matches_the_oracle():
    lm, am, symbols, t_lens, u_lens = small_case(1)
    oc, o_am, o_lm = ref.oracle_reference(lm, am, symbols, 0, t_lens, u_lens)
    for b in range(3):
        T, U = int(t_lens[b]), int(u_lens[b])
        cost, alpha, beta, oe, ob = ref.lattice_f64(lm[b], am[b], symbols[b], 0, T, U)
        assert abs(cost - oc[b]) < 1e-9 * max(1.0, abs(cost))
        assert abs(alpha[T - 1, U] + beta[T - 1, U] + cost) < 1e-9
        # the logits gradient summed over u is sum_u occ * softmax minus the arc occupancies scattered to their symbols
        x = (am[b, :T, None, :] + lm[b, None, :U + 1, :]).astype(np.float64)
        p = np.exp(x - x.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
        g = (oe + ob)[:, :, None] * p
        g[:, :, 0] -= ob
        for u in range(U):
            g[:, u, symbols[b, u]] -= oe[:, u]
        np.testing.assert_allclose(g.sum(1), o_am[b, :T], rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(g.sum(0), o_lm[b, :U + 1], rtol=1e-6, atol=1e-7)
        assert abs(ob.sum() - T) < 1e-9 and abs(oe.sum() - U) < 1e-9


def test_helper_torch_costs_match_the_oracle():
    lm, am, symbols, t_lens, u_lens = small_case(2)
    oc, o_am, o_lm = ref.oracle_reference(lm, am, symbols, 0, t_lens, u_lens)
    l = torch.tensor(lm, dtype=torch.float64, requires_grad=True)
    a = torch.tensor(am, dtype=torch.float64, requires_grad=True)
    costs = ref.loss_torch_f64(l, a, symbols, 0, t_lens, u_lens)
    # the oracle sees the float32 sum am + lm (one rounding of 6e-8 relative per logit), this expression the float64 one
    np.testing.assert_allclose(costs.detach().numpy(), oc, rtol=1e-6)
    costs.sum().backward()
    np.testing.assert_allclose(a.grad.numpy(), o_am, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(l.grad.numpy(), o_lm, rtol=1e-6, atol=1e-7)


def test_helper_matches_path_enumeration_on_a_2x2_lattice():
    rng = np.random.default_rng(3)
    lm = rng.normal(size=(2, 5)); am = rng.normal(size=(2, 5))
    symbols = [3]
    total, oe, ob = ref.enumerate_paths(lm, am, symbols, 1, 2, 1)      # T = 2, U = 1: two paths
    cost, _, _, oe2, ob2 = ref.lattice_f64(lm, am, symbols, 1, 2, 1)
    assert abs(-np.log(total) - cost) < 1e-12
    np.testing.assert_allclose(oe2, oe, atol=1e-12)
    np.testing.assert_allclose(ob2, ob, atol=1e-12)
    lm3, am3, sy3, _, _ = small_case(4)                                # and a 4 x 4 one: 20 paths
    total, oe, ob = ref.enumerate_paths(lm3[0], am3[0], sy3[0], 0, 4, 3)
    cost, _, _, oe2, ob2 = ref.lattice_f64(lm3[0], am3[0], sy3[0], 0, 4, 3)
    assert abs(-np.log(total) - cost) < 1e-12
    np.testing.assert_allclose(oe2, oe, atol=1e-12)
    np.testing.assert_allclose(ob2, ob, atol=1e-12)


def test_align_cases_of_the_gpu_test_have_a_clear_margin():
    """The forced-alignment comparison on the GPU keeps a case only if the float64 best / second-best margin exceeds
    1e-3; every seeded case must, so none is dropped there."""
    import test_rnnt_simple_gpu as g
    for case in g.ALIGN_CASES:
        margins = [m for _, m in g.align_margins(*g.align_case(*case))]
        assert min(margins) > 1e-3, (case, margins)


def test_cpu_tensors_raise_no_cpu_path():
    import wenet_celoss_amd as w
    lm, am, symbols, _, _ = small_case(5)
    args = (torch.tensor(lm), torch.tensor(am), torch.tensor(symbols), 0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.rnnt_loss_simple(*args)
    with pytest.raises(RuntimeError, match="no CPU path"):
        w.rnnt_simple_forced_align(*args)


def test_host_argument_checks():
    import wenet_celoss_amd as w
    lm, am, symbols, _, _ = small_case(6)
    lm, am, symbols = torch.tensor(lm), torch.tensor(am), torch.tensor(symbols)
    bd = torch.tensor([[0, 0, 3, 6], [0, 1, 1, 4], [0, 0, 0, 2]])
    with pytest.raises(ValueError, match="begin"):
        w.rnnt_loss_simple(lm, am, symbols, 0, boundary=bd)
    bd[1, 1] = 0; bd[2, 0] = 1
    with pytest.raises(ValueError, match="begin"):
        w.rnnt_simple_forced_align(lm, am, symbols, 0, boundary=bd)
    bd[2, 0] = 0; bd[0, 3] = 7
    with pytest.raises(ValueError, match="frame ends"):
        w.rnnt_loss_simple(lm, am, symbols, 0, boundary=bd)
    bd[0, 3] = 6; bd[0, 2] = 4
    with pytest.raises(ValueError, match="symbol ends"):
        w.rnnt_loss_simple(lm, am, symbols, 0, boundary=bd)
    with pytest.raises(ValueError, match="termination_symbol"):
        w.rnnt_loss_simple(lm, am, symbols, 7)
    with pytest.raises(ValueError, match="reduction"):
        w.rnnt_loss_simple(lm, am, symbols, 0, reduction="avg")
    with pytest.raises(ValueError, match="symbols"):
        w.rnnt_loss_simple(lm, am, symbols[:, :2], 0)
    bad = symbols.clone(); bad[0, 0] = 9
    with pytest.raises(ValueError, match="outside"):
        w.rnnt_loss_simple(lm, am, bad, 0)
    with pytest.raises(TypeError):
        w.rnnt_loss_simple(lm, am, symbols, 0, delay_penalty=0.1)


def test_entry_points_reject_bad_arguments_without_launch():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    one = ctypes.c_void_p(256)          # a non-null pointer that is never dereferenced: every check precedes the launches

    def stats(B=2, T=4, U1=3, V=8, blank=0, p=one, sws=1 << 30, rws=1 << 30):
        return lib.wr_rnnt_simple_stats(p, p, p, p, p, B, T, U1, V, blank, p, sws, p, rws, null)

    def grad(B=2, T=4, U1=3, V=8, blank=0, p=one, sws=1 << 30, rws=1 << 30):
        return lib.wr_rnnt_simple_grad(p, p, p, p, p, B, T, U1, V, blank, null, p, p, null, null, p, sws, p, rws, null)

    for fn in (stats, grad):
        assert fn(p=null) == -1 and b"null" in lib.wr_last_error()
        assert fn(blank=8) == -1 and b"blank" in lib.wr_last_error()
        assert fn(blank=-1) == -1 and b"blank" in lib.wr_last_error()
        assert fn(U1=1100) == -2 and b"1024" in lib.wr_last_error()
        assert fn(V=1) == -1 and b"2 classes" in lib.wr_last_error()
        assert fn(B=0) == -1
        assert fn(sws=16) == -3 and b"workspace" in lib.wr_last_error()
        assert fn(rws=16) == -3 and b"workspace" in lib.wr_last_error()
    assert lib.wr_rnnt_simple_workspace_bytes(0, 4, 3, 8) == 0
    small = lib.wr_rnnt_simple_workspace_bytes(2, 10, 5, 50)
    big = lib.wr_rnnt_simple_workspace_bytes(16, 1000, 151, 5000)
    assert 0 < small < big
    assert big < 16 * 1000 * 151 * 4 * 8                   # a few floats per lattice cell,
    assert big * 400 < 16 * 1000 * 151 * 5000 * 4          # far below the logits tensor


class _Enc(torch.nn.Module):
    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)

    def output_size(self):
        return self.proj.out_features


def _model(**kw):
    import wenet_celoss_amd as w
    torch.manual_seed(0)
    return w.Transducer(23, 0, _Enc(8, 12), w.RNNPredictor(23, 10, 10, 0.0, 14, 2, dropout=0.0),
                        w.TransducerJoint(23, 12, 10, 16), ctc_weight=0.0, transducer_weight=1.0, **kw)


def test_transducer_without_the_simple_loss_is_unchanged():
    before = set(_model().state_dict().keys())
    assert set(_model(simple_loss_weight=0.0).state_dict().keys()) == before
    assert not any(k.startswith("simple_") for k in before)
    import inspect
    import wenet_celoss_amd as w
    assert list(inspect.signature(w.Transducer.__init__).parameters)[-1] == "simple_loss_weight"


def test_transducer_with_the_simple_loss_adds_exactly_the_two_heads():
    before = set(_model().state_dict().keys())
    m = _model(simple_loss_weight=0.5)
    added = set(m.state_dict().keys()) - before
    assert added == {"simple_am_proj.weight", "simple_am_proj.bias", "simple_lm_proj.weight", "simple_lm_proj.bias"}
    assert before <= set(m.state_dict().keys())
    assert tuple(m.simple_am_proj.weight.shape) == (23, 12) and tuple(m.simple_lm_proj.weight.shape) == (23, 10)
