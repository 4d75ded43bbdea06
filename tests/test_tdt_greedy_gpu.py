"""TDT greedy search on the device (wr_greedy_search_tdt, DeviceDecoder.greedy_tdt, Transducer.tdt_greedy_search_batch)
against the float64 loop of tests/tdt_greedy_ref.py over copies of the same modules.

Wherever device tokens are compared with that loop, the loop's smallest top-1 / top-2 gap over every token and every
duration decision is asserted to be >= 1e-3 first (the bound of tests/test_transducer_tdt_gpu.py for J = 16 fp32 rows): a
condition on the reference, not a tolerance on the result.  The seeds were chosen on the CPU so that the reference alone
meets it, together with the other conditions each test states; widening `ffn_out` (SCALE) widens every gap alike."""
import copy
import functools
from collections import Counter, namedtuple

import pytest
import torch

import tdt_greedy_ref as ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V, E, P, J, H = 11, 8, 8, 16, 12
GAP = 1e-3
LOOKS = (1, 2, 4, 0)

Case = namedtuple("Case", "pred joint enc lens V durations n_steps")


def modules(seed, kind="lstm", vocab=V, D=3, embed_rows=None, scale=1.0):
    import wenet_celoss_amd as w
    torch.manual_seed(seed)
    rows = embed_rows or vocab
    if kind == "lstm":
        pred = w.RNNPredictor(rows, P, P, 0.0, H, 2, dropout=0.0)
    elif kind == "embedding":
        pred = w.EmbeddingPredictor(rows, P, 0.0, n_head=2, history_size=2)
    else:
        pred = w.ConvPredictor(rows, P, 0.0, history_size=2)
    joint = w.TransducerJoint(vocab + D, E, P, J)
    with torch.no_grad():
        joint.ffn_out.weight.mul_(scale)
        joint.ffn_out.bias.mul_(scale)
    return pred.eval(), joint.eval()


def make_case(seed, lens, durations, n_steps, T=None, kind="lstm", vocab=V, embed_rows=None, scale=1.0):
    pred, joint = modules(seed, kind, vocab, len(durations), embed_rows, scale)
    T = T or max(lens)
    enc = torch.randn(len(lens), T, E, generator=torch.Generator().manual_seed(seed + 1000))
    return Case(pred, joint, enc, list(lens), vocab, tuple(durations), n_steps)


def reference(c, durations="own", n_steps=None, joint=None, dup=()):
    durations = c.durations if durations == "own" else durations
    return ref.decode(c.pred, joint or c.joint, c.enc, c.lens, c.V, durations, 0, n_steps or c.n_steps, dup)


def device(c, tmax=None, max_hyp=None, joint=None):
    from wenet_celoss_amd.decoder import DeviceDecoder
    N, T, _ = c.enc.shape
    return DeviceDecoder(copy.deepcopy(c.pred).to(DEV), copy.deepcopy(joint or c.joint).to(DEV), N, N, tmax or T,
                         T * c.n_steps if max_hyp is None else max_hyp)


def run_tdt(dec, c, durations=None, n_steps=None):
    return dec.greedy_tdt(c.enc.to(DEV), torch.tensor(c.lens, dtype=torch.int32), durations or c.durations,
                          n_steps=n_steps or c.n_steps, blank=0, return_frames=True)


def check(got, want, what=""):
    toks, frames = got
    print(what, "tokens", toks, "frames", frames, "smallest gap", min(r.gap for r in want))
    assert min(r.gap for r in want) >= GAP
    assert toks == [r.tokens for r in want], what
    assert frames == [r.frames for r in want], what


# ------------------------------------------------------------------------------------------ 1: batch vs the reference --
SEED_BATCH, SCALE_BATCH, N_STEPS_BATCH = 3, 1.0, 2      # chosen on the CPU: smallest gap 3.7e-3 (5.5e-3 in the tie test)


@functools.lru_cache(maxsize=None)
def batch_case():
    c = make_case(SEED_BATCH, (12, 9, 1, 7, 12), (0, 1, 2), N_STEPS_BATCH, scale=SCALE_BATCH)
    want = reference(c)
    return c, want, batch_conditions(c, want)


def batch_conditions(c, want):
    """What the reference of test 1 has to show; a list of the conditions that fail."""
    bad = []
    if min(r.gap for r in want) < GAP:
        bad.append("gap")
    if sum(len(r.tokens) >= 2 for r in want) < 2:
        bad.append("two streams with two tokens")
    fewer = reference(c, n_steps=c.n_steps - 1)
    if not any(a.tokens != b.tokens for a, b in zip(want, fewer)):
        bad.append("n_steps rule")
    if not any(k == 0 and d == 2 for r in want for _, k, d in r.trace):
        bad.append("blank with d = 2")
    if not any(r.end > n for r, n in zip(want, c.lens)):
        bad.append("overshoot")
    return bad


@pytest.fixture(scope="module")
def batch_decoder():
    return device(batch_case()[0])


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "launches"])
@pytest.mark.parametrize("look", LOOKS)
def test_batch_equals_the_float64_loop(batch_decoder, look, graph):
    c, want, failed_conditions = batch_case()
    assert failed_conditions == []
    batch_decoder.set_graph(graph)
    batch_decoder.set_lookahead(look)
    check(run_tdt(batch_decoder, c), want, f"look {look} graph {graph}")
    for r, n in zip(want, c.lens):
        assert all(0 <= f < n for f in r.frames) and r.frames == sorted(r.frames)


# --------------------------------------------------------------------------------- 2: other duration sets --
SEED_124, SCALE_124 = 0, 1.0
SEED_08, SCALE_08 = 0, 1.0


@pytest.mark.parametrize("durations, seed, scale, T", [((1, 2, 4), SEED_124, SCALE_124, 12), ((0, 8), SEED_08, SCALE_08, 20)],
                         ids=["1-2-4", "0-8"])
def test_other_duration_sets(durations, seed, scale, T):
    c = make_case(seed, (T, T - 3, 5), durations, 2, scale=scale)
    want = reference(c)
    assert any(r.tokens for r in want)
    taken = {d for r in want for _, _, d in r.trace}
    assert min(durations) in taken and max(durations) in taken             # the longest jump: >= the look-ahead for (0, 8)
    dec = device(c)
    for look in LOOKS:
        dec.set_lookahead(look)
        check(run_tdt(dec, c), want, f"durations {durations} look {look}")


# ------------------------------------------------------------------------------------------------ 3: exact ties --
def tie_case():
    """Test 1's model with the most frequent token's ffn_out row copied into the last token row, and the most frequent
    duration's row copied into the next duration column -> (case, joiner, {copy: original column}, the token and the
    duration copied)."""
    c, want, _ = batch_case()
    tok = [k for k, _ in Counter(k for r in want for k in r.tokens).most_common() if k < c.V - 1][0]
    dur = [j for j, _ in Counter(c.durations.index(d) for r in want for _, _, d in r.trace).most_common()
           if j < len(c.durations) - 1][0]
    joint = copy.deepcopy(c.joint)
    with torch.no_grad():
        for lo, hi in ((tok, c.V - 1), (c.V + dur, c.V + dur + 1)):
            joint.ffn_out.weight[hi] = joint.ffn_out.weight[lo]
            joint.ffn_out.bias[hi] = joint.ffn_out.bias[lo]
    return c, joint, {c.V - 1: tok, c.V + dur + 1: c.V + dur}, (tok, c.durations[dur])


def test_exact_ties_go_to_the_lowest_index():
    c, joint, dup, (tok, d_lo) = tie_case()
    want = reference(c, joint=joint, dup=dup)
    tokens = [k for r in want for k in r.tokens]
    assert tok in tokens and c.V - 1 not in tokens
    taken = {d for r in want for _, _, d in r.trace}
    assert d_lo in taken and c.durations[c.durations.index(d_lo) + 1] not in taken
    dec = device(c, joint=joint)
    for look in LOOKS:
        dec.set_lookahead(look)
        check(run_tdt(dec, c), want, f"ties look {look}")


# ------------------------------------------------------------------------------- 4: width steps of tdt_rows_kernel --
SEED_305, SCALE_305 = 0, 1.0
SEED_2054, SCALE_2054 = 0, 1.0


@pytest.mark.parametrize("width, seed, scale", [(305, SEED_305, SCALE_305), (2054, SEED_2054, SCALE_2054)])
def test_joiner_widths(width, seed, scale):
    c = make_case(seed, (8, 5, 8), (0, 1, 2), 2, vocab=width - 3, scale=scale)
    want = reference(c)
    assert sum(len(r.tokens) for r in want) >= 3
    assert max(k for r in want for k in r.tokens) >= 256                   # a token beyond the first 256-column pass
    dec = device(c)
    for look in (1, 4):
        dec.set_lookahead(look)
        check(run_tdt(dec, c), want, f"width {width} look {look}")


# -------------------------------------------------------------------------------------- 5: stateless predictors --
SEED_EMBEDDING, SCALE_EMBEDDING = 0, 1.0
SEED_CONV, SCALE_CONV = 0, 1.0


@pytest.mark.parametrize("kind, seed, scale", [("embedding", SEED_EMBEDDING, SCALE_EMBEDDING), ("conv", SEED_CONV, SCALE_CONV)])
def test_stateless_predictors(kind, seed, scale):
    c = make_case(seed, (10, 6, 10), (0, 1, 2), 2, kind=kind, scale=scale)
    want = reference(c)
    assert sum(len(r.tokens) >= 2 for r in want) >= 2                      # the token history matters
    dec = device(c)
    for look in (1, 4):
        dec.set_lookahead(look)
        check(run_tdt(dec, c), want, f"{kind} look {look}")


# -------------------------------------------------------------------------- 6: one handle, interleaved calls --
SEED_MIX, SCALE_MIX = 0, 1.0


@functools.lru_cache(maxsize=None)
def mix_case():
    # the embedding table has a row for every joiner column, so that the plain search may emit any of them
    c = make_case(SEED_MIX, (10, 7, 10), (0, 1, 2), 2, embed_rows=V + 3, scale=SCALE_MIX)
    return c, reference(c), reference(c, durations=(0, 1, 3)), reference(c, durations=None)


def test_one_handle_serves_interleaved_calls():
    c, want012, want013, want_plain = mix_case()
    assert [r.tokens for r in want012] != [r.tokens for r in want013]
    assert min(r.gap for r in want_plain) >= GAP and any(r.tokens for r in want_plain)
    dec = device(c, max_hyp=c.enc.shape[1] * c.n_steps)
    dec.set_graph(True)
    enc, lens = c.enc.to(DEV), torch.tensor(c.lens, dtype=torch.int32)
    for look in (1, 2):
        dec.set_lookahead(look)
        plain0 = dec.greedy(enc, lens, n_steps=c.n_steps, blank=0)
        check(run_tdt(dec, c, (0, 1, 2)), want012, "(0, 1, 2)")
        check(run_tdt(dec, c, (0, 1, 3)), want013, "(0, 1, 3)")
        check(run_tdt(dec, c, (0, 1, 2)), want012, "(0, 1, 2) again")
        plain1 = dec.greedy(enc, lens, n_steps=c.n_steps, blank=0)
        assert plain0 == plain1 == [r.tokens for r in want_plain]


# ----------------------------------------------------------------------------------------- 7, 8: the model --
class TinySubsampling(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.subsampling_rate: int = 4
        self.right_context: int = 6


class TinyEncoder(torch.nn.Module):
    """Linear + frame mask; returns (encoder_out, mask) like wenet encoders (the stand-in of test_transducer_gpu.py)."""

    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)
        self.embed = TinySubsampling()

    def forward(self, xs, xs_lens, decoding_chunk_size=0, num_decoding_left_chunks=-1):
        T = xs.size(1)
        mask = (torch.arange(T, device=xs.device)[None, :] < xs_lens[:, None].to(xs.device)).unsqueeze(1)
        return torch.tanh(self.proj(xs)), mask


def model():
    """The model of tests/test_transducer_tdt_gpu.py (seed 38: its float64 loop's smallest gap is 1.7e-2)."""
    import wenet_celoss_amd as w
    torch.manual_seed(38)
    return w.Transducer(V, 0, TinyEncoder(8, E), w.RNNPredictor(V, P, P, 0.0, H, 2, dropout=0.0),
                        w.TransducerJoint(V + 3, E, P, J), transducer_weight=1.0, hw_weight=0.0,
                        tdt_durations=(0, 1, 2), tdt_sigma=0.05).to(DEV).eval()


def test_device_and_host_loop_agree(monkeypatch):
    from wenet_celoss_amd.search.greedy_search import tdt_greedy_search
    m = model()
    speech = torch.randn(1, 12, 8, generator=torch.Generator().manual_seed(138)).to(DEV)
    with torch.no_grad():
        enc = torch.tanh(m.encoder.proj(speech))
    lens = torch.tensor([12], dtype=torch.int32)
    on_device = tdt_greedy_search(m, enc, lens, n_steps=3, return_frames=True)
    monkeypatch.setenv("WR_TDT_HOST", "1")
    on_host = tdt_greedy_search(m, enc, lens, n_steps=3, return_frames=True)
    print("device", on_device, "host", on_host)
    assert len(on_host[0][0]) >= 2
    assert on_device == on_host
    assert tdt_greedy_search(m, enc, lens, n_steps=3) == on_host[0]


def test_batch_equals_single():
    m = model()
    lens = [12, 7, 10]
    speech = torch.randn(3, 12, 8, generator=torch.Generator().manual_seed(138)).to(DEV)
    slen = torch.tensor(lens, dtype=torch.int32, device=DEV)
    toks, frames = m.tdt_greedy_search_batch(speech, slen, n_steps=3, return_frames=True)
    assert toks == m.tdt_greedy_search_batch(speech, slen, n_steps=3)
    single = [m.greedy_search(speech[i:i + 1, :n], slen[i:i + 1], n_steps=3) for i, n in enumerate(lens)]
    print("batch", toks, frames, "single", single)
    assert all(dist == 0 for _, dist in single)
    assert toks == [hyps[0] for hyps, _ in single]
    assert sum(len(t) >= 2 for t in toks) >= 2
    assert all(len(f) == len(t) and all(0 <= x < n for x in f) for f, t, n in zip(frames, toks, lens))


# ------------------------------------------------------------------------------------ 9: hypothesis capacity --
def test_more_tokens_than_the_decoder_was_sized_for_is_an_error():
    c, want, _ = batch_case()
    assert max(len(r.tokens) for r in want) >= 2
    dec = device(c, max_hyp=1)
    with pytest.raises(RuntimeError, match="sized for 1"):
        run_tdt(dec, c)
