"""Host-side checks of TDT forced alignment: argument validation in Python and in the library (before any HIP call, with
the loss's codes and texts), the ABI, and the Transducer dispatch with a stub in place of the device call.  No GPU is
needed and none is used."""
import ctypes
import re

import pytest
import torch

from conftest import ROOT


def _cpu_call(durations=(0, 1, 2), blank=0, sigma=0.0, V=6, logits=None, targets=None, llens=(2,), tlens=(1,), **kw):
    import wenet_celoss_amd as w
    D = len(durations) if hasattr(durations, "__len__") else 1
    logits = torch.zeros(1, 2, 2, V + D) if logits is None else logits
    targets = torch.ones(1, 1, dtype=torch.int32) if targets is None else targets
    return w.rnnt_tdt_forced_align(logits, targets, torch.tensor(llens, dtype=torch.int32),
                                   torch.tensor(tlens, dtype=torch.int32), durations, blank=blank, sigma=sigma, **kw)


@pytest.mark.parametrize("bad", [dict(durations=()), dict(durations=tuple(range(9)) + (9,)), dict(durations=(0, 9)),
                                 dict(durations=(-1, 1)), dict(durations=(1, 1)), dict(durations=(2, 1)),
                                 dict(durations=(0,)), dict(durations=(0.0, 1.0)), dict(durations=(True, 2)),
                                 dict(durations=3), dict(sigma=-0.1), dict(sigma=float("inf")), dict(sigma=float("nan")),
                                 dict(sigma="x"), dict(blank=6), dict(blank=-7), dict(logits=torch.zeros(2, 2, 9)),
                                 dict(logits=torch.zeros(1, 2, 2, 3)), dict(llens=(0,)), dict(llens=(3,)),
                                 dict(tlens=(2,)), dict(tlens=(-1,)), dict(targets=torch.full((1, 1), 6, dtype=torch.int32)),
                                 dict(targets=torch.full((1, 1), -1, dtype=torch.int32)),
                                 dict(targets=torch.ones(1, 2, dtype=torch.int32)), dict(llens=(2, 2))])
def test_bad_values_raise_value_error_before_the_device_check(bad):
    with pytest.raises(ValueError, match="rnnt_tdt_forced_align"):
        _cpu_call(**bad)


@pytest.mark.parametrize("good", [dict(), dict(durations=(1,)), dict(durations=[0, 2]), dict(durations=tuple(range(9))),
                                  dict(sigma=0.05), dict(blank=5), dict(blank=-1), dict(blank=-6), dict(llens=(1,)),
                                  dict(tlens=(0,), targets=torch.full((1, 1), -1, dtype=torch.int32)),
                                  dict(return_blank_jumps=True), dict(logits=torch.zeros(1, 2, 2, 9, dtype=torch.bfloat16))])
def test_good_values_reach_the_device_check(good):
    with pytest.raises(RuntimeError, match="no CPU path"):
        _cpu_call(**good)


def test_export_and_binding():
    import wenet_celoss_amd as w
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    assert "rnnt_tdt_forced_align" in w.__all__ and callable(w.rnnt_tdt_forced_align)
    text = open(ROOT + "/include/wr_api.h").read()
    assert "TDT forced alignment" in text and "Tie rule" in text
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"\bwr_rnnt_tdt_align\s*\(", text)
    assert hasattr(lib, "wr_rnnt_tdt_align") and "wr_rnnt_tdt_align" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["wr_rnnt_tdt_align"][1]) == 20
    assert _lib.API_VERSION == 3 and lib.wr_api_version() == 3


def test_library_rejects_bad_arguments_without_launch_as_the_loss_does():
    from wenet_celoss_amd import _lib
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    one = ctypes.c_void_p(256)          # a placeholder that is not null; every call below is refused before it is read
    big = 1 << 40

    def durs(*d):
        return (ctypes.c_int32 * max(len(d), 1))(*d)

    def align(B=2, T=4, U1=3, V=8, blank=0, d=(0, 1, 2), D=None, sigma=0.0, wsb=big, dtype=0, ptr=null, outs=null):
        rc = lib.wr_rnnt_tdt_align(ptr, dtype, ptr, ptr, ptr, B, T, U1, V, blank, durs(*d), len(d) if D is None else D,
                                   sigma, outs, outs, null, outs, ptr, wsb, null)
        return rc, lib.wr_last_error().decode()

    def loss(B=2, T=4, U1=3, V=8, blank=0, d=(0, 1, 2), D=None, sigma=0.0, wsb=big, dtype=0, **_):
        rc = lib.wr_rnnt_tdt_loss_fwd(null, dtype, null, null, null, B, T, U1, V, blank, durs(*d),
                                      len(d) if D is None else D, sigma, null, null, wsb, null)
        return rc, lib.wr_last_error().decode()

    shared = [dict(D=0), dict(d=tuple(range(9)), D=10), dict(d=(0, 2, 1)), dict(d=(1, 1)), dict(d=(-1, 1)), dict(d=(0, 9)),
              dict(d=(0,)), dict(sigma=-1.0), dict(sigma=float("nan")), dict(sigma=float("inf")), dict(blank=8),
              dict(blank=-1), dict(U1=1100), dict(B=4000, T=4000, U1=1000), dict(B=0), dict(V=0), dict(dtype=7),
              dict(wsb=16), dict()]
    codes = set()
    for kw in shared:
        (rc, err), (rc_l, err_l) = align(**kw), loss(**kw)
        assert rc == rc_l and rc in (-1, -2, -3), kw
        assert err.startswith("rnnt_tdt_align: ") and err_l.startswith("rnnt_tdt_loss_fwd: "), (kw, err, err_l)
        assert err[len("rnnt_tdt_align: "):] == err_l[len("rnnt_tdt_loss_fwd: "):], kw
        codes.add(rc)
    assert codes == {-1, -2, -3}
    assert align()[1] == "rnnt_tdt_align: null pointer argument"
    # the inputs are there, a required output is not
    rc, err = align(ptr=one)
    assert rc == -1 and err == "rnnt_tdt_align: label_frames, label_durations or scores is null"
    # a null durations array
    rc = lib.wr_rnnt_tdt_align(null, 0, null, null, null, 2, 4, 3, 8, 0, null, 3, 0.0, null, null, null, null, null, big, null)
    assert rc == -1 and b"durations is null" in lib.wr_last_error()
    # the workspace is the loss's: no size query of its own
    assert not hasattr(lib, "wr_rnnt_tdt_align_workspace_bytes")


class _Enc(torch.nn.Module):
    def __init__(self, idim, odim):
        super().__init__()
        self.proj = torch.nn.Linear(idim, odim)

    def output_size(self):
        return self.proj.out_features

    def forward(self, xs, xs_lens, decoding_chunk_size=0, num_decoding_left_chunks=-1):
        mask = (torch.arange(xs.size(1))[None, :] < xs_lens[:, None]).unsqueeze(1)
        return torch.tanh(self.proj(xs)), mask


def _model(joint_outputs=23, **kw):
    import wenet_celoss_amd as w
    torch.manual_seed(0)
    return w.Transducer(23, 0, _Enc(8, 12), w.RNNPredictor(23, 10, 10, 0.0, 14, 2, dropout=0.0),
                        w.TransducerJoint(joint_outputs, 12, 10, 16), ctc_weight=0.0, transducer_weight=1.0, **kw)


class _StubJoint(torch.nn.Module):
    """Stands in for TransducerJoint's forward, which is a device call: (B, T, U+1, outputs) in plain torch"""

    def __init__(self, outputs):
        super().__init__()
        self.outputs = outputs

    def forward(self, enc_out, pred_out):
        return (enc_out.sum(-1)[:, :, None, None] + pred_out.sum(-1)[:, None, :, None]).expand(-1, -1, -1, self.outputs)


SPEECH = torch.zeros(2, 5, 8)
SLEN = torch.tensor([5, 3], dtype=torch.int32)
TEXT = torch.tensor([[3, 5, 2], [4, -1, -1]])
TLEN = torch.tensor([3, 1], dtype=torch.int32)


def test_transducer_dispatch_with_a_stub_device_call(monkeypatch):
    from wenet_celoss_amd import transducer as tr
    seen = {}

    def stub(logits, targets, logit_lengths, target_lengths, durations, blank=0, sigma=0.0, return_blank_jumps=False):
        seen.update(shape=tuple(logits.shape), dtype=logits.dtype, targets=targets.tolist(), llens=logit_lengths.tolist(),
                    tlens=target_lengths.tolist(), durations=durations, blank=blank, sigma=sigma, jumps=return_blank_jumps,
                    ldtype=logit_lengths.dtype, tdtype=targets.dtype)
        out = ("frames", "durations", "scores")
        return out + ("jumps",) if return_blank_jumps else out

    def refuse(*a, **k):
        raise AssertionError("a TDT model must not reach the regular-lattice alignment")

    monkeypatch.setattr(tr, "rnnt_tdt_forced_align", stub)
    monkeypatch.setattr(tr, "joint_rnnt_forced_align", refuse)
    monkeypatch.setattr(tr, "rnnt_forced_align", refuse)
    m = _model(26, tdt_durations=(0, 1, 2), tdt_sigma=0.05).eval()
    m.joint = _StubJoint(26)
    assert m.tdt_forced_align(SPEECH, SLEN, TEXT, TLEN) == ("frames", "durations", "scores")
    assert seen == dict(shape=(2, 5, 4, 26), dtype=torch.float32, targets=[[3, 5, 2], [4, 0, 0]], llens=[5, 3],
                        tlens=[3, 1], durations=(0, 1, 2), blank=0, sigma=0.05, jumps=False, ldtype=torch.int32,
                        tdtype=torch.int32)
    assert m.tdt_forced_align(SPEECH, SLEN, TEXT, TLEN, return_blank_jumps=True)[3] == "jumps" and seen["jumps"]
    # forced_align(head="joint") on a TDT model is that path, with its documented pair
    seen.clear()
    assert m.forced_align(SPEECH, SLEN, TEXT, TLEN) == ("frames", "scores")
    assert seen["shape"] == (2, 5, 4, 26) and seen["durations"] == (0, 1, 2) and not seen["jumps"]
    with pytest.raises(ValueError, match="simple_loss_weight"):
        m.forced_align(SPEECH, SLEN, TEXT, TLEN, head="simple")          # untouched


def test_non_tdt_model_keeps_its_path_and_refuses_tdt_forced_align(monkeypatch):
    from wenet_celoss_amd import transducer as tr
    m = _model().eval()
    with pytest.raises(ValueError, match="no tdt_durations"):
        m.tdt_forced_align(SPEECH, SLEN, TEXT, TLEN)
    calls = []
    monkeypatch.setattr(tr, "rnnt_tdt_forced_align", lambda *a, **k: calls.append("tdt"))
    monkeypatch.setattr(tr, "joint_rnnt_forced_align", lambda *a, **k: calls.append("joint") or ("f", "s"))
    assert m.forced_align(SPEECH, SLEN, TEXT, TLEN) == ("f", "s") and calls == ["joint"]
