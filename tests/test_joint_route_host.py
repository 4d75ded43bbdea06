"""The host side of the joiner backward issues the calls it issued before its dispatch became one table, and the call
helper names the entry point it called.  No GPU: tests/joint_call_trace.py replaces the library by a recorder.

tests/golden/joint_backward_calls.json was recorded by tests/golden/make_joint_backward_calls.py from the commit before
`backward_route` existed (three interleaved copies of the dispatch): per case of the grid, the ordered entry points with
their scalar arguments, null pointers and the dtype the gradient was handed over in.  It is the independent statement of
the table: `joint_backward` must replay it to the letter, and `backward_route` alone must agree with it too."""
import contextlib
import json
import os

import pytest
import torch

import joint_call_trace as tr
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "joint_backward_calls.json")) as f:
        return json.load(f)


def _cases(fixture):
    """case id -> recorded calls."""
    return {c: r["calls"] for s in fixture["sequences"] for r in s["records"] for c in r["cases"]}


def test_fixture_covers_the_grid(fixture):
    from wenet_celoss_amd.joint import TERMS_F16
    assert fixture["case_fields"] == list(tr.FIELDS)
    assert fixture["dims"] == {"B": tr.B, "T": tr.T, "U1": tr.U1, "activation": tr.ACT, "workspace_bytes": tr.WS_BYTES,
                               "logit_lengths": tr.LLENS, "target_lengths": tr.TLENS}
    ids = [c for s in fixture["sequences"] for r in s["records"] for c in r["cases"]]
    want = [tr.case_id(c) for c in tr.grid(TERMS_F16)]
    assert len(want) == 1920 and len(ids) == len(set(ids)) and sorted(ids) == sorted(want)
    seqs = [json.dumps(s["sequence"]) for s in fixture["sequences"]]
    assert len(seqs) == len(set(seqs)) == 20
    for s in fixture["sequences"]:
        assert s["records"] and all(tr.sequence(r["calls"]) == s["sequence"] and r["cases"] for r in s["records"])


def test_joint_backward_issues_the_recorded_calls(fixture):
    import wenet_celoss_amd as pkg
    recorded = _cases(fixture)
    wrong = []
    for case in tr.grid(pkg.joint.TERMS_F16):
        got = json.loads(json.dumps(tr.record(pkg, case)))
        if got != recorded[tr.case_id(case)]:
            wrong.append((tr.case_id(case), got, recorded[tr.case_id(case)]))
    assert not wrong, f"{len(wrong)} of 1920 cases differ; first: {wrong[0]}"


def test_backward_route_states_the_recorded_table(fixture):
    """The pure function against the same records: library or kernels, the dZ and dW entry points (dW where the record
    has one: need_w), the dtype the gradient is handed over in, and the `terms` the split entry points get."""
    from wenet_celoss_amd.joint import TERMS_F16, backward_route
    recorded = _cases(fixture)
    for case in tr.grid(TERMS_F16):
        terms, gdt, V, J, amp_backward, mm_out_dtype, _, need_w = case
        route = backward_route(terms, tr.DTYPES[gdt], V, J, amp_backward, mm_out_dtype)
        seq = tr.sequence(recorded[tr.case_id(case)])
        what = tr.case_id(case)
        if seq[0][0] == "_amp_backward_library":
            assert route.library and route.grad_dtype == tr.DTYPES[seq[0][1]] == tr.DTYPES[gdt], what
            continue
        assert not route.library and len(seq) == 1 + need_w, what
        assert (route.dz, route.grad_dtype) == (seq[0][0], tr.DTYPES[seq[0][1]]), what
        if need_w:
            assert (route.dw, route.grad_dtype) == (seq[1][0], tr.DTYPES[seq[1][1]]), what
        for name, _, t in seq:
            assert t is None or t == route.terms, what


@pytest.mark.parametrize("name,args", [
    ("wr_joint_db_f16", (None, None, None, 2, 3, 2, 40, None, None, 0)),
    ("wr_joint_db_bf16", (None, None, None, 2, 3, 2, 40, None, None, 0)),
    ("wr_joint_bwd_dz_split_bf16", (None, None, None, None, None, None, 2, 3, 2, 8, 40, 0, 1, None, None, None, 0)),
    ("wr_joint_bwd_dw_split_bf16", (None, None, None, None, 2, 3, 2, 8, 40, 1, None, None, None, 0)),
])
def test_call_names_the_symbol_it_called(monkeypatch, name, args):
    """`_lib.call` on the real library with null pointers (refused by the argument checks, before any launch, as in
    test_abi.py): the error names the entry point that was called."""
    from wenet_celoss_amd import _lib
    monkeypatch.setattr(_lib, "current_stream", lambda device=None: None)
    monkeypatch.setattr(torch.cuda, "device", lambda device=None: contextlib.nullcontext())
    with pytest.raises(RuntimeError) as e:
        _lib.call(name, *args, device=None)
    assert str(e.value).startswith(name + " failed ("), str(e.value)


def test_workspace_is_a_fresh_byte_tensor_of_the_queried_size():
    from wenet_celoss_amd import _lib
    n = _lib.load().wr_joint_split_workspace_bytes(512, 4232)
    a = _lib.workspace("wr_joint_split_workspace_bytes", 512, 4232, device="cpu")
    b = _lib.workspace("wr_joint_split_workspace_bytes", 512, 4232, device="cpu")
    assert n > 0 and a.dtype == torch.uint8 and a.shape == (n,) and a.data_ptr() != b.data_ptr()
