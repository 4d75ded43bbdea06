"""The Python host layer -- the fused and memory-bounded loss nodes, the losses that take logits, TDT alignment, the
searches of `DeviceDecoder`, the loss block and hypothesis scores of `Transducer`, the argument checks of the k2-style
losses -- issues the calls it issued at the
commit tests/golden/host_calls.json was recorded from (by tests/golden/make_host_calls.py, before the RNN-T and TDT twins
of that layer were folded into shared paths), returns the same host results and refuses the same bad calls with the same
messages.  No GPU: tests/host_call_trace.py replaces the library by a recorder."""
import json
import os

import pytest

import host_call_trace as tr
from conftest import GOLDEN


@pytest.fixture(scope="module")
def recorded():
    """case id -> record."""
    with open(os.path.join(GOLDEN, "host_calls.json")) as f:
        doc = json.load(f)
    assert doc["workspace_bytes"] == tr.WS_BYTES
    ids = [c for r in doc["records"] for c in r["cases"]]
    assert len(ids) == len(set(ids))
    return {c: {k: v for k, v in r.items() if k != "cases"} for r in doc["records"] for c in r["cases"]}


def test_fixture_covers_the_cases(recorded):
    import wenet_celoss_amd as pkg
    assert sorted(recorded) == sorted(tr.cases(pkg))
    refused = [c for c, r in recorded.items() if "raises" in r]
    assert refused and all(c.startswith("refusal: ") for c in refused)
    assert all("raises" in r for c, r in recorded.items() if c.startswith("refusal: "))


def test_the_plain_entry_points_are_called_with_both_regularisers_at_zero(recorded):
    names = {c["name"] for c in recorded["bounded rnnt budget=rows2 need_w=1 lambda=0.0 penalty=0.0 fp32"]["calls"]}
    assert {"wr_rnnt_loss_sweeps", "wr_joint_rnnt_grad"} <= names and not any(n.endswith("_lattice") for n in names)
    names = {c["name"] for c in recorded["rnnt_loss fp32 lambda=0.0 penalty=0.0 inplace=0"]["calls"]}
    assert names == {"wr_rnnt_workspace_bytes", "wr_rnnt_loss_fwd", "backward", "wr_rnnt_loss_bwd"}


def test_the_bucketed_costs_come_back_in_the_callers_order(recorded):
    want = [100.0 * u + t for t, u in zip(tr.BUCKET_T, tr.BUCKET_U)]
    for case in ("bucketed", "bucketed budget", "bucketed buckets=2"):
        assert recorded[case]["result"]["loss"]["values"] == want, case
        assert sum(c["name"] == "wr_rnnt_workspace_bytes" for c in recorded[case]["calls"]) >= 2, case   # one per group


def test_the_host_layer_issues_the_recorded_calls(recorded):
    import wenet_celoss_amd as pkg
    wrong = []
    for name, case in tr.cases(pkg).items():
        got = json.loads(json.dumps(tr.record(pkg, case)))
        if got != recorded[name]:
            wrong.append((name, got, recorded[name]))
    assert not wrong, f"{len(wrong)} of {len(recorded)} cases differ; first: {wrong[0]}"
