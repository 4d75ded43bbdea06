#!/usr/bin/env python3
"""Record tests/golden/joint_backward_calls.json: what `joint_backward` asks of the library, case by case, at the commit
the host call path is compared against.  The package is imported from a checkout of THAT commit, given on the command
line, never from this tree:

    git worktree add /tmp/parent <commit>        (or: git archive <commit> | tar -x -C /tmp/parent)
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_joint_backward_calls.py /tmp/parent

No library is built or loaded (tests/joint_call_trace.py replaces it by a recorder).  Cases with the same record share it,
and records are filed under their sequence of entry points, so the file stays small."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "wenet-celoss_amd")):
        sys.exit(__doc__)
    checkout = os.path.abspath(sys.argv[1])
    assert checkout != os.path.dirname(os.path.dirname(HERE)), "record from a checkout of the earlier commit, not this tree"
    sys.path.insert(0, checkout)
    sys.path.insert(1, os.path.dirname(HERE))
    import wenet_celoss_amd as pkg
    import joint_call_trace as tr
    assert os.path.dirname(pkg.__file__).startswith(checkout), pkg.__file__
    groups = {}
    for case in tr.grid(pkg.joint.TERMS_F16):
        calls = tr.record(pkg, case)
        by_record = groups.setdefault(json.dumps(tr.sequence(calls)), {})
        by_record.setdefault(json.dumps(calls), []).append(tr.case_id(case))
    doc = {"dims": {"B": tr.B, "T": tr.T, "U1": tr.U1, "activation": tr.ACT, "workspace_bytes": tr.WS_BYTES,
                    "logit_lengths": tr.LLENS, "target_lengths": tr.TLENS},
           "case_fields": list(tr.FIELDS),
           "sequences": [{"sequence": json.loads(seq),
                          "records": [{"calls": json.loads(calls), "cases": cases} for calls, cases in by_record.items()]}
                         for seq, by_record in groups.items()]}
    path = os.path.join(HERE, "joint_backward_calls.json")
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": ' + (json.dumps(v) if k != "sequences" else "[\n" + ",\n".join(
            '  {"sequence": ' + json.dumps(s["sequence"]) + ',\n   "records": [\n' + ",\n".join(
                "    " + json.dumps(r) for r in s["records"]) + "]}" for s in v) + "]") for k, v in doc.items()) + "\n}\n")
    n = sum(len(r["cases"]) for s in doc["sequences"] for r in s["records"])
    print(f"{path}: {n} cases, {len(doc['sequences'])} sequences, "
          f"{sum(len(s['records']) for s in doc['sequences'])} records, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
