#!/usr/bin/env python3
"""Record tests/golden/host_calls.json: what the Python host layer asks of the library, case by case, at the commit the
host layer is compared against.  The package is imported from a checkout of THAT commit, given on the command line, never
from this tree:

    git worktree add /tmp/parent <commit>        (or: git archive <commit> | tar -x -C /tmp/parent)
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_host_calls.py /tmp/parent

No library is built or loaded (tests/host_call_trace.py replaces it by a recorder).  Cases with the same record share it,
so the file stays small.

Not reached on CPU tensors: the bucketed two-op branch of `Transducer.compute_loss` (the joiner resolves to a 16-bit
mode under CUDA autocast only, and autocast leaves CPU tensors alone); tests/test_transducer_gpu.py
(test_amp_two_op_path_buckets_ragged_batches) covers it on the device and tests/test_rnnt_latency_host.py
(test_transducer_compute_loss_hands_the_options_to_every_route) its keywords on the host.  Nor the n-best rescoring tail
(`Transducer._rescore`): `transducer_attention_rescoring` and `tdt_attention_rescoring` are recorded up to their refusal
of the other kind of model only, since past it they run the encoder, a beam search and the attention decoder;
tests/test_transducer_gpu.py (test_attention_rescoring_matches_float64) and tests/test_tdt_beam_gpu.py
(test_cal_tdt_score_and_attention_rescoring) cover the tail on the device."""
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
    import host_call_trace as tr
    assert os.path.dirname(pkg.__file__).startswith(checkout), pkg.__file__
    groups = {}
    for name, rec in tr.record_all(pkg).items():
        groups.setdefault(json.dumps(rec), []).append(name)
    assert len(pkg.fused.plan_buckets(tr.BUCKET_T, tr.BUCKET_U, max_buckets=4)) >= 2
    path = os.path.join(HERE, "host_calls.json")
    with open(path, "w") as f:
        f.write('{"workspace_bytes": %d,\n "records": [\n' % tr.WS_BYTES)
        f.write(",\n".join('  {"cases": ' + json.dumps(names) + ",\n   " + rec[1:] for rec, names in groups.items()))
        f.write("]}\n")
    print(f"{path}: {sum(len(n) for n in groups.values())} cases, {len(groups)} records, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
