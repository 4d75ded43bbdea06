"""The workgroup order of the RNN-T streaming passes (logical_block, wenet-celoss_amd/csrc/wr_common.hpp), restated.

Workgroup i of a grid of G runs on XCD i & 7; rnnt_lse_kernel and rnnt_grad_kernel work on the rows of logical block
logical_block(i, G, mode, c).  For every G, mode and c that must be a permutation of range(G), and under mode 2 the
workgroups of one XCD must get the contiguous ranges the header states.  (The issue's mode 1, one contiguous region per
XCD, was measured and removed: profiles/xcd_row_order.md.)  The restatement is also held against the
header's own function, compiled for the host.
"""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = (1, 2, 5)


def logical_block(i, G, mode, c):
    x, j = i & 7, i >> 3
    if mode == 2 and c > 0:
        span = 8 * c
        if i < G // span * span:
            return i // span * span + x * c + j % c
    return i


def grids(c):
    return [1, 3, 7, 8, 9, 15, 16, 17, 63, 64, 65, 8 * c - 1, 8 * c, 8 * c + 1, 16 * c + 5]


CASES = [(mode, c, G) for mode in (0, 2) for c in CS for G in grids(c)]


@pytest.mark.parametrize("mode,c,G", CASES)
def test_permutation(mode, c, G):
    assert sorted(logical_block(i, G, mode, c) for i in range(G)) == list(range(G))


@pytest.mark.parametrize("mode", [0, 1, 3, -1])
@pytest.mark.parametrize("c", CS)
def test_every_other_mode_is_the_identity(mode, c):
    """Mode 0, and any value that is not a mode (1 was the XCD-region order, measured and removed)."""
    for G in grids(c):
        assert [logical_block(i, G, mode, c) for i in range(G)] == list(range(G))


@pytest.mark.parametrize("mode,c,G", [k for k in CASES if k[0] == 2])
def test_mode2_xcd_runs(mode, c, G):
    """Inside window w (8c blocks) XCD x gets [8cw + xc, 8cw + xc + c) in order; the G % 8c blocks at the end are the
    identity."""
    span = 8 * c
    full = G // span * span
    for w in range(G // span):
        for x in range(8):
            mine = [logical_block(i, G, 2, c) for i in range(w * span + x, (w + 1) * span, 8)]
            assert mine == list(range(w * span + x * c, w * span + x * c + c))
    assert [logical_block(i, G, 2, c) for i in range(full, G)] == list(range(full, G))


_PROBE = r"""
#include "wr_common.hpp"
extern "C" unsigned probe_logical_block(unsigned i, unsigned G, int mode, unsigned c) { return wr::logical_block(i, G, mode, c); }
"""


def test_header_agrees_with_the_restatement(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src, so = tmp_path / "probe.hip", tmp_path / "probe.so"
    src.write_text(_PROBE)
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "wenet-celoss_amd", "csrc")]
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-fPIC", "-shared"] + inc + [str(src), "-o", str(so)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lib = ctypes.CDLL(str(so))
    fn = lib.probe_logical_block
    fn.restype = ctypes.c_uint
    fn.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_int, ctypes.c_uint]
    for mode, c, G in CASES + [(2, 0, 17), (3, 2, 40), (1, 302, 347011), (2, 302, 347011), (2, 1208, 1208000)]:
        step = max(1, G // 4096)
        for i in list(range(0, G, step)) + [G - 1]:
            assert fn(i, G, mode, c) == logical_block(i, G, mode, c), (i, G, mode, c)
