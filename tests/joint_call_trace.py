"""Record what `joint_backward` asks of the library, on CPU tensors and without the library.

Used twice: tests/golden/make_joint_backward_calls.py runs it over a checkout of the commit the fixture is recorded from,
tests/test_joint_route_host.py over the working tree; the two records must be identical.  The package reaches the device
through three seams only, and all three are replaced: `_lib.load` returns a recorder (every `*_workspace_bytes` query
answers WS_BYTES, everything else 0), `_lib.current_stream` returns None, `torch.cuda.device` is a null context; and
`torch.mm` accepts `out_dtype` on the CPU.

A record lists, in order, every entry point reached with its scalar arguments, the positions of its null pointers and --
for those whose first argument is the logits gradient -- the dtype that gradient was handed over in, read from the bytes
at the pointer (the gradient is all ones: 1.0 looks different in float32, float16 and bfloat16).  The vocabulary and joiner
sizes are written as "V" and "J", so that cases which differ only in them share a record in the fixture."""
import contextlib
import ctypes
import itertools
import os

import torch

WS_BYTES = 64
B, T, U1, ACT = 5, 7, 9, 4
LLENS, TLENS = [7, 5, 3, 7, 1], [8, 2, 0, 5, 8]
DTYPES = {"fp32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
_ONE = {b"\x00\x00\x80\x3f": "fp32", b"\x00\x3c\x00\x3c": "f16", b"\x80\x3f\x80\x3f": "bf16"}
FIELDS = ("terms", "gout_dtype", "V", "J", "amp_backward", "mm_out_dtype", "gout_zero_in_padding", "need_w")
# entry points whose first argument is the logits gradient
_TAKES_GRADIENT = ("wr_joint_bwd_dz", "wr_joint_bwd_dw", "wr_joint_db_")


def grid(terms_f16):
    """The 1920 cases, as tuples in FIELDS order."""
    return list(itertools.product((0, 1, 3, terms_f16), DTYPES, (28, 30, 36, 40, 44), (8, 6), ("library", "kernels"),
                                  (True, False), (True, False), (True, False)))


class _Recorder:
    def __init__(self, signatures, V, J):
        self.signatures, self.calls = signatures, []
        self.names = {V: "V", J: "J"}
        assert not {V, J} & {B, T, U1, ACT, WS_BYTES, 0, 1, 2, 3, 16}, "V or J collides with another scalar"

    def __getattr__(self, name):
        if name not in self.signatures:
            raise AttributeError(name)
        argtypes = self.signatures[name][1]

        def fn(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments for {len(argtypes)}"
            scalars, null, first = [], [], None
            for i, (a, ty) in enumerate(zip(args, argtypes)):
                if ty is ctypes.c_void_p:
                    a = a.value if isinstance(a, ctypes.c_void_p) else a
                    if not a:
                        null.append(i)
                    elif i == 0:
                        first = a
                else:
                    scalars.append(self.names.get(a, a))
            rec = {"name": name, "scalars": scalars, "null": null}
            if name.startswith(_TAKES_GRADIENT) and not name.endswith("_workspace_bytes"):
                rec["gradient"] = _ONE[ctypes.string_at(first, 4)]
            self.calls.append(rec)
            return WS_BYTES if name.endswith("_workspace_bytes") else 0
        return fn


def _mm(mm):
    def wrapped(a, b, out_dtype=None):
        return mm(a, b) if out_dtype is None else mm(a.to(out_dtype), b.to(out_dtype))
    return wrapped


class _NullDevice(contextlib.nullcontext):
    def __init__(self, device=None):
        super().__init__()


@contextlib.contextmanager
def _seams(pkg_lib, jm, recorder, amp_backward, mm_out_dtype):
    """The replacements listed in the module docstring, undone on exit."""
    saved = [(pkg_lib, "load", pkg_lib.load), (pkg_lib, "current_stream", pkg_lib.current_stream),
             (torch.cuda, "device", torch.cuda.device), (torch, "mm", torch.mm),
             (jm, "_mm_takes_out_dtype", jm._mm_takes_out_dtype), (jm, "_amp_backward_library", jm._amp_backward_library)]
    old_env = os.environ.get("WR_AMP_BACKWARD")
    library = jm._amp_backward_library

    def library_spy(*a, **k):
        recorder.calls.append({"name": "_amp_backward_library", "gradient": {v: n for n, v in DTYPES.items()}[a[1].dtype]})
        return library(*a, **k)
    try:
        pkg_lib.load = lambda: recorder
        pkg_lib.current_stream = lambda device=None: None
        torch.cuda.device = _NullDevice
        torch.mm = _mm(torch.mm)
        jm._mm_takes_out_dtype = lambda: mm_out_dtype
        jm._amp_backward_library = library_spy
        os.environ["WR_AMP_BACKWARD"] = amp_backward
        yield
    finally:
        for obj, name, value in saved:
            setattr(obj, name, value)
        if old_env is None:
            del os.environ["WR_AMP_BACKWARD"]
        else:
            os.environ["WR_AMP_BACKWARD"] = old_env


def record(pkg, case):
    """The calls `pkg.joint.joint_backward` makes for `case` (a tuple in FIELDS order): the list described above."""
    terms, gdt, V, J, amp_backward, mm_out_dtype, zero_pad, need_w = case
    ep, pp, w = torch.zeros(B, T, J), torch.zeros(B, U1, J), torch.zeros(V, J)
    gout = torch.ones(B, T, U1, V, dtype=DTYPES[gdt])
    llens, tlens = torch.tensor(LLENS, dtype=torch.int32), torch.tensor(TLENS, dtype=torch.int32)
    rec = _Recorder(pkg._lib.SIGNATURES, V, J)
    with _seams(pkg._lib, pkg.joint, rec, amp_backward, mm_out_dtype):
        out = pkg.joint.joint_backward(gout, ep, pp, w, llens, tlens, terms, need_w, True, zero_pad, ACT)
    assert [o is not None for o in out] == [True, True, need_w, True]
    return rec.calls


def sequence(calls):
    """The summary a record is filed under: (entry point, dtype the gradient reached it in, `terms` it was given) of the
    compute calls in order; None where an entry point takes no gradient or no `terms` (the split ones take `terms` as
    their last scalar before the workspace size)."""
    return [[c["name"], c.get("gradient"), c["scalars"][-2] if "_split" in c["name"] else None]
            for c in calls if not c["name"].endswith("_workspace_bytes")]


def case_id(case) -> str:
    """A case as the fixture spells it: its FIELDS joined by blanks, flags as 0 / 1."""
    return " ".join(str(int(x)) if isinstance(x, bool) else str(x) for x in case)
