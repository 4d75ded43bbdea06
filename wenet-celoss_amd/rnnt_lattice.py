"""What the k2 RNN-T losses share (rnnt_simple.py, rnnt_smoothed.py, rnnt_pruned.py, k2.py): the ``rnnt_type=`` /
``delay_penalty=`` arguments, the boundary / symbols preparation with its one host sync and the device check, the lattice
sweeps, the occupancy layout and the diagnostics (csrc/rnnt_lattice.hip; the contract is in include/wr_api.h, "Lattice
types and the delay penalty"; DESIGN.md, "Modified lattice and delay penalty").

  rnnt_type = "regular"    a label arc stays on its frame, (t,u) -> (t,u+1); a final blank leaves (T_b-1, U_b)
  rnnt_type = "modified"   a label arc consumes a frame, (t,u) -> (t+1,u+1): exactly one arc per frame, T_b >= U_b
  delay_penalty            ``delay_penalty * ((T_b - 1) / 2 - t)`` added to every label arc's log-probability

``"constrained"`` is not offered (NotImplementedError).  There is one path: every loss hands its lattice type and penalty
to the `*_lattice` / `*_cols` entry points, which for the defaults launch the kernels of the plain entry points.
"""
from __future__ import annotations

import math
from typing import Tuple

import torch

from . import _lib


def check_lattice(what: str, rnnt_type, delay_penalty) -> Tuple[int, float]:
    """(wr_lattice code, penalty as float) or ValueError / NotImplementedError; needs no device."""
    if rnnt_type == "constrained":
        raise NotImplementedError(f"{what}: rnnt_type 'constrained' is not implemented (\"regular\" and \"modified\" are)")
    if not isinstance(rnnt_type, str) or rnnt_type not in _lib.LATTICES:
        raise ValueError(f"{what}: rnnt_type must be \"regular\" or \"modified\" (got {rnnt_type!r})")
    try:
        pen = float(delay_penalty)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: delay_penalty must be a number (got {delay_penalty!r})") from None
    if not (pen >= 0.0 and math.isfinite(pen)):
        raise ValueError(f"{what}: delay_penalty must be finite and not negative (got {delay_penalty})")
    return _lib.LATTICES[rnnt_type], pen


_REDUCTIONS = {"none": lambda costs: costs, "mean": torch.Tensor.mean, "sum": torch.Tensor.sum}


def reducer(reduction):
    """The tail of every loss front end: the function that takes the costs (B,) to themselves ("none"), their plain
    batch mean or their sum; ValueError for any other name.  A front end asks for it where it checks `reduction` and
    applies it to what its node returns."""
    if not isinstance(reduction, str) or reduction not in _REDUCTIONS:
        raise ValueError("reduction should be one of 'none', 'mean', or 'sum'")
    return _REDUCTIONS[reduction]


def is_default(lat: int, pen: float) -> bool:
    return lat == 0 and pen == 0.0


def require_device(what: str, who: str, *tensors) -> None:
    if not all(t.is_cuda for t in tensors):
        raise RuntimeError(f"wenet_celoss_amd.{what}: {who} must live on a HIP device (this package has no CPU path)")


def prepare(what: str, who: str, on, B: int, T: int, U: int, boundary, symbols=None, V: int = 0, more=(),
            min_frames: int = 0):
    """Boundary, symbols and device of a k2 loss -> (T_b int32, U_b int32, symbols int32 or None) on the device of
    ``on[0]``.  ``boundary`` None = rows ``(0, 0, U, T)``.  One host sync checks the rows (begins zero, 0 <= U_b <= U,
    0 <= T_b <= T), the labels inside each length (within [0, V); those past it become 0), whatever ``more`` adds --
    (one-element count of violations on the device, error text) pairs -- and T_b >= ``min_frames``.  Full lengths with
    nothing else to check need no sync.  The device check (``who`` names the tensors ``on``) comes last, so bad values
    in CPU tensors still raise ValueError."""
    dev = on[0].device
    if boundary is None:
        bd = torch.tensor([0, 0, U, T], dtype=torch.int64, device=dev).repeat(B, 1)
    else:
        if boundary.dim() != 2 or boundary.shape[0] != B or boundary.shape[1] != 4:
            raise ValueError(f"{what}: boundary must be (B, 4) = ({B}, 4), got {tuple(boundary.shape)}")
        bd = boundary.to(device=dev, dtype=torch.int64)
    counts, sy = list(more), None
    if symbols is not None:
        sy = symbols.to(device=dev)
        inside = torch.arange(U, device=dev)[None, :] < bd[:, 2:3]
        counts.insert(0, ((inside & ((sy < 0) | (sy >= V))).sum().reshape(1),
                          f"{what}: a symbol inside its boundary lies outside [0, {V})"))
        sy = torch.where(inside, sy, torch.zeros((), dtype=sy.dtype, device=dev)).to(torch.int32).contiguous()
    if boundary is not None or counts:
        host = (torch.cat([bd.reshape(-1)] + [c for c, _ in counts]) if counts else bd.reshape(-1)).cpu()  # one host sync
        rows = host[:4 * B].reshape(B, 4)
        if B and int(rows[:, :2].abs().max()) != 0:
            raise ValueError(f"{what}: boundary rows must begin at (0, 0) (got {rows[:, :2].tolist()})")
        if B and (int(rows[:, 2].min()) < 0 or int(rows[:, 2].max()) > U):
            raise ValueError(f"{what}: boundary symbol ends must lie in [0, {U}] (got {rows[:, 2].tolist()})")
        if B and (int(rows[:, 3].min()) < 0 or int(rows[:, 3].max()) > T):
            raise ValueError(f"{what}: boundary frame ends must lie in [0, {T}] (got {rows[:, 3].tolist()})")
        for bad, (_, text) in zip(host[4 * B:].tolist(), counts):
            if bad != 0:
                raise ValueError(text)
        if B and int(rows[:, 3].min()) < min_frames:
            raise ValueError(f"{what}: boundary frame ends must be at least {min_frames} (got {rows[:, 3].tolist()})")
    require_device(what, who, *on)
    return bd[:, 3].to(torch.int32).contiguous(), bd[:, 2].to(torch.int32).contiguous(), sy


def sweeps(rws: torch.Tensor, ll, tl, B: int, T: int, U1: int, lat: int, pen: float) -> torch.Tensor:
    """The lattice sweeps over the arcs a statistics call left in the RNN-T workspace ``rws``: costs (B,) float32."""
    costs = torch.empty(B, dtype=torch.float32, device=rws.device)
    _lib.call("wr_rnnt_lattice_sweeps", ll, tl, B, T, U1, lat, pen, costs, rws, rws.numel(), device=rws.device)
    return costs


def occupancies_to_k2(occ_emit: torch.Tensor, occ_blank: torch.Tensor, lat: int):
    """(B, T, U+1) arc occupancies -> k2's (px_grad, py_grad): px_grad (B, U, T+1) with a zero last column for the
    regular lattice, (B, U, T) for the modified one; py_grad (B, U+1, T)."""
    B, T, U1 = occ_emit.shape
    if lat == _lib.LATTICES["modified"]:
        px_grad = occ_emit[:, :, :U1 - 1].transpose(1, 2).contiguous()
    else:
        px_grad = torch.zeros(B, U1 - 1, T + 1, dtype=torch.float32, device=occ_emit.device)
        px_grad[:, :, :T] = occ_emit[:, :, :U1 - 1].transpose(1, 2)
    return px_grad, occ_blank.transpose(1, 2).contiguous()


@torch.no_grad()
def lattice(rws: torch.Tensor, ll, tl, B: int, T: int, U1: int, lat: int, pen: float):
    """Diagnostics: the sweeps, then (costs, alpha, beta, flag) -- alpha / beta as plain (B, T, U+1) tensors, flag the
    workspace's "row statistics were redone by the direct kernel" word (a one-element int32 tensor)."""
    costs = sweeps(rws, ll, tl, B, T, U1, lat, pen)
    alpha = torch.empty(B, T, U1, dtype=torch.float32, device=rws.device)
    beta = torch.empty_like(alpha)
    _lib.call("wr_rnnt_lattice_export", rws, rws.numel(), ll, tl, B, T, U1, lat, alpha, beta, device=rws.device)
    flag = rws[-256:-252].view(torch.int32).clone()       # the last 256-byte slot of the workspace (wr_common.hpp RnntWs)
    return costs, alpha, beta, flag
