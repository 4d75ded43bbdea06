"""TransducerJoint with the reference's interface, backed by the MFMA kernels.

Mirror of ``wenet/transducer/joint.py:9-70``: same constructor arguments and
parameter names (``enc_ffn``, ``pred_ffn``, ``ffn_out`` -- reference checkpoints
load unchanged), same ``forward(enc_out, pred_out) -> (B, T, U, V)``.

The two pre-join projections are plain library GEMMs on small tensors
(torch.nn.Linear on rocBLAS).  Everything after them -- broadcast add, tanh,
the 512 -> V contraction and its backward w.r.t. the activations -- is the
fused HIP path (``wr_joint_fwd`` / ``wr_joint_bwd_dz`` / ``wr_joint_bwd_dw``); only the
two reductions of ``dZ`` over u / t are library sum calls.

Precision (extension, default exact fp32): ``precision="bf16x3"`` (or env ``WR_JOINT_PRECISION=bf16x3``) runs the
forward contraction on the bf16 matrix cores with every fp32 operand split in two (three MFMA terms, fp32
accumulation): logits within 1e-4 of the fp32 result relative to their scale, 2.7x faster.
``precision="bf16"`` is the single-term AMP mode (the reference under ``--use_amp`` runs this Linear in fp16):
under autocast the logits come out in the autocast dtype.
``precision="f16"`` is the same single-term mode with float16 operands (``wr_joint_fwd_f16``: the operand format of the
reference's ``ffn_out`` under its default fp16 autocast, 11 significand bits against bf16's 8); its logits follow the
``"bf16"`` rule.
Every forward is launched by ``joint_forward``.  In the backward, which entry points compute the activation gradient
``dZ = dY W`` and the weight gradient ``dW = dY^T H`` (the same split as the forward, the f16 kernels, the exact kernels,
or the vendor GEMM library for a 16-bit gradient) and whether the gradient is widened first is the table in
``backward_route``'s docstring, run by ``joint_backward``; the bias gradient is summed in fp32.
``precision="autocast"`` is resolved at every call (``effective_precision``): ``"fp32"`` outside autocast (the reference's
``cv`` pass and runs without ``--use_amp``), ``"bf16"`` under bf16 autocast, ``"f16"`` under fp16 autocast -- the
recommended ``WR_JOINT_PRECISION`` for ``--use_amp``.

Supported configurations: ``joint_mode='add'`` (the only mode the reference accepts, joint.py:22); every
``activation`` of ``get_activation`` (common.py:228-242: tanh -- shipped --, relu, hardtanh, selu, swish, gelu; value
and derivative are evaluated inside the kernels from the pre-activation), ``prejoin_linear`` on (shipped, conf/encoder_bias_conformer_rnnt_*.yaml:21-26) or off,
``postjoin_linear`` off (shipped) or on (training forward; distributed over the two addends, see
``pre_activation``).
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import os

import torch
from torch import nn

from . import _lib

# name -> `terms` code of the kernels; TERMS_F16 selects the f16 single-term entry points; "autocast" is resolved per call
TERMS_F16 = 16
_PRECISIONS = {"fp32": 0, "bf16x3": 3, "bf16": 1, "f16": TERMS_F16, "autocast": None}


def activation_code(activation: str) -> int:
    """wr_activation code of a get_activation name (wenet/utils/common.py:228-242)."""
    if activation not in _lib.ACTIVATIONS:
        raise KeyError(f"joint activation must be one of {sorted(_lib.ACTIVATIONS)}, got {activation!r}")
    return _lib.ACTIVATIONS[activation]


_TORCH_ACTIVATIONS = {"tanh": nn.Tanh, "relu": nn.ReLU, "hardtanh": nn.Hardtanh, "selu": nn.SELU, "swish": nn.SiLU,
                      "gelu": nn.GELU}


def _resolve_precision(precision: Optional[str]) -> str:
    if precision is None:
        precision = os.environ.get("WR_JOINT_PRECISION", "fp32")
    if precision not in _PRECISIONS:
        raise ValueError(f"joint precision must be one of {sorted(_PRECISIONS)}, got {precision!r}")
    return precision


def effective_precision(precision: str, autocast_enabled: bool, autocast_dtype) -> str:
    """The mode a call runs in: "autocast" becomes "fp32" outside autocast, "bf16" under bf16 autocast and "f16" under fp16
    autocast; every other name stands for itself."""
    if precision != "autocast":
        return precision
    if not autocast_enabled:
        return "fp32"
    if autocast_dtype == torch.float16:
        return "f16"
    if autocast_dtype == torch.bfloat16:
        return "bf16"
    return "fp32"


def _call_precision(precision: Optional[str]) -> str:
    """_resolve_precision, then effective_precision under the current CUDA autocast state."""
    precision = _resolve_precision(precision)
    on = torch.is_autocast_enabled("cuda")
    return effective_precision(precision, on, torch.get_autocast_dtype("cuda") if on else None)


def joiner_workspace(terms: int, J: int, V: int, dev):
    """Workspace of a joiner forward (also of wr_joint_rnnt_stats / wr_joint_rnnt_grad, which run the same forward)."""
    return _lib.workspace("wr_joint_workspace_bytes" if terms == 0 else "wr_joint_split_workspace_bytes", J, V, device=dev)


def joint_forward(ep, pp, w, b, llens, tlens, terms: int, act: int, out=None, out_dtype=torch.float32, stats=None):
    """Launch the joiner forward into `out` (B, T, U1, V; allocated in `out_dtype` when None) and return it.  The one
    place that picks the entry point: exact fp32 (`terms` 0), f16 single term (TERMS_F16) or bf16 split (1 / 3 terms);
    `stats` = (targets, blank, RNN-T workspace) asks for the variant whose epilogue also leaves the loss's row statistics
    in that workspace (fp32 logits; the plain and the epilogue variant write bit-identical logits).  Inputs contiguous."""
    B, T, J = ep.shape
    U1 = pp.shape[1]
    V = w.shape[0]
    dev = ep.device
    if out is None:
        out = torch.empty(B, T, U1, V, dtype=out_dtype, device=dev)
    ws = joiner_workspace(terms, J, V, dev)
    head, dims = (ep, pp, w, b, llens, tlens), (B, T, U1, J, V, act)
    if stats is not None:
        targets, blank, rws = stats
        if terms == 0:
            _lib.call("wr_joint_fwd_lse", *head, targets, *dims, blank, out, ws, ws.numel(), rws, rws.numel(), device=dev)
        else:
            _lib.call("wr_joint_fwd_split_lse", *head, targets, *dims, blank, terms, out, ws, ws.numel(), rws, rws.numel(),
                      device=dev)
    elif terms == 0:
        _lib.call("wr_joint_fwd", *head, *dims, out, ws, ws.numel(), device=dev)
    elif terms == TERMS_F16:
        _lib.call("wr_joint_fwd_f16", *head, *dims, out, _lib.dtype_code(out.dtype), ws, ws.numel(), device=dev)
    else:
        _lib.call("wr_joint_fwd_split", *head, *dims, terms, out, _lib.dtype_code(out.dtype), ws, ws.numel(), device=dev)
    return out


class _JointFn(torch.autograd.Function):
    # Under AMP (executor.py:91 wraps the forward in autocast) the pre-join Linear layers hand over fp16/bf16
    # activations; the MFMA kernels are exact-fp32, so inputs are cast up and the logits come out fp32.
    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, ep, pp, w, b, llens, tlens, terms=0, out_dtype=torch.float32, act=0):
        if not ep.is_cuda:
            raise RuntimeError("wenet_celoss_amd.TransducerJoint: tensors must live on a HIP device "
                               "(this package has no CPU path)")
        ep, pp, w, b = ep.contiguous(), pp.contiguous(), w.contiguous(), b.contiguous()
        out = joint_forward(ep, pp, w, b, llens, tlens, terms, act, out_dtype=out_dtype if terms else torch.float32)
        ctx.save_for_backward(ep, pp, w, llens, tlens)
        ctx.terms = terms
        ctx.act = act
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, gout):
        ep, pp, w, llens, tlens = ctx.saved_tensors
        d_ep, d_pp, d_w, d_b = joint_backward(gout, ep, pp, w, llens, tlens, ctx.terms, ctx.needs_input_grad[2],
                                              ctx.needs_input_grad[3], act=ctx.act)
        return d_ep, d_pp, d_w, d_b, None, None, None, None, None


_MM_OUT_DTYPE = None


def _mm_takes_out_dtype() -> bool:
    """torch.mm(bf16, bf16, out_dtype=float32) -- fp32 results of a bf16 GEMM without a rounding to bf16 in between -- is what
    the library form of the AMP backward needs; a PyTorch without it keeps the backward on this package's kernels."""
    global _MM_OUT_DTYPE
    if _MM_OUT_DTYPE is None:
        try:
            a = torch.zeros(8, 8, dtype=torch.bfloat16, device="cuda")
            _MM_OUT_DTYPE = torch.mm(a, a, out_dtype=torch.float32).dtype == torch.float32
        except (TypeError, RuntimeError):
            _MM_OUT_DTYPE = False
    return _MM_OUT_DTYPE


class Route(NamedTuple):
    """What `backward_route` decides.  `library`: the vendor GEMMs (`_amp_backward_library`), `dz` / `dw` are then None.
    Otherwise the two entry points, the dtype the gradient is handed to them in (its own, or widened to float32) and the
    `terms` the split ones are given."""
    library: bool
    dz: Optional[str]
    dw: Optional[str]
    grad_dtype: torch.dtype
    terms: int


def backward_route(terms: int, gout_dtype, V: int, J: int, amp_backward: str, mm_out_dtype: bool) -> Route:
    """Where a logits gradient of dtype `gout_dtype` goes in the backward of a joiner run with `terms`; `amp_backward` is
    the value of WR_AMP_BACKWARD, `mm_out_dtype` that of `_mm_takes_out_dtype()`.  The single statement of the dispatch:

    A bfloat16 gradient under TERMS_F16 ("f16" under bf16 autocast) is first read as terms = 1.  With
    ok16 = V % 8 == 0 and V >= 32 and J % 4 == 0, rows are tried in order:

      terms     gradient     condition                      dZ / dW entry points              gradient handed over
      1         bf16, f16    ok16, not "kernels", mm        library GEMMs                     as it is
      F16       f16          ok16, not "kernels", mm        library GEMMs                     as it is
      0         any          --                             wr_joint_bwd_dz / _dw             float32
      F16       any          V % 4 != 0 or V < 32           wr_joint_bwd_dz / _dw             float32
      F16       f16          ok16                           wr_joint_bwd_dz_f16 / _dw_f16     as it is
      F16       any          otherwise                      wr_joint_bwd_dz_f16 / _dw_f16     float32 (rounded to f16 in the kernel)
      1, 3      bf16         ok16                           .._dz_split_bf16 / _dw_split_bf16 as it is
      1, 3      any          otherwise                      dZ, dW chosen separately (below)  float32
          dZ: wr_joint_bwd_dz_split when V % 4 == 0 and V >= 32, else wr_joint_bwd_dz
          dW: wr_joint_bwd_dw_split when V % 4 == 0 and J % 4 == 0, else wr_joint_bwd_dw

    Kept as they were, not repaired here:
      * the dW rule has no V >= 32, so V % 4 == 0 and V < 32 pairs the exact dZ with the split dW (F16 goes exact for both);
      * the dW rule tests J % 4 and the dZ rule does not: with V >= 32 the library refuses such a J in the dZ call already
        (so does every F16 kernel row), and the test only decides for V < 32;
      * a float16 gradient under terms 1 or 3 is only ever taken as it is by the library row; the kernels get it widened;
      * V % 8 != 0 (with V % 4 == 0) widens a 16-bit gradient although the kernels round it back to the same values."""
    bf16, f16 = torch.bfloat16, torch.float16
    if terms == TERMS_F16 and gout_dtype == bf16:
        terms = 1
    half = f16 if terms == TERMS_F16 else bf16            # the 16-bit format this mode's kernels take as it is
    ok16 = terms != 0 and V % 8 == 0 and V >= 32 and J % 4 == 0
    if (ok16 and amp_backward != "kernels" and mm_out_dtype
            and (terms == 1 and gout_dtype in (bf16, f16) or terms == TERMS_F16 and gout_dtype == f16)):
        return Route(True, None, None, gout_dtype, terms)
    grad = half if ok16 and gout_dtype == half else torch.float32
    if terms == 0 or (terms == TERMS_F16 and (V % 4 != 0 or V < 32)):
        return Route(False, "wr_joint_bwd_dz", "wr_joint_bwd_dw", grad, 0)
    if terms == TERMS_F16:
        return Route(False, "wr_joint_bwd_dz_f16", "wr_joint_bwd_dw_f16", grad, terms)
    sfx = "_bf16" if grad == bf16 else ""
    return Route(False, "wr_joint_bwd_dz_split" + sfx if V % 4 == 0 and V >= 32 else "wr_joint_bwd_dz",
                 "wr_joint_bwd_dw_split" + sfx if V % 4 == 0 and J % 4 == 0 else "wr_joint_bwd_dw", grad, terms)


def _valid_cells(llens, tlens, T: int, U1: int):
    """(B, T, U1) bool: the cells inside [0, T_b) x [0, U_b]; the rest is padding."""
    dev = llens.device
    tt = torch.arange(T, device=dev)[None, :, None] < llens[:, None, None]
    uu = torch.arange(U1, device=dev)[None, None, :] <= tlens[:, None, None]
    return tt & uu


def _amp_backward_library(lib, gout, ep, pp, w, llens, tlens, need_w, need_b, gout_zero_in_padding, act):
    """Single-term (AMP) backward with a 16-bit (bfloat16 or float16) logits gradient: the two contractions dH = dY W and [dW | db] = dY^T [H | 1]
    are plain 16-bit GEMMs with fp32 accumulation and fp32 results -- they go to the vendor GEMM library (measured at the
    B = 16 BASELINE slice: 11.9 + 15.8 ms against 23.0 + 34.5 ms for this package's single-term kernels, which stay
    reachable with WR_AMP_BACKWARD=kernels); what is fused around them stays here: ``wr_joint_dz_act`` applies the
    activation's derivative to dH in place and writes H in bf16 (zero in padded cells), ``wr_joint_db_bf16`` / ``_f16`` sums
    the gradient's columns for the bias; the gradient tensor is never widened.  (`lib`, the loaded library, is not used:
    the entry points are reached through `_lib.call`.)"""
    B, T, J = ep.shape
    U1 = pp.shape[1]
    V = w.shape[0]
    dev = ep.device
    M = B * T * U1
    g2 = gout.view(M, V)
    dt = gout.dtype                                 # bfloat16, or float16 (autocast's default dtype: the reference's --use_amp)
    dz = torch.mm(g2, w.to(dt), out_dtype=torch.float32).view(B, T, U1, J)
    hb = torch.empty(M, J, dtype=dt, device=dev) if need_w else None
    _lib.call("wr_joint_dz_act", dz, ep, pp, llens, tlens, B, T, U1, J, act, hb, _lib.dtype_code(dt), J, device=dev)
    d_ep = dz.sum(dim=2)
    d_pp = dz.sum(dim=1)
    d_w = d_b = None
    if need_w:                                      # H is zero in padded cells: they contribute nothing ...
        gw = g2
        if not gout_zero_in_padding and llens is not None:
            # ... unless the gradient there is not finite (0 * NaN = NaN would poison every column of d_w): padded rows
            # are selected to zero, as the kernels' cell mask does -- one pass over the gradient, only when the caller
            # does not guarantee zeros there (the RNN-T loss does: no pass on the training path)
            gw = torch.where(_valid_cells(llens, tlens, T, U1).view(M, 1), g2, torch.zeros((), dtype=dt, device=dev))
        d_w = torch.mm(gw.t(), hb, out_dtype=torch.float32)
    if need_b:                                      # (as one more column of that GEMM, N = J + 8, the library padded to
        d_b = torch.empty(V, dtype=torch.float32, device=dev)       # its next tile: 23.3 ms against 15.8 + 3)
        ws = _lib.workspace("wr_joint_db_workspace_bytes", B, T, U1, V, device=dev)
        if gout_zero_in_padding:
            llens = tlens = None
        _lib.call("wr_joint_db_bf16" if dt == torch.bfloat16 else "wr_joint_db_f16", g2, llens, tlens, B, T, U1, V, d_b,
                  ws, ws.numel(), device=dev)
    return d_ep, d_pp, d_w, d_b


def joint_backward(gout, ep, pp, w, llens, tlens, terms: int, need_w: bool, need_b: bool,
                   gout_zero_in_padding: bool = False, act: int = 0, dz_out=None, h_out=None):
    """Backward of the joiner from the logits gradient `gout` (B,T,U1,V): returns (d_ep, d_pp, d_w, d_b).
    Shared by the joiner's autograd Function and by the fused joiner + RNN-T loss Function (fused.py); which entry points
    it reaches is `backward_route`'s table.
    `gout_zero_in_padding`: the caller guarantees gout == 0 outside [0,T_b) x [0,U_b] (the RNN-T gradient pass
    zero-fills there).  The activation gradient still gets the lengths (it skips padded tiles and writes H = 0 in
    padded cells), but the weight-gradient reduction then needs no per-row mask: padded rows contribute 0 * 0.
    `dz_out` / `h_out`: fp32 (B,T,U1,J) buffers for dZ and H of the kernel routes (the memory-bounded fused node
    reuses one pair for all its slices); allocated here when None.  (Before the dispatch became one table, the "f16"
    mode's fall-back to the exact kernels allocated its own pair whatever was passed; no caller passes one there.)"""
    B, T, J = ep.shape
    U1 = pp.shape[1]
    V = w.shape[0]
    dev = ep.device
    amp = os.environ.get("WR_AMP_BACKWARD", "library")
    # (the probe behind _mm_takes_out_dtype launches a GEMM the first time: not asked where the answer cannot matter)
    mm = gout.dtype != torch.float32 and amp != "kernels" and _mm_takes_out_dtype()
    route = backward_route(terms, gout.dtype, V, J, amp, mm)
    # AMP step: the loss hands back a 16-bit gradient for 16-bit logits; where the route takes it as it is (bf16 values are
    # their own hi parts) there is no widening pass over the logits-sized tensor, half the gradient bytes in dZ and dW
    gout = gout.to(route.grad_dtype).contiguous()
    if route.library:
        return _amp_backward_library(_lib.load(), gout, ep, pp, w, llens, tlens, need_w, need_b, gout_zero_in_padding, act)

    def extra(name):
        """The arguments only some entry points take: the f16 ones the gradient's dtype code, the split ones `terms`."""
        return (_lib.dtype_code(gout.dtype),) if name.endswith("_f16") else (), (route.terms,) if "_split" in name else ()

    dz = dz_out if dz_out is not None else torch.empty(B, T, U1, J, dtype=torch.float32, device=dev)
    h = (h_out if h_out is not None else torch.empty_like(dz)) if need_w else None
    code, tm = extra(route.dz)
    ws = ()
    if route.dz != "wr_joint_bwd_dz":
        ws = _lib.workspace("wr_joint_dz_split_workspace_bytes", J, V, device=dev)
        ws = (ws, ws.numel())
    _lib.call(route.dz, gout, *code, ep, pp, w, llens, tlens, B, T, U1, J, V, act, *tm, dz, h, *ws, device=dev)
    d_ep = dz.sum(dim=2)
    d_pp = dz.sum(dim=1)
    d_w = d_b = None
    if gout_zero_in_padding:
        llens = tlens = None
    if need_w:
        d_w = torch.empty(V, J, dtype=torch.float32, device=dev)
        d_b = torch.empty(V, dtype=torch.float32, device=dev)
        code, tm = extra(route.dw)
        if route.dw == "wr_joint_bwd_dw":
            ws = _lib.workspace("wr_joint_dw_workspace_bytes", J, V, device=dev)
        else:
            ws = _lib.workspace("wr_joint_dw_split_workspace_bytes", B, T, U1, J, V, device=dev)
        _lib.call(route.dw, gout, *code, h, llens, tlens, B, T, U1, J, V, *tm, d_w, d_b, ws, ws.numel(), device=dev)
    elif need_b:
        g2 = gout.float().view(-1, V)
        if llens is not None:
            g2 = torch.where(_valid_cells(llens, tlens, T, U1).view(-1, 1), g2, torch.zeros((), device=dev))
        d_b = g2.sum(0)
    if not need_b:
        d_b = None
    return d_ep, d_pp, d_w, d_b


def joint_logits(ep: torch.Tensor, pp: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor,
                 logit_lengths: Optional[torch.Tensor] = None,
                 target_lengths: Optional[torch.Tensor] = None, precision: Optional[str] = None,
                 activation: str = "tanh") -> torch.Tensor:
    """ffn_out(act(ep[:, :, None] + pp[:, None])) -> (B, T, U1, V); `activation` one of _lib.ACTIVATIONS (default tanh).  With lengths, cells in the
    padded region are left unwritten (they are never read by the RNN-T loss).  ``precision``: see the
    module docstring ("fp32" exact, "bf16x3" split, "bf16" / "f16" AMP, "autocast" resolved per call)."""
    precision = _call_precision(precision)
    terms = _PRECISIONS[precision]
    out_dtype = torch.float32
    if precision in ("bf16", "f16") and torch.is_autocast_enabled("cuda"):
        out_dtype = torch.get_autocast_dtype("cuda")
    if (logit_lengths is None) != (target_lengths is None):
        raise RuntimeError("joint_logits: pass both length tensors or neither")
    if logit_lengths is not None:
        logit_lengths = logit_lengths.to(device=ep.device, dtype=torch.int32).contiguous()
        target_lengths = target_lengths.to(device=ep.device, dtype=torch.int32).contiguous()
    return _JointFn.apply(ep, pp, w_out, b_out, logit_lengths, target_lengths, terms, out_dtype, activation_code(activation))


class TransducerJoint(nn.Module):
    """wenet/transducer/joint.py:9-70."""

    def __init__(self, voca_size: int, enc_output_size: int, pred_output_size: int, join_dim: int,
                 prejoin_linear: bool = True, postjoin_linear: bool = False, joint_mode: str = "add",
                 activation: str = "tanh", precision: Optional[str] = None):
        assert joint_mode in ["add"]
        super().__init__()
        self.activation = activation
        self.act_code = activation_code(activation)      # KeyError for an unknown name, as get_activation's lookup
        self.activatoin = _TORCH_ACTIVATIONS[activation]()   # the reference's attribute (sic); used by the export body only
        self.precision = precision                 # None: WR_JOINT_PRECISION or exact fp32
        self.prejoin_linear = prejoin_linear
        self.postjoin_linear = postjoin_linear
        self.joint_mode = joint_mode
        if not self.prejoin_linear and not self.postjoin_linear:
            assert enc_output_size == pred_output_size == join_dim
        self.enc_ffn: Optional[nn.Linear] = None
        self.pred_ffn: Optional[nn.Linear] = None
        if self.prejoin_linear:
            self.enc_ffn = nn.Linear(enc_output_size, join_dim)
            self.pred_ffn = nn.Linear(pred_output_size, join_dim)
        self.post_ffn: Optional[nn.Linear] = None
        if self.postjoin_linear:
            self.post_ffn = nn.Linear(enc_output_size, join_dim)          # joint.py:39-41 (applied to a join_dim tensor)
        self.ffn_out = nn.Linear(join_dim, voca_size)

    def pre_activation(self, enc_out: torch.Tensor, pred_out: torch.Tensor):
        """The two addends whose broadcast sum enters the activation: (B, T, J), (B, U, J).
        prejoin_linear (joint.py:55-58): enc_ffn / pred_ffn.  postjoin_linear (:66-67) applies a Linear to the 4-D sum
        enc[:, :, None] + pred[:, None]; a Linear distributes over the sum, post(e + p) = (W e + b) + W p, so it is
        applied to the two small addends instead of the (B, T, U, J) tensor (same value up to fp32 rounding of one
        addition per element; the 4-D tensor is never formed)."""
        if self.prejoin_linear and self.enc_ffn is not None and self.pred_ffn is not None:
            enc_out = self.enc_ffn(enc_out)
            pred_out = self.pred_ffn(pred_out)
        if self.postjoin_linear and self.post_ffn is not None:
            enc_out = self.post_ffn(enc_out)
            pred_out = torch.nn.functional.linear(pred_out, self.post_ffn.weight)
        return enc_out, pred_out

    def _export_forward(self, enc_out: torch.Tensor, pred_out: torch.Tensor) -> torch.Tensor:
        """TorchScript-export body of the joiner for the step export `forward_joint_step` (transducer.py:619-622):
        a scripted artefact cannot reach the ctypes library, so it carries the reference's module graph
        (joint.py:55-69).  Never executed in eager mode -- `forward` below is the only eager entry."""
        enc = enc_out
        pred = pred_out
        if self.enc_ffn is not None and self.pred_ffn is not None:
            enc = self.enc_ffn(enc_out)
            pred = self.pred_ffn(pred_out)
        out = enc.unsqueeze(2) + pred.unsqueeze(1)
        if self.post_ffn is not None:
            out = self.post_ffn(out)
        return self.ffn_out(self.activatoin(out))

    @torch.jit.unused      # backed by a ctypes autograd Function: opaque to TorchScript (train.py:203-205 smoke export)
    def forward(self, enc_out: torch.Tensor, pred_out: torch.Tensor,
                logit_lengths: Optional[torch.Tensor] = None,
                target_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        """enc_out (B, T, E), pred_out (B, U, P) -> (B, T, U, V).  The optional lengths are an
        extension (skip cells the loss never reads); the reference call passes none."""
        enc_out, pred_out = self.pre_activation(enc_out, pred_out)
        return joint_logits(enc_out, pred_out, self.ffn_out.weight, self.ffn_out.bias, logit_lengths, target_lengths,
                            self.precision, self.activation)

    @torch.jit.unused      # reaches the ctypes library through do_rnnt_pruning
    def forward_pruned(self, enc_out: torch.Tensor, pred_out: torch.Tensor, ranges: torch.Tensor) -> torch.Tensor:
        """The joiner on a band of label positions: enc_out (B, T, E), pred_out (B, U+1, P), ranges (B, T, R) as
        `get_rnnt_prune_ranges` returns them -> logits (B, T, R, V) for `rnnt_loss_pruned`, ``logits[b,t,r]`` the
        joiner's output at the cell ``(t, ranges[b,t,r])``.  `pre_activation`, the gather of both addends onto the band
        (`do_rnnt_pruning`), the module's activation on their sum and `ffn_out` (a plain (B*T*R, J) x (J, V) product)."""
        from .rnnt_pruned import do_rnnt_pruning
        ep, pp = self.pre_activation(enc_out, pred_out)
        if ep.dtype != pp.dtype:
            pp = pp.to(ep.dtype)
        am_p, lm_p = do_rnnt_pruning(ep, pp, ranges)
        return self.ffn_out(self.activatoin(am_p + lm_p))
