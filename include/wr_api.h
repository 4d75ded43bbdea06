/*
 * wr_api.h -- C ABI of libwr_mi355x.so: the MI355X (gfx950) implementation of
 * WeNet's CTC / RNN-T loss and transducer-decode hot path.
 *
 * This is the drop-in boundary.  The reference has no
 * native interface on this path: its seams are Python call sites into
 * third-party libraries.  Each entry point below names the reference call site
 * it replaces; INTEGRATION.md shows the ctypes binding a maintainer would add
 * on the reference side.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / C++ types.
 *  - Every pointer named *_d is DEVICE memory owned by the caller (PyTorch's
 *    allocator in practice).  The library never allocates or frees device
 *    memory and never synchronises the device: all work is enqueued on the
 *    caller's stream (`stream` is a hipStream_t passed as void*; NULL = the
 *    default stream).  Entry points are re-entrant; there is no global mutable
 *    state besides a thread-local error string.
 *  - Return value: 0 on success, a negative WR_E* code otherwise;
 *    wr_last_error() returns a human-readable message for the calling thread.
 *    Non-finite losses are values, not errors (the reference skips such steps
 *    upstream: wenet/utils/executor.py:124-125,171).
 *  - dtype codes: WR_F32 (the parity bar), WR_F16, WR_BF16 (AMP; accumulate in
 *    fp32, gradients returned in the input dtype).
 */
#ifndef WR_API_H_
#define WR_API_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an existing signature or struct layout changes (callers built against another version must not
 * bind): 1 = round 1; 2 = round 2 (an `activation` argument inside wr_joint_fwd / wr_joint_bwd_dz / *_split,
 * wr_transducer_weights grew the predictor-variant fields); 3 = this header. */
#define WR_API_VERSION 3

enum wr_dtype { WR_F32 = 0, WR_F16 = 1, WR_BF16 = 2 };

/* lattice types of the k2 RNN-T losses ("Lattice types and the delay penalty" below) */
enum wr_lattice { WR_LATTICE_REGULAR = 0, WR_LATTICE_MODIFIED = 1 };
/* joiner activation (TransducerJoint(activation=...), wenet/transducer/joint.py:25 -> wenet/utils/common.py:228-242);
 * "tanh" is the shipped configuration, "swish" is torch.nn.SiLU, "gelu" the erf form (torch.nn.GELU default) */
enum wr_activation { WR_ACT_TANH = 0, WR_ACT_RELU = 1, WR_ACT_HARDTANH = 2, WR_ACT_SELU = 3, WR_ACT_SWISH = 4, WR_ACT_GELU = 5 };

enum wr_status {
    WR_OK = 0,
    WR_EINVAL = -1,      /* bad argument (null pointer, non-positive size, blank out of range ...) */
    WR_EUNSUPPORTED = -2,/* shape outside what the kernels cover (message says which limit) */
    WR_EWORKSPACE = -3,  /* workspace too small */
    WR_ELAUNCH = -4      /* HIP reported a launch error */
};

int wr_api_version(void);
const char *wr_last_error(void);

/* Benchmarking hook: process-wide launch-shape knobs of the streaming kernels.  Results never depend
 * on them; the defaults are the measured best.  key 0: workgroups per CU of the RNN-T row-lse pass,
 * key 1: of the RNN-T gradient pass (0, the default: automatic -- one row per wave in the row-lse pass, about 104 KB of
 * logits per wave in the gradient pass; n > 0: a persistent grid of n workgroups per CU as in round 1), key 2: non-temporal bits (1: gradient-pass loads, 2: gradient-pass
 * stores, 4: row-lse loads; default 7), key 3 / key 4: 16-byte vectors in flight per lane in the gradient (4, 8 or 16;
 * default 16) / row-lse pass (4, 8 or 16; default 16),
 * key 5: exact-fp32 joiner forward (default: fragment-layout operands; 1: the first forward kernel, bit-identical), key 6: decoder GEMM lane
 * tile (0: by occupancy, 1: 32 lanes, 2: 64 lanes; for GEMMs of more than 256 tiles 3: 4-wave workgroups, 4: one wave
 * per tile instead of 128-lane workgroups -- every form gives bit-identical results), key 7: column parts of the split
 * joiner forward (0: automatic),
 * key 8: retired (the 64-cell split dZ tiling was removed), key 9 / key 10: exact dW / dZ tiling (0: 256 x 256 blocks,
 * 1: the first tilings of joint.hip), key 11: greedy / beam micro-step with an LSTM predictor (0: projection folded
 * into pred_ffn -- one launch less, the default; 1: two launches), key 12: single-term (AMP) split joiner forward
 * (0: 64 lattice cells per workgroup, two workgroups per CU, the default; 1: 64 cells, one workgroup per CU; 2: 128
 * cells -- measured slower), key 13: its logit stores (0: cell-major tiles through a per-wave LDS stage as whole lines, the
 * default; 1: transposed tiles stored from registers in 8/16-byte pieces -- measured slower).  Keys 6-13 pick between kernels that compute the
 * same sums; the two dZ tilings are bit-identical, the dW tilings differ in the order of fp32 additions, the folded
 * projection in the rounding of one composed weight matrix (formed in float64).  key 14: dead-cell skip of the RNN-T
 * gradient pass (1, the default: a cell whose every exponential is provably +0 -- its log-occupancy and the bounds of
 * its blank and label terms below -110 nats, a finite row log-sum-exp -- is written as grad_costs[b] * 0 without
 * reading its logits; 0: every valid cell reads its logits) -- bit-identical results either way.  key 15 / key 16: which
 * rows a workgroup of the RNN-T row-lse / gradient pass visits (2, the default: XCD runs -- of every 8c consecutive
 * 4-row blocks, the workgroups that land on XCD x take the c blocks from x*c on, so each XCD streams contiguous rows;
 * 0 or any other value: block i is workgroup i, the order before), key 17: that c (0, the default: 8 * U1max) --
 * bit-identical results either way; measurements in profiles/xcd_row_order.md. */
int wr_tune_set(int key, int value);

/* ------------------------------------------------------------------------
 * RNN-T loss + gradient w.r.t. the joiner logits (log-softmax fused).
 * Replaces torchaudio.functional.rnnt_loss(logits, targets, logit_lengths,
 * target_lengths, blank, clamp, reduction) as called at
 *   wenet/transducer/transducer.py:142-147  (training, reduction="mean")
 *   wenet/transducer/transducer.py:296-301  (rescoring, reduction='none').
 *
 * Shapes (as torchaudio): logits [B, Tmax, U1max, V] contiguous,
 * targets [B, U1max-1] int32, logit_lengths [B] int32, target_lengths [B] int32.
 * U1max = max target length + 1.
 *
 * The op is split where autograd splits it, so that the logits-sized tensor is
 * touched the algorithmic minimum of three times (read, read, write):
 *   wr_rnnt_loss_fwd : pass 1 (row log-sum-exp, blank/label log-probs) +
 *                      alpha/beta lattice sweeps -> costs[B]; lattice state is
 *                      kept in the caller's workspace.
 *   wr_rnnt_loss_bwd : pass 3, grads = grad_costs[b] * d cost_b / d logits,
 *                      zero outside [0,T_b) x [0,U_b].  `grads_d` may alias
 *                      `logits_d` (in-place).  grad_costs_d may be NULL (= 1).
 * Reduction ("mean" = mean over batch, not length-normalised) is the caller's:
 * it is a B-element operation folded into grad_costs.
 * ---------------------------------------------------------------------- */
size_t wr_rnnt_workspace_bytes(int B, int Tmax, int U1max);

int wr_rnnt_loss_fwd(const void *logits_d, int dtype,
                     const int32_t *targets_d, const int32_t *logit_lengths_d,
                     const int32_t *target_lengths_d,
                     int B, int Tmax, int U1max, int V, int blank,
                     float *costs_d /* [B] out */,
                     void *workspace_d, size_t workspace_bytes, void *stream);

int wr_rnnt_loss_bwd(const void *logits_d, int dtype,
                     const int32_t *targets_d, const int32_t *logit_lengths_d,
                     const int32_t *target_lengths_d,
                     int B, int Tmax, int U1max, int V, int blank, float clamp,
                     const float *grad_costs_d /* [B] or NULL */,
                     void *grads_d /* same shape/dtype as logits; may alias */,
                     const void *workspace_d, size_t workspace_bytes, void *stream);

/* The lattice sweeps alone, for a workspace whose row statistics (denom and the skip / emit log-probabilities) were
 * already produced by the joiner's fused epilogue (wr_joint_fwd_lse / wr_joint_fwd_split_lse below): pass 1 -- one
 * full read of the logits -- is skipped.  The epilogue sums exponentials against the first logit a lane sees instead
 * of a running maximum; if a row spreads over more than 88 nats that sum overflows, the epilogue raises a flag in
 * the workspace and this entry point runs the stand-alone pass 1 over `logits_d` (fp32, as written by the joiner)
 * before the sweeps -- otherwise that kernel returns at once.  costs as wr_rnnt_loss_fwd; wr_rnnt_loss_bwd follows
 * unchanged. */
int wr_rnnt_loss_fwd_from_lse(const float *logits_d, const int32_t *targets_d,
                              const int32_t *logit_lengths_d, const int32_t *target_lengths_d,
                              int B, int Tmax, int U1max, int V, int blank, float *costs_d /* [B] out */,
                              void *workspace_d, size_t workspace_bytes, void *stream);

/* The lattice sweeps alone, with no logits at all: for a workspace whose row statistics were written by
 * wr_joint_rnnt_stats (below), which repairs an overflowed row itself -- there is no pass-1 fallback here.  costs as
 * wr_rnnt_loss_fwd. */
int wr_rnnt_loss_sweeps(const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                        float *costs_d /* [B] out */, void *workspace_d, size_t workspace_bytes, void *stream);

/* Diagnostic view of the lattice state left in the workspace by wr_rnnt_loss_fwd
 * (tests compare alpha/beta with the oracle): copies alpha and beta into plain
 * [B, Tmax, U1max] float arrays (entries outside the valid region are 0). */
int wr_rnnt_export_lattice(const void *workspace_d, size_t workspace_bytes,
                           const int32_t *logit_lengths_d, const int32_t *target_lengths_d,
                           int B, int Tmax, int U1max,
                           float *alpha_d, float *beta_d, void *stream);

/* ------------------------------------------------------------------------
 * CTC loss + gradient with the log-softmax fused in.
 * Replaces  ys_hat = ys_hat.log_softmax(2); loss = nn.CTCLoss(...)(ys_hat, ys_pad, hlens, ys_lens)
 * at wenet/transformer/ctc.py:60-61 (blank = 0, zero_infinity = False).
 *
 * logits [B, Tmax, V] contiguous = the PRE-softmax output of ctc_lo, batch-major
 * (no transpose needed); targets [B, Smax] int32, entries beyond
 * target_lengths[b] are never read; lengths [B] int32.  nll[b] = -log p(y_b | x_b)
 * per utterance (infeasible alignment -> +inf, a value, not an error);
 * reduction ('sum' then /B in the reference, ctc.py:61-63) is the caller's and
 * is folded into grad_nll.  grads = grad_nll[b] * d nll_b / d logits, zero for
 * t >= input_lengths[b]; grads_d may alias logits_d.  Limits: Smax <= 511,
 * V <= 16384.
 * ---------------------------------------------------------------------- */
size_t wr_ctc_workspace_bytes(int B, int Tmax, int Smax);

int wr_ctc_loss_fwd(const void *logits_d, int dtype,
                    const int32_t *targets_d, const int32_t *input_lengths_d,
                    const int32_t *target_lengths_d,
                    int B, int Tmax, int Smax, int V, int blank,
                    float *nll_d /* [B] out */,
                    void *workspace_d, size_t workspace_bytes, void *stream);

int wr_ctc_loss_bwd(const void *logits_d, int dtype,
                    const int32_t *targets_d, const int32_t *input_lengths_d,
                    const int32_t *target_lengths_d,
                    int B, int Tmax, int Smax, int V, int blank,
                    const float *grad_nll_d /* [B] or NULL */,
                    void *grads_d,
                    const void *workspace_d, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Transducer joint network (the one dense contraction on the path).
 * Replaces TransducerJoint.forward, wenet/transducer/joint.py:45-70, from the
 * point where the two pre-join projections exist:
 *   ep = enc_ffn(enc) [B, T, J],  pp = pred_ffn(pred) [B, U1, J]   (joint.py:55-58)
 *   out[b,t,u,:] = ffn_out(act(ep[b,t,:] + pp[b,u,:]))              (joint.py:60-69)
 * `activation` is a wr_activation code (tanh in the shipped configuration; the text below writes tanh for it).
 * w_out [V, J] and b_out [V] are ffn_out.weight / .bias in nn.Linear layout.
 * fp32 throughout (exact-fp32 MFMA).  J a multiple of 4, at most 512.
 * The activation tensor tanh(ep+pp) [B,T,U1,J] is never written to HBM in the
 * forward pass.  If both length arrays are given, 64-cell tiles that lie wholly
 * in the padded region (t >= T_b or u > U_b) are skipped and `out` is left
 * untouched there -- the RNN-T loss never reads those cells.
 *
 * wr_joint_bwd_dz: dz[b,t,u,:] = (gout[b,t,u,:] @ w_out) * (1 - tanh(ep+pp)^2),
 * zero in padded cells when lengths are given; h_d (optional, [B,T,U1,J])
 * receives tanh(ep+pp) for the weight gradient (wr_joint_bwd_dw).  d ep = sum_u dz
 * and d pp = sum_t dz are plain library reductions on the host side.
 * ---------------------------------------------------------------------- */
size_t wr_joint_workspace_bytes(int J, int V);

int wr_joint_fwd(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                 const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                 int B, int T, int U1, int J, int V, int activation,
                 float *out_d /* [B,T,U1,V] */,
                 void *workspace_d, size_t workspace_bytes, void *stream);

/* wr_joint_fwd with pass 1 of the RNN-T loss fused into its epilogue (transducer.py:132 + the first pass of :142-147):
 * a forward workgroup owns every column of its 64 lattice cells, so while the logits leave for HBM it also writes
 * denom(t,u) = logsumexp_v and the blank / label log-probabilities of every valid cell into the RNN-T workspace
 * (wr_rnnt_workspace_bytes(B, T, U1)); wr_rnnt_loss_fwd_from_lse then only runs the lattice sweeps.  Both length
 * arrays are required; targets [B, U1-1] as for wr_rnnt_loss_fwd. */
int wr_joint_fwd_lse(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                     const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d,
                     int B, int T, int U1, int J, int V, int activation, int blank,
                     float *out_d /* [B,T,U1,V] */,
                     void *workspace_d, size_t workspace_bytes,
                     void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

/* Joiner + RNN-T loss without a logits tensor (the memory-bounded fused node, fused.py `logits_budget`).
 *
 * wr_joint_rnnt_stats: the joiner forward with the row statistics of wr_joint_fwd_lse as its only output -- denom and the
 * blank / label log-probabilities go into the RNN-T workspace, no logit is stored.  A row whose partial sums overflow
 * (more than 88 nats of spread) is repaired by a second launch of the same kernel with a running maximum, whose
 * workgroups leave at once unless the first launch raised the flag.  Then wr_rnnt_loss_sweeps.
 * terms: 0 = exact fp32 (workspace wr_joint_workspace_bytes), 3 = split precision (wr_joint_split_workspace_bytes).
 *
 * wr_joint_rnnt_grad: the loss gradient grad_costs[b] * d cost_b / d logits of the cells [cell_begin, cell_end) of the
 * flattened (B, T, U1) lattice into g_out [(cell_end - cell_begin), V]: every 64-cell logits tile is recomputed by the
 * same forward kernel (bit-identical to the logits the statistics were taken from) and turned into the gradient in its
 * epilogue with the formula of wr_rnnt_loss_bwd (same clamp, same zero outside [0,T_b) x [0,U_b]).  Needs the workspace
 * after wr_joint_rnnt_stats + wr_rnnt_loss_sweeps; it only reads it.  w_ready != 0: `workspace_d` already holds the
 * re-laid W of an earlier wr_joint_rnnt_grad call with the same W, terms and kernel selection (the slices of one backward
 * share it); 0 = lay it out first.  Other arguments as wr_joint_rnnt_stats. */
int wr_joint_rnnt_stats(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                        const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d,
                        int B, int T, int U1, int J, int V, int activation, int blank, int terms,
                        void *workspace_d, size_t workspace_bytes,
                        void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

int wr_joint_rnnt_grad(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                       const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d,
                       int B, int T, int U1, int J, int V, int activation, int blank, float clamp, int terms,
                       const float *grad_costs_d /* [B] or NULL */,
                       const void *rnnt_workspace_d, size_t rnnt_workspace_bytes,
                       long long cell_begin, long long cell_end, float *g_out_d /* [cell_end - cell_begin, V] */,
                       void *workspace_d, size_t workspace_bytes, int w_ready, void *stream);

int wr_joint_bwd_dz(const float *gout_d /* [B,T,U1,V] */, const float *ep_d, const float *pp_d,
                    const float *w_out_d,
                    const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                    int B, int T, int U1, int J, int V, int activation,
                    float *dz_d /* [B,T,U1,J] */, float *h_d /* [B,T,U1,J] or NULL */, void *stream);

/* Split-precision joiner on the bf16 matrix cores (opt-in; the exact-fp32 entry points above stay the default).
 * Same operator and arguments as wr_joint_fwd; every fp32 operand is split into bf16 hi + lo parts and
 *   terms = 3:  a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, fp32 accumulation -- logits within 1e-4 (relative to
 *               their scale) of the fp32 result, at several times the rate of the exact-fp32 MFMA;
 *   terms = 1:  a_hi*b_hi only: the AMP path (the reference under --use_amp, executor.py:91, runs ffn_out in
 *               fp16 with fp32 accumulation).
 * out_d has out_dtype (WR_F32 / WR_F16 / WR_BF16).  J a multiple of 4, at most 512 (as the exact entry points). */
size_t wr_joint_split_workspace_bytes(int J, int V);

int wr_joint_fwd_split(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                       const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                       int B, int T, int U1, int J, int V, int activation, int terms,
                       void *out_d /* [B,T,U1,V] */, int out_dtype,
                       void *workspace_d, size_t workspace_bytes, void *stream);

/* The single-term mode on the f16 matrix cores (v_mfma_f32_32x32x16_f16): ep + pp, the activation and w_out rounded to
 * float16 (nearest even; subnormals kept, beyond +-65504 -> +-inf as torch's .half()), fp32 accumulation -- the
 * operand format of the reference's ffn_out under fp16 autocast (executor.py:91, --use_amp with the default dtype).
 * Arguments, out_dtype and workspace (wr_joint_split_workspace_bytes) as wr_joint_fwd_split with terms = 1. */
int wr_joint_fwd_f16(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                     const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                     int B, int T, int U1, int J, int V, int activation,
                     void *out_d /* [B,T,U1,V] */, int out_dtype,
                     void *workspace_d, size_t workspace_bytes, void *stream);

/* wr_joint_fwd_split with the RNN-T loss's row statistics fused into the epilogue (see wr_joint_fwd_lse); fp32 logits. */
int wr_joint_fwd_split_lse(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                           const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d,
                           int B, int T, int U1, int J, int V, int activation, int blank, int terms,
                           float *out_d /* [B,T,U1,V] */,
                           void *workspace_d, size_t workspace_bytes,
                           void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

/* wr_joint_bwd_dz on the bf16 matrix cores, same split as wr_joint_fwd_split (terms = 3: gout and w_out split into
 * bf16 hi + lo, three MFMA terms, fp32 accumulation; terms = 1: single bf16 product).  Same outputs as
 * wr_joint_bwd_dz (H = tanh(ep+pp) recomputed with the exact tanhf).  V a multiple of 4, at least 32. */
size_t wr_joint_dz_split_workspace_bytes(int J, int V);

int wr_joint_bwd_dz_split(const float *gout_d /* [B,T,U1,V] */, const float *ep_d, const float *pp_d,
                          const float *w_out_d,
                          const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                          int B, int T, int U1, int J, int V, int activation, int terms,
                          float *dz_d /* [B,T,U1,J] */, float *h_d /* [B,T,U1,J] or NULL */,
                          void *workspace_d, size_t workspace_bytes, void *stream);

/* The same with the logits gradient in bf16 -- what the loss hands back for the 16-bit logits of the AMP step
 * (reference: executor.py:91 autocast; torch casts the Linear's incoming gradient the same way).  bf16 values are their
 * own hi parts: no conversion pass, half the gradient bytes, results identical to wr_joint_bwd_dz_split on the same
 * values widened to fp32.  V a multiple of 8, at least 32. */
int wr_joint_bwd_dz_split_bf16(const void *gout_bf16_d /* [B,T,U1,V] bf16 */, const float *ep_d, const float *pp_d,
                               const float *w_out_d,
                               const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                               int B, int T, int U1, int J, int V, int activation, int terms,
                               float *dz_d /* [B,T,U1,J] */, float *h_d /* [B,T,U1,J] or NULL */,
                               void *workspace_d, size_t workspace_bytes, void *stream);

/* wr_joint_bwd_dz_split (terms = 1) on the f16 matrix cores: dY and W rounded to float16, fp32 accumulation.  gout_dtype
 * WR_F32 (rounded to f16 in the kernel; V a multiple of 4) or WR_F16 (taken as it is; V a multiple of 8); V at least 32.
 * Workspace: wr_joint_dz_split_workspace_bytes. */
int wr_joint_bwd_dz_f16(const void *gout_d /* [B,T,U1,V] */, int gout_dtype, const float *ep_d, const float *pp_d,
                        const float *w_out_d,
                        const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                        int B, int T, int U1, int J, int V, int activation,
                        float *dz_d /* [B,T,U1,J] */, float *h_d /* [B,T,U1,J] or NULL */,
                        void *workspace_d, size_t workspace_bytes, void *stream);

/* Second half of the activation gradient for callers that form dH = gout . W themselves (the AMP step hands that plain
 * bf16 contraction to the vendor GEMM library): dz[cell, j] = dH[cell, j] * act'(ep + pp) in place (zero in padded cells
 * when lengths are given) and, unless h_d is NULL, h[cell, 0..J) = act(ep + pp) (zero in padded cells) as fp32, fp16 or bf16
 * with row stride h_ld >= J (a multiple of 4).  When h_ld > J, column J of a row is 1 in valid cells and 0 in padded
 * ones and columns J+1 .. h_ld-1 are 0: gout^T h then carries the bias gradient in column J.  J a multiple of 4. */
int wr_joint_dz_act(float *dz_d /* [B,T,U1,J] in: dH, out: dZ */, const float *ep_d, const float *pp_d,
                    const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                    int B, int T, int U1, int J, int activation,
                    void *h_d /* [B,T,U1,h_ld] or NULL */, int h_dtype /* WR_F32 | WR_F16 | WR_BF16 */, int h_ld, void *stream);

/* Bias gradient from a bf16 logits gradient: db[v] = sum over lattice cells of gout[cell, v], padded cells excluded when
 * lengths are given (the AMP step, whose weight gradient is a vendor-library GEMM).  V a multiple of 8.  Deterministic. */
size_t wr_joint_db_workspace_bytes(int B, int T, int U1, int V);

int wr_joint_db_bf16(const void *gout_bf16_d /* [B,T,U1,V] bf16 */,
                     const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                     int B, int T, int U1, int V, float *db_d /* [V] */,
                     void *workspace_d, size_t workspace_bytes, void *stream);

/* The same for a float16 gradient (torch.cuda.amp.autocast's default dtype, the reference's --use_amp). */
int wr_joint_db_f16(const void *gout_f16_d /* [B,T,U1,V] fp16 */,
                    const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                    int B, int T, int U1, int V, float *db_d /* [V] */,
                    void *workspace_d, size_t workspace_bytes, void *stream);

/* Weight gradient of ffn_out:  dw[v, :] = sum over lattice cells of gout[cell, v] * h[cell, :],
 * db[v] = sum of gout[cell, v]  (h = tanh(ep+pp) as written by wr_joint_bwd_dz).  With lengths, cells in the
 * padded region do not contribute.  db_d may be NULL.  Deterministic (partial slabs + ordered reduction). */
size_t wr_joint_dw_workspace_bytes(int J, int V);

int wr_joint_bwd_dw(const float *gout_d /* [B,T,U1,V] */, const float *h_d /* [B,T,U1,J] */,
                    const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                    int B, int T, int U1, int J, int V,
                    float *dw_d /* [V,J] */, float *db_d /* [V] or NULL */,
                    void *workspace_d, size_t workspace_bytes, void *stream);

/* wr_joint_bwd_dw on the bf16 matrix cores (terms as in wr_joint_fwd_split): dw = gout^T h, db = column sums of gout
 * (kept in fp32), padded cells excluded when lengths are given.  V and J multiples of 4.  Deterministic. */
size_t wr_joint_dw_split_workspace_bytes(int B, int T, int U1, int J, int V);

int wr_joint_bwd_dw_split(const float *gout_d /* [B,T,U1,V] */, const float *h_d /* [B,T,U1,J] */,
                          const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                          int B, int T, int U1, int J, int V, int terms,
                          float *dw_d /* [V,J] */, float *db_d /* [V] or NULL */,
                          void *workspace_d, size_t workspace_bytes, void *stream);

/* The same with the logits gradient in bf16 (see wr_joint_bwd_dz_split_bf16); workspace as wr_joint_bwd_dw_split. */
int wr_joint_bwd_dw_split_bf16(const void *gout_bf16_d /* [B,T,U1,V] bf16 */, const float *h_d /* [B,T,U1,J] */,
                               const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                               int B, int T, int U1, int J, int V, int terms,
                               float *dw_d /* [V,J] */, float *db_d /* [V] or NULL */,
                               void *workspace_d, size_t workspace_bytes, void *stream);

/* wr_joint_bwd_dw_split (terms = 1) on the f16 matrix cores: dY and h rounded to float16, fp32 accumulation; db summed in
 * fp32 from the gradient as given.  gout_dtype WR_F32 or WR_F16; V and J multiples of 4.  Workspace:
 * wr_joint_dw_split_workspace_bytes. */
int wr_joint_bwd_dw_f16(const void *gout_d /* [B,T,U1,V] */, int gout_dtype, const float *h_d /* [B,T,U1,J] */,
                        const int32_t *logit_lengths_d /* nullable */, const int32_t *target_lengths_d /* nullable */,
                        int B, int T, int U1, int J, int V,
                        float *dw_d /* [V,J] */, float *db_d /* [V] or NULL */,
                        void *workspace_d, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Transducer decoding: batched greedy search, batched prefix beam search and
 * the predictor step API, with every per-step operation on the device.
 *
 * Replaces
 *   greedy  wenet/transducer/search/greedy_search copy.py:6-63 -- the upstream core loop behind
 *           Transducer.greedy_search (wenet/transducer/transducer.py:515-598)
 *   beam    PrefixBeamSearch.prefix_beam_search, wenet/transducer/search/prefix_beam_search.py:42-148
 *           (called from Transducer.beam_search, transducer.py:332-377)
 *   step    RNNPredictor.forward_step, wenet/transducer/predictor.py:160-200 (EmbeddingPredictor.forward_step
 *           :325-372 and ConvPredictor.forward_step :455-481 with predictor_type 1 / 2), and the joiner for
 *           step shapes (joint.py:45-70), i.e. forward_predictor_step / forward_joint_step
 *           (transducer.py:613-629)
 *
 * Weights are passed in the reference modules' own (nn.Linear / nn.LSTM / nn.Embedding) layouts;
 * wr_decoder_create re-lays them out k-major once into the caller's workspace.
 * The decoder handle owns no device memory; it holds the launch configuration, the captured
 * hipGraphs of the micro-steps and an internal work stream that is ordered against the caller's
 * stream with events (no device-wide synchronisation).  wr_greedy_search synchronises its own work
 * stream once every 16 micro-steps to test the "lanes still decoding" word (the reference
 * synchronises on every step); wr_prefix_beam_search and wr_predictor_step never do.
 * Limits: lanes <= 1024, vocabulary <= 16384, LSTM layers <= 4, beam <= 16, layer widths <= 1024.
 * ---------------------------------------------------------------------- */
#define WR_MAX_LSTM_LAYERS 4

typedef struct wr_transducer_weights {
    int32_t vocab_size;   /* V */
    int32_t enc_dim;      /* E: encoder output size */
    int32_t pred_dim;     /* P: predictor output size (RNNPredictor.projection out) */
    int32_t embed_dim;    /* D */
    int32_t hidden;       /* H: LSTM hidden size */
    int32_t n_layers;     /* L */
    int32_t join_dim;     /* J */
    int32_t activation;   /* wr_activation of the joiner (0 = tanh) */
    const float *embed;                        /* predictor.embed.weight       [V, D] ([embed_rows, D] if embed_rows > 0) */
    const float *w_ih[WR_MAX_LSTM_LAYERS];     /* predictor.rnn.weight_ih_l{k} [4H, D or H], gate order i,f,g,o */
    const float *w_hh[WR_MAX_LSTM_LAYERS];     /* predictor.rnn.weight_hh_l{k} [4H, H] */
    const float *b_ih[WR_MAX_LSTM_LAYERS];     /* predictor.rnn.bias_ih_l{k}   [4H] */
    const float *b_hh[WR_MAX_LSTM_LAYERS];     /* predictor.rnn.bias_hh_l{k}   [4H] */
    const float *proj_w, *proj_b;              /* predictor.projection         [P, H], [P] */
    const float *enc_ffn_w, *enc_ffn_b;        /* joint.enc_ffn                [J, E], [J] */
    const float *pred_ffn_w, *pred_ffn_b;      /* joint.pred_ffn               [J, P], [J] */
    const float *out_w, *out_b;                /* joint.ffn_out                [V, J], [V] */
    /* The stateless predictors of wenet/transducer/predictor.py:203-481 (not in the shipped configuration).  Their
     * state is the embeddings of the last context_size - 1 tokens; it travels through the same cache tensors as the
     * LSTM state: n_layers = context_size - 1 "layers" of width hidden = embed_dim = pred_dim (slot 0 oldest), the
     * cell-state tensors are carried and ignored.  LSTM fields above are unused (may be NULL) for types 1 and 2. */
    int32_t predictor_type;    /* 0 RNNPredictor (LSTM), 1 EmbeddingPredictor, 2 ConvPredictor */
    int32_t context_size;      /* history_size + 1: 2..5 */
    int32_t n_head;            /* type 1: heads of the positional weighting; n_head * context_size <= 64 */
    int32_t pred_activation;   /* wr_activation applied after the LayerNorm */
    float ln_eps;              /* LayerNorm epsilon */
    int32_t embed_rows;        /* rows of predictor.embed.weight when that differs from V (a predictor stepped on its own
                                * through wr_predictor_step has no joiner vocabulary); 0 = vocab_size.  The LSTM path keeps a
                                * table of W_ih(layer 0) . embed[v] with that many rows. */
    const float *pos_w;                        /* type 1: pos_embed.weight     [n_head, D * context_size] (bias unused) */
    const float *ffn_w, *ffn_b;                /* type 1: ffn                  [D, D], [D] */
    const float *norm_w, *norm_b;              /* types 1, 2: norm             [D], [D] */
    const float *conv_w, *conv_b;              /* type 2: conv.weight [D, 1, context_size], conv.bias [D] or NULL */
} wr_transducer_weights;

typedef struct wr_decoder wr_decoder;

size_t wr_decoder_workspace_bytes(const wr_transducer_weights *w, int max_lanes, int max_utt, int Tmax,
                                  int max_hyp, int max_beam);

/* max_lanes: streams decoded together (greedy) or utterances x beam (beam search);
 * max_utt: utterances per call; Tmax: encoder frames; max_hyp: greedy hypothesis capacity. */
int wr_decoder_create(const wr_transducer_weights *w, int max_lanes, int max_utt, int Tmax, int max_hyp,
                      int max_beam, void *workspace_d, size_t workspace_bytes, void *stream,
                      wr_decoder **out);
int wr_decoder_destroy(wr_decoder *h);
/* hipGraph replay of the per-step kernel sequence.  Default: on for greedy search (the host polls a "lanes still
 * active" word once per replay), off for prefix beam search (fixed frame count, plain launches measured faster).
 * enable = 0 / 1 forces both off / on. */
int wr_decoder_set_graph(wr_decoder *h, int enable);
/* Greedy look-ahead: evaluate the joiner for `frames` (1..4) consecutive encoder frames of every stream per
 * micro-step.  A stream's predictor output only changes after a non-blank, so a run of blanks is consumed in one
 * micro-step instead of `frames`; decisions are walked in frame order through the same state machine and stop at
 * the first emission, so the token sequences are those of the one-frame loop (frames = 1).
 * frames = 0 (the default): chosen before every graph replay from the share of blank decisions in the previous one
 * (>= 75 % blank: 4 frames, >= 62 %: 2, else 1; never more than 256 joiner rows per micro-step). */
int wr_decoder_set_lookahead(wr_decoder *h, int frames);

/* enc_out [N, T, E] fp32, enc_lens [N]; hyps [N, max_hyp] / hyp_lens [N] out (tokens beyond
 * max_hyp are counted in hyp_lens but not stored).  Each lane follows the reference loop exactly:
 * predictor stepped only after a non-blank, at most n_steps emissions per frame. */
int wr_greedy_search(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, int N, int T,
                     int n_steps, int blank, int32_t *hyps_d, int32_t *hyp_lens_d, void *stream);

/* Streaming (chunk-synchronous) greedy search: the stateful reset_cache() / forward_greedy_search(chunk)
 * pair that the reference's C++ runtime drives ("wenet/transducer/transducer ref.py":541-606, consumed at
 * runtime/core/decoder/torch_asr_model.cc:126,313).  reset != 0 starts N fresh streams; otherwise the
 * predictor cache, last token, "predictor must step" flag, per-frame emission counter and predictor
 * output of every stream carry over from the previous call.  hyps/hyp_lens receive the tokens emitted in
 * THIS chunk.  reference_new_cache != 0 reproduces the reference's `new_cache = self.cache` at the top of
 * each chunk (the not-yet-committed predictor state of the previous chunk is dropped); 0 keeps it, which
 * makes chunked decoding identical to decoding the concatenated frames with wr_greedy_search. */
int wr_greedy_search_chunk(wr_decoder *h, const float *enc_chunk_d, const int32_t *chunk_lens_d, int N, int T,
                           int n_steps, int blank, int reset, int reference_new_cache, int32_t *hyps_d,
                           int32_t *hyp_lens_d, void *stream);

/* enc_out [B, T, E], ctc_logp [B, T, V] = log_softmax(ctc_lo(enc_out)) (ctc.py:66-75).
 * Out: hyps [B, beam, Tmax+1] (each begins with the seed blank, padded with -1), hyp_lens [B, beam],
 * scores [B, beam] float64 (best first), n_hyps [B]. */
int wr_prefix_beam_search(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d,
                          const float *ctc_logp_d, int B, int T, int beam, float ctc_weight,
                          float transducer_weight, int blank, int32_t *hyps_d, int32_t *hyp_lens_d,
                          double *scores_d, int32_t *n_hyps_d, void *stream);

/* One predictor step for N lanes: tokens [N], cache_h / cache_c [L, N, H] in;
 * out [N, P], new_h / new_c [L, N, H] out (padding is applied by the caller, predictor.py:9-15). */
int wr_predictor_step(wr_decoder *h, const int32_t *tokens_d, const float *cache_h_d,
                      const float *cache_c_d, int N, float *out_d, float *new_h_d, float *new_c_d,
                      void *stream);

/* ------------------------------------------------------------------------
 * Hot-word greedy search with the gate inside the device step: the fork's default
 * decode path, wenet/transducer/search/greedy_search.py:297-430 (`basic_greedy_search_both`, selected by
 * loss_mode='both', wenet/transducer/transducer.py:43,559-597), around wenet/transformer/context_bias.py::ContextBias.
 *
 * Per predictor step the reference calls ContextBias.forward_predictor_bias (:375-381: multi-head attention of the
 * predictor output over the encoded hot-word list, LayerNorm, Linear over the concatenation, LayerNorm) and
 * ContextBias.forward_hw_pred_both (:388-394: the two-class "is a hot word being spoken" gate), takes the gate's
 * top-1 on the host (.item()), and with context_filter_state == 'on' runs the "go-back" (:365-392): when the gate
 * flips 0 -> 1 the token emitted after the gate-0 step is withdrawn and decoding resumes from that step's frame with
 * biasing forced on until the frame of the flip.  Here all of it lives in the captured micro-step:
 *   - gate: the classifier attends from ONE query to ONE key (the encoder bias feature of frame t), so its softmax
 *     weight is exactly 1 and its output is a function of the frame alone (q / k projections cannot influence it):
 *     the gate of every frame is evaluated up front by one kernel (hw_gate_table_kernel) and looked up per step;
 *   - predictor biasing: one fused kernel per micro-step (query projection, attention over the list, output
 *     projection, LayerNorm, combine Linear, LayerNorm) for the variant -- hot-word list or empty list -- that the gate
 *     selected; the joiner activation picks the matching biased encoder stream;
 *   - gate trace, go-back rewind and the withdrawn token are part of the update kernel's state machine; the host
 *     reads back once per graph replay, exactly as in wr_greedy_search.
 * The loop-invariant tensors are the caller's (the reference computes them before its loop, :327-336, with the same
 * module): bias_hidden of the hot-word list and of the empty list, and the biased encoder outputs.
 *
 * Weights in the reference module's layouts (nn.Linear [out, in], LayerNorm [dim]); LayerNorm eps = 1e-5.
 * dim = embedding_size = encoder output size = predictor output size (the module requires all three equal);
 * dim <= 512, hw_dim <= 256, n_labels <= 8, heads divides dim, lists of at most max_ctx entries.
 * ---------------------------------------------------------------------- */
typedef struct wr_hotword_weights {
    int32_t dim, heads, hw_dim, n_labels;
    /* ContextBias.predictor_bias (MultiHeadedAttention, attention.py:35-45) */
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b, *o_w, *o_b;          /* linear_q / _k / _v / _out: [dim, dim], [dim] */
    const float *bias_norm_w, *bias_norm_b;                              /* predictor_bias_bias_norm */
    const float *combine_w, *combine_b;                                  /* predictor_bias_combine [dim, 2 dim], [dim] */
    const float *out_norm_w, *out_norm_b;                                /* predictor_bias_out_norm */
    /* gate: hw_output_layer_enc -> hw_bias.linear_v -> hw_bias.linear_out -> hw_bias_norm -> hw_output_layer */
    const float *hw_enc_w, *hw_enc_b;                                    /* [hw_dim, dim], [hw_dim] */
    const float *hw_v_w, *hw_v_b, *hw_o_w, *hw_o_b;                      /* [hw_dim, hw_dim], [hw_dim] */
    const float *hw_norm_w, *hw_norm_b;                                  /* [hw_dim] */
    const float *hw_out_w, *hw_out_b;                                    /* [n_labels, hw_dim], [n_labels] */
} wr_hotword_weights;

size_t wr_hotword_workspace_bytes(const wr_decoder *h, const wr_hotword_weights *hw, int max_ctx);

/* Attach the hot-word module to a decoder handle (weights re-laid k-major once into `workspace_d`, which the caller
 * keeps alive with the handle). */
int wr_decoder_attach_hotword(wr_decoder *h, const wr_hotword_weights *hw, int max_ctx,
                              void *workspace_d, size_t workspace_bytes, void *stream);

/* enc_hot / enc_cold [N, T, dim]: ContextBias.forward_encoder_bias of the encoder output with the hot-word list /
 * the empty list (first return value); enc_feat [N, T, dim]: its second return value for the hot-word list;
 * hidden_hot [n_ctx_hot, dim], hidden_cold [n_ctx_cold, dim]: ContextBias.forward_bias_hidden of the two lists
 * (shared by all N streams).  filter_on = (context_filter_state == 'on').  Out: hyps [N, max_hyp] / hyp_lens [N] as
 * wr_greedy_search; trace [N, trace_cap] / trace_lens [N]: the gate trace (`result` in the reference, whose edit
 * distance to the hot-word labels is the second return value of the reference function). */
int wr_greedy_search_hotword(wr_decoder *h, const float *enc_hot_d, const float *enc_cold_d, const float *enc_feat_d,
                             const int32_t *enc_lens_d, const float *hidden_hot_d, int n_ctx_hot,
                             const float *hidden_cold_d, int n_ctx_cold, int N, int T, int n_steps, int blank,
                             int filter_on, int32_t *hyps_d, int32_t *hyp_lens_d, int32_t *trace_d, int trace_cap,
                             int32_t *trace_lens_d, void *stream);

/* ------------------------------------------------------------------------
 * CTC decode modes, from the ctc_lo output on; the log-softmax is fused.
 * Replaces ASRModel.ctc_greedy_search (wenet/transformer/asr_model.py:281-324) and
 * ASRModel._ctc_prefix_beam_search (:326-409; C++ twin runtime/core/decoder/ctc_prefix_beam_search.cc:107-238,
 * known-answer test runtime/core/test/ctc_prefix_beam_search_test.cc:30-73).
 * logits [B, T, V] pre-softmax, lens [B].
 * Greedy: hyps [B, T] / hyp_lens [B] / scores [B].  As in the reference, frames past an utterance's length are
 * filled with `eos` before duplicate/blank removal, and scores[b] is the maximum over all T frames of the
 * best log-probability.
 * Prefix beam: hyps [B, beam, T] (padded with -1), hyp_lens [B, beam], scores [B, beam] float64 (best first),
 * n_hyps [B]; any number of utterances at once (the reference asserts batch size 1).  beam <= 16.
 * ---------------------------------------------------------------------- */
size_t wr_ctc_decode_workspace_bytes(int B, int T, int beam);

int wr_ctc_greedy_search(const float *logits_d, const int32_t *lens_d, int B, int T, int V, int blank, int eos,
                         int32_t *hyps_d, int32_t *hyp_lens_d, float *scores_d,
                         void *workspace_d, size_t workspace_bytes, void *stream);

int wr_ctc_prefix_beam_search(const float *logits_d, const int32_t *lens_d, int B, int T, int V, int beam,
                              int blank, int32_t *hyps_d, int32_t *hyp_lens_d, double *scores_d,
                              int32_t *n_hyps_d, void *workspace_d, size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Streaming CTC prefix beam search: the search of wr_ctc_prefix_beam_search continued from a state block across
 * chunks, for any number of streams at once, with the Viterbi score and one frame index per token of every
 * hypothesis.  The chunk-driven twin in the reference is runtime/core/decoder/ctc_prefix_beam_search.cc:107-211
 * (Search() once per encoder chunk, cur_hyps_ / abs_time_step_ kept between calls, viterbi_likelihood() and Times());
 * its known-answer test is runtime/core/test/ctc_prefix_beam_search_test.cc:30-73.
 *
 * State.  Each stream holds the number of frames consumed, a_next, and an ordered list, best first, of at most `beam`
 * entries.  An entry holds tokens; pb, pnb: float64 blank-ending and non-blank-ending summed scores; vb, vnb: float64
 * Viterbi scores of the two endings; times_b, times_nb: one frame index per token, for the best blank-ending and
 * non-blank-ending path.  A fresh stream has a_next = 0 and one entry: tokens = (), pb = 0, pnb = -inf, vb = 0, vnb = 0,
 * both times lists empty (ctc_prefix_beam_search.cc:44-48; vnb = -inf would give the same results).  Derived:
 *   vit(e)   = vb > vnb ? vb : vnb
 *   times(e) = vb > vnb ? times_b : times_nb      (an exact tie takes times_nb, as the reference's `>` does)
 *
 * One frame.  Its absolute index is a = a_next.  Its top-`beam` symbols are found exactly as wr_ctc_prefix_beam_search
 * finds them (the fused fp32 log-softmax, value descending, lower index on a tie, p = (double)logp[s]).  The visiting
 * order is the Python search's: symbol outer, entries inner in list order.  Contributions go into an insertion-ordered
 * dictionary `next`; a new key starts with pb = pnb = vb = vnb = -inf, ctp = -inf and empty times.  ctp is the best token
 * log-probability that set the key's times_nb in this frame; it exists only inside the frame.
 *   s == blank, key tokens:
 *       pb = log_add(pb, e.pb + p, e.pnb + p);  vb = vit(e) + p;  times_b = times(e)
 *   s == last token of e, key tokens:
 *       pnb = log_add(pnb, e.pnb + p)
 *       if vnb < e.vnb + p: vnb = e.vnb + p; then, if ctp < p: ctp = p, times_nb = e.times_nb with its last element
 *       replaced by a
 *   s == last token of e, also key tokens + (s,):
 *       pnb = log_add(pnb, e.pb + p)
 *       if vnb < e.vb + p: vnb = e.vb + p, ctp = p, times_nb = e.times_b + (a,)
 *   otherwise, key tokens + (s,):
 *       pnb = log_add(pnb, e.pb + p, e.pnb + p)
 *       if vnb < vit(e) + p: vnb = vit(e) + p, ctp = p, times_nb = times(e) + (a,)
 * The sums are float64, left to right (wenet/utils/common.py:268-276); the Viterbi values are plain float64 adds.
 * After the frame: stable descending sort by log_add(pb, pnb); the first `beam` entries are the new list; a_next += 1.
 * The Viterbi fields never influence pruning.  (The reference iterates an unordered_map, so its order where two
 * contributions meet in one key is unspecified; ours is the Python search's.)  Consequence: every hypothesis's times
 * has as many elements as tokens, is strictly increasing, and lies in [0, a_next).
 *
 * One call consumes lens[b] frames of stream b from a chunk logits [B, T, V], 0 <= lens[b] <= T; zero leaves the stream
 * untouched.  Then it exports, for every stream: hyps [B, beam, Lcap] (padded with -1), hyp_lens [B, beam], scores
 * [B, beam] float64 = log_add(pb, pnb), viterbi [B, beam] float64 = vit(e), times [B, beam, Lcap] (padded with -1; all
 * -1 for an entry neither of whose endings has a path, vit(e) = -inf), n_hyps [B], n_frames [B] = a_next.
 * reset != 0 starts fresh streams before consuming.
 *
 * Two equalities define "correct".  (1) For any one-chunk call, hyps / hyp_lens / scores / n_hyps are bit-identical to
 * wr_ctc_prefix_beam_search on the same logits.  (2) For any split of a stream's frames into chunks -- width 1, chunks
 * in which some streams have lens[b] = 0, ragged splits across the streams of one call -- every output after the last
 * chunk is bit-identical to the one-chunk call: a row's log-softmax does not depend on its neighbours and the per-frame
 * arithmetic is one fixed sequence.
 *
 * The state block is caller-owned and opaque, wr_ctc_stream_state_bytes(B, beam, Lcap) bytes; B, beam and Lcap must not
 * change between the calls of one stream set (a block that no call with this beam and Lcap has written starts fresh,
 * as after a reset).  frames_done is a host value: the chunk widths T summed over the earlier calls since the reset.
 * Refused before any HIP call, in this order: the shape checks of the other CTC decode modes (B, T positive, V > 1,
 * blank inside V: WR_EINVAL; V > 16320: WR_EUNSUPPORTED); a null pointer (WR_EINVAL); beam outside [1, 16] or beam > V
 * (WR_EUNSUPPORTED); Lcap < 1, frames_done < 0, reset != 0 with frames_done != 0 (WR_EINVAL); frames_done + T > Lcap
 * (WR_EUNSUPPORTED: a prefix gains at most one token per frame, so Lcap frames can never overflow the sequences); a
 * state block or workspace below its query's size (WR_EWORKSPACE).  Everything runs on the caller's stream; there is no
 * device-wide synchronisation and no allocation.  The size queries answer a non-positive argument (or beam > 16) with 0.
 * These entry points only add to the ABI: WR_API_VERSION stays 3 (see its rule above).
 * ---------------------------------------------------------------------- */
size_t wr_ctc_stream_state_bytes(int B, int beam, int Lcap);
size_t wr_ctc_stream_workspace_bytes(int B, int T, int beam);

int wr_ctc_prefix_beam_search_chunk(const float *logits_d, const int32_t *lens_d, int B, int T, int V, int beam, int blank,
                                    int reset, int frames_done, int Lcap, void *state_d, size_t state_bytes,
                                    int32_t *hyps_d, int32_t *hyp_lens_d, double *scores_d, double *viterbi_d,
                                    int32_t *times_d, int32_t *n_hyps_d, int32_t *n_frames_d, void *workspace_d,
                                    size_t workspace_bytes, void *stream);

/* ------------------------------------------------------------------------
 * Context-graph biasing in the CTC prefix beam search: the streaming search above with the classical phrase biasing of
 * the reference runtime (runtime/core/decoder/context_graph.{h,cc}, ctc_prefix_beam_search.h:53-83 and
 * ctc_prefix_beam_search.cc:137-193, 213-234: UpdateContext / CopyContext, total_score(), UpdateFinalContext()).
 * Everything the contract above says of a frame holds unchanged -- the top-`beam` symbols, the visiting order, the
 * float64 sums, the Viterbi riders, the times; what follows is what is added.
 *
 * The graph is a deterministic table of S states in device memory, state 0 the root:
 *   arc_begin int32[S+1]  CSR offsets into the arcs      arc_token int32[A]  strictly increasing within a state
 *   arc_next  int32[A]                                   arc_score float32[A]
 *   escape    float32[S], escape[0] = 0                  final     int32[S], final[0] = 1
 *   next(state, token) = (arc_next, arc_score, state == 0, final[arc_next] != 0)   if state has an arc on token
 *                      = (0, escape[state], false, false)                           otherwise
 * (context_graph.cc:86-108: the token that breaks a partial match is not retried from the root.)
 *
 * Every entry also holds ctx_state (int32), ctx_score (float64) and tags, one int32 per token: bit 0 a start boundary
 * at this token, bit 1 an end boundary at this token.  A fresh stream's entry has ctx_state = 0, ctx_score = 0, no tags.
 * A contribution that leaves the prefix unchanged (a blank, the same token again) copies the three fields of its source
 * entry e; one that appends token s takes (st, sc, start, end) = next(e.ctx_state, s) and sets ctx_state = st,
 * ctx_score = e.ctx_score + (double)sc, tags = e.tags + (start | end << 1,).  The table is deterministic and copies keep
 * the state, so the three fields are a function of the token sequence alone: every contributor to a key sets the same
 * values (the reference lets the first one set them).  After the frame: stable descending sort by
 * total = log_add(pb, pnb) + ctx_score, in float64; the first `beam` entries are the new list.
 *
 * Export.  Beside the plain call's outputs: ctc_scores [B, beam] float64 = log_add(pb, pnb); context_scores [B, beam]
 * float64; tags [B, beam, Lcap] (padded with -1); context_states [B, beam] (the entry's ctx_state as the stream holds
 * it).  scores = ctc_scores + context_scores, the float64 add of the prune.  finalize != 0 exports "as if the stream
 * ended here" (UpdateFinalContext): for every entry with ctx_state != 0 the exported context score gains
 * (double)escape[ctx_state], then the exported list is sorted again, stable and descending, by the new totals.  Tags
 * are not touched (a start tag of an abandoned match stays, as in the reference), and neither is the state block: the
 * caller may go on feeding chunks.  A chunk with every lens[b] == 0 is legal: it finalises without new frames.
 *
 * Two departures from the reference, both deliberate: the bonus is summed in float64 (the reference's is a float), and
 * the graph is whatever table the caller built -- the Python builder commits a phrase that is a proper prefix of
 * another at its last token, where determinising the reference's FST would take that bonus back.
 *
 * The state block has its own layout (a fourth double-buffered list for the tags, two more scalars per entry) and its
 * own size query; the plain block and wr_ctc_stream_state_bytes are unchanged, and a block written by one form starts
 * fresh under the other.  The workspace is wr_ctc_stream_workspace_bytes(B, T, beam).  Refused before any HIP call, in
 * this order: everything wr_ctc_prefix_beam_search_chunk refuses, in its order (a null output among the four new ones
 * counts with the null pointers); S < 1 or A < 0, then a null table pointer (WR_EINVAL); S > 65536 or A > 1048576
 * (WR_EUNSUPPORTED).  The table's contents are the builder's responsibility: the kernel clamps every arc_next it reads
 * into [0, S) and every CSR bound into [0, A] before using it as an index, so a bad table gives wrong bonuses, never an
 * out-of-range access.  Addition only: WR_API_VERSION stays 3.
 * ---------------------------------------------------------------------- */
size_t wr_ctc_context_stream_state_bytes(int B, int beam, int Lcap);

int wr_ctc_prefix_beam_search_context_chunk(const float *logits_d, const int32_t *lens_d, int B, int T, int V, int beam,
                                            int blank, int reset, int frames_done, int Lcap, void *state_d,
                                            size_t state_bytes, const int32_t *arc_begin_d, const int32_t *arc_token_d,
                                            const int32_t *arc_next_d, const float *arc_score_d, const float *escape_d,
                                            const int32_t *final_d, int S, int A, int finalize, int32_t *hyps_d,
                                            int32_t *hyp_lens_d, double *scores_d, double *viterbi_d, int32_t *times_d,
                                            int32_t *n_hyps_d, int32_t *n_frames_d, double *ctc_scores_d,
                                            double *context_scores_d, int32_t *tags_d, int32_t *context_states_d,
                                            void *workspace_d, size_t workspace_bytes, void *stream);

/* RNN-T forced alignment: the single best path through the lattice of wr_rnnt_loss_fwd (a Viterbi pass: the forward
 * sweep with max in place of log-add-exp, one decision bit per cell, and a backtrace).  No reference call site: the
 * reference aligns with the CTC head only (wenet/bin/alignment.py); this is the transducer head's counterpart.
 *   A(0,0) = 0, A(t,u) = max(A(t-1,u) + blank(t-1,u), A(t,u-1) + emit(t,u-1)), scores[b] = A(T_b-1,U_b) + blank(T_b-1,U_b)
 * in fp64 over the fp32 log-probabilities of pass 1.  Tie rule: the emit predecessor wins only if its candidate is
 * strictly greater; on equality or a NaN comparison the blank predecessor wins (a NaN candidate makes the value NaN), so
 * the path is always a valid monotone one.  label_frames [B, U1max-1] int32: the frame at which label u+1 is emitted on
 * the best path (non-decreasing in u), -1 for u >= U_b.  scores [B] double.
 * Lengths: 1 <= logit_lengths[b] <= Tmax and 0 <= target_lengths[b] <= U1max-1 (the maxima need not equal the padded
 * sizes, unlike the loss; the caller checks them); targets within [0, V) inside each length.
 * wr_rnnt_align: pass 1 over the logits (fp32, fp16 or bf16, as wr_rnnt_loss_fwd), then the Viterbi kernel.  Workspace:
 * wr_rnnt_workspace_bytes(B, Tmax, U1max).
 * wr_rnnt_align_from_stats: the Viterbi kernel alone, on an RNN-T workspace whose row statistics wr_joint_rnnt_stats
 * wrote (no logits tensor; that call repairs an overflowed row itself).  `targets_d` are the labels the statistics
 * were taken with (they are not read again: the emit log-probabilities carry them). */
int wr_rnnt_align(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                  const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank,
                  int32_t *label_frames_d /* [B, U1max-1] out */, double *scores_d /* [B] out */,
                  void *workspace_d, size_t workspace_bytes, void *stream);

int wr_rnnt_align_from_stats(const int32_t *targets_d, const int32_t *logit_lengths_d, const int32_t *target_lengths_d,
                             int B, int Tmax, int U1max, int32_t *label_frames_d /* [B, U1max-1] out */,
                             double *scores_d /* [B] out */, void *rnnt_workspace_d, size_t rnnt_workspace_bytes,
                             void *stream);

/* The additive-joiner ("simple") RNN-T loss: the transducer loss of logits(b,t,u,v) = am[b,t,v] + lm[b,u,v], which is
 * what k2's rnnt_loss_simple computes (wenet/transducer/transducer_k2_loss.py:140-157), without a (B,T,U1,V) tensor.
 * am [B,T,V], lm [B,U1,V] fp32; symbols [B,U1-1]; lengths as wr_rnnt_loss_fwd (1 <= logit_lengths[b] <= T or 0 for an
 * empty utterance, 0 <= target_lengths[b] <= U1-1); V >= 2, U1 <= 1024.  Two workspaces: the RNN-T one
 * (wr_rnnt_workspace_bytes(B,T,U1)) and this loss's own scratch (wr_rnnt_simple_workspace_bytes: the row maxima of am and
 * lm, and a few floats per lattice cell for the gradient -- never logits-sized).
 *
 * wr_rnnt_simple_stats: the row statistics of every valid cell into the RNN-T workspace, in the layout and with the
 * conventions of pass 1 of wr_rnnt_loss_fwd: denom(t,u) = log sum_v exp(am[t,v] + lm[u,v]) as a [T x V].[V x U1]
 * contraction of the exponentiated, max-shifted operands (exact-fp32 MFMA), and the skewed blank / label log-probabilities
 * (emit = 0 at u == U_b).  wr_rnnt_loss_sweeps, wr_rnnt_export_lattice and wr_rnnt_align_from_stats follow unchanged.
 * A valid cell whose factored sum is zero, not finite or below 1e-20 (the peaks of am[t] and lm[u] sit on different
 * symbols and are both tall) raises the flag word of the RNN-T workspace; a second, direct kernel (one wave per cell,
 * running maximum over am + lm) is always enqueued and redoes every cell then -- its workgroups leave at once
 * otherwise.  No host synchronisation.
 *
 * wr_rnnt_simple_grad: d_am [B,T,V] and d_lm [B,U1,V] (fp32, every element written, zero for t >= T_b and u > U_b) of
 * sum_b grad_costs[b] * cost_b (NULL = 1; no clamp, as k2), as two MFMA contractions over u and over t plus the scatter
 * terms at the blank and the labels, summed in a fixed order: bit-identical run to run.  Needs both workspaces after
 * wr_rnnt_simple_stats + wr_rnnt_loss_sweeps; it only reads the RNN-T one.  With the flag raised the contractions are
 * replaced by direct sums of occupancy * softmax.  occ_emit_d / occ_blank_d [B,T,U1] (nullable): the arc occupancies
 * exp(alpha(t,u) + emit(t,u) + beta(t,u+1) - ll) and exp(alpha(t,u) + blank(t,u) + beta(t+1,u) - ll) (beta := 0 past the
 * final cell), zero outside the valid region, not scaled by grad_costs -- k2's px_grad / py_grad transposed. */
size_t wr_rnnt_simple_workspace_bytes(int B, int T, int U1, int V);

int wr_rnnt_simple_stats(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                         const int32_t *logit_lengths_d, const int32_t *target_lengths_d,
                         int B, int T, int U1, int V, int blank,
                         void *simple_workspace_d, size_t simple_workspace_bytes,
                         void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

int wr_rnnt_simple_grad(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                        const int32_t *logit_lengths_d, const int32_t *target_lengths_d,
                        int B, int T, int U1, int V, int blank,
                        const float *grad_costs_d /* [B] or NULL */,
                        float *d_am_d /* [B,T,V] out */, float *d_lm_d /* [B,U1,V] out */,
                        float *occ_emit_d /* [B,T,U1] out or NULL */, float *occ_blank_d /* [B,T,U1] out or NULL */,
                        void *simple_workspace_d, size_t simple_workspace_bytes,
                        const void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

/* The smoothed additive-joiner loss: k2's rnnt_loss_smoothed, regular lattice.  Shapes, lengths and both workspaces'
 * roles as wr_rnnt_simple_*; the scratch is larger (wr_rnnt_smoothed_workspace_bytes: it begins with the simple loss's
 * layout and adds rows of B*T, B*U1 and V floats and a partial-sum area of max(ceil(B*U1/64), B*ceil(T/64)) * V floats).
 * With ll = lm_only_scale, la = am_only_scale (both >= 0, ll + la <= 1), c = 1 - ll - la:
 *
 *   Zl[b,u]   = log sum_v exp(lm[b,u,v])                                  lm-only normaliser
 *   pbar[v]   = (1 / (B*U1)) sum_{b,u} softmax(lm[b,u,:])[v] + tiny       "unigram"; tiny = smallest normal fp32
 *   N[b,t]    = log sum_v exp(am[b,t,v]) * pbar[v]                        am-only normaliser
 *   denom     = log sum_v exp(am[b,t,v] + lm[b,u,v])                      as wr_rnnt_simple_stats
 *   emit(t,u)  = c*(am[t,y_u] + lm[u,y_u] - denom(t,u)) + ll*(lm[u,y_u] - Zl[u]) + la*(am[t,y_u] + log pbar[y_u] - N[t])
 *   blank(t,u) = c*(am[t,blank] + lm[u,blank] - denom(t,u)) + ll*(lm[u,blank] - Zl[u]) + la*(am[t,blank] + log pbar[blank] - N[t])
 *
 * pbar is the mean over ALL B*U1 rows of lm, rows past U_b included (k2's definition): padded rows of lm must be finite
 * when la > 0.  A scale that is exactly 0 drops its branch: no term, no kernel (with la == 0 nothing beyond the simple
 * loss's kernels reads am).  ll == la == 0 runs wr_rnnt_simple_stats / wr_rnnt_simple_grad's kernels and nothing else:
 * the same bits, and the scratch then needs only wr_rnnt_simple_workspace_bytes (the part these calls touch; with a
 * non-zero scale wr_rnnt_smoothed_workspace_bytes).  wr_rnnt_simple_stats / wr_rnnt_simple_grad are these calls with
 * ll = la = 0 (wr_rnnt_simple_grad requires d_am and d_lm).  Order of the argument checks in these four calls and wr_rnnt_smoothed_grad_lattice: shapes and
 * scales (WR_EINVAL / WR_EUNSUPPORTED; the bound V <= 256 * 65535 belongs to the smoothing kernels' grids and applies
 * only with a non-zero scale), then both workspace sizes (WR_EWORKSPACE), then null pointers (WR_EINVAL): a call with a
 * null pointer and a workspace that is too small returns WR_EWORKSPACE.
 *
 * wr_rnnt_smoothed_stats: wr_rnnt_simple_stats' kernels (the direct repair pass included), then the arcs above written
 * over the skewed log-probabilities of the RNN-T workspace.  wr_rnnt_loss_sweeps / wr_rnnt_export_lattice follow.
 *
 * wr_rnnt_smoothed_grad: the gradient of sum_b g_b * cost_b (g = grad_costs, NULL = 1).  With oe / ob the arc occupancies
 * of the interpolated lattice, occ = oe + ob, sigma = softmax:
 *   d am[b,t,v] = g_b*[ c*sum_u occ(t,u)*sigma(am[t]+lm[u])[v] + la*C(t)*q_t[v] - (c+la)*(sum_u oe(t,u)[v=y_u] + sum_u ob(t,u)[v=blank]) ]
 *                 C(t) = sum_u occ(t,u),  q_t[v] = exp(am[t,v] - N[t]) * pbar[v]
 *   d lm[b,u,v] = g_b*[ c*sum_t occ(t,u)*sigma(am[t]+lm[u])[v] + ll*R(u)*sigma(lm[u])[v] - (c+ll)*(sum_t oe(t,u)[v=y_u] + sum_t ob(t,u)[v=blank]) ]
 *                 + (1/(B*U1)) * s[v] * (h[v] - sum_w s[w]*h[w]),  s = sigma(lm[b,u]),  R(u) = sum_t occ(t,u)
 *   h[v]        = la * sum_b g_b*[ sum_t C_b(t)*exp(am[b,t,v] - N[b,t]) - (sum_{t,u} oe_b(t,u)[v=y_u] + sum_{t,u} ob_b(t,u)[v=blank]) / pbar[v] ]
 * The h term reaches every row of lm, padded ones included, and couples the utterances of a batch (la > 0 only); with
 * la == 0 padded rows of d_lm are exactly zero; d_am rows t >= T_b are always exactly zero.  Every arc is subtracted at
 * its own symbol (a label equal to the blank has both of its cell's arcs subtracted at the blank), which is the
 * derivative of the arcs as written; wr_rnnt_simple_grad keeps the case chain of wr_rnnt_loss_bwd there.  No float
 * atomics, fixed summation order: bit-identical run to run.  d_am_d == d_lm_d == NULL: only the occupancies are written
 * (both occupancy outputs are then required).  Needs wr_rnnt_smoothed_stats + wr_rnnt_loss_sweeps on the same workspaces
 * and the same two scales. */
size_t wr_rnnt_smoothed_workspace_bytes(int B, int T, int U1, int V);

int wr_rnnt_smoothed_stats(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                           const int32_t *logit_lengths_d, const int32_t *target_lengths_d,
                           int B, int T, int U1, int V, int blank, float lm_only_scale, float am_only_scale,
                           void *smoothed_workspace_d, size_t smoothed_workspace_bytes,
                           void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

int wr_rnnt_smoothed_grad(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                          const int32_t *logit_lengths_d, const int32_t *target_lengths_d,
                          int B, int T, int U1, int V, int blank, float lm_only_scale, float am_only_scale,
                          const float *grad_costs_d /* [B] or NULL */,
                          float *d_am_d /* [B,T,V] out */, float *d_lm_d /* [B,U1,V] out */,
                          float *occ_emit_d /* [B,T,U1] out or NULL */, float *occ_blank_d /* [B,T,U1] out or NULL */,
                          void *smoothed_workspace_d, size_t smoothed_workspace_bytes,
                          const void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

/* Pruned RNN-T training: k2's get_rnnt_prune_ranges / do_rnnt_pruning / rnnt_loss_pruned for the regular lattice type
 * (the second half of the recipe whose first half is the additive-joiner loss above: its arc occupancies choose, per
 * frame, a band of R label positions on which the real joiner and the real loss are evaluated).  Lengths as
 * wr_rnnt_simple_stats: logit_lengths[b] = T_b in [0, T], target_lengths[b] = U_b in [0, U1-1].  1 <= R <= U1
 * everywhere.  ranges [B,T,R] int64 with ranges[b,t,r] = ranges[b,t,0] + r inside [0, U1-1]: the caller checks what it
 * did not get from wr_rnnt_prune_ranges (the kernels clamp or skip an index outside that interval, they never read or
 * write out of bounds).  No host synchronisation, no float atomics: every result is bit-identical run to run.
 *
 * wr_rnnt_prune_ranges: px_grad [B,U1-1,T+1] and py_grad [B,U1,T] fp32 are the emit / blank arc occupancies in k2's
 * layout (frames minor; px_grad may be NULL when U1 == 1).  Per utterance, one workgroup:
 *   1. for u0 in [0, U1-R]: score(u0,t) = ((py[u0,t] + py[u0+1,t]) + ... + py[u0+R-1,t]) - (u0 > 0 ? px[u0-1,t] : 0),
 *      in fp64 in exactly that order; s_begin[t] = the u0 of the largest score, the lowest u0 on ties;
 *   2. for t >= T_b - 1: s_begin[t] = max(U_b - R + 1, 0);
 *   3. over all T frames: s = suffix_min(s); x = t - s; x = suffix_min(x); x = max(x, 0); s = t - x;
 *   4. ranges[b,t,r] = s_begin[t] + r.
 * Consequences of 2-3: s_begin[0] = 0, 0 <= s_begin[t+1] - s_begin[t] <= 1, 0 <= s_begin <= min(U1-R, max(U_b-R+1, 0)).
 *
 * wr_rnnt_prune_gather: am [B,T,C], lm [B,U1,C] of `dtype` -> am_pruned, lm_pruned [B,T,R,C]:
 * am_pruned[b,t,r] = am[b,t], lm_pruned[b,t,r] = lm[b, ranges[b,t,r]].
 * wr_rnnt_prune_scatter: its backward.  d_am[b,t] = sum_r g_am_pruned[b,t,r]; d_lm[b,u] = the sum of g_lm_pruned[b,t,r]
 * over the (t,r) with ranges[b,t,r] == u, in ascending t (one r at most per t), zero where nothing points; fp32
 * accumulation, one writer per output element.  Either (gradient, output) pair may be NULL.
 *
 * wr_rnnt_pruned_stats: logits [B,T,R,V] (fp32, fp16 or bf16, as wr_rnnt_loss_fwd) are the joiner's outputs on the band.
 * Fills the skewed log-probability array of an RNN-T workspace (wr_rnnt_workspace_bytes(B,T,U1)) with (-inf, -inf), then
 * one wave per row (b,t,r), u = ranges[b,t,r] (rows with t >= T_b or u > U_b are skipped, their logits never read),
 * writes denom(t,u) and (blank - denom, emit - denom) at the skew position of the cell (t,u), emit = 0 at u == U_b: the
 * conventions of pass 1 of wr_rnnt_loss_fwd.  wr_rnnt_loss_sweeps, wr_rnnt_export_lattice and wr_rnnt_align_from_stats
 * follow unchanged.  A cell outside the band has -inf on both arcs (no path crosses it); an utterance whose band holds
 * no complete path gets cost +inf (a value, not an error; its gradient is not finite).
 * wr_rnnt_pruned_grad: grads [B,T,R,V] in the logits' dtype (may alias logits; otherwise at the same address modulo 16,
 * WR_EINVAL if not: the rows are split into 16-byte vectors by the logits' address) of sum_b grad_costs[b] * cost_b (NULL = 1;
 * no clamp, as k2), every element written: the expression of wr_rnnt_loss_bwd with the lattice read at u = ranges[b,t,r],
 * except that a label equal to the blank has both its terms subtracted (the derivative of the loss as defined, k2's
 * autograd result) where wr_rnnt_loss_bwd keeps torchaudio's first-match chain; grad_costs[b] * 0 in skipped rows.
 * HBM traffic of the two calls: 3 * sizeof(element) * V bytes per valid row. */
int wr_rnnt_prune_ranges(const float *px_grad_d, const float *py_grad_d, const int32_t *logit_lengths_d,
                         const int32_t *target_lengths_d, int B, int T, int U1, int R,
                         int64_t *ranges_d /* [B,T,R] out */, void *stream);

int wr_rnnt_prune_gather(const void *am_d, const void *lm_d, const int64_t *ranges_d, int dtype, int B, int T, int U1,
                         int R, int C, void *am_pruned_d /* [B,T,R,C] out */, void *lm_pruned_d /* [B,T,R,C] out */,
                         void *stream);

int wr_rnnt_prune_scatter(const void *g_am_pruned_d, const void *g_lm_pruned_d, const int64_t *ranges_d, int dtype,
                          int B, int T, int U1, int R, int C, void *d_am_d /* [B,T,C] out or NULL */,
                          void *d_lm_d /* [B,U1,C] out or NULL */, void *stream);

int wr_rnnt_pruned_stats(const void *logits_d, int dtype, const int32_t *symbols_d, const int64_t *ranges_d,
                         const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1, int R,
                         int V, int blank, void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

int wr_rnnt_pruned_grad(const void *logits_d, int dtype, const int32_t *symbols_d, const int64_t *ranges_d,
                        const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1, int R,
                        int V, int blank, const float *grad_costs_d /* [B] or NULL */, void *grads_d,
                        const void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

/* Lattice types and the delay penalty: k2's rnnt_type = "modified" and delay_penalty for the three losses above (the
 * additive-joiner loss, its smoothed form, the pruned loss).  k2 cannot be built for ROCm; this text is the contract.
 * blank(t,u) / emit(t,u) are the blank / label log-probabilities of cell (t,u), 0 <= t < T_b, 0 <= u <= U_b, as the
 * statistics call of the loss leaves them in the RNN-T workspace (for the pruned loss -inf outside the band).
 *
 * Delay penalty (either lattice): pen(b,t) = delay_penalty * ((T_b - 1) / 2 - t) is added to every label arc,
 * emit'(t,u) = emit(t,u) + pen(b,t): formed in fp64, added to the stored fp32 value in fp64, rounded once.  In the smoothed
 * loss that is after the interpolation.  It applies iff delay_penalty > 0; negative or non-finite values: WR_EINVAL.
 *
 * WR_LATTICE_REGULAR: the lattice of wr_rnnt_loss_fwd (a label arc (t,u) -> (t,u+1), a final blank out of (T_b-1,U_b)).
 * WR_LATTICE_MODIFIED: nodes (t,u), 0 <= t <= T_b; blank arc (t,u) -> (t+1,u) with blank(t,u), label arc (t,u) ->
 * (t+1,u+1) with emit'(t,u) for u < U_b.  Every frame carries exactly one arc; the last frame may carry a label.
 *   alpha(0,0) = 0, alpha(0,u>0) = -inf, alpha(t,u) = logadd(alpha(t-1,u) + blank(t-1,u), alpha(t-1,u-1) + emit'(t-1,u-1))
 *   beta(T_b,U_b) = 0, beta(T_b,u != U_b) = -inf, beta(t,u) = logadd(blank(t,u) + beta(t+1,u), emit'(t,u) + beta(t+1,u+1))
 *   ll = alpha(T_b,U_b) = beta(0,0), cost = -ll
 *   occ_blank(t,u) = exp(alpha(t,u) + blank(t,u) + beta(t+1,u) - ll), occ_emit(t,u) = exp(alpha(t,u) + emit'(t,u) +
 *   beta(t+1,u+1) - ll); occ_blank + occ_emit = exp(alpha + beta - ll) at every cell.
 *   d cost / d logits[t,u,:] = (occ_blank + occ_emit) softmax - occ_blank [v = blank] - occ_emit [v = label]; a label
 *   equal to the blank has both terms subtracted (in wr_rnnt_smoothed_grad_lattice whatever the scales).
 * T_b < U_b has no path: cost +inf for that utterance (a value, not an error; its gradient is not finite, the other
 * utterances are unaffected).  T_b = 0: cost 0, zero gradient.  A cell no path reaches carries -inf.
 *
 * wr_rnnt_lattice_sweeps replaces wr_rnnt_loss_sweeps after wr_rnnt_simple_stats / wr_rnnt_smoothed_stats /
 * wr_rnnt_pruned_stats, ONCE per statistics call (it rewrites the stored label arcs): adds the penalty, and for the
 * modified lattice lays the arcs out in plain [b][t][u] rows inside the same workspace and runs the frame-synchronous
 * sweeps (T_b dependent steps).  alpha / beta (fp64), ll and the costs land where wr_rnnt_loss_sweeps puts them for the
 * regular lattice; the modified lattice keeps its arrays elsewhere in the workspace, so only the *_lattice calls below,
 * given the same lattice_type, may read it (wr_rnnt_align_from_stats and wr_rnnt_export_lattice may not).
 * WR_LATTICE_REGULAR with delay_penalty 0 is wr_rnnt_loss_sweeps: the same kernel, the same shapes accepted (the other
 * settings and wr_rnnt_lattice_export also need B * (T + U1 - 1) * U1 < 2^31).  So is every *_lattice / *_cols call
 * below with the defaults: they launch the kernels of the plain entry points, which is the one path callers need.
 * wr_rnnt_lattice_export: wr_rnnt_export_lattice for either type: alpha / beta [B,T,U1] fp32 (rows t < T_b; zero outside
 * the boundary).
 * wr_rnnt_smoothed_grad_lattice: wr_rnnt_smoothed_grad (both scales 0: wr_rnnt_simple_grad, and like
 * wr_rnnt_smoothed_stats / wr_rnnt_smoothed_grad it then requires only wr_rnnt_simple_workspace_bytes of scratch)
 * reading the lattice of `lattice_type`; the penalty needs no argument, it is inside the stored label arcs.
 * wr_rnnt_pruned_grad_lattice: wr_rnnt_pruned_grad likewise; it forms the label term from the logits, so it takes the
 * penalty too (the value given to wr_rnnt_lattice_sweeps).
 * wr_rnnt_prune_ranges_cols: wr_rnnt_prune_ranges with px_grad [B,U1-1,px_cols], px_cols = T + 1 (regular) or T (the
 * modified lattice's layout, no extra frame column); only columns t < T are read, the rule is unchanged. */
int wr_rnnt_lattice_sweeps(const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1,
                           int lattice_type, double delay_penalty, float *costs_d /* [B] out */, void *workspace_d,
                           size_t workspace_bytes, void *stream);

int wr_rnnt_lattice_export(const void *workspace_d, size_t workspace_bytes, const int32_t *logit_lengths_d,
                           const int32_t *target_lengths_d, int B, int T, int U1, int lattice_type,
                           float *alpha_d /* [B,T,U1] out */, float *beta_d /* [B,T,U1] out */, void *stream);

int wr_rnnt_smoothed_grad_lattice(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                                  const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1,
                                  int V, int blank, float lm_only_scale, float am_only_scale, int lattice_type,
                                  const float *grad_costs_d /* [B] or NULL */, float *d_am_d, float *d_lm_d,
                                  float *occ_emit_d /* [B,T,U1] out or NULL */, float *occ_blank_d /* [B,T,U1] out or NULL */,
                                  void *smoothed_workspace_d, size_t smoothed_workspace_bytes,
                                  const void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

int wr_rnnt_pruned_grad_lattice(const void *logits_d, int dtype, const int32_t *symbols_d, const int64_t *ranges_d,
                                const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1,
                                int R, int V, int blank, int lattice_type, double delay_penalty,
                                const float *grad_costs_d /* [B] or NULL */, void *grads_d,
                                const void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream);

int wr_rnnt_prune_ranges_cols(const float *px_grad_d, int px_cols, const float *py_grad_d,
                              const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1, int R,
                              int64_t *ranges_d /* [B,T,R] out */, void *stream);

/* FastEmit and the delay penalty for the full-lattice loss (wr_rnnt_loss_fwd / _bwd, the joiner's fused forms and the
 * memory-bounded node).  This text is the contract.  Notation as above: cell (t,u) of utterance b, 0 <= t < T_b,
 * 0 <= u <= U_b; blank(t,u) / emit(t,u) are the log-softmax values at the blank and label columns.  Regular lattice only.
 *
 * Delay penalty, delay_penalty = d >= 0: the rule above, emit'(t,u) = emit(t,u) + d * ((T_b - 1) / 2 - t), formed in
 * fp64, added to the stored fp32 value in fp64 and rounded once; d = 0 gives emit' = emit.  alpha, beta and
 * cost_b = -alpha-terminal are those of the lattice with emit', so the returned cost includes the penalty, as in k2.  With
 * lambda = 0 the gradient is the true derivative of that cost.
 *
 * FastEmit (Yu et al., ICASSP 2021), fastemit_lambda = lambda >= 0.  Let ll = -cost.
 *   occ_blank(t,u) = exp(alpha + blank + beta(t+1,u) - ll)      (at the final cell exp(alpha + blank - ll))
 *   occ_emit(t,u)  = exp(alpha + emit' + beta(t,u+1) - ll),     occ_blank + occ_emit = exp(alpha + beta - ll)
 * The gradient with respect to the arc log-probabilities is -occ_blank for the blank arc and -(1 + lambda) occ_emit for
 * the label arc; the gradient with respect to the logits is that, taken exactly through the log-softmax:
 *   g[t,u,v] = softmax_v (occ_blank + (1 + lambda) occ_emit) - [v = blank] occ_blank - [v = label] (1 + lambda) occ_emit
 * This is the warp-transducer convention on log-probabilities, not NeMo's fused approximation (which leaves the softmax
 * term unscaled).  The returned costs do NOT depend on lambda: they are bit-identical to the costs at lambda = 0 with
 * the same d.  FastEmit is a gradient-level regulariser.
 * Where the case chain of the plain gradient drops the label term -- the label equals the blank at a cell that has a blank
 * term, or u = U_b -- there is no FastEmit term either.  clamp, grad_costs, padding (exact zeros) and a gradient written
 * over the logits behave as in wr_rnnt_loss_bwd.
 *
 * In the kernels' terms only per-row constants change.  With cmd = alpha + cost - denom:
 *   be_eff  = logadd(beta, log lambda + emit' + beta(t,u+1))   fp64, only where the label term exists and lambda > 0;
 *                                                              else be_eff = beta
 *   c2      = fl(fl(cmd + be_eff) log2e)
 *   lab_sub = fl(cmd + beta(t,u+1) + pen(b,t) + log1p(lambda)),   blank_sub unchanged
 * emit' is read from the workspace (the stored label arc, which after the sweeps below holds the penalised value), never
 * from the logits.  There is no second exponential per element.  Rows whose exponentials are all provably +0 are skipped
 * as in wr_rnnt_loss_bwd, by the same quantities: main bound alpha + cost + be_eff, label bound alpha + cost + beta(t,u+1)
 * + pen + log1p(lambda), blank bound unchanged.
 *
 * wr_rnnt_loss_fwd_lattice: wr_rnnt_loss_fwd's row pass, then wr_rnnt_lattice_sweeps (penalty into the stored arcs, the
 * unchanged sweeps).  wr_rnnt_loss_fwd_from_lse_lattice: wr_rnnt_loss_fwd_from_lse likewise (repair pass, then those
 * sweeps).  wr_rnnt_loss_bwd_lattice / wr_joint_rnnt_grad_lattice: wr_rnnt_loss_bwd / wr_joint_rnnt_grad over such a
 * workspace, given the same delay_penalty; the memory-bounded node runs wr_joint_rnnt_stats + wr_rnnt_lattice_sweeps first.
 * lattice_type: WR_LATTICE_REGULAR; WR_LATTICE_MODIFIED returns WR_EUNSUPPORTED (the argument is there so that it can
 * follow), any other code WR_EINVAL.  Negative or non-finite delay_penalty / fastemit_lambda: WR_EINVAL.  With a penalty
 * B * (T + U1 - 1) * U1 < 2^31 is required as well.  With both at 0 every one of the four launches exactly the kernels
 * and template instantiations of its plain entry point. */
int wr_rnnt_loss_fwd_lattice(const void *logits_d, int dtype, const int32_t *targets_d,
                             const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                             int V, int blank, int lattice_type, double delay_penalty, float *costs_d /* [B] out */,
                             void *workspace_d, size_t workspace_bytes, void *stream);

int wr_rnnt_loss_fwd_from_lse_lattice(const float *logits_d, const int32_t *targets_d, const int32_t *logit_lengths_d,
                                      const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank,
                                      int lattice_type, double delay_penalty, float *costs_d /* [B] out */,
                                      void *workspace_d, size_t workspace_bytes, void *stream);

int wr_rnnt_loss_bwd_lattice(const void *logits_d, int dtype, const int32_t *targets_d,
                             const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                             int V, int blank, float clamp, int lattice_type, double delay_penalty, double fastemit_lambda,
                             const float *grad_costs_d /* [B] or NULL */, void *grads_d, const void *workspace_d,
                             size_t workspace_bytes, void *stream);

int wr_joint_rnnt_grad_lattice(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                               const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d,
                               int B, int T, int U1, int J, int V, int activation, int blank, float clamp, int terms,
                               int lattice_type, double delay_penalty, double fastemit_lambda,
                               const float *grad_costs_d /* [B] or NULL */, const void *rnnt_workspace_d,
                               size_t rnnt_workspace_bytes, long long cell_begin, long long cell_end, float *g_out_d,
                               void *workspace_d, size_t workspace_bytes, int w_ready, void *stream);

/* Token-and-duration transducer (TDT; Xu et al., ICML 2023 -- the loss of NeMo's Parakeet-TDT models).  This text is the
 * contract.  The joiner's output row holds a token part and a duration part; an arc emits a token AND jumps d frames.
 *
 * Inputs.  logits [B, Tmax, U1max, V + D], contiguous, of `dtype` (WR_F32 / WR_F16 / WR_BF16): columns [0, V) are token
 * logits, columns [V, V + D) duration logits.  durations[D]: a HOST array of ints, strictly increasing, 0 <= d <= 8,
 * 1 <= D <= 9, at least one entry >= 1 (else WR_EINVAL).  targets, logit_lengths (T_b), target_lengths (U_b) as in
 * wr_rnnt_loss_fwd.  blank in [0, V).  sigma >= 0, finite: NeMo's logit under-normalisation.
 *
 * Arc log-probabilities at cell (t,u), t < T_b, u <= U_b:
 *   tok_k = log_softmax(logits[..., :V])_k - sigma          dur_n = log_softmax(logits[..., V:])_n
 * Arcs from (t,u), with d = durations[n]:
 *   blank, d >= 1:                  to (t + d, u),      weight tok_blank + dur_n
 *   label y_{u+1}, u < U_b, d >= 0: to (t + d, u + 1),  weight tok_label + dur_n
 * Nodes exist for t < T_b only.  The single terminal is reached by a blank arc from (t, U_b) with t + d == T_b, exactly.
 * A blank arc with t + d > T_b does not exist; one with t + d == T_b at u < U_b does not exist; a label arc needs
 * t + d <= T_b - 1.
 *
 * cost_b = -log sum over paths from (0,0) to the terminal of exp(sum of arc weights).  No path: cost_b = +inf -- a value,
 * as for an infeasible band: that utterance's gradient is not finite and the other utterances are unaffected.  T_b = 0:
 * cost 0, the sweeps' convention.  durations = {1} is k2's modified lattice on the token logits.
 *
 * Gradient: the exact derivative of the cost as defined -- no clamp, no FastEmit, no dead-row skip.  With a = alpha(t,u),
 * ll = -cost, beta(T_b, U_b) = 0, beta(T_b, u != U_b) = -inf:
 *   ob_n = exp(a + tok_blank + dur_n + beta(t + d, u) - ll)        where that arc exists, else 0
 *   ol_n = exp(a + tok_label + dur_n + beta(t + d, u + 1) - ll)    where that arc exists, else 0
 *   Ob = sum ob_n,  Ol = sum ol_n,  O = Ob + Ol = exp(a + beta(t,u) - ll)
 *   d cost / d token logit k    = softmax_k * O - [k = blank] Ob - [k = label] Ol    (both when the label is the blank)
 *   d cost / d duration logit n = softmaxD_n * O - (ob_n + ol_n)
 * A valid cell that no path reaches or leaves (alpha or beta is -inf) gets exactly grad_costs[b] * 0, never NaN.  Cells
 * with t >= T_b or u > U_b get grad_costs[b] * 0 and are never read.  grads may alias logits (both at the same offset
 * within a 16-byte line).
 *
 * wr_rnnt_tdt_loss_fwd: row statistics, both sweeps (fp64 state), the gradient's per-cell records; costs [B].
 * wr_rnnt_tdt_loss_bwd: the streamed gradient over a workspace wr_rnnt_tdt_loss_fwd filled for the same arguments.
 * wr_rnnt_tdt_export_lattice: alpha / beta as plain [B, Tmax, U1max] floats (0 outside the lattice), for tests.
 * Refused before any launch: D outside [1, 9], a duration outside [0, 8] or not strictly increasing, all durations 0,
 * negative or non-finite sigma, blank outside [0, V), null pointers (WR_EINVAL); U1max > 1024 or B * (Tmax + U1max - 1) *
 * U1max >= 2^31 (WR_EUNSUPPORTED); a workspace below wr_rnnt_tdt_workspace_bytes (WR_EWORKSPACE; 0 for a bad shape). */
size_t wr_rnnt_tdt_workspace_bytes(int B, int Tmax, int U1max, int D);

int wr_rnnt_tdt_loss_fwd(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                         const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank,
                         const int32_t *durations /* [D], host */, int D, double sigma, float *costs_d /* [B] out */,
                         void *workspace_d, size_t workspace_bytes, void *stream);

int wr_rnnt_tdt_loss_bwd(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                         const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank,
                         const int32_t *durations /* [D], host */, int D, double sigma,
                         const float *grad_costs_d /* [B] or NULL */, void *grads_d, const void *workspace_d,
                         size_t workspace_bytes, void *stream);

int wr_rnnt_tdt_export_lattice(const void *workspace_d, size_t workspace_bytes, const int32_t *logit_lengths_d,
                               const int32_t *target_lengths_d, int B, int Tmax, int U1max, int D,
                               float *alpha_d /* [B,Tmax,U1max] out */, float *beta_d /* [B,Tmax,U1max] out */,
                               void *stream);

/* Joiner + TDT loss without a logits tensor (the memory-bounded TDT node, fused.py `joint_rnnt_tdt_loss`).  This text is
 * the contract; the loss, its arcs, sigma and the gradient are those of "Token-and-duration transducer" above.
 *
 * The joiner (ep, pp, w_out, b_out, activation, J: as wr_joint_fwd) has W = V + D output rows: w_out [W, J], b_out [W];
 * columns [0, V) of its logits are token logits, [V, W) duration logits.  Exact fp32 only, and only the default forward
 * kernel: under wr_tune_set(5, 1) these entry points return WR_EUNSUPPORTED.  `workspace_d` as wr_joint_workspace_bytes
 * (J, W); `tdt_workspace_d` as wr_rnnt_tdt_workspace_bytes(B, T, U1, D).
 *
 * wr_joint_tdt_stats: the joiner forward with the row statistics of wr_rnnt_tdt_loss_fwd as its only output.  Per cell
 * t < T_b, u <= U_b it writes the token log-sum-exp, {tok_blank, tok_label} (tok_label = -inf at u = U_b or for a label
 * outside [0, V)) and the D duration log-probabilities into the TDT workspace; no logit is stored.  The token sum follows
 * wr_joint_rnnt_stats: a row that spreads over more than 88 nats raises a flag in the workspace, and a second launch with a
 * running maximum, whose workgroups leave at once unless the flag is set, repairs it.  The duration log-sum-exp takes a
 * true maximum.  Then wr_rnnt_tdt_sweeps.
 *
 * wr_rnnt_tdt_sweeps: both sweeps and the gradient's per-cell records over statistics that are already in the workspace
 * (the part of wr_rnnt_tdt_loss_fwd behind its row pass); costs [B] as wr_rnnt_tdt_loss_fwd.
 *
 * wr_joint_tdt_grad: grad_costs[b] * d cost_b / d logits of the cells [cell_begin, cell_end) of the flattened (B, T, U1)
 * lattice into g_out [(cell_end - cell_begin), W], fp32.  Every 64-cell logits tile is recomputed by the same forward
 * kernel (bit-identical to the logits the statistics came from) and turned into the gradient in its epilogue with the
 * formula of wr_rnnt_tdt_loss_bwd: no clamp, no FastEmit, no dead-row skip; both subtractions when the label is the blank.
 * Rows outside [0,T_b) x [0,U_b] are 0.  Needs the TDT workspace after wr_joint_tdt_stats + wr_rnnt_tdt_sweeps and only
 * reads it.  w_ready as in wr_joint_rnnt_grad.
 *
 * Refused before any launch, under the entry point's name: the durations contract with the codes and texts of
 * wr_rnnt_tdt_loss_fwd; V = W - D < 2; blank outside [0, V); negative or non-finite sigma; null pointers (grad_costs and,
 * with U1 == 1, targets may be null) (WR_EINVAL); U1 > 1024 or B * (T + U1 - 1) * U1 >= 2^31 (WR_EUNSUPPORTED); either
 * workspace below its size (WR_EWORKSPACE); cell_begin / cell_end outside [0, B * T * U1] or cell_begin >= cell_end
 * (WR_EINVAL); what the joiner refuses (join_dim, activation). */
int wr_joint_tdt_stats(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                       const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d,
                       int B, int T, int U1, int J, int W, int activation, int blank,
                       const int32_t *durations /* [D], host */, int D, double sigma,
                       void *workspace_d, size_t workspace_bytes,
                       void *tdt_workspace_d, size_t tdt_workspace_bytes, void *stream);

int wr_rnnt_tdt_sweeps(const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                       const int32_t *durations /* [D], host */, int D, float *costs_d /* [B] out */,
                       void *workspace_d, size_t workspace_bytes, void *stream);

int wr_joint_tdt_grad(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                      const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d,
                      int B, int T, int U1, int J, int W, int activation, int blank,
                      const int32_t *durations /* [D], host */, int D, double sigma,
                      const float *grad_costs_d /* [B] or NULL */,
                      const void *tdt_workspace_d, size_t tdt_workspace_bytes,
                      long long cell_begin, long long cell_end, float *g_out_d /* [cell_end - cell_begin, W] */,
                      void *workspace_d, size_t workspace_bytes, int w_ready, void *stream);

/* TDT forced alignment: the single best path through the lattice above.  This text is the contract.  Inputs, arc weights
 * tok_k and dur_n, sigma, the duration rules and the terminal are exactly those of "Token-and-duration transducer".
 *
 * With A(0,0) = 0, A(t,u) is the max over incoming arcs of (A(src) + tok) + dur: blank arcs from (t - d, u), d >= 1, and
 * label arcs from (t - d, u - 1), d >= 0, the latter for t <= T_b - 1.  score_b is the max over the blank arcs from
 * (T_b - d, U_b) into the terminal.  All sums are float64, over the float32 arc log-probabilities that the row-statistics
 * pass stores.  score_b <= -cost_b of wr_rnnt_tdt_loss_fwd.
 *
 * Tie rule.  A larger candidate wins.  Between equal candidates a blank arc beats a label arc; within one kind the
 * smaller d wins.  A NaN candidate never wins, and a cell with no winning candidate is unreachable (-inf).  The terminal
 * follows the same rule.
 *
 * Outputs per utterance.  label_frames[b, u]: the frame t at which the arc that emits label u + 1 leaves;
 * label_durations[b, u]: that arc's jump d (the value, not its index); both -1 for u >= U_b.  blank_jumps[b, t]
 * (optional, may be NULL): the jump of the blank arc that leaves frame t on the best path -- a blank has d >= 1, so at
 * most one does -- 0 if none and 0 for t >= T_b.  scores[b]: score_b.  The three arrays determine the whole path.
 * No path (durations = {2}, T_b = 3, U_b = 0; or T_b = 0): scores[b] = -inf, labels -1, jumps 0, and the other
 * utterances are unaffected.  A non-finite logit inside one utterance: the call returns and that utterance's outputs
 * stay in range -- frames in [-1, T_b), durations in the set or -1, and either a structurally valid path or the no-path
 * outputs; every other utterance's outputs are bit-identical to those of the same batch without it.
 *
 * The workspace is that of wr_rnnt_tdt_workspace_bytes: the decisions take one byte per cell of its beta region.
 * Refusals, codes and texts are those of wr_rnnt_tdt_loss_fwd under this function's name; a null label_frames or
 * label_durations (with U1max > 1) or a null scores is WR_EINVAL. */
int wr_rnnt_tdt_align(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                      const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank,
                      const int32_t *durations /* [D], host */, int D, double sigma,
                      int32_t *label_frames_d /* [B, U1max-1] out */, int32_t *label_durations_d /* [B, U1max-1] out */,
                      int32_t *blank_jumps_d /* [B, Tmax] out, or NULL */, double *scores_d /* [B] out */,
                      void *workspace_d, size_t workspace_bytes, void *stream);

/* TDT greedy search: the greedy decode of a token-and-duration model, batched, with every decision on the device.  This
 * text is the contract.
 *
 * The handle is a wr_decoder built from the model's own modules, so its vocab_size is the joiner's width V + D: columns
 * [0, V) of a logits row are token logits, columns [V, V + D) duration logits, V = vocab_size - D the token vocabulary.
 * durations[D]: a HOST array with the loss's contract (1 <= D <= 9, values in [0, 8], strictly increasing, at least one
 * >= 1).  enc_out [N, T, E] fp32, enc_lens [N]; T_n = min(enc_lens[n], T).  blank in [0, V).
 *
 * Every stream n follows this loop on its own, starting with t = 0, the predictor stepped on `blank` from a zero state,
 * no label since the last frame advance (nb = 0):
 *   while t < T_n:
 *     k = argmax of the token part, j = argmax of the duration part of the joiner's row for (frame t, predictor state);
 *     d = durations[j]
 *     k == blank:  t += max(d, 1);  nb = 0                                    (the predictor does not step)
 *     otherwise:   k is emitted, at frame t;  the predictor steps on k;  nb = d > 0 ? 0 : nb + 1;  t += d;
 *                  if nb >= n_steps:  t += 1, nb = 0                          (at most n_steps labels without an advance)
 * Ties: both argmaxes are taken on the raw fp32 logits (a log-softmax is monotone within a part) and an exact tie goes to
 * the lowest index, as numpy / torch argmax.  Overshoot: a jump may carry t past T_n; that ends the stream, it is not an
 * error, and a label decided at frame t < T_n is emitted whatever its jump.
 *
 * Out: hyps [N, max_hyp] / hyp_lens [N] as wr_greedy_search (tokens beyond max_hyp are counted in hyp_lens but not
 * stored); hyp_frames [N, max_hyp] or NULL: the frame t at which each stored token was emitted (non-decreasing, < T_n).
 *
 * wr_decoder_set_graph and wr_decoder_set_lookahead apply: with `frames` look-ahead the joiner rows of frames t .. t +
 * frames - 1 are evaluated against one predictor state and walked in frame order by the rule above -- a blank with d = 2
 * consults the row of t + 2 next and never that of t + 1, a blank with d >= frames ends the walk, a label ends it -- so
 * the tokens and frames do not depend on the setting.  frames = 0 means 1 here: the adaptive rule of wr_greedy_search was
 * measured no faster than 1 at 64 streams and slower at one (consecutive frames waste the rows a jump skips).  The durations travel in the state block every call uploads, never
 * in a captured graph: calls with different durations, and wr_greedy_search, may alternate on one handle.
 *
 * Refused before any launch, in this order: D outside [1, 9], a null durations array, a duration outside [0, 8] or not
 * strictly increasing, all durations 0, n_steps < 1, a null enc_out / enc_lens / hyps / hyp_lens, a null handle; then N
 * or T beyond the handle's capacities, V = vocab_size - D < 2, blank outside [0, V), an embedding table (embed_rows) with
 * fewer than V rows (all WR_EINVAL). */
int wr_greedy_search_tdt(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, int N, int T,
                         int n_steps, int blank, const int32_t *durations /* [D], host */, int D,
                         int32_t *hyps_d, int32_t *hyp_lens_d, int32_t *hyp_frames_d /* [N, max_hyp] or NULL */,
                         void *stream);

/* TDT prefix beam search: the prefix beam search of a token-and-duration model, batched, with every decision on the
 * device: n-best lists, the CTC / transducer score mixture, the input of attention rescoring.  This text is the contract.
 *
 * It is the smallest generalisation of wr_prefix_beam_search (one expansion per hypothesis per frame) and time-synchronous
 * as NeMo's TDT beam search is: in a step only the hypotheses standing at the earliest frame are expanded, the others wait
 * and compete with their scores as they are.
 *
 * The handle, the split of a logits row into V token and D duration columns (V = vocab_size - D), durations[D] (HOST) and
 * blank are as for wr_greedy_search_tdt.  enc_out [B, T, E] fp32, enc_lens [B]; T_b = min(enc_lens[b], T).  ctc_logp
 * [B, T, V] = log_softmax(ctc_lo(enc_out)) over the TOKEN vocabulary, or NULL: then (ctc_weight, transducer_weight) must be
 * (0, 1) and nothing is mixed.
 *
 * State, per utterance b: an ordered list (best first) of at most `beam` entries (tokens, t, score, predictor state),
 * starting as one entry ([blank], 0, 0.0, zero state).  Scores are float64.
 * One step, while any entry has t < T_b:
 *   1. f = min t over the entries.  Entries with t == f are ACTIVE, entries with t > f WAIT -- finished ones (t == T_b)
 *      included, which never become active.
 *   2. For each active entry the joiner's row for (frame t, predictor stepped on its last token from its state), fp32:
 *      l = log_softmax(row[0:V]), ld = log_softmax(row[V:V+D]) (the loss's sigma is a training device and is not used);
 *      mix[k] = l[k] without a posterior, else logf(tw * expf(l[k]) + cw * expf(ctc_logp[b, t, k])): the mixture of
 *      wr_prefix_beam_search at the ENTRY's frame.
 *   3. Its candidates: the `beam` best tokens by mix, descending, an exact tie to the lowest index -> ranks r = 0 ..
 *      beam-1; then of the beam x D pairs with value v = mix[k_r] + ld[j] (one fp32 add) the best `beam` by v, descending,
 *      ties to the lower r, then the lower j.  An fp32 add is monotone in each operand, so no pair of a token outside the
 *      first `beam` can precede, under that order, the `beam` pairs its betters form with the same j: this IS the best
 *      `beam` of all V x D pairs.  The candidate's score is (double)((float)score + v): the reference's fp32 add of a
 *      float-cast score, as in wr_prefix_beam_search.
 *   4. Every arc advances: t' = min(t + max(durations[j], 1), T_b).  A blank keeps the tokens and the predictor state, a
 *      label appends k and takes the stepped state.  A label with duration 0 advances one frame like a blank with duration
 *      0 (the reference search's one-symbol-per-frame restriction); its duration probability is kept, and it fuses with
 *      the d = 1 arc of the same label.
 *   5. The pool, in the order of the current beam: a waiting entry itself (unchanged), an active entry's `beam` candidates
 *      in the order of 3.
 *   6. Fusion: candidates with equal tokens AND equal t' are one class (one lattice state); its representative is the first
 *      in pool order and accumulates the others in pool order with float64 log_add.  A waiting entry may fuse with an
 *      expansion.
 *   7. Stable descending sort of the representatives by fused score; the first `beam` are the new beam.
 * f strictly increases, so the search ends after at most T_b steps, when every entry has t == T_b; entries clamped to T_b
 * with equal tokens fuse.  With durations = (1,) every entry is active at the same frame and ld = 0 exactly: the rule is
 * wr_prefix_beam_search on the V token columns.  As there, V >= beam is what the search is built for: with fewer token
 * columns than `beam` the missing candidates appear with value -inf.
 *
 * Out, as wr_prefix_beam_search: hyps [B, beam, Tmax+1] (each begins with the seed blank, padded with -1; a label consumes
 * a frame, so Tmax + 1 suffices), hyp_lens [B, beam], scores [B, beam] float64 (best first), n_hyps [B].
 *
 * The host replays 16 steps, reads back how many utterances still run and stops when none does (jumps make the step count
 * smaller than T); the budget is T + 1 steps.  wr_decoder_set_graph applies (default: replayed from a graph, as the greedy
 * searches that poll); the durations travel in the state block every call uploads, never in a captured graph, so calls
 * with different durations, wr_prefix_beam_search and the greedy searches may alternate on one handle.
 *
 * Refused before any HIP call, in this order (all WR_EINVAL): the duration checks of wr_greedy_search_tdt; a null enc_out /
 * enc_lens / hyps / hyp_lens / scores / n_hyps (ctc_logp may be null); a null handle; beam outside [1, max_beam]; B * beam
 * or T beyond the handle; V = vocab_size - D < 2; blank outside [0, V); an embedding table with fewer than V rows; a null
 * ctc_logp with (ctc_weight, transducer_weight) != (0, 1). */
int wr_prefix_beam_search_tdt(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d,
                              const float *ctc_logp_d /* [B, T, V] or NULL */, int B, int T, int beam, float ctc_weight,
                              float transducer_weight, int blank, const int32_t *durations /* [D], host */, int D,
                              int32_t *hyps_d, int32_t *hyp_lens_d, double *scores_d, int32_t *n_hyps_d, void *stream);

/* Streaming transducer prefix beam search: the prefix beam search of a plain or a token-and-duration transducer continued
 * chunk by chunk, for B streams at once, where every hypothesis carries its summed score, a Viterbi score and the absolute
 * encoder frame at which each of its tokens was emitted, and the current n-best is exported after every chunk.  This text
 * is the contract.  Addition only: WR_API_VERSION stays 3.
 *
 * Search steps.  Steps 1-7 of "TDT prefix beam search" above apply unchanged; the plain search (durations NULL, D = 0) is
 * that rule with durations = (1,) and no duration columns, i.e. wr_prefix_beam_search.  Frames t are absolute, counted
 * from the stream's reset.
 * Viterbi score and times.  Every entry additionally carries vscore (float64, 0.0 at the seed) and times[], one frame per
 * token after the seed blank.  A candidate made from an entry with frame t and pair value v has
 * vscore' = (double)((float)vscore + v), the same fp32 add as the score; its times are the entry's, a label appends t (the
 * frame it was emitted at, not t'), a blank appends nothing.  A waiting entry keeps both.
 * Fusion (step 6).  The class's score is accumulated as before.  Its vscore is the maximum over its members; its times are
 * those of the member holding that maximum, an exact tie going to the first in pool order.  Its tokens, t' and predictor
 * state stay the representative's (all members agree on them).
 * Non-final chunks.  A chunk adds lens[b] = min(chunk_lens[b], T) frames to stream b; F_b is the number of frames received
 * so far.  Steps run while some entry has t < F_b; entries with t >= F_b wait for the next chunk.  In a call not flagged
 * final nothing is clamped: t' = t + max(d, 1).
 * Final chunks.  Before its first step a call flagged final for stream b sets T_b = F_b (after adding its frames), clamps
 * every t > T_b to T_b (a no-op for the plain search), and fuses and stably re-sorts the beam in beam order exactly as a step
 * does; it then steps with t' = min(..., T_b).  A final call with lens[b] = 0 does only the clamp, fuse and sort.  After it
 * the stream accepts nothing until it is reset: whatever chunk_lens says, the device leaves it as it is.
 * Untouched streams.  With lens[b] = 0 and no flag the stream is left untouched.
 *
 * Consequences.  One call with reset and final over a whole utterance gives the hyps, lens, scores and n_hyps of
 * wr_prefix_beam_search (plain) / wr_prefix_beam_search_tdt (durations), bit for bit.  Any chunking of a stream's frames
 * with the final flag on the chunk that holds its last frame equals the one-chunk call in every output: always for the plain
 * search, and for a token-and-duration model whenever that final chunk holds at least max(durations) frames of the stream
 * (or is its first chunk), since then no arc made earlier reaches past the end.  With a shorter final chunk -- a final call
 * of no frames is the extreme -- an arc made before the end was known may stand beyond T_b until the final call clamps it;
 * the result is the rule above and may differ from the whole-utterance search, which clamps at once and so fuses before
 * it prunes.
 *
 * State.  wr_decoder_attach_beam_stream gives the handle a caller-owned block (wr_decoder_beam_stream_workspace_bytes) for
 * max_streams streams of `beam` entries and at most max_frames frames each: the hypotheses, times, lengths, scores and
 * Viterbi scores, with Lcap = max_frames + 1 slots per hypothesis.  The block must stay alive and untouched while the streams
 * run; attaching again replaces it and ends every stream.  wr_decoder_create's signature and workspace are as before.  The
 * predictor state of the entries lives in the handle's lanes: any other search or wr_predictor_step on the handle
 * overwrites it, after which every stream must be reset before its next chunk.
 *
 * The chunk call.  enc_chunk [B, T, E] fp32, chunk_lens [B]; ctc_logp_chunk [B, T, V] as in the whole-utterance searches
 * (required by the plain search; NULL for a token-and-duration model needs weights (0, 1)); durations[D] HOST, or NULL with
 * D = 0 for a plain model; flags HOST int32 [B] or NULL (all 0): bit 0 resets the stream first, bit 1 marks the call final.
 * Out: hyps [B, beam, Lcap] (each begins with the seed blank, padded with -1), times [B, beam, Lcap] (the seed's slot -1,
 * padding -1), hyp_lens [B, beam], scores and vscores [B, beam] float64 (best first by score), n_hyps [B] -- the current
 * n-best of every stream, untouched and finished ones included.  wr_decoder_set_graph applies as to the whole-utterance
 * searches; chunk-dependent values travel in the uploaded state block, never in a captured graph.
 *
 * Refused before any HIP call, in this order (WR_EINVAL): the duration checks of wr_greedy_search_tdt (when durations or D
 * is given); a null enc_chunk / chunk_lens / output pointer; a null handle; no attached stream state; B or beam different
 * from the attached ones; T outside [1, Tmax]; V = vocab_size - D < 2; an embedding table with fewer than V rows; a missing
 * posterior (see above); blank outside [0, V); flag bits beyond 3; then per stream: a reset whose chunk exceeds max_frames;
 * a stream without the reset flag that was never reset, or whose lanes another search has overwritten; a final flag for a
 * stream that has had its final call; chunk widths T summed since the stream's reset exceeding max_frames (counted on the
 * host for every running stream, whatever chunk_lens holds); durations or blank different from those a running stream was
 * started with. */
size_t wr_decoder_beam_stream_workspace_bytes(const wr_decoder *h, int max_streams, int beam, int max_frames);

int wr_decoder_attach_beam_stream(wr_decoder *h, int max_streams, int beam, int max_frames, void *workspace_d,
                                  size_t workspace_bytes);

int wr_prefix_beam_search_chunk(wr_decoder *h, const float *enc_chunk_d, const int32_t *chunk_lens_d,
                                const float *ctc_logp_chunk_d /* [B, T, V] or NULL */, int B, int T, int beam,
                                float ctc_weight, float transducer_weight, int blank,
                                const int32_t *durations /* [D], host; NULL with D = 0: plain */, int D,
                                const int32_t *flags /* [B], host, or NULL */, int32_t *hyps_d, int32_t *times_d,
                                int32_t *hyp_lens_d, double *scores_d, double *vscores_d, int32_t *n_hyps_d, void *stream);

/* Context-graph biasing in the streaming transducer prefix beam search: the search of "Streaming transducer prefix beam
 * search" above, plain or token-and-duration, with the phrase biasing of "Context-graph biasing in the CTC prefix beam
 * search".  The reference runtime drafts it (runtime/core/decoder/rnnt_prefix_beam_search.{h,cc}: a context_graph_ member,
 * a commented-out UpdateOutputs with start / end boundaries, FinalizeSearch() -> UpdateFinalContext()) and does not finish
 * it.  Both contracts hold unchanged; this text states only what is added.  Addition only: WR_API_VERSION stays 3.
 *
 * Graph.  The table of the CTC contract, unchanged: arc_begin[S+1], arc_token[A] strictly increasing within a state,
 * arc_next[A], arc_score[A] float32, escape[S], final[S]; state 0 is the root; next(state, token) as defined there, the
 * token that breaks a partial match not being retried from the root.  For a token-and-duration model the tokens are
 * token-column indices < V = vocab_size - D.  The table must be the same from a stream's reset to its end: that is the
 * caller's responsibility.
 * Per-entry fields.  Every entry of a stream additionally carries ctx_state (int32, 0 at the seed), ctx_score (float64, 0.0
 * at the seed) and tags[], one int32 per token after the seed blank: bit 0 a start boundary at this token, bit 1 an end
 * boundary at this token.  The seed's slot is -1, as for times.
 * Candidates (steps 3-4 of the TDT rule).  A waiting entry and a blank arc copy the three fields of the source entry e.  A
 * label arc appending token k, whatever its duration (0 and jumps beyond 1 included: the graph is walked once per token),
 * takes (st, sc, start, end) = next(e.ctx_state, k) and sets ctx_state = st, ctx_score = e.ctx_score + (double)sc,
 * tags = e.tags + (start | end << 1,).  The candidate's score and vscore are computed exactly as before,
 * (double)((float)score + v): the bonus never enters the fp32 cast, and score stays the pure transducer (or mixed) score.
 * The first prune -- the top-`beam` tokens or pairs of steps 2-3 -- is unbiased, as first_beam is in the CTC search.
 * Fusion (step 6).  Unchanged.  The three fields are a function of the token sequence alone (the table is deterministic and
 * copies keep the state), so all members of a class agree on them; the class takes them from its representative.  Its times
 * still come from the Viterbi-best member.
 * Prune (step 7), and the fuse-and-re-sort a final call does before its first step: a stable descending sort of the
 * representatives by total = fused_score + ctx_score, one float64 add; the first `beam` are the new beam, in that order.
 *
 * Export.  Beside the outputs of wr_prefix_beam_search_chunk: trans_scores [B, beam] float64 (the pure fused score),
 * context_scores [B, beam] float64, tags [B, beam, Lcap] (the seed's slot -1, padded with -1), context_states [B, beam]
 * (the entry's ctx_state as the stream holds it).  scores = trans_scores + context_scores, the add of the prune; vscores
 * stay pure.  Beyond n_hyps[b]: scores and trans_scores -inf, context_scores 0.0, context_states 0.
 * Flag bit 2 (value 4), per stream, exports that stream "as if it ended here" (UpdateFinalContext): every entry with
 * ctx_state != 0 gains (double)escape[ctx_state] in the exported context score, and the exported list of that stream is
 * sorted again, stable and descending, by the new totals.  Tags and the state block are not touched, and the stream goes
 * on.  Bit 2 is independent of bit 1, the final flag: bit 1 ends the stream's frames and clamps arcs, bit 2 is about the
 * exported bonus only.  A call with lens[b] == 0 and only bit 2 for stream b steps nothing and exports it finalised (its
 * chunk width T still counts against max_frames on the host, as every call's does).
 *
 * Consequences.  With an empty graph (S = 1, A = 0) every output of wr_prefix_beam_search_chunk is reproduced bit for bit;
 * tags are all 0 and context scores all 0.0.  With a graph whose arc scores are all 0.0 the same outputs are bit for bit,
 * but tags are set: the graph is still walked.  Any chunking equals the one-chunk call bit for bit in all outputs, under the
 * existing condition for token-and-duration streams.  Bit 2 in the middle of a stream does not change what later chunks
 * return.
 * Departures, as for the CTC form: the bonus is summed in float64, and nested phrases commit at the shorter phrase's last
 * token (the table is whatever the caller built).
 *
 * State.  wr_decoder_attach_beam_context_stream gives the handle a block of the biased form's own layout
 * (wr_decoder_beam_context_stream_workspace_bytes): the plain block's contents, then ctx_score, ctx_state and a
 * double-buffered int32 [2][B * beam][Lcap] tag list -- larger than the plain block for every shape.  The plain size query,
 * attach and layout are unchanged.  Attaching one form replaces the other and ends every stream; a plain chunk call cannot
 * continue a biased stream or the reverse.  As for the plain streams, any other search or wr_predictor_step on the handle
 * in between means every stream must be reset.
 *
 * The chunk call takes the arguments of wr_prefix_beam_search_chunk up to n_hyps, then the six table pointers (device), S,
 * A, the four new outputs, and the stream.  The table pointers, S, A and the flags travel in the uploaded state block, never
 * in a captured graph.  The kernels clamp every arc_next into [0, S), every CSR bound into [0, A] and every stored
 * ctx_state into [0, S) before use as an index: a bad table gives wrong bonuses, never an out-of-range access.
 *
 * Refused before any HIP call, in this order: everything wr_prefix_beam_search_chunk refuses, in its order ("no attached
 * stream state" means the biased form's; a null among the four new outputs counts with the null outputs; flag bits beyond
 * 7 instead of beyond 3); S < 1 or A < 0, then a null table pointer (WR_EINVAL); S > 65536 or A > 1048576
 * (WR_EUNSUPPORTED).  wr_prefix_beam_search_chunk itself keeps refusing flag bits beyond 3. */
size_t wr_decoder_beam_context_stream_workspace_bytes(const wr_decoder *h, int max_streams, int beam, int max_frames);

int wr_decoder_attach_beam_context_stream(wr_decoder *h, int max_streams, int beam, int max_frames, void *workspace_d,
                                          size_t workspace_bytes);

int wr_prefix_beam_search_context_chunk(wr_decoder *h, const float *enc_chunk_d, const int32_t *chunk_lens_d,
                                        const float *ctc_logp_chunk_d /* [B, T, V] or NULL */, int B, int T, int beam,
                                        float ctc_weight, float transducer_weight, int blank,
                                        const int32_t *durations /* [D], host; NULL with D = 0: plain */, int D,
                                        const int32_t *flags /* [B], host, or NULL */, int32_t *hyps_d, int32_t *times_d,
                                        int32_t *hyp_lens_d, double *scores_d, double *vscores_d, int32_t *n_hyps_d,
                                        const int32_t *arc_begin_d, const int32_t *arc_token_d, const int32_t *arc_next_d,
                                        const float *arc_score_d, const float *escape_d, const int32_t *final_d, int S, int A,
                                        double *trans_scores_d, double *context_scores_d, int32_t *tags_d,
                                        int32_t *context_states_d, void *stream);

/* Measurement hook: the three counters the last polling search on this handle read back (host memory, no HIP call).
 * Greedy searches: streams still active, blank decisions, emissions.  wr_prefix_beam_search_tdt: utterances still running
 * (0 after a successful call), steps taken summed over the utterances, hypotheses expanded. */
int wr_decoder_last_counters(const wr_decoder *h, int32_t *out /* [3], host */);

/* CTC forced alignment: Viterbi over the T x (2S+1) lattice, replacing
 * forced_align, wenet/utils/ctc_util.py:27-83 (CLI wenet/bin/alignment.py:215).  logits [B, Tmax, V]: pre-softmax
 * ctc_lo output, or log-posteriors if normalized != 0 (the reference is handed ctc.log_softmax(...)).
 * alignment [B, Tmax]: the token (blank or label) aligned to each frame, -1 past input_lengths[b].
 * fp32 scores and first-candidate tie rule as the reference; Smax >= 1.  An utterance with target_lengths[b] <= 0
 * has the one all-blank path: alignment[b, t] = blank for t < input_lengths[b], whatever targets[b] holds. */
size_t wr_ctc_align_workspace_bytes(int B, int Tmax, int Smax);

int wr_ctc_forced_align(const float *logits_d, int normalized, const int32_t *targets_d,
                        const int32_t *input_lengths_d, const int32_t *target_lengths_d,
                        int B, int Tmax, int Smax, int V, int blank, int32_t *alignment_d,
                        void *workspace_d, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* WR_API_H_ */
