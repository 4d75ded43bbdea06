// Token-and-duration transducer (TDT) loss and forced alignment: the entry points (include/wr_api.h, "Token-and-duration
// transducer", "TDT forced alignment", "Joiner + TDT loss without a logits tensor").  Host
// code only: every argument is checked here, before the first HIP call; the kernels and their launches are in
// rnnt_lattice.hip and, for the joiner's TDT epilogues, joint.hip (rnnt_tdt.hpp).
#include "rnnt_tdt.hpp"

namespace wr {
namespace {

int tdt_shape(const char *what, int B, int T, int U1, int D)
{
    WR_REQUIRE(B > 0 && T > 0 && U1 > 0, WR_EINVAL, "%s: B, T, U1 must be positive (got %d,%d,%d)", what, B, T, U1);
    WR_REQUIRE(D >= 1 && D <= kTdtMaxD, WR_EINVAL, "%s: D=%d durations (1 to %d are supported)", what, D, kTdtMaxD);
    WR_REQUIRE(U1 <= kRnntMaxCols, WR_EUNSUPPORTED, "%s: U1=%d exceeds the sweep kernel's limit of %d label columns", what,
               U1, kRnntMaxCols);
    WR_REQUIRE((long)B * (T + U1 - 1) * U1 < (1L << 31), WR_EUNSUPPORTED, "%s: more than 2^31 lattice positions", what);
    return WR_OK;
}

// everything wr_rnnt_tdt_loss_fwd and _bwd check alike, up to the workspace size
int tdt_check(const char *what, int dtype, int B, int T, int U1, int V, int blank, const int32_t *durations, int D,
              double sigma, size_t workspace_bytes, TdtDur *dur)
{
    WR_REQUIRE(B > 0 && T > 0 && U1 > 0 && V > 0, WR_EINVAL, "%s: B, T, U1, V must be positive (got %d,%d,%d,%d)", what, B,
               T, U1, V);
    WR_REQUIRE(dtype == WR_F32 || dtype == WR_F16 || dtype == WR_BF16, WR_EINVAL, "%s: unknown dtype %d", what, dtype);
    WR_TRY(tdt_durations(what, durations, D, dur));
    WR_REQUIRE(sigma >= 0.0 && sigma < (double)__builtin_huge_valf(), WR_EINVAL,
               "%s: sigma %g must be finite and not negative", what, sigma);
    WR_REQUIRE(blank >= 0 && blank < V, WR_EINVAL, "%s: blank %d out of range [0,%d)", what, blank, V);
    WR_TRY(tdt_shape(what, B, T, U1, D));
    const size_t need = tdt_ws_layout(B, T, U1, D).total;
    WR_REQUIRE(workspace_bytes >= need, WR_EWORKSPACE, "%s: workspace %zu < required %zu", what, workspace_bytes, need);
    return WR_OK;
}

// everything wr_joint_tdt_stats and wr_joint_tdt_grad check alike before the joiner's own refusals (joint_tdt_epi): the
// TDT contract in tdt_check's order, on a joiner of width W = V + D
int joint_tdt_check(const char *what, const void *ep_d, const void *pp_d, const void *w_out_d, const void *b_out_d,
                    const void *logit_lengths_d, const void *target_lengths_d, const void *targets_d, int B, int T, int U1,
                    int J, int W, int blank, const int32_t *durations, int D, double sigma, const void *workspace_d,
                    const void *tdt_workspace_d, size_t tdt_workspace_bytes, TdtDur *dur)
{
    WR_REQUIRE(B > 0 && T > 0 && U1 > 0 && J > 0 && W > 0, WR_EINVAL, "%s: B, T, U1, J, W must be positive (got %d,%d,%d,%d,%d)",
               what, B, T, U1, J, W);
    WR_TRY(tdt_durations(what, durations, D, dur));
    WR_REQUIRE(W - D >= 2, WR_EINVAL, "%s: a joiner of W=%d outputs with D=%d durations has V = W - D = %d token columns (at "
               "least 2 are needed)", what, W, D, W - D);
    WR_REQUIRE(blank >= 0 && blank < W - D, WR_EINVAL, "%s: blank %d out of range [0,%d)", what, blank, W - D);
    WR_REQUIRE(sigma >= 0.0 && sigma < (double)__builtin_huge_valf(), WR_EINVAL,
               "%s: sigma %g must be finite and not negative", what, sigma);
    WR_REQUIRE(ep_d && pp_d && w_out_d && b_out_d && logit_lengths_d && target_lengths_d && workspace_d && tdt_workspace_d &&
                   (targets_d || U1 == 1),
               WR_EINVAL, "%s: null pointer argument", what);
    WR_TRY(tdt_shape(what, B, T, U1, D));
    const size_t need = tdt_ws_layout(B, T, U1, D).total;
    WR_REQUIRE(tdt_workspace_bytes >= need, WR_EWORKSPACE, "%s: TDT workspace %zu < required %zu", what, tdt_workspace_bytes,
               need);
    return WR_OK;
}

}  // namespace
}  // namespace wr

using namespace wr;

extern "C" size_t wr_rnnt_tdt_workspace_bytes(int B, int Tmax, int U1max, int D)
{
    if (B <= 0 || Tmax <= 0 || U1max <= 0 || D < 1 || D > kTdtMaxD) return 0;
    return tdt_ws_layout(B, Tmax, U1max, D).total;
}

extern "C" int wr_rnnt_tdt_loss_fwd(const void *logits_d, int dtype, const int32_t *targets_d,
                                    const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax,
                                    int U1max, int V, int blank, const int32_t *durations, int D, double sigma,
                                    float *costs_d, void *workspace_d, size_t workspace_bytes, void *stream)
{
    TdtDur dur;
    WR_TRY(tdt_check("rnnt_tdt_loss_fwd", dtype, B, Tmax, U1max, V, blank, durations, D, sigma, workspace_bytes, &dur));
    WR_REQUIRE(logits_d && logit_lengths_d && target_lengths_d && costs_d && workspace_d && (targets_d || U1max == 1),
               WR_EINVAL, "rnnt_tdt_loss_fwd: null pointer argument");
    return tdt_loss_fwd_body(logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V, blank, dur,
                             sigma, costs_d, workspace_d, static_cast<hipStream_t>(stream));
}

extern "C" int wr_rnnt_tdt_loss_bwd(const void *logits_d, int dtype, const int32_t *targets_d,
                                    const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax,
                                    int U1max, int V, int blank, const int32_t *durations, int D, double sigma,
                                    const float *grad_costs_d, void *grads_d, const void *workspace_d,
                                    size_t workspace_bytes, void *stream)
{
    TdtDur dur;
    WR_TRY(tdt_check("rnnt_tdt_loss_bwd", dtype, B, Tmax, U1max, V, blank, durations, D, sigma, workspace_bytes, &dur));
    WR_REQUIRE(logits_d && logit_lengths_d && target_lengths_d && grads_d && workspace_d && (targets_d || U1max == 1),
               WR_EINVAL, "rnnt_tdt_loss_bwd: null pointer argument");
    WR_REQUIRE(((reinterpret_cast<uintptr_t>(logits_d) ^ reinterpret_cast<uintptr_t>(grads_d)) & 15) == 0, WR_EINVAL,
               "rnnt_tdt_loss_bwd: logits and grads must sit at the same offset within a 16-byte line");
    return tdt_loss_bwd_body(logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V, blank, D,
                             grad_costs_d, grads_d, workspace_d, static_cast<hipStream_t>(stream));
}

extern "C" int wr_rnnt_tdt_align(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                                 const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank,
                                 const int32_t *durations, int D, double sigma, int32_t *label_frames_d,
                                 int32_t *label_durations_d, int32_t *blank_jumps_d, double *scores_d, void *workspace_d,
                                 size_t workspace_bytes, void *stream)
{
    TdtDur dur;
    WR_TRY(tdt_check("rnnt_tdt_align", dtype, B, Tmax, U1max, V, blank, durations, D, sigma, workspace_bytes, &dur));
    WR_REQUIRE(logits_d && logit_lengths_d && target_lengths_d && workspace_d && (targets_d || U1max == 1), WR_EINVAL,
               "rnnt_tdt_align: null pointer argument");
    WR_REQUIRE(scores_d && ((label_frames_d && label_durations_d) || U1max == 1), WR_EINVAL,
               "rnnt_tdt_align: label_frames, label_durations or scores is null");
    return tdt_align_body(logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V, blank, dur,
                          sigma, label_frames_d, label_durations_d, blank_jumps_d, scores_d, workspace_d,
                          static_cast<hipStream_t>(stream));
}

extern "C" int wr_rnnt_tdt_export_lattice(const void *workspace_d, size_t workspace_bytes, const int32_t *logit_lengths_d,
                                          const int32_t *target_lengths_d, int B, int Tmax, int U1max, int D,
                                          float *alpha_d, float *beta_d, void *stream)
{
    WR_TRY(tdt_shape("rnnt_tdt_export_lattice", B, Tmax, U1max, D));
    const size_t need = tdt_ws_layout(B, Tmax, U1max, D).total;
    WR_REQUIRE(workspace_bytes >= need, WR_EWORKSPACE, "rnnt_tdt_export_lattice: workspace %zu < required %zu",
               workspace_bytes, need);
    WR_REQUIRE(workspace_d && logit_lengths_d && target_lengths_d && alpha_d && beta_d, WR_EINVAL,
               "rnnt_tdt_export_lattice: null pointer argument");
    return tdt_export_body(workspace_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, D, alpha_d, beta_d,
                           static_cast<hipStream_t>(stream));
}

extern "C" int wr_joint_tdt_stats(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                                  const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d,
                                  int B, int T, int U1, int J, int W, int activation, int blank, const int32_t *durations,
                                  int D, double sigma, void *workspace_d, size_t workspace_bytes, void *tdt_workspace_d,
                                  size_t tdt_workspace_bytes, void *stream)
{
    TdtDur dur;
    WR_TRY(joint_tdt_check("joint_tdt_stats", ep_d, pp_d, w_out_d, b_out_d, logit_lengths_d, target_lengths_d, targets_d, B, T,
                           U1, J, W, blank, durations, D, sigma, workspace_d, tdt_workspace_d, tdt_workspace_bytes, &dur));
    return joint_tdt_epi("joint_tdt_stats", false, ep_d, pp_d, w_out_d, b_out_d, logit_lengths_d, target_lengths_d, targets_d, B,
                         T, U1, J, W, activation, blank, D, (float)sigma, nullptr, tdt_workspace_d, 0, 0, nullptr, workspace_d,
                         workspace_bytes, false, static_cast<hipStream_t>(stream));
}

extern "C" int wr_rnnt_tdt_sweeps(const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                                  const int32_t *durations, int D, float *costs_d, void *workspace_d, size_t workspace_bytes,
                                  void *stream)
{
    TdtDur dur;
    WR_REQUIRE(B > 0 && Tmax > 0 && U1max > 0, WR_EINVAL, "rnnt_tdt_sweeps: B, T, U1 must be positive (got %d,%d,%d)", B, Tmax,
               U1max);
    WR_TRY(tdt_durations("rnnt_tdt_sweeps", durations, D, &dur));
    WR_TRY(tdt_shape("rnnt_tdt_sweeps", B, Tmax, U1max, D));
    const size_t need = tdt_ws_layout(B, Tmax, U1max, D).total;
    WR_REQUIRE(workspace_bytes >= need, WR_EWORKSPACE, "rnnt_tdt_sweeps: workspace %zu < required %zu", workspace_bytes, need);
    WR_REQUIRE(logit_lengths_d && target_lengths_d && costs_d && workspace_d, WR_EINVAL,
               "rnnt_tdt_sweeps: null pointer argument");
    return tdt_sweeps_body(logit_lengths_d, target_lengths_d, B, Tmax, U1max, dur, costs_d, workspace_d,
                           static_cast<hipStream_t>(stream));
}

extern "C" int wr_joint_tdt_grad(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                                 const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d,
                                 int B, int T, int U1, int J, int W, int activation, int blank, const int32_t *durations, int D,
                                 double sigma, const float *grad_costs_d, const void *tdt_workspace_d,
                                 size_t tdt_workspace_bytes, long long cell_begin, long long cell_end, float *g_out_d,
                                 void *workspace_d, size_t workspace_bytes, int w_ready, void *stream)
{
    TdtDur dur;
    WR_TRY(joint_tdt_check("joint_tdt_grad", ep_d, pp_d, w_out_d, b_out_d, logit_lengths_d, target_lengths_d, targets_d, B, T, U1,
                           J, W, blank, durations, D, sigma, workspace_d, tdt_workspace_d, tdt_workspace_bytes, &dur));
    WR_REQUIRE(g_out_d, WR_EINVAL, "joint_tdt_grad: null pointer argument");
    WR_REQUIRE(0 <= cell_begin && cell_begin < cell_end && cell_end <= (long long)B * T * U1, WR_EINVAL,
               "joint_tdt_grad: cell range [%lld, %lld) outside [0, %lld)", cell_begin, cell_end, (long long)B * T * U1);
    return joint_tdt_epi("joint_tdt_grad", true, ep_d, pp_d, w_out_d, b_out_d, logit_lengths_d, target_lengths_d, targets_d, B, T,
                         U1, J, W, activation, blank, D, (float)sigma, grad_costs_d, const_cast<void *>(tdt_workspace_d),
                         (long)cell_begin, (long)cell_end, g_out_d, workspace_d, workspace_bytes, w_ready != 0,
                         static_cast<hipStream_t>(stream));
}
