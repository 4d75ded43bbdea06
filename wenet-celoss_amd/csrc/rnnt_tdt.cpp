// Token-and-duration transducer (TDT) loss and forced alignment: the entry points (include/wr_api.h, "Token-and-duration
// transducer", "TDT forced alignment").  Host
// code only: every argument is checked here, before the first HIP call; the kernels and their launches are in
// rnnt_lattice.hip (rnnt_tdt.hpp).
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
