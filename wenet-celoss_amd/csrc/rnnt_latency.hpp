// FastEmit and the delay penalty for the full-lattice RNN-T loss (include/wr_api.h, "FastEmit and the delay penalty for
// the full-lattice loss"): what the entry points of rnnt_latency.cpp share with the kernels' files.
//
// Both regularisers live in the per-row constants of the three gradient producers (rnnt_grad_kernel in rnnt_loss.hip,
// joint_epi_rows_init in joint_lse.hpp, which the bounded node runs per slice); the delay penalty is also inside the
// stored label arcs, where wr_rnnt_lattice_sweeps puts it before the unchanged sweeps.
#pragma once

#include "rnnt_lattice.hpp"
#include "wr_common.hpp"

namespace wr {

// The regularisers as the kernels take them.  log_lambda = log(fastemit_lambda), -inf for 0 (no FastEmit term is formed);
// log1p_lambda = log1p(fastemit_lambda).  The defaults are the plain loss.
struct RnntReg {
    double delay_penalty = 0.0;
    double log_lambda = -__builtin_huge_val();
    double log1p_lambda = 0.0;
};

// what the regularised instantiation of rnnt_grad_kernel takes as its one extra argument
struct RnntRegArgs {
    const float2 *lp_skew;     // [B, S, U1] {skip, emit'}: the stored arcs, penalised by wr_rnnt_lattice_sweeps
    RnntReg reg;
};
template <typename A>
__device__ __forceinline__ const A &only_arg(const A &a) { return a; }

// log(exp(a) + exp(b)) in fp64.  A NaN operand gives NaN (fmax alone would drop it); -inf operands are exact.
__device__ __forceinline__ double log_add_d(double a, double b)
{
    if (a == b) return a + 0.69314718055994530942;       // also both -inf
    return fmax(a, b) + log1p(exp(-fabs(a - b)));
}

// rnnt_loss.hip: the bodies of wr_rnnt_loss_fwd / _fwd_from_lse / _bwd under the name `what`; delay_penalty > 0 runs
// wr_rnnt_lattice_sweeps instead of the plain sweeps, reg != nullptr the regularised gradient instantiation.
int rnnt_loss_fwd_body(const char *what, const void *logits_d, int dtype, const int32_t *targets_d,
                       const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V,
                       int blank, double delay_penalty, float *costs_d, void *workspace_d, size_t workspace_bytes,
                       void *stream);
int rnnt_loss_fwd_from_lse_body(const char *what, const float *logits_d, const int32_t *targets_d,
                                const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                                int V, int blank, double delay_penalty, float *costs_d, void *workspace_d,
                                size_t workspace_bytes, void *stream);
int rnnt_loss_bwd_body(const char *what, const void *logits_d, int dtype, const int32_t *targets_d,
                       const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V,
                       int blank, float clamp, const float *grad_costs_d, void *grads_d, const void *workspace_d,
                       size_t workspace_bytes, const RnntReg *reg, void *stream);

// joint.hip: the body of wr_joint_rnnt_grad; reg != nullptr runs the kEpiGradReg epilogue
int joint_rnnt_grad_body(const char *what, const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                         const int32_t *logit_lengths_d, const int32_t *target_lengths_d, const int32_t *targets_d, int B,
                         int T, int U1, int J, int V, int activation, int blank, float clamp, int terms,
                         const float *grad_costs_d, const void *rnnt_workspace_d, size_t rnnt_workspace_bytes,
                         long long cell_begin, long long cell_end, float *g_out_d, void *workspace_d, size_t workspace_bytes,
                         int w_ready, const RnntReg *reg, void *stream);

}  // namespace wr
