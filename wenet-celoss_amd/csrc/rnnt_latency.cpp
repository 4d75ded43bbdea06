// FastEmit and the delay penalty for the full-lattice RNN-T loss: the `*_lattice` forms of wr_rnnt_loss_fwd,
// wr_rnnt_loss_fwd_from_lse, wr_rnnt_loss_bwd and wr_joint_rnnt_grad (include/wr_api.h, "FastEmit and the delay penalty
// for the full-lattice loss").  Host code only: each checks its regularisers and runs the body of the plain entry point
// (rnnt_loss.hip, joint.hip), which with both at 0 launches exactly what the plain entry point launches.
#include <math.h>

#include "rnnt_latency.hpp"

namespace wr {
namespace {

// WR_OK and `*reg` (use = either regulariser is above 0), or the error of a value the family does not have.  With a
// penalty the prepare kernel indexes B * (T + U1 - 1) * U1 positions, which is checked here, before pass 1 is launched.
int latency_check(const char *what, int lattice_type, double delay_penalty, double fastemit_lambda, int B, int T, int U1,
                  RnntReg *reg, bool *use)
{
    if (int rc = lattice_check(what, lattice_type, delay_penalty)) return rc;
    WR_REQUIRE(fastemit_lambda >= 0.0 && fastemit_lambda < (double)__builtin_huge_valf(), WR_EINVAL,
               "%s: fastemit_lambda %g must be finite and not negative", what, fastemit_lambda);
    WR_REQUIRE(lattice_type == WR_LATTICE_REGULAR, WR_EUNSUPPORTED,
               "%s: the full-lattice loss has the regular lattice only (lattice type %d)", what, lattice_type);
    WR_REQUIRE(!(delay_penalty > 0.0) || B <= 0 || T <= 0 || U1 <= 0 || (long)B * (T + U1 - 1) * U1 < (1L << 31),
               WR_EUNSUPPORTED, "%s: more than 2^31 lattice positions", what);
    reg->delay_penalty = delay_penalty;
    reg->log_lambda = fastemit_lambda > 0.0 ? log(fastemit_lambda) : -(double)__builtin_huge_valf();
    reg->log1p_lambda = log1p(fastemit_lambda);
    *use = delay_penalty > 0.0 || fastemit_lambda > 0.0;
    return WR_OK;
}

}  // namespace
}  // namespace wr

using namespace wr;

extern "C" int wr_rnnt_loss_fwd_lattice(const void *logits_d, int dtype, const int32_t *targets_d,
                                        const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax,
                                        int U1max, int V, int blank, int lattice_type, double delay_penalty, float *costs_d,
                                        void *workspace_d, size_t workspace_bytes, void *stream)
{
    RnntReg reg;
    bool use;
    WR_TRY(latency_check("rnnt_loss_fwd_lattice", lattice_type, delay_penalty, 0.0, B, Tmax, U1max, &reg, &use));
    return rnnt_loss_fwd_body("rnnt_loss_fwd_lattice", logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax,
                              U1max, V, blank, delay_penalty, costs_d, workspace_d, workspace_bytes, stream);
}

extern "C" int wr_rnnt_loss_fwd_from_lse_lattice(const float *logits_d, const int32_t *targets_d,
                                                 const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B,
                                                 int Tmax, int U1max, int V, int blank, int lattice_type,
                                                 double delay_penalty, float *costs_d, void *workspace_d,
                                                 size_t workspace_bytes, void *stream)
{
    RnntReg reg;
    bool use;
    WR_TRY(latency_check("rnnt_loss_fwd_from_lse_lattice", lattice_type, delay_penalty, 0.0, B, Tmax, U1max, &reg, &use));
    return rnnt_loss_fwd_from_lse_body("rnnt_loss_fwd_from_lse_lattice", logits_d, targets_d, logit_lengths_d, target_lengths_d,
                                       B, Tmax, U1max, V, blank, delay_penalty, costs_d, workspace_d, workspace_bytes, stream);
}

extern "C" int wr_rnnt_loss_bwd_lattice(const void *logits_d, int dtype, const int32_t *targets_d,
                                        const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax,
                                        int U1max, int V, int blank, float clamp, int lattice_type, double delay_penalty,
                                        double fastemit_lambda, const float *grad_costs_d, void *grads_d,
                                        const void *workspace_d, size_t workspace_bytes, void *stream)
{
    RnntReg reg;
    bool use;
    WR_TRY(latency_check("rnnt_loss_bwd_lattice", lattice_type, delay_penalty, fastemit_lambda, B, Tmax, U1max, &reg, &use));
    return rnnt_loss_bwd_body("rnnt_loss_bwd_lattice", logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax,
                              U1max, V, blank, clamp, grad_costs_d, grads_d, workspace_d, workspace_bytes, use ? &reg : nullptr,
                              stream);
}

extern "C" int wr_joint_rnnt_grad_lattice(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                                          const int32_t *logit_lengths_d, const int32_t *target_lengths_d,
                                          const int32_t *targets_d, int B, int T, int U1, int J, int V, int activation,
                                          int blank, float clamp, int terms, int lattice_type, double delay_penalty,
                                          double fastemit_lambda, const float *grad_costs_d, const void *rnnt_workspace_d,
                                          size_t rnnt_workspace_bytes, long long cell_begin, long long cell_end,
                                          float *g_out_d, void *workspace_d, size_t workspace_bytes, int w_ready, void *stream)
{
    RnntReg reg;
    bool use;
    WR_TRY(latency_check("joint_rnnt_grad_lattice", lattice_type, delay_penalty, fastemit_lambda, B, T, U1, &reg, &use));
    return joint_rnnt_grad_body("joint_rnnt_grad_lattice", ep_d, pp_d, w_out_d, b_out_d, logit_lengths_d, target_lengths_d,
                                targets_d, B, T, U1, J, V, activation, blank, clamp, terms, grad_costs_d, rnnt_workspace_d,
                                rnnt_workspace_bytes, cell_begin, cell_end, g_out_d, workspace_d, workspace_bytes, w_ready,
                                use ? &reg : nullptr, stream);
}
