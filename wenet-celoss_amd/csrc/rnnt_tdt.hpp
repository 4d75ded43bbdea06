// Token-and-duration transducer (TDT) loss: what the entry points of rnnt_tdt.cpp share with the kernels of
// rnnt_lattice.hip (include/wr_api.h, "Token-and-duration transducer").
//
// A TDT workspace holds, per utterance b, S = Tmax + U1max - 1 anti-diagonals of U1max cells (cell (t,u) at element
// (t + u) * U1max + u, as the regular lattice stores its arcs) and plain [b][t][u] rows:
//   tok     float2 {tok_blank, tok_label}   anti-diagonal    log-softmax over the V token columns, - sigma
//   dur     float[D]                        anti-diagonal    log-softmax over the D duration columns
//   alpha   double                          anti-diagonal
//   beta    double                          anti-diagonal    (alignment: one decision byte per cell in its first eighth)
//   denom   float                           plain            log-sum-exp of the token columns
//   rec     float[3 + D]                    plain            the gradient's row constants (tdt_record_kernel)
//   ll, cost  double[B];  dump  double[B][2][kRnntMaxCols]   (absorbs the stores of idle sweep lanes)
//   flag    int32                                            a partial sum of the joiner's statistics epilogue overflowed
//                                                            (wr_joint_tdt_stats; joint_lse.hpp has the protocol)
#pragma once

#include "wr_common.hpp"

namespace wr {

constexpr int kTdtMaxDur = 8;                 // largest frame jump of one arc
constexpr int kTdtMaxD = kTdtMaxDur + 1;      // number of durations: strictly increasing values in [0, 8]
constexpr int kTdtRec = 3;                    // record: {log O - denom, Ob, Ol}, then D per-duration values

// which durations exist, by jump: slot[d] = index n with durations[n] == d, or -1.  Passed to the kernels by value, so a
// loop unrolled over d = 0 .. 8 tests wave-uniform scalars.
struct TdtDur {
    int slot[kTdtMaxD];
    int D;
};

// The durations contract of every TDT entry point (the loss here, wr_greedy_search_tdt in decode_tdt.cpp): WR_OK and the
// table of jumps, or the error of a duration set the lattice does not have.  Host code, no HIP call.
inline int tdt_durations(const char *what, const int32_t *durations, int D, TdtDur *out)
{
    WR_REQUIRE(D >= 1 && D <= kTdtMaxD, WR_EINVAL, "%s: D=%d durations (1 to %d are supported)", what, D, kTdtMaxD);
    WR_REQUIRE(durations != nullptr, WR_EINVAL, "%s: durations is null", what);
    for (int d = 0; d < kTdtMaxD; ++d) out->slot[d] = -1;
    out->D = D;
    for (int n = 0; n < D; ++n) {
        WR_REQUIRE(durations[n] >= 0 && durations[n] <= kTdtMaxDur, WR_EINVAL,
                   "%s: durations[%d]=%d lies outside [0, %d]", what, n, durations[n], kTdtMaxDur);
        WR_REQUIRE(n == 0 || durations[n] > durations[n - 1], WR_EINVAL,
                   "%s: durations must be strictly increasing (durations[%d]=%d after %d)", what, n, durations[n],
                   durations[n - 1]);
        out->slot[durations[n]] = n;
    }
    WR_REQUIRE(durations[D - 1] >= 1, WR_EINVAL, "%s: at least one duration must be 1 or more (no arc would consume a frame)",
               what);
    return WR_OK;
}

struct TdtWs {
    int K;            // waves of a sweep workgroup
    int S;            // anti-diagonals per utterance
    size_t tok_off, dur_off, alpha_off, beta_off, denom_off, rec_off, ll_off, cost_off, dump_off, flag_off, total;
};

inline TdtWs tdt_ws_layout(int B, int Tmax, int U1max, int D)
{
    TdtWs w;
    w.K = rnnt_cols_per_lane(U1max);
    w.S = Tmax + U1max - 1;
    const size_t diag = (size_t)B * w.S * U1max;
    const size_t cells = (size_t)B * Tmax * U1max;
    size_t off = 0;
    w.tok_off = off;   off = align_up(off + diag * sizeof(float2), 256);
    w.dur_off = off;   off = align_up(off + diag * D * sizeof(float), 256);
    w.alpha_off = off; off = align_up(off + diag * sizeof(double), 256);
    w.beta_off = off;  off = align_up(off + diag * sizeof(double), 256);
    w.denom_off = off; off = align_up(off + cells * sizeof(float), 256);
    w.rec_off = off;   off = align_up(off + cells * (kTdtRec + D) * sizeof(float), 256);
    w.ll_off = off;    off = align_up(off + (size_t)B * sizeof(double), 256);
    w.cost_off = off;  off = align_up(off + (size_t)B * sizeof(double), 256);
    w.dump_off = off;  off = align_up(off + (size_t)B * 2 * kRnntMaxCols * sizeof(double), 256);
    w.flag_off = off;  off = align_up(off + sizeof(int32_t), 256);
    w.total = off;
    return w;
}

// rnnt_lattice.hip: the launches behind the entry points of rnnt_tdt.cpp, which has checked every argument.
// Forward: row statistics, both sweeps, the per-cell records.  Backward: the streamed gradient.
int tdt_loss_fwd_body(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                      const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank, const TdtDur &dur,
                      double sigma, float *costs_d, void *workspace_d, hipStream_t st);
// Both sweeps and the per-cell records over a workspace whose row statistics (tok, dur, denom) are in place: the tail of
// tdt_loss_fwd_body, and all of wr_rnnt_tdt_sweeps.
int tdt_sweeps_body(const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                    const TdtDur &dur, float *costs_d, void *workspace_d, hipStream_t st);
int tdt_loss_bwd_body(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                      const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank, int D,
                      const float *grad_costs_d, void *grads_d, const void *workspace_d, hipStream_t st);
int tdt_export_body(const void *workspace_d, const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B,
                    int Tmax, int U1max, int D, float *alpha_d, float *beta_d, hipStream_t st);
// Forced alignment: row statistics, then the Viterbi sweep and its backtrace (one decision byte per cell in `beta`).
int tdt_align_body(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                   const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank, const TdtDur &dur,
                   double sigma, int32_t *label_frames_d, int32_t *label_durations_d, int32_t *blank_jumps_d,
                   double *scores_d, void *workspace_d, hipStream_t st);

// joint.hip: the joiner forward with the TDT statistics (grad = false) or gradient (cells [cell_begin, cell_end) into
// g_out_d) epilogue over the TDT workspace `tws`, for wr_joint_tdt_stats / wr_joint_tdt_grad.  Refuses what the joiner
// refuses (join_dim, activation, its workspace, the direct forward kernel) before any launch.
int joint_tdt_epi(const char *what, bool grad, const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                  const int32_t *llens, const int32_t *tlens, const int32_t *targets_d, int B, int T, int U1, int J, int W,
                  int act, int blank, int D, float sigma, const float *grad_costs_d, void *tws, long cell_begin, long cell_end,
                  float *g_out_d, void *workspace_d, size_t workspace_bytes, bool w_ready, hipStream_t st);

}  // namespace wr
