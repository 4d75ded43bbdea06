// Row statistics of the RNN-T loss as an epilogue of the joiner forward kernels (joint.hip, joint_split.hip).
//
// A forward workgroup owns 64 lattice cells and ALL V columns of their logits, so it can produce what pass 1 of
// the loss (rnnt_lse_kernel: one more read of the 96.6 GB logits tensor at the BASELINE shape) would compute from
// them: denom(t,u) = logsumexp_v logits, skip = logit[blank] - denom, emit = logit[y_u] - denom -- written straight
// into the RNN-T workspace layout (RnntWs: denom row-major, {skip, emit} skewed by anti-diagonal).  The loss then
// only runs its lattice sweeps (wr_rnnt_loss_fwd_from_lse).  Reference call sites fused here:
// wenet/transducer/transducer.py:132 (joint) and the first pass of :142-147 (rnnt_loss).
//
// Mechanics: in the MFMA C/D layout a lane holds, per 32-column tile, ONE column of 32 rows (2 row tiles x 16
// registers).  The kernels are matrix-core bound and their epilogue does not overlap with the MFMAs of the same
// wave, so the per-logit work is kept to four instructions: each lane keeps, per row, a partial sum
//     s = sum over the columns it has seen of 2^(x*log2e - ref),     ref = the first such x*log2e,
// with no running maximum and no rescaling (an online max would cost two exponentials per logit).  After the last
// column the (ref, s) pairs of a row (32 lanes x `waves`) are merged through LDS (the activation tile's storage,
// dead by then) as log-sum-exp of ref + log2(s).  A later logit more than 2^127 times the first one a lane saw
// overflows s to +inf: such a workgroup raises the workspace's `repair` flag instead of writing garbage, and
// wr_rnnt_loss_fwd_from_lse then runs the stand-alone pass 1 over the logits (never seen with real joiner outputs:
// it takes a spread of more than 88 nats inside one row).  The blank / label logits of a row are read back from
// the logits the workgroup has just written (L2-resident), 128 loads per workgroup.
#pragma once
#include "rnnt_latency.hpp"
#include "wr_common.hpp"

namespace wr {

// Epilogue modes of the forward kernels (template argument EPI):
//   kEpiStore     the logits leave for HBM (the joiner);
//   kEpiStoreLse  the logits leave and the row statistics are written (wr_joint_fwd_lse / wr_joint_fwd_split_lse);
//   kEpiStats     the row statistics only, no logit is stored (wr_joint_rnnt_stats): the blank / label logit of a row is
//                 parked in LDS by the lane that holds its column; `online` = the repair launch (below);
//   kEpiGrad      the RNN-T loss gradient of the cells [m_begin, m_end) instead of their logits (wr_joint_rnnt_grad):
//                 the formula and case chain of rnnt_grad_kernel (rnnt_loss.hip) with per-row constants from LDS, out row
//                 m - m_begin.  The logits are recomputed with the same k order, so they are bit-identical to the ones the
//                 statistics were taken from.
//   kEpiGradReg   kEpiGrad with FastEmit and / or the delay penalty (wr_joint_rnnt_grad_lattice): only the per-row
//                 constants differ (joint_epi_rows_init), the per-element epilogue is kEpiGrad's.  The regularisers are
//                 one more kernel argument (an RnntReg behind the others: the kernels end in a parameter pack that is
//                 empty in every other mode, so those keep their arguments and their code); lp_skew then holds the
//                 penalised label arcs.
//   kEpiTdtStats  kEpiStats for the token-and-duration loss (wr_joint_tdt_stats; frag kernel only): the row is V token and D
//                 duration columns, the partial sums take the token columns alone, and the D duration logits are parked
//                 beside the blank / label logit; what tdt_stats_kernel (rnnt_lattice.hip) writes goes into a TDT
//                 workspace.  The TDT side is one more kernel argument (a JointTdt, where kEpiGradReg has its RnntReg).
//   kEpiTdtGrad   kEpiGrad for that loss (wr_joint_tdt_grad): tdt_grad_kernel's per-element formula over the records of
//                 tdt_record_kernel, no clamp.
enum JointEpi : int { kEpiStore = 0, kEpiStoreLse = 1, kEpiStats = 2, kEpiGrad = 3, kEpiGradReg = 4, kEpiTdtStats = 5,
                      kEpiTdtGrad = 6 };
constexpr bool joint_epi_is_grad(int epi) { return epi == kEpiGrad || epi == kEpiGradReg; }
constexpr bool joint_epi_is_tdt(int epi) { return epi == kEpiTdtStats || epi == kEpiTdtGrad; }

struct JointLse {
    const int32_t *targets;   // [B, U1-1]
    int blank;
    int S;                    // anti-diagonals per utterance (RnntWs::S)
    float2 *lp_skew;          // [B, S, U1]   {skip, emit}
    float *denom;             // [B, T, U1]
    int32_t *repair;          // set to 1 when a partial sum overflowed (RnntWs::flag_off)
    // kEpiStats: the repair launch runs only if *run_if != 0 and keeps a running maximum (no overflow possible)
    const int32_t *run_if = nullptr;
    int online = 0;
    // kEpiGrad: the lattice of the sweeps and the gradient's scalars; cells [m_begin, m_end) of the flattened lattice
    const double *alpha_skew = nullptr, *beta_skew = nullptr, *cost = nullptr;
    const float *grad_costs = nullptr;   // [B] or null (= 1)
    float clamp = -1.f;
    long m_begin = 0, m_end = 0;
};

// The TDT side of kEpiTdtStats / kEpiTdtGrad.  The kernel's V is then the joiner's width V + D; the JointLse beside it
// carries targets, blank, S, the repair protocol, grad_costs and the cell range, with lp_skew = the workspace's `tok` array
// (the same anti-diagonal layout) and denom = its `denom`.
struct JointTdt {
    int V, D;                 // token columns [0, V), duration columns [V, V + D)
    float sigma;
    float *dur;               // [B, S, U1, D]   kEpiTdtStats writes it
    const float *rec;         // [B, T, U1, 3 + D]   kEpiTdtGrad reads it
};
constexpr int kJointTdtMaxD = 9;              // = kTdtMaxD (rnnt_tdt.hpp)

// The row-statistics block over an RNN-T workspace laid out by `w` (what the store and statistics modes need; the
// gradient mode's fields are the caller's to add).
inline JointLse joint_lse_over(const int32_t *targets_d, int blank, const RnntWs &w, char *rws)
{
    return JointLse{targets_d, blank, w.S, reinterpret_cast<float2 *>(rws + w.lp_off),
                    reinterpret_cast<float *>(rws + w.denom_off), reinterpret_cast<int32_t *>(rws + w.flag_off)};
}

// The RNN-T side of a joiner entry point `what` that fills or reads the loss's workspace: labels, blank, the sweep's
// column limit and the workspace size, in the order every such entry point reports them.  `terms` >= 0 (the rnnt_stats /
// rnnt_grad entry points, which pick the joiner's precision themselves): that code and the cell count as well.
inline int joint_rnnt_side_check(const char *what, const int32_t *targets_d, int B, int T, int U1, int V, int blank, int terms,
                                 size_t rws_bytes)
{
    WR_REQUIRE(targets_d || U1 == 1, WR_EINVAL, "%s: targets is null", what);
    WR_REQUIRE(terms < 0 || terms == 0 || terms == 3, WR_EUNSUPPORTED, "%s: terms must be 0 (exact fp32) or 3 (split), got %d",
               what, terms);
    WR_REQUIRE(blank >= 0 && blank < V, WR_EINVAL, "%s: blank %d out of range [0,%d)", what, blank, V);
    WR_REQUIRE(U1 <= kRnntMaxCols, WR_EUNSUPPORTED, "%s: U1=%d exceeds the loss's limit of %d", what, U1, kRnntMaxCols);
    WR_REQUIRE(terms < 0 || (long)B * T * U1 < (1L << 31), WR_EUNSUPPORTED, "%s: more than 2^31 lattice cells", what);
    const size_t need = rnnt_ws_layout(B, T, U1).total;
    WR_REQUIRE(rws_bytes >= need, WR_EWORKSPACE, "%s: RNN-T workspace %zu < required %zu", what, rws_bytes, need);
    return WR_OK;
}

constexpr int kLseRows = 64;  // cells per workgroup (= kBM = kSM)

// Per-row constants of the kEpiStats / kEpiGrad epilogues, in LDS behind everything else the kernel keeps there
// (joint_epi_rows_bytes).  Stats: lab = the row's label column (-1: none), xb / xl = the parked blank / label logit.
// Grad (rnnt_grad_kernel's names): c2 = (cmd + beta) log2e, bsub / lsub = the exponents of the blank / label terms minus
// the logit, blk / lab = their columns (-1: no such term), go = grad_costs[b]; a padded row has c2 = -inf and go = 0.
struct EpiRows {
    int *lab, *blk;
    float *xb, *xl, *c2, *bsub, *lsub, *go;
};
__host__ __device__ inline size_t joint_epi_rows_bytes() { return (size_t)8 * kLseRows * sizeof(float); }
// the TDT modes' row block behind it: xd[n][row], the parked duration logit n (statistics) or rec[3 + n] (gradient)
__host__ __device__ inline size_t joint_epi_tdt_rows_bytes() { return (size_t)kJointTdtMaxD * kLseRows * sizeof(float); }

__device__ __forceinline__ EpiRows joint_epi_rows(void *base)
{
    float *f = static_cast<float *>(base);
    EpiRows r;
    r.lab = reinterpret_cast<int *>(f);
    r.blk = reinterpret_cast<int *>(f + kLseRows);
    r.xb = f + 2 * kLseRows;
    r.xl = f + 3 * kLseRows;
    r.c2 = f + 4 * kLseRows;
    r.bsub = f + 5 * kLseRows;
    r.lsub = f + 6 * kLseRows;
    r.go = f + 7 * kLseRows;
    return r;
}

// Fill the per-row constants of the 64 cells m0.. (threads 0..63; the caller synchronises before the epilogues read them).
template <int EPI, typename... Reg>
__device__ __forceinline__ void joint_epi_rows_init(const JointLse &a, const EpiRows &er, const int32_t *llens,
                                                    const int32_t *tlens, long m0, long M, int T, int U1,
                                                    const Reg &...reg_args)
{
    static_assert(!joint_epi_is_tdt(EPI), "the TDT modes fill their rows with joint_epi_tdt_rows_init");
    static_assert((EPI == kEpiGradReg) == (sizeof...(Reg) == 1), "kEpiGradReg takes the regularisers, no other mode does");
    const int row = threadIdx.x;
    if (row >= kLseRows) return;
    const long m = m0 + row;
    int b = 0, t = 0, u = 0, T_ = 0, U = -1;
    if (m < M) {
        const long bt = m / U1;
        u = (int)(m - bt * U1);
        b = (int)(bt / T);
        t = (int)(bt - (long)b * T);
        T_ = llens[b];
        U = tlens[b];
    }
    const bool valid = m < M && t < T_ && u <= U;
    if (EPI == kEpiStats) {
        er.lab[row] = (valid && u < U) ? a.targets[(size_t)b * (U1 - 1) + u] : -1;
        er.xb[row] = 0.f;
        er.xl[row] = 0.f;
        return;
    }
    if (!valid) {
        er.c2[row] = kNegInf;
        er.bsub[row] = 0.f;
        er.lsub[row] = 0.f;
        er.blk[row] = -1;
        er.lab[row] = -1;
        er.go[row] = 0.f;
        return;
    }
    // rnnt_grad_kernel, term by term (fp64 where it is)
    const size_t dbase = (size_t)b * a.S * U1;
    const int s = t + u;
    const bool final_cell = t == T_ - 1 && u == U;
    const bool has_b1 = t < T_ - 1;
    const bool blank_special = final_cell || has_b1;
    const double al = a.alpha_skew[dbase + (size_t)s * U1 + u];
    const double be = a.beta_skew[dbase + (size_t)s * U1 + u];
    const double cost = a.cost[b];
    const float d = a.denom[m];
    double b1 = 0.0, b2 = 0.0;
    if (has_b1) b1 = a.beta_skew[dbase + (size_t)(s + 1) * U1 + u];
    int lab = -1;
    bool has_lab = false;
    if (u < U) {
        lab = a.targets[(size_t)b * (U1 - 1) + u];
        if (lab == a.blank && blank_special) lab = -1;
        else has_lab = true;
    }
    if (has_lab) b2 = a.beta_skew[dbase + (size_t)(s + 1) * U1 + (u + 1)];
    const double ac = al + cost;
    const double cmd = ac - (double)d;
    double bm = be, lpen = 0.0;
    if constexpr (EPI == kEpiGradReg) {
        // rnnt_grad_kernel with REG: be_eff in the main term, pen + log1p(lambda) in the label term
        const RnntReg &reg = only_arg(reg_args...);
        if (has_lab) {
            lpen = delay_pen(reg.delay_penalty, T_ > T ? T : T_, t) + reg.log1p_lambda;
            if (reg.log_lambda > (double)kNegInf)
                bm = log_add_d(be, reg.log_lambda + (double)a.lp_skew[dbase + (size_t)s * U1 + u].y + b2);
        }
    }
    er.c2[row] = (float)(cmd + bm) * kLog2e;
    er.bsub[row] = final_cell ? (float)cmd : (has_b1 ? (float)(cmd + b1) : 0.f);
    if constexpr (EPI == kEpiGradReg) er.lsub[row] = has_lab ? (float)(cmd + b2 + lpen) : 0.f;
    else er.lsub[row] = has_lab ? (float)(cmd + b2) : 0.f;
    er.blk[row] = blank_special ? a.blank : -1;
    er.lab[row] = has_lab ? lab : -1;
    er.go[row] = a.grad_costs ? a.grad_costs[b] : 1.f;
}

// The same for the TDT modes.  Statistics: lab = the row's label column (-1: none, or outside the token columns).
// Gradient (tdt_grad_kernel's names): c2 = rec[0] log2e, bsub / lsub = rec[1] / rec[2] (what the blank / label column
// subtracts), xd[n][row] = rec[3 + n], go = grad_costs[b]; a padded row has c2 = -inf and zeros.
template <int EPI>
__device__ __forceinline__ void joint_epi_tdt_rows_init(const JointLse &a, const JointTdt &td, const EpiRows &er, float *xd,
                                                        const int32_t *llens, const int32_t *tlens, long m0, long M, int T,
                                                        int U1)
{
    static_assert(joint_epi_is_tdt(EPI), "TDT modes only");
    const int row = threadIdx.x;
    if (row >= kLseRows) return;
    const long m = m0 + row;
    int b = 0, t = 0, u = 0, T_ = 0, U = -1;
    if (m < M) {
        const long bt = m / U1;
        u = (int)(m - bt * U1);
        b = (int)(bt / T);
        t = (int)(bt - (long)b * T);
        T_ = llens[b];
        U = tlens[b];
    }
    const bool valid = m < M && t < T_ && u <= U;
    int lab = (valid && u < U) ? a.targets[(size_t)b * (U1 - 1) + u] : -1;
    if (lab >= td.V) lab = -1;
    er.lab[row] = lab;
    if (EPI == kEpiTdtStats) {
        er.xb[row] = 0.f;
        er.xl[row] = 0.f;
        return;
    }
    const float *rc = td.rec + (size_t)m * (3 + td.D);
    er.c2[row] = valid ? rc[0] * kLog2e : kNegInf;
    er.bsub[row] = valid ? rc[1] : 0.f;
    er.lsub[row] = valid ? rc[2] : 0.f;
    er.go[row] = !valid ? 0.f : (a.grad_costs ? a.grad_costs[b] : 1.f);
    for (int n = 0; n < td.D; ++n) xd[n * kLseRows + row] = valid ? rc[3 + n] : 0.f;
}

// kEpiTdtStats: joint_epi_park, and the duration logit of column `col` in [V, V + D)
__device__ __forceinline__ void joint_epi_tdt_park(const EpiRows &er, float *xd, int blank, const JointTdt &td, int row,
                                                   int col, float x)
{
    if (col == blank) er.xb[row] = x;
    if (col == er.lab[row]) er.xl[row] = x;
    if (col >= td.V && col < td.V + td.D) xd[(col - td.V) * kLseRows + row] = x;
}

// kEpiTdtGrad: the gradient of logit x of `row`, column `col` < V + D (tdt_grad_kernel's fix: both subtractions apply when
// the label is the blank; a duration column takes its record value and the logit is not used)
__device__ __forceinline__ float joint_epi_tdt_grad(const EpiRows &er, const float *xd, int blank, int vtok, int row, int col,
                                                    float x)
{
    float val = fast_exp2(fmaf(x, kLog2e, er.c2[row]));
    if (col == blank) val -= er.bsub[row];
    if (col == er.lab[row]) val -= er.lsub[row];
    if (col >= vtok) val = xd[(col - vtok) * kLseRows + row];
    return val * er.go[row];
}

// kEpiStats: park the blank / label logit of `row` if this lane holds its column
__device__ __forceinline__ void joint_epi_park(const EpiRows &er, int blank, int row, int col, float x)
{
    if (col == blank) er.xb[row] = x;
    if (col == er.lab[row]) er.xl[row] = x;
}

// kEpiGrad: the gradient of logit x of `row`, column `col` (rnnt_grad_kernel's fix + finish)
__device__ __forceinline__ float joint_epi_grad(const EpiRows &er, float clamp, int row, int col, float x)
{
    float val = fast_exp2(fmaf(x, kLog2e, er.c2[row]));
    if (col == er.blk[row]) val -= fast_exp2((x + er.bsub[row]) * kLog2e);
    else if (col == er.lab[row]) val -= fast_exp2((x + er.lsub[row]) * kLog2e);
    if (clamp > 0.f) val = fminf(fmaxf(val, -clamp), clamp);
    return val * er.go[row];
}

// kEpiGrad, a tile whose 64 cells are all padded: no matrix work, its rows of the gradient are 0
__device__ __forceinline__ void joint_epi_zero_rows(float *out, long m0, long M, long m_begin, int V)
{
    const long m1 = m0 + kLseRows < M ? m0 + kLseRows : M;
    float *o = out + (size_t)(m0 - m_begin) * V;
    const long n = (m1 - m0) * (long)V;
    for (long i = threadIdx.x; i < n; i += blockDim.x) o[i] = 0.f;
}

// statistics exchange: [64 rows][waves * 32 entries] floats (one log-sum-exp per lane and row), overlaid on the
// activation tile after the k-loops
__host__ __device__ inline size_t joint_lse_exchange_bytes(int waves) { return (size_t)kLseRows * waves * 32 * sizeof(float); }

// one logit of column `col` (col >= V: padding, contributes nothing); first = this is the lane's first column
__device__ __forceinline__ void joint_lse_add(float &ref, float &s, float x, bool in, bool first)
{
    const float y = x * kLog2e;
    if (first) {
        ref = in ? y : -3.0e38f;
        s = in ? 1.f : 0.f;
    } else {
        s += in ? fast_exp2(y - ref) : 0.f;           // ref = -3e38 (nothing seen yet) gives +inf: caught below
    }
}

// the same with a running maximum (the repair launch of kEpiStats: two exponentials per logit, no overflow)
__device__ __forceinline__ void joint_lse_add_online(float &ref, float &s, float x, bool in, bool first)
{
    const float y = x * kLog2e;
    if (first) {
        ref = in ? y : -3.0e38f;
        s = in ? 1.f : 0.f;
    } else if (in) {
        if (y > ref) {
            s = s * fast_exp2(ref - y) + 1.f;
            ref = y;
        } else {
            s += fast_exp2(y - ref);
        }
    }
}

template <int EPI>
__device__ __forceinline__ void joint_lse_add_mode(const JointLse &a, float &ref, float &s, float x, bool in, bool first)
{
    if ((EPI == kEpiStats || EPI == kEpiTdtStats) && a.online) joint_lse_add_online(ref, s, x, in, first);
    else joint_lse_add(ref, s, x, in, first);
}

// kEpiTdtStats: what tdt_stats_kernel writes for cell m (row `row` of the tile), called by a whole wave with the row's
// token log-sum-exp `d`.  The duration log-sum-exp is that kernel's, one parked logit per lane with a true maximum.
__device__ __forceinline__ void joint_tdt_write_row(const JointLse &a, const JointTdt &td, const int *parked_lab,
                                                    const float *parked_xb, const float *parked_xl, const float *parked_xd,
                                                    const int32_t *llens, const int32_t *tlens, int row, long m, long M, int T,
                                                    int U1, float d)
{
    const int lane = threadIdx.x & 63;
    const int D = td.D;
    float x = kNegInf;
    if (lane < D) x = parked_xd[lane * kLseRows + row];
    const float y = x * kLog2e;
    const float mx = wave_max(y);
    const float sd = wave_sum(lane < D ? fast_exp2(y - mx) : 0.f);
    const float dd = (mx + fast_log2(sd)) * kLn2;
    if (m >= M) return;
    const long bt = m / U1;
    const int u = (int)(m - bt * U1);
    const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
    if (t >= llens[b] || u > tlens[b]) return;                // same rows as tdt_stats_kernel writes
    const size_t k = ((size_t)b * a.S + (t + u)) * U1 + u;
    if (lane < D) td.dur[k * D + lane] = x - dd;
    if (lane == 0) {
        const float em = parked_lab[row] >= 0 ? (parked_xl[row] - d) - td.sigma : kNegInf;
        a.denom[m] = d;
        a.lp_skew[k] = make_float2((parked_xb[row] - d) - td.sigma, em);
    }
}

// Merge and write.  ref/s: this lane's statistics, index rt * 16 + r <-> row 32 rt + (r&3) + 8 (r>>2) + 4 half.
// `xch` must be free for joint_lse_exchange_bytes(WAVES) bytes and every wave must have finished with whatever
// lived there (the caller synchronises before the call); `out` = the logits this workgroup has stored, or null with
// `parked_xb` / `parked_xl` = the blank / label logits parked in LDS (kEpiStats; EpiRows::xb / xl, passed by value so that
// they stay LDS addresses).
// kEpiTdtStats (`tdt_args` = the JointTdt, with `parked_lab` / `parked_xd` = EpiRows::lab and the TDT row block): a merged
// row goes to joint_tdt_write_row instead.
template <int WAVES, typename... Tdt>
__device__ __forceinline__ void joint_lse_finish(const JointLse &a, float *xch, const float (&ref)[32], const float (&s)[32],
                                                 const int32_t *llens, const int32_t *tlens, const float *out, long m0,
                                                 long M, int T, int U1, int V, const float *parked_xb = nullptr,
                                                 const float *parked_xl = nullptr, const int *parked_lab = nullptr,
                                                 const float *parked_xd = nullptr, const Tdt &...tdt_args)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    constexpr int E = WAVES * 32;                         // entries per row
    bool bad = false;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        const int row = 32 * (i >> 4) + (i & 3) + 8 * ((i & 15) >> 2) + 4 * half;
        // this lane's log-sum-exp (log2 domain); a lane that saw no valid column holds s = 0 -> -inf: no weight
        const float e = s[i] > 0.f ? ref[i] + fast_log2(s[i]) : -3.0e38f;
        bad = bad || !(s[i] < 3.0e38f);                   // +inf or NaN: overflowed
        xch[(size_t)row * E + wave * 32 + l31] = e;
    }
    if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) *a.repair = 1;
    __threadfence_block();                                // this workgroup's logit stores are visible to its own loads below
    __syncthreads();
    constexpr int RPW = kLseRows / WAVES;                 // rows merged by one wave
    constexpr int EPL = (E + 63) / 64;                    // entries per lane
#pragma unroll 1
    for (int q = 0; q < RPW; ++q) {
        const int row = wave * RPW + q;
        float e[EPL];
        float mx = -3.0e38f;
#pragma unroll
        for (int j = 0; j < EPL; ++j) {
            const int idx = lane + 64 * j;
            e[j] = idx < E ? xch[(size_t)row * E + idx] : -3.0e38f;
            mx = fmaxf(mx, e[j]);
        }
        mx = wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < EPL; ++j) sum += fast_exp2(e[j] - mx);
        sum = wave_sum(sum);
        const long m = m0 + row;
        if constexpr (sizeof...(Tdt) == 1) {
            joint_tdt_write_row(a, only_arg(tdt_args...), parked_lab, parked_xb, parked_xl, parked_xd, llens, tlens, row, m, M, T,
                                U1, (mx + fast_log2(sum)) * kLn2);
        } else if (lane == 0 && m < M) {
            const long bt = m / U1;
            const int u = (int)(m - bt * U1);
            const int b = (int)(bt / T), t = (int)(bt - (long)b * T);
            const int U = tlens[b];
            if (t < llens[b] && u <= U) {                 // same rows as rnnt_lse_kernel writes
                const float d = (mx + fast_log2(sum)) * kLn2;
                float xb, em = 0.f;
                if (parked_xb != nullptr) {
                    xb = parked_xb[row];
                    if (u < U) em = parked_xl[row] - d;
                } else {
                    const float *orow = out + (size_t)m * V;
                    xb = __builtin_nontemporal_load(orow + a.blank);
                    if (u < U) em = __builtin_nontemporal_load(orow + a.targets[(size_t)b * (U1 - 1) + u]) - d;
                }
                a.denom[m] = d;
                a.lp_skew[((size_t)b * a.S + (t + u)) * U1 + u] = make_float2(xb - d, em);
            }
        }
    }
}

// joint_split.hip: the kEpiStats / kEpiGrad modes of the split-precision forward (terms = 3); `workspace` as
// wr_joint_split_workspace_bytes; w_ready: it already holds W's bf16 images from an earlier call with the same W
int joint_fwd_split_epi(const float *ep_d, const float *pp_d, const float *w_out_d, const float *b_out_d,
                        const int32_t *llens, const int32_t *tlens, int B, int T, int U1, int J, int V, int act, int epi,
                        const JointLse &lse, float *out_d, void *workspace_d, size_t workspace_bytes, hipStream_t st,
                        bool w_ready = false, const RnntReg *reg = nullptr /* kEpiGradReg */);

}  // namespace wr
