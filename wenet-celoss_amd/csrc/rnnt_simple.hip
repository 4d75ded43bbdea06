// Additive-joiner ("simple") RNN-T loss for MI355X (gfx950): the transducer loss whose joiner is a plain sum,
//     logit(b,t,u,v) = am[b,t,v] + lm[b,u,v]
// (k2's rnnt_loss_simple as the reference calls it, wenet/transducer/transducer_k2_loss.py:140-157).  No (B,T,U+1,V)
// tensor exists anywhere: the row normaliser and both gradients factor into contractions over one index,
//     denom(t,u) = ma[t] + ml[u] + log sum_v e^{am[t,v]-ma[t]} e^{lm[u,v]-ml[u]}          [T x V].[V x U1]   K = V
//     d am[t,v]  = e^{am[t,v]-ma[t]} sum_u G(t,u) e^{lm[u,v]-ml[u]}  - scatter terms       [T x U1].[U1 x V]  K = U1
//     d lm[u,v]  = e^{lm[u,v]-ml[u]} sum_t G(t,u) e^{am[t,v]-ma[t]}  - scatter terms       [U1 x T].[T x V]   K = T
//     G(t,u)     = occ(t,u) e^{ma[t]+ml[u]-denom(t,u)},  occ(t,u) = exp(alpha + beta - ll)  (node occupancy)
// with ma / ml the row maxima of am / lm.  Arithmetic: v_mfma_f32_32x32x2_f32 (exact fp32), operands exponentiated on
// the fly; the lattice sweeps between the two halves are rnnt_loss.hip's (wr_rnnt_loss_sweeps), on the same workspace.
//
//   wr_rnnt_simple_stats
//     simple_rowmax_kernel     one wave per row of am and of lm: ma, ml; clears the workspace flag
//     simple_stats_kernel      64 (t) x 64 (u) tile per workgroup, 4 waves of one 32 x 32 MFMA tile each; per 32-deep
//                              v-slice the two exponentiated operand tiles are built in LDS (k-major, +1 padded);
//                              epilogue: log, + ma + ml, the blank / label logits gathered, denom and the skewed
//                              log-probabilities stored.  2*T*U1*V flop per utterance.
//     simple_stats_direct_kernel   the repair pass: one wave per cell, online (max, sum) over am + lm.  Always enqueued;
//                              its workgroups leave at once unless the fast kernel raised the flag.
//   wr_rnnt_simple_grad
//     simple_occ_kernel        one thread per cell: G (and its transpose), the two arc occupancies, in fp64 then rounded
//     simple_chain_kernel      per utterance: for every label position the next position with the same label
//     simple_grad_gemm_kernel  both gradient contractions (one template, two launches): 64 rows x 128 columns per
//                              workgroup, operands straight from L2 into registers (A k-major and coalesced, B
//                              exponentiated on the fly), epilogue multiplies by the output's own exponential
//     simple_grad_direct_kernel    the flagged case: per output element sum_k occ * e^{am+lm-denom} in a fixed order
//     simple_fix_am_kernel / simple_fix_lm_kernel   the scatter terms, one writer per address, fixed summation order
//
// Range.  The factored sum S = sum_v e^{am-ma} e^{lm-ml} loses every term whose product (or one factor) falls below the
// smallest normal float, 1.18e-38; V such terms weigh at most V * 1.18e-38 < 2.6e-29 (V < 2^31).  With S >= kSafeSum =
// 1e-20 what is lost is below 3e-9 of S, under half an fp32 ulp.  A valid cell whose S is below that, zero or not finite
// (am's and lm's peaks on different symbols, both tall) raises the flag, and every cell is then redone by the direct
// kernels -- in the gradient too, where e^{ma+ml-denom} = 1/S would overflow for the same cells.  Nothing is read back
// on the host.  No float atomics anywhere: every sum has a fixed order, so results are bit-identical run to run.
#include "rnnt_lattice.hpp"
#include "row_stream.hpp"
#include "wr_common.hpp"
#include "wr_launch.hpp"

namespace wr {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr float kSafeSum = 1e-20f;
constexpr int kTile = 64;          // lattice tile edge of the stats kernel; row tile of the gradient contraction
constexpr int kSliceV = 32;        // v-slice depth of the stats kernel
constexpr int kPad = kTile + 1;    // k-major LDS row stride (floats)
constexpr int kGemmCols = 128;     // output columns per workgroup of the gradient contraction (4 waves x 32)
constexpr int kGemmPF = 8;         // k-steps (of 2) whose operands are loaded together

struct SimpleWs {
    size_t ma_off, ml_off, g_off, gt_off, ob_off, oe_off, nxt_off, head_off, total;
};

inline SimpleWs simple_ws_layout(int B, int T, int U1)
{
    SimpleWs w;
    const size_t cells = (size_t)B * T * U1;
    size_t off = 0;
    w.ma_off = off;  off = align_up(off + (size_t)B * T * sizeof(float), 256);
    w.ml_off = off;  off = align_up(off + (size_t)B * U1 * sizeof(float), 256);
    w.g_off = off;   off = align_up(off + cells * sizeof(float), 256);      // G [B,T,U1]
    w.gt_off = off;  off = align_up(off + cells * sizeof(float), 256);      // G transposed [B,U1,T]
    w.ob_off = off;  off = align_up(off + cells * sizeof(float), 256);      // grad_costs * occ_blank [B,T,U1]
    w.oe_off = off;  off = align_up(off + cells * sizeof(float), 256);      // grad_costs * occ_emit  [B,T,U1]
    w.nxt_off = off; off = align_up(off + (size_t)B * U1 * sizeof(int32_t), 256);
    w.head_off = off; off = align_up(off + (size_t)B * U1 * sizeof(int32_t), 256);
    w.total = off;
    return w;
}

// ------------------------------------------------------------------------------------------------ row maxima --
// rows [0, B*T) are am's, rows [B*T, B*T + B*U1) are lm's
__global__ __launch_bounds__(256) void simple_rowmax_kernel(const float *__restrict__ am, const float *__restrict__ lm,
                                                            long rows_am, long rows_lm, int V, float *__restrict__ ma,
                                                            float *__restrict__ ml, int32_t *__restrict__ flag)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) *flag = 0;
    const int lane = threadIdx.x & (kWave - 1);
    const long r = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows_am + rows_lm) return;
    const bool is_am = r < rows_am;
    const float *__restrict__ row = is_am ? am + (size_t)r * V : lm + (size_t)(r - rows_am) * V;
    typedef VecOf<float>::type vec_t;
    const RowSplit<float> sp(row, V);
    float m = kNegInf;
    if (lane < sp.h) m = fmaxf(m, row[lane]);
    if (lane < sp.tail) m = fmaxf(m, row[sp.h + 4 * sp.nv + lane]);
    const vec_t *__restrict__ body = reinterpret_cast<const vec_t *>(row + sp.h);
    for (int i = lane; i < sp.nv; i += kWave) {
        const vec_t x = body[i];
        m = fmaxf(fmaxf(m, fmaxf(x[0], x[1])), fmaxf(x[2], x[3]));
    }
    m = wave_max(m);
    if (lane == 0) {
        if (is_am) ma[r] = m;
        else ml[r - rows_am] = m;
    }
}

// ------------------------------------------------------------------------------------ row statistics, MFMA --
// grid (ceil(U1/64), ceil(T/64), B), 256 threads.  Wave w owns the 32 x 32 tile (w >> 1, w & 1) of the 64 x 64 block.
__global__ __launch_bounds__(256) void simple_stats_kernel(
    const float *__restrict__ am, const float *__restrict__ lm, const int32_t *__restrict__ symbols,
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int T, int U1, int V, int blank, int S,
    const float *__restrict__ ma, const float *__restrict__ ml, float2 *__restrict__ lp_skew, float *__restrict__ denom,
    int32_t *__restrict__ flag)
{
    __shared__ float At[kSliceV * kPad];     // e^{am - ma}, [k][t]
    __shared__ float Lt[kSliceV * kPad];     // e^{lm - ml}, [k][u]
    const int b = blockIdx.z, t0 = blockIdx.y * kTile, u0 = blockIdx.x * kTile;
    const int Tb = clampi(llens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
    if (t0 >= Tb || u0 > Ub) return;          // the whole tile lies outside [0,T_b) x [0,U_b]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int kv = tid & 31, rg = tid >> 5;   // this thread fills element (row rg + 8 i, k = kv) of both tiles

    const float *__restrict__ amb = am + (size_t)b * T * V;
    const float *__restrict__ lmb = lm + (size_t)b * U1 * V;
    const float *__restrict__ mab = ma + (size_t)b * T;
    const float *__restrict__ mlb = ml + (size_t)b * U1;

    // rows beyond the tensor are clamped to its last row (their results are never stored)
    size_t arow[8], lrow[8];
    float mar[8], mlr[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int t = min(t0 + rg + 8 * i, T - 1), u = min(u0 + rg + 8 * i, U1 - 1);
        arow[i] = (size_t)t * V;
        lrow[i] = (size_t)u * V;
        mar[i] = mab[t];
        mlr[i] = mlb[u];
    }
    float ra[8], rl[8];
    auto load_slice = [&](int k0) {
        const int v = min(k0 + kv, V - 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) { ra[i] = amb[arow[i] + v]; rl[i] = lmb[lrow[i] + v]; }
    };
    f32x16 acc = (f32x16){0};
    const float *__restrict__ Ah = At + half * kPad + 32 * (wave >> 1) + l31;     // + k * kPad
    const float *__restrict__ Bh = Lt + half * kPad + 32 * (wave & 1) + l31;

    load_slice(0);
    for (int k0 = 0; k0 < V; k0 += kSliceV) {
        const bool in = k0 + kv < V;
        __syncthreads();                      // the previous slice's fragments have been read
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            At[kv * kPad + rg + 8 * i] = in ? fast_exp2((ra[i] - mar[i]) * kLog2e) : 0.f;
            Lt[kv * kPad + rg + 8 * i] = in ? fast_exp2((rl[i] - mlr[i]) * kLog2e) : 0.f;
        }
        __syncthreads();
        if (k0 + kSliceV < V) load_slice(k0 + kSliceV);      // in flight under the MFMAs below
#pragma unroll
        for (int k = 0; k < kSliceV; k += 2)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ah[k * kPad], Bh[k * kPad], acc, 0, 0, 0);
    }

    const int u = u0 + 32 * (wave & 1) + l31;
    const bool ucol = u <= Ub;
    int lab = -1;
    float lmk = 0.f, lml = 0.f, mlu = 0.f;
    if (ucol) {
        mlu = mlb[u];
        lmk = lmb[(size_t)u * V + blank];
        if (u < Ub) {
            lab = symbols[(size_t)b * (U1 - 1) + u];
            lml = lmb[(size_t)u * V + lab];
        }
    }
    bool bad = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int t = t0 + 32 * (wave >> 1) + (r & 3) + 8 * (r >> 2) + 4 * half;      // C/D layout of the 32x32 MFMA
        if (!ucol || t >= Tb) continue;
        const float s = acc[r];
        if (!(s >= kSafeSum && s < __builtin_huge_valf())) bad = true;                // 0, too small, inf or NaN
        const double d = ((double)mab[t] + (double)mlu) + (double)logf(s);       // rounded once, when stored
        const float xb = amb[(size_t)t * V + blank] + lmk;
        const float em = lab >= 0 ? (float)((double)(amb[(size_t)t * V + lab] + lml) - d) : 0.f;
        denom[((size_t)b * T + t) * U1 + u] = (float)d;
        lp_skew[((size_t)b * S + t + u) * U1 + u] = make_float2((float)((double)xb - d), em);
    }
    if (bad) *flag = 1;
}

// ------------------------------------------------------------------------------------ row statistics, direct --
// One wave per cell, online (max, sum) over am + lm.  Leaves at once unless the flag is raised.
__global__ __launch_bounds__(256) void simple_stats_direct_kernel(
    const float *__restrict__ am, const float *__restrict__ lm, const int32_t *__restrict__ symbols,
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int B, int T, int U1, int V, int blank, int S,
    float2 *__restrict__ lp_skew, float *__restrict__ denom, const int32_t *__restrict__ flag)
{
    if (*flag == 0) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int wpb = blockDim.x >> 6;
    const long ncells = (long)B * T * U1;
    const int cells = T * U1;
    for (long r = (long)blockIdx.x * wpb + (threadIdx.x >> 6); r < ncells; r += (long)gridDim.x * wpb) {
        const int b = (int)(r / cells);
        const int c = (int)(r - (long)b * cells);
        const int t = c / U1, u = c - t * U1;
        const int Tb = clampi(llens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
        if (t >= Tb || u > Ub) continue;
        const float *__restrict__ a = am + ((size_t)b * T + t) * V;
        const float *__restrict__ l = lm + ((size_t)b * U1 + u) * V;
        // online (max, sum) in the natural domain: x - m is exact for the terms that carry the sum
        float m = -3.0e38f, sum = 0.f;
        for (int v = lane; v < V; v += kWave) {
            const float x = a[v] + l[v];
            const float nm = fmaxf(m, x);
            sum = sum * fast_exp2((m - nm) * kLog2e) + fast_exp2((x - nm) * kLog2e);
            m = nm;
        }
        const float M = wave_max(m);
        const float s = wave_sum(sum * fast_exp2((m - M) * kLog2e));
        const double d = (double)M + (double)logf(s);       // rounded once, when stored
        if (lane == 0) {
            float em = 0.f;
            if (u < Ub) {
                const int lab = symbols[(size_t)b * (U1 - 1) + u];
                em = (float)((double)(a[lab] + l[lab]) - d);
            }
            denom[r] = (float)d;
            lp_skew[((size_t)b * S + t + u) * U1 + u] = make_float2((float)((double)(a[blank] + l[blank]) - d), em);
        }
    }
}

// ------------------------------------------------------------------------------------------- occupancies --
// One thread per cell.  Exponents are formed in fp64 (the lattice state's precision) and only then rounded, as
// rnnt_grad_kernel forms its own.  g = G * grad_costs[b]; with the flag raised g holds grad_costs[b] * occ instead (the
// direct gradient kernel's factor; e^{ma+ml-denom} may overflow there).  g is further scaled by `gscale`.
// LAT: the lattice type (rnnt_lattice.hpp).  kLatModified reads plain rows and a label arc leads to (t+1, u+1): beta of
// the terminal row T_b is 0 at U_b and -inf elsewhere, so the last frame keeps the blank out of (T_b-1, U_b) and the
// label out of (T_b-1, U_b-1).  A delay penalty needs nothing here: it is inside the stored label arc.
template <int LAT>
__global__ __launch_bounds__(256) void simple_occ_kernel(
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int B, int T, int U1, int S,
    const double *__restrict__ alpha_skew, const double *__restrict__ beta_skew, const float2 *__restrict__ lp_skew,
    const float *__restrict__ denom, const double *__restrict__ cost_ws, const float *__restrict__ ma,
    const float *__restrict__ ml, const float *__restrict__ grad_costs, const int32_t *__restrict__ flag, float gscale,
    float *__restrict__ g, float *__restrict__ gt, float *__restrict__ ob, float *__restrict__ oe,
    float *__restrict__ occ_emit_out, float *__restrict__ occ_blank_out)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)B * T * U1) return;
    const int cells = T * U1;
    const int b = (int)(r / cells);
    const int c = (int)(r - (long)b * cells);
    const int t = c / U1, u = c - t * U1;
    const int Tb = clampi(llens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
    float gv = 0.f, fb = 0.f, fe = 0.f;
    float go = 1.f;
    if (t < Tb && u <= Ub) {
        if (grad_costs) go = grad_costs[b];
        const size_t dbase = (size_t)b * S * U1;
        const int s = t + u;
        const size_t k = dbase + lat_idx<LAT>(t, u, U1);
        const double al = alpha_skew[k];
        const double be = beta_skew[k];
        const double ac = al + cost_ws[b];                      // cost = -ll
        const float2 lp = lp_skew[k];
        const double lo = ac + be;                              // log occupancy of the node
        if (*flag != 0) gv = (float)exp(lo);
        else gv = (float)exp(lo + (((double)ma[(size_t)b * T + t] + (double)ml[(size_t)b * U1 + u]) - (double)denom[r]));
        if (LAT == kLatModified) {
            if (t < Tb - 1) {
                fb = (float)exp(ac + (double)lp.x + beta_skew[k + U1]);
                if (u < Ub) fe = (float)exp(ac + (double)lp.y + beta_skew[k + U1 + 1]);
            } else {                                            // the last frame: beta(T_b, .) is 0 at U_b, -inf elsewhere
                if (u == Ub) fb = (float)exp(ac + (double)lp.x);
                if (u == Ub - 1) fe = (float)exp(ac + (double)lp.y);
            }
        } else {
            if (t < Tb - 1) fb = (float)exp(ac + (double)lp.x + beta_skew[dbase + (size_t)(s + 1) * U1 + u]);
            else if (u == Ub) fb = (float)exp(ac + (double)lp.x);   // the final cell: beta := 0
            if (u < Ub) fe = (float)exp(ac + (double)lp.y + beta_skew[dbase + (size_t)(s + 1) * U1 + (u + 1)]);
        }
    }
    const float gs = gv * go * gscale;                          // gscale: 1 (exact), or c of the smoothed loss
    g[r] = gs;
    gt[((size_t)b * U1 + u) * T + t] = gs;
    ob[r] = fb * go;
    oe[r] = fe * go;
    if (occ_emit_out) occ_emit_out[r] = fe;
    if (occ_blank_out) occ_blank_out[r] = fb;
}

// nxt[b,u]: the next label position u' > u with symbols[b,u'] == symbols[b,u] (inside U_b), -1 if none;
// head[b,u]: 1 if no earlier position holds the same label.  O(U^2) compares per utterance, on U <= 1023.
__global__ void simple_chain_kernel(const int32_t *__restrict__ symbols, const int32_t *__restrict__ tlens, int U1,
                                    int32_t *__restrict__ nxt, int32_t *__restrict__ head)
{
    const int b = blockIdx.x;
    const int Ub = clampi(tlens[b], 0, U1 - 1);
    const int32_t *__restrict__ sy = symbols + (size_t)b * (U1 - 1);
    for (int u = threadIdx.x; u < U1; u += blockDim.x) {
        int32_t n = -1, h = 0;
        if (u < Ub) {
            const int lab = sy[u];
            for (int j = u + 1; j < Ub; ++j)
                if (sy[j] == lab) { n = j; break; }
            h = 1;
            for (int j = 0; j < u; ++j)
                if (sy[j] == lab) { h = 0; break; }
        }
        nxt[(size_t)b * U1 + u] = n;
        head[(size_t)b * U1 + u] = h;
    }
}

// ------------------------------------------------------------------------- gradient contractions, MFMA --
// out[b,m,v] = e^{X[b,m,v] - mx[b,m]} * sum_{k < K_b} A[b,k,m] * e^{Y[b,k,v] - my[b,k]}   for m < M_b, 0 for M_b <= m < M
//   AM = true : m = t, k = u  (A = G transposed [B,U1,T], X = am, Y = lm)   -> d am before the scatter terms
//   AM = false: m = u, k = t  (A = G [B,T,U1],           X = lm, Y = am)   -> d lm before the scatter terms
// grid (ceil(V/128), ceil(M/64), B), 256 threads: wave w owns columns 32 w .. 32 w + 31 of the chunk and both 32-row
// tiles.  Operands go straight into registers, kGemmPF k-steps at a time: A is k-major (lanes along m: one 128-byte
// line), Y's lanes run along v.  Operands outside [0,K_b) are selected to zero (their inputs may hold anything).
template <bool AM>
__global__ __launch_bounds__(256) void simple_grad_gemm_kernel(
    const float *__restrict__ A, const float *__restrict__ X, const float *__restrict__ mx,
    const float *__restrict__ Y, const float *__restrict__ my, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, int T, int U1, int V, const int32_t *__restrict__ flag, float *__restrict__ out)
{
    if (*flag != 0) return;                   // the direct kernel writes everything
    const int b = blockIdx.z;
    const int Tb = clampi(llens[b], 0, T), Ub1 = clampi(tlens[b], 0, U1 - 1) + 1;
    const int M = AM ? T : U1, K = AM ? U1 : T;
    const int Mb = Tb > 0 ? (AM ? Tb : Ub1) : 0, Kb = AM ? Ub1 : Tb;
    const int m0 = blockIdx.y * kTile;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    const int col = blockIdx.x * kGemmCols + 32 * wave + l31;
    const bool cin = col < V;
    float *__restrict__ ob = out + (size_t)b * M * V;

    f32x16 acc[2] = {(f32x16){0}, (f32x16){0}};
    if (m0 < Mb) {
        const float *__restrict__ Ab = A + (size_t)b * K * M;
        const float *__restrict__ Yb = Y + (size_t)b * K * V;
        const float *__restrict__ myb = my + (size_t)b * K;
        const int r0 = min(m0 + l31, M - 1), r1 = min(m0 + 32 + l31, M - 1);     // clamped rows are never stored
        const int cc = min(col, V - 1);
        for (int kk = 0; kk < Kb; kk += 2 * kGemmPF) {
            float a0[kGemmPF], a1[kGemmPF], y[kGemmPF], mk[kGemmPF];
#pragma unroll
            for (int i = 0; i < kGemmPF; ++i) {
                const int k = min(kk + 2 * i + half, K - 1);
                a0[i] = Ab[(size_t)k * M + r0];
                a1[i] = Ab[(size_t)k * M + r1];
                y[i] = Yb[(size_t)k * V + cc];
                mk[i] = myb[k];
            }
#pragma unroll
            for (int i = 0; i < kGemmPF; ++i) {
                const bool kin = kk + 2 * i + half < Kb;
                const float e = (kin && cin) ? fast_exp2((y[i] - mk[i]) * kLog2e) : 0.f;
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(kin ? a0[i] : 0.f, e, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(kin ? a1[i] : 0.f, e, acc[1], 0, 0, 0);
            }
        }
    }
    if (!cin) return;
    const float *__restrict__ Xb = X + (size_t)b * M * V;
    const float *__restrict__ mxb = mx + (size_t)b * M;
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = m0 + 32 * rt + (r & 3) + 8 * (r >> 2) + 4 * half;
            if (m >= M) continue;
            float val = 0.f;
            if (m < Mb) val = fast_exp2((Xb[(size_t)m * V + col] - mxb[m]) * kLog2e) * acc[rt][r];
            ob[(size_t)m * V + col] = val;
        }
}

// ------------------------------------------------------------------------ gradient main term, direct --
// The flagged case: out[b,m,v] = sum_{k < K_b} occ(m,k) * e^{am + lm - denom}, one thread per output element, k ascending.
// grid (ceil(V/256), min(M, 64), B), rows strided over grid y (few workgroups: the launch is empty in the ordinary case).
// `occ` is simple_occ_kernel's g ([B,T,U1], grad_costs * occupancy when the flag is up).
template <bool AM>
__global__ __launch_bounds__(256) void simple_grad_direct_kernel(
    const float *__restrict__ occ, const float *__restrict__ denom, const float *__restrict__ X,
    const float *__restrict__ Y, const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int T, int U1,
    int V, const int32_t *__restrict__ flag, float *__restrict__ out)
{
    if (*flag == 0) return;
    const int b = blockIdx.z;
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int Tb = clampi(llens[b], 0, T), Ub1 = clampi(tlens[b], 0, U1 - 1) + 1;
    const int M = AM ? T : U1, K = AM ? U1 : T;
    const int Mb = Tb > 0 ? (AM ? Tb : Ub1) : 0, Kb = AM ? Ub1 : Tb;
    for (int m = blockIdx.y; m < M; m += gridDim.y) {
        float acc = 0.f;
        if (m < Mb) {
            const float x = X[((size_t)b * M + m) * V + v];
            const float *__restrict__ Yb = Y + (size_t)b * K * V + v;
            for (int k = 0; k < Kb; ++k) {
                const size_t cell = AM ? ((size_t)b * T + m) * U1 + k : ((size_t)b * T + k) * U1 + m;
                acc += occ[cell] * fast_exp2(((x + Yb[(size_t)k * V]) - denom[cell]) * kLog2e);
            }
        }
        out[((size_t)b * M + m) * V + v] = acc;
    }
}

// ------------------------------------------------------------------------------------------ scatter terms --
// A label equal to the blank follows the project's RNN-T loss (rnnt_grad_kernel, torchaudio's case chain, first match
// wins): at v == blank a cell subtracts its blank arc wherever it has one (t < T_b - 1, and the final cell) and its emit
// arc only where it has none (t == T_b - 1, u < U_b).
// d am[t, blank] -= sum_u occ_blank(t,u) ; d am[t, lab_u] -= occ_emit(t,u).  One wave per (b, t).  Positions that share a
// label are summed along their chain by the first of them (one writer per address); a label equal to the blank joins the
// blank's sum (last frame only, see above).  wave_sum is a fixed butterfly: the same bits every run.
// `wgt` weighs what is subtracted (1 here; c + am_only_scale / c + lm_only_scale under smoothing), and `every_arc` drops
// the case chain: the smoothed loss subtracts every arc at its own symbol, the derivative of its arcs as written.
__global__ __launch_bounds__(256) void simple_fix_am_kernel(
    const float *__restrict__ ob, const float *__restrict__ oe, const int32_t *__restrict__ nxt,
    const int32_t *__restrict__ head, const int32_t *__restrict__ symbols, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, int B, int T, int U1, int V, int blank, float wgt, bool every_arc,
    float *__restrict__ d_am)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long r = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= (long)B * T) return;
    const int b = (int)(r / T), t = (int)(r - (long)b * T);
    const int Tb = clampi(llens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
    if (t >= Tb) return;
    const float *__restrict__ obr = ob + (size_t)r * U1;
    const float *__restrict__ oer = oe + (size_t)r * U1;
    const int32_t *__restrict__ sy = symbols + (size_t)b * (U1 - 1);
    const int32_t *__restrict__ nx = nxt + (size_t)b * U1;
    float *__restrict__ row = d_am + (size_t)r * V;
    float part = 0.f;
    for (int u = lane; u <= Ub; u += kWave) {
        part += obr[u];
        if (u < Ub && sy[u] == blank && (every_arc || t == Tb - 1)) part += oer[u];
    }
    const float tot = wave_sum(part);
    if (lane == 0) row[blank] -= wgt * tot;
    for (int u = lane; u < Ub; u += kWave) {
        const int lab = sy[u];
        if (lab == blank || head[(size_t)b * U1 + u] == 0) continue;
        float s = oer[u];
        for (int j = nx[u]; j >= 0; j = nx[j]) s += oer[j];
        row[lab] -= wgt * s;
    }
}

// d lm[u, blank] -= sum_t occ_blank(t,u) ; d lm[u, lab_u] -= sum_t occ_emit(t,u).  One workgroup per (b, 64 columns u):
// thread (u, phase) sums t = phase, phase + 4, ... ; the four phases are added in order.
__global__ __launch_bounds__(256) void simple_fix_lm_kernel(
    const float *__restrict__ ob, const float *__restrict__ oe, const int32_t *__restrict__ symbols,
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int T, int U1, int V, int blank, float wgt,
    bool every_arc, float *__restrict__ d_lm)
{
    __shared__ float sb[4][64], se[4][64];
    const int b = blockIdx.y;
    const int ul = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int u = blockIdx.x * 64 + ul;
    const int Tb = clampi(llens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
    float pb = 0.f, pe = 0.f;
    if (u <= Ub)
        for (int t = ph; t < Tb; t += 4) {
            const size_t cell = ((size_t)b * T + t) * U1 + u;
            pb += ob[cell];
            pe += oe[cell];
        }
    sb[ph][ul] = pb;
    se[ph][ul] = pe;
    __syncthreads();
    if (ph != 0 || u > Ub || Tb <= 0) return;
    const float tb = ((sb[0][ul] + sb[1][ul]) + sb[2][ul]) + sb[3][ul];
    const float te = ((se[0][ul] + se[1][ul]) + se[2][ul]) + se[3][ul];
    float *__restrict__ row = d_lm + ((size_t)b * U1 + u) * V;
    const int lab = u < Ub ? symbols[(size_t)b * (U1 - 1) + u] : -1;
    if (lab == blank) row[blank] -= wgt * (tb + (every_arc ? te : oe[((size_t)b * T + (Tb - 1)) * U1 + u]));
    else {
        row[blank] -= wgt * tb;
        if (lab >= 0) row[lab] -= wgt * te;
    }
}

// ================================================================================= the smoothed loss ==
// k2's rnnt_loss_smoothed (include/wr_api.h has the contract): every arc of the lattice above is interpolated with an
// lm-only and an am-only estimate,
//     arc = c * (am + lm - denom) + ll * (lm - Zl[u]) + la * (am + log pbar - N[t]),     c = 1 - ll - la
// Zl the row log-sum-exp of lm, pbar the mean row softmax of lm over all B * U1 rows (+ the smallest normal float),
// N[t] = log sum_v e^{am[t,v]} pbar[v].  denom, the sweeps and the contractions stay as they are; what is new is
//   forward   smooth_lm_rows_kernel     one wave per row of lm: Zl, and the two lm-only arc terms of the row
//             smooth_colsum_kernel      (la > 0) column sums of the row softmaxes, 64 rows per workgroup, rows ascending
//             smooth_pbar_kernel        (la > 0) the partial sums added in order: pbar, log pbar
//             smooth_am_norm_kernel     (la > 0) one wave per row of am: N, and the am-only blank term of the row
//             smooth_interp_kernel      one thread per skewed position: rewrites the skewed log-probabilities (after the direct
//                                       repair kernel, so it sees final denom values)
//   backward  smooth_occ_rows_kernel / smooth_occ_cols_kernel    C(t) = sum_u occ, sum_t occ_blank, sum_t occ_emit
//             smooth_h_part_kernel / smooth_h_kernel   (la > 0) h[v] pbar[v] over all B * T rows, 64 rows per partial sum
//             smooth_am_row_kernel      (la > 0) d am[t] += la C(t) q_t
//             smooth_lm_row_kernel      d lm[u] += sigma(lm[u]) (ll R(u) + (h - <sigma, h>) / (B U1)), the second part for
//                                       la > 0 only and then for every row of lm, padded ones included
// A scale that is exactly 0 drops its branch (no launch, no term).  Every sum has one writer and a fixed order.
constexpr int kSmoothRows = 64;     // rows per partial column sum
constexpr float kTinyF = 1.17549435e-38f;
constexpr int kOccPhases = 16;    // phases of t in smooth_occ_cols_kernel (its workgroup has 64 * kOccPhases threads)

struct SmoothWs {
    SimpleWs s;
    size_t zl_off, lb_off, le_off, n_off, ab_off, cg_off, rb_off, re_off, pbar_off, lpbar_off, h_off, part_off, total;
    int lm_chunks, t_chunks;
};

inline SmoothWs smooth_ws_layout(int B, int T, int U1, int V)
{
    SmoothWs w;
    w.s = simple_ws_layout(B, T, U1);
    w.lm_chunks = (int)(((long)B * U1 + kSmoothRows - 1) / kSmoothRows);
    w.t_chunks = (T + kSmoothRows - 1) / kSmoothRows;
    const size_t bu = (size_t)B * U1 * sizeof(float), bt = (size_t)B * T * sizeof(float), vb = (size_t)V * sizeof(float);
    const size_t parts = (size_t)w.lm_chunks > (size_t)B * w.t_chunks ? (size_t)w.lm_chunks : (size_t)B * w.t_chunks;
    size_t off = w.s.total;
    w.zl_off = off;    off = align_up(off + bu, 256);      // Zl [B,U1]
    w.lb_off = off;    off = align_up(off + bu, 256);      // lm[u,blank] - Zl[u]
    w.le_off = off;    off = align_up(off + bu, 256);      // lm[u,y_u] - Zl[u]
    w.n_off = off;     off = align_up(off + bt, 256);      // N [B,T]
    w.ab_off = off;    off = align_up(off + bt, 256);      // am[t,blank] + log pbar[blank] - N[t]
    w.cg_off = off;    off = align_up(off + bt, 256);      // grad_costs * C(t)
    w.rb_off = off;    off = align_up(off + bu, 256);      // grad_costs * sum_t occ_blank(t,u)
    w.re_off = off;    off = align_up(off + bu, 256);      // grad_costs * sum_t occ_emit(t,u)
    w.pbar_off = off;  off = align_up(off + vb, 256);
    w.lpbar_off = off; off = align_up(off + vb, 256);
    w.h_off = off;     off = align_up(off + vb, 256);
    w.part_off = off;  off = align_up(off + parts * vb, 256);
    w.total = off;
    return w;
}

// One wave per row of lm (every row, padded ones too: pbar is defined over all of them).
__global__ __launch_bounds__(256) void smooth_lm_rows_kernel(
    const float *__restrict__ lm, const float *__restrict__ ml, const int32_t *__restrict__ symbols,
    const int32_t *__restrict__ tlens, long rows, int U1, int V, int blank, float *__restrict__ zl,
    float *__restrict__ lb, float *__restrict__ le)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long r = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const float *__restrict__ row = lm + (size_t)r * V;
    const float m = ml[r];
    float sum = 0.f;
#pragma unroll 8
    for (int v = lane; v < V; v += kWave) sum += fast_exp2((row[v] - m) * kLog2e);
    sum = wave_sum(sum);
    if (lane != 0) return;
    const double z = (double)m + (double)logf(sum);
    zl[r] = (float)z;
    const int b = (int)(r / U1), u = (int)(r - (long)b * U1);
    const int Ub = clampi(tlens[b], 0, U1 - 1);
    float fb = 0.f, fe = 0.f;
    if (u <= Ub) fb = (float)((double)row[blank] - z);
    if (u < Ub) fe = (float)((double)row[symbols[(size_t)b * (U1 - 1) + u]] - z);
    lb[r] = fb;
    le[r] = fe;
}

// part[chunk, v] = sum over the chunk's rows (ascending) of e^{x[r,v] - sub[r]} (pbar: x = lm, sub = Zl).
// grid (chunks, ceil(V/256)).
__global__ __launch_bounds__(256) void smooth_colsum_kernel(const float *__restrict__ x, const float *__restrict__ sub,
                                                            long rows, int V, float *__restrict__ part)
{
    const int v = blockIdx.y * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const long r0 = (long)blockIdx.x * kSmoothRows;
    const long r1 = r0 + kSmoothRows < rows ? r0 + kSmoothRows : rows;
    float acc = 0.f;
#pragma unroll 8
    for (long r = r0; r < r1; ++r) acc += fast_exp2((x[(size_t)r * V + v] - sub[r]) * kLog2e);
    part[(size_t)blockIdx.x * V + v] = acc;
}

__global__ __launch_bounds__(256) void smooth_pbar_kernel(const float *__restrict__ part, int chunks, long rows, int V,
                                                          float *__restrict__ pbar, float *__restrict__ lpbar)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    float acc = 0.f;
#pragma unroll 16
    for (int c = 0; c < chunks; ++c) acc += part[(size_t)c * V + v];
    const float p = acc / (float)rows + kTinyF;
    pbar[v] = p;
    lpbar[v] = logf(p);
}

// One wave per valid row of am: N[t] = ma[t] + log sum_v e^{am[t,v] - ma[t]} pbar[v]; the sum holds the term of am's
// maximum, pbar >= the smallest normal float, so it is never zero.
__global__ __launch_bounds__(256) void smooth_am_norm_kernel(
    const float *__restrict__ am, const float *__restrict__ ma, const float *__restrict__ pbar,
    const float *__restrict__ lpbar, const int32_t *__restrict__ llens, int B, int T, int V, int blank,
    float *__restrict__ nrm, float *__restrict__ ab)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long r = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= (long)B * T) return;
    const int b = (int)(r / T), t = (int)(r - (long)b * T);
    if (t >= clampi(llens[b], 0, T)) {
        if (lane == 0) { nrm[r] = 0.f; ab[r] = 0.f; }
        return;
    }
    const float *__restrict__ row = am + (size_t)r * V;
    const float m = ma[r];
    float sum = 0.f;
#pragma unroll 4
    for (int v = lane; v < V; v += kWave) sum += fast_exp2((row[v] - m) * kLog2e) * pbar[v];
    sum = wave_sum(sum);
    if (lane != 0) return;
    const double n = (double)m + (double)logf(sum);
    nrm[r] = (float)n;
    ab[r] = (float)(((double)row[blank] + (double)lpbar[blank]) - n);
}

// One thread per position (b, s = t + u, u) of the skewed layout, so that a wave reads and writes whole lines of it
// (a thread per (b,t,u) touches one 32-byte sector per cell).  AM: the am-only branch is present (the only form that
// reads am).
template <bool AM>
__global__ __launch_bounds__(256) void smooth_interp_kernel(
    const float *__restrict__ am, const int32_t *__restrict__ symbols, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, int B, int T, int U1, int V, int S, float c, float ll, float la,
    const float *__restrict__ lb, const float *__restrict__ le, const float *__restrict__ nrm,
    const float *__restrict__ ab, const float *__restrict__ lpbar, float2 *__restrict__ lp_skew)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)B * S * U1) return;
    const long diag = (long)S * U1;
    const int b = (int)(r / diag);
    const long cc = r - b * diag;
    const int sd = (int)(cc / U1), u = (int)(cc - (long)sd * U1), t = sd - u;
    const int Tb = clampi(llens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
    if (t < 0 || t >= Tb || u > Ub) return;
    const size_t idx = (size_t)r;
    const float2 lp = lp_skew[idx];
    double x = (double)c * (double)lp.x, y = 0.0;
    if (ll != 0.f) x += (double)ll * (double)lb[(size_t)b * U1 + u];
    if (AM) x += (double)la * (double)ab[(size_t)b * T + t];
    if (u < Ub) {
        y = (double)c * (double)lp.y;
        if (ll != 0.f) y += (double)ll * (double)le[(size_t)b * U1 + u];
        if (AM) {
            const int lab = symbols[(size_t)b * (U1 - 1) + u];
            y += (double)la * (((double)am[((size_t)b * T + t) * V + lab] + (double)lpbar[lab]) - (double)nrm[(size_t)b * T + t]);
        }
    }
    lp_skew[idx] = make_float2((float)x, (float)y);
}

// cg[b,t] = sum_u (ob + oe)(t,u): one wave per (b,t); ob / oe are zero outside the valid region.
__global__ __launch_bounds__(256) void smooth_occ_rows_kernel(const float *__restrict__ ob, const float *__restrict__ oe,
                                                              long rows, int U1, float *__restrict__ cg)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long r = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    float part = 0.f;
    for (int u = lane; u < U1; u += kWave) part += ob[(size_t)r * U1 + u] + oe[(size_t)r * U1 + u];
    part = wave_sum(part);
    if (lane == 0) cg[r] = part;
}

// rb[b,u] = sum_t ob(t,u), re[b,u] = sum_t oe(t,u): sixteen phases of t per workgroup (the loop is a chain of
// dependent L2 round trips, so its length is the kernel's time), added in order.  grid (ceil(U1/64), B), 1024 threads.
__global__ __launch_bounds__(1024) void smooth_occ_cols_kernel(const float *__restrict__ ob, const float *__restrict__ oe,
                                                              int T, int U1, float *__restrict__ rb, float *__restrict__ re)
{
    __shared__ float sb[kOccPhases][64], se[kOccPhases][64];
    const int b = blockIdx.y;
    const int ul = threadIdx.x & 63, ph = threadIdx.x >> 6;
    const int u = blockIdx.x * 64 + ul;
    float pb = 0.f, pe = 0.f;
    if (u < U1) {
#pragma unroll 8
        for (int t = ph; t < T; t += kOccPhases) {
            const size_t cell = ((size_t)b * T + t) * U1 + u;
            pb += ob[cell];
            pe += oe[cell];
        }
    }
    sb[ph][ul] = pb;
    se[ph][ul] = pe;
    __syncthreads();
    if (ph != 0 || u >= U1) return;
    float tb = sb[0][ul], te = se[0][ul];
#pragma unroll
    for (int p = 1; p < kOccPhases; ++p) { tb += sb[p][ul]; te += se[p][ul]; }
    rb[(size_t)b * U1 + u] = tb;
    re[(size_t)b * U1 + u] = te;
}

// h is kept as hp[v] = h[v] * pbar[v] = la * sum_b (sum_t cg[b,t] q_t[v] - what the arcs of b subtract at v), which is
// bounded (q_t[v] = e^{am - N + log pbar[v]} <= 1) where h itself overflows for a symbol that lm never predicts.
// part[b * TC + tc, v] = sum_{t in chunk tc, t < T_b} cg[b,t] q_t[v], and from chunk 0 of every utterance minus what its
// arcs subtract at v.  grid (ceil(V/256), TC, B).
__global__ __launch_bounds__(256) void smooth_h_part_kernel(
    const float *__restrict__ am, const float *__restrict__ nrm, const float *__restrict__ cg,
    const float *__restrict__ rb, const float *__restrict__ re, const float *__restrict__ lpbar,
    const int32_t *__restrict__ symbols, const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int T,
    int U1, int V, int blank, float *__restrict__ part)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const int b = blockIdx.z, tc = blockIdx.y;
    const int Tb = clampi(llens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
    const int t0 = tc * kSmoothRows, t1 = min(t0 + kSmoothRows, Tb);
    const float *__restrict__ amb = am + (size_t)b * T * V + v;
    const float lp = lpbar[v];
    float acc = 0.f;
#pragma unroll 8
    for (int t = t0; t < t1; ++t)
        acc += cg[(size_t)b * T + t] * fast_exp2(((amb[(size_t)t * V] - nrm[(size_t)b * T + t]) + lp) * kLog2e);
    if (tc == 0 && Tb > 0) {
        float sub = 0.f;
        for (int u = 0; u <= Ub; ++u) {
            if (v == blank) sub += rb[(size_t)b * U1 + u];
            if (u < Ub && symbols[(size_t)b * (U1 - 1) + u] == v) sub += re[(size_t)b * U1 + u];
        }
        acc -= sub;
    }
    part[((size_t)b * gridDim.y + tc) * V + v] = acc;
}

__global__ __launch_bounds__(256) void smooth_h_kernel(const float *__restrict__ part, int parts, int V, float la,
                                                       float *__restrict__ hp)
{
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    float acc = 0.f;
#pragma unroll 16
    for (int p = 0; p < parts; ++p) acc += part[(size_t)p * V + v];
    hp[v] = la * acc;
}

// d am[b,t,v] += la * cg[b,t] * q_t[v],  q_t[v] = e^{am - N + log pbar[v]}, on the valid rows: one wave per row.
__global__ __launch_bounds__(256) void smooth_am_row_kernel(
    const float *__restrict__ am, const float *__restrict__ nrm, const float *__restrict__ cg,
    const float *__restrict__ lpbar, const int32_t *__restrict__ llens, int B, int T, int V, float la,
    float *__restrict__ d_am)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long r = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= (long)B * T) return;
    const int b = (int)(r / T), t = (int)(r - (long)b * T);
    if (t >= clampi(llens[b], 0, T)) return;
    const float *__restrict__ row = am + (size_t)r * V;
    float *__restrict__ out = d_am + (size_t)r * V;
    const float n = nrm[r], f = la * cg[r];
#pragma unroll 4
    for (int v = lane; v < V; v += kWave) out[v] += f * fast_exp2(((row[v] - n) + lpbar[v]) * kLog2e);
}

// d lm[b,u,v] += s[v] * ll * (rb + re)[b,u] + (r[v] hp[v] - s[v] sum_w r[w] hp[w]) * inv_rows,  s = e^{lm[b,u] - Zl[b,u]},
// r[v] = s[v] / pbar[v] <= B * U1 (pbar holds s[v] / (B * U1) of this very row).
// UNI (la > 0): every row of lm; otherwise the valid rows only, and the padded ones stay exactly zero.
template <bool UNI>
__global__ __launch_bounds__(256) void smooth_lm_row_kernel(
    const float *__restrict__ lm, const float *__restrict__ zl, const float *__restrict__ rb,
    const float *__restrict__ re, const float *__restrict__ hp, const float *__restrict__ pbar,
    const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, long rows, int T, int U1, int V, float ll, float inv_rows,
    float *__restrict__ d_lm)
{
    const int lane = threadIdx.x & (kWave - 1);
    const long r = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int b = (int)(r / U1), u = (int)(r - (long)b * U1);
    const bool valid = clampi(llens[b], 0, T) > 0 && u <= clampi(tlens[b], 0, U1 - 1);
    if (!UNI && !valid) return;
    const float *__restrict__ row = lm + (size_t)r * V;
    float *__restrict__ out = d_lm + (size_t)r * V;
    const float z = zl[r];
    const float f = valid ? ll * (rb[r] + re[r]) : 0.f;
    float dot = 0.f;
    if (UNI) {
#pragma unroll 4
        for (int v = lane; v < V; v += kWave) dot += fast_exp2((row[v] - z) * kLog2e) / pbar[v] * hp[v];
        dot = wave_sum(dot);
    }
#pragma unroll 4
    for (int v = lane; v < V; v += kWave) {
        const float s = fast_exp2((row[v] - z) * kLog2e);
        out[v] += UNI ? s * f + (s / pbar[v] * hp[v] - s * dot) * inv_rows : s * f;
    }
}

int simple_check(const char *what, int B, int T, int U1, int V, int blank)
{
    WR_REQUIRE(B > 0 && T > 0 && U1 > 0, WR_EINVAL, "%s: B, T, U1 must be positive (got %d,%d,%d)", what, B, T, U1);
    WR_REQUIRE(V >= 2, WR_EINVAL, "%s: V = %d, at least 2 classes are needed", what, V);
    WR_REQUIRE(blank >= 0 && blank < V, WR_EINVAL, "%s: blank %d out of range [0,%d)", what, blank, V);
    WR_REQUIRE(U1 <= kRnntMaxCols, WR_EUNSUPPORTED, "%s: U1=%d exceeds the sweep kernel's limit of %d label columns", what,
               U1, kRnntMaxCols);
    WR_REQUIRE((long)B * T * U1 < (1L << 31), WR_EUNSUPPORTED, "%s: more than 2^31 lattice cells", what);
    WR_REQUIRE(B <= 65535 && T <= 64 * 65535, WR_EUNSUPPORTED, "%s: B is limited to 65535 and T to 64 * 65535 (got %d,%d)",
               what, B, T);
    return WR_OK;
}

// The kernels of wr_rnnt_simple_stats (arguments checked by the caller).
int simple_stats_launch(const float *am_d, const float *lm_d, const int32_t *symbols_d, const int32_t *logit_lengths_d,
                        const int32_t *target_lengths_d, int B, int T, int U1, int V, int blank, const SimpleWs &sw,
                        const RnntWs &w, char *sws, char *ws, hipStream_t st)
{
    float *ma = reinterpret_cast<float *>(sws + sw.ma_off), *ml = reinterpret_cast<float *>(sws + sw.ml_off);
    float2 *lp = reinterpret_cast<float2 *>(ws + w.lp_off);
    float *denom = reinterpret_cast<float *>(ws + w.denom_off);
    int32_t *flag = reinterpret_cast<int32_t *>(ws + w.flag_off);

    const long rows_am = (long)B * T, rows_lm = (long)B * U1;
    WR_TRY(launch("simple_rowmax_kernel", simple_rowmax_kernel, dim3((unsigned)((rows_am + rows_lm + 3) / 4)), dim3(256), 0,
                  st, am_d, lm_d, rows_am, rows_lm, V, ma, ml, flag));
    WR_TRY(launch("simple_stats_kernel", simple_stats_kernel, dim3((U1 + kTile - 1) / kTile, (T + kTile - 1) / kTile, B),
                  dim3(256), 0, st, am_d, lm_d, symbols_d, logit_lengths_d, target_lengths_d, T, U1, V, blank, w.S, ma, ml,
                  lp, denom, flag));
    long blocks = ((long)B * T * U1 + 3) / 4;
    if (blocks > 256L * 16) blocks = 256L * 16;
    return launch("simple_stats_direct_kernel", simple_stats_direct_kernel, dim3((unsigned)blocks), dim3(256), 0, st, am_d,
                  lm_d, symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V, blank, w.S, lp, denom, flag);
}

// The occupancies (always) and, unless `occ_only`, the kernels of wr_rnnt_simple_grad up to the contractions: G scaled by
// `gscale`.  The scatter terms follow in simple_fix_launch, after whatever the caller adds to the rows.
int simple_grad_launch(const float *am_d, const float *lm_d, const int32_t *symbols_d, const int32_t *logit_lengths_d,
                       const int32_t *target_lengths_d, int B, int T, int U1, int V, const float *grad_costs_d,
                       float *d_am_d, float *d_lm_d, float *occ_emit_d, float *occ_blank_d, const SimpleWs &sw,
                       const RnntWs &w, char *sws, const char *ws, float gscale, bool occ_only, bool modified,
                       hipStream_t st)
{
    const float *ma = reinterpret_cast<const float *>(sws + sw.ma_off), *ml = reinterpret_cast<const float *>(sws + sw.ml_off);
    float *g = reinterpret_cast<float *>(sws + sw.g_off), *gt = reinterpret_cast<float *>(sws + sw.gt_off);
    float *ob = reinterpret_cast<float *>(sws + sw.ob_off), *oe = reinterpret_cast<float *>(sws + sw.oe_off);
    int32_t *nxt = reinterpret_cast<int32_t *>(sws + sw.nxt_off), *head = reinterpret_cast<int32_t *>(sws + sw.head_off);
    const float *denom = reinterpret_cast<const float *>(ws + w.denom_off);
    const int32_t *flag = reinterpret_cast<const int32_t *>(ws + w.flag_off);
    const long cells = (long)B * T * U1;

    const LatView lv = lattice_view(w, ws, modified);
    // (the modified arm first: the order of the arms is the order of the kernels in the code object)
    WR_TRY(with_bool(modified, [&](auto mod) {
        constexpr int LAT = mod.value ? kLatModified : kLatRegular;
        return launch("simple_occ_kernel", simple_occ_kernel<LAT>, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st,
                      logit_lengths_d, target_lengths_d, B, T, U1, w.S, lv.alpha, lv.beta, lv.lp, denom,
                      reinterpret_cast<const double *>(ws + w.cost_off), ma, ml, grad_costs_d, flag, gscale, g, gt, ob, oe,
                      occ_emit_d, occ_blank_d);
    }));
    if (occ_only) return WR_OK;
    WR_TRY(launch("simple_chain_kernel", simple_chain_kernel, dim3(B), dim3(256), 0, st, symbols_d, target_lengths_d, U1,
                  nxt, head));

    const unsigned vg = (unsigned)((V + kGemmCols - 1) / kGemmCols), vd = (unsigned)((V + 255) / 256);
    WR_TRY(launch("simple_grad_gemm_kernel<am>", simple_grad_gemm_kernel<true>, dim3(vg, (T + kTile - 1) / kTile, B),
                  dim3(256), 0, st, gt, am_d, ma, lm_d, ml, logit_lengths_d, target_lengths_d, T, U1, V, flag, d_am_d));
    WR_TRY(launch("simple_grad_gemm_kernel<lm>", simple_grad_gemm_kernel<false>, dim3(vg, (U1 + kTile - 1) / kTile, B),
                  dim3(256), 0, st, g, lm_d, ml, am_d, ma, logit_lengths_d, target_lengths_d, T, U1, V, flag, d_lm_d));
    WR_TRY(launch("simple_grad_direct_kernel<am>", simple_grad_direct_kernel<true>, dim3(vd, T < 64 ? T : 64, B), dim3(256),
                  0, st, g, denom, am_d, lm_d, logit_lengths_d, target_lengths_d, T, U1, V, flag, d_am_d));
    return launch("simple_grad_direct_kernel<lm>", simple_grad_direct_kernel<false>, dim3(vd, U1 < 64 ? U1 : 64, B),
                  dim3(256), 0, st, g, denom, lm_d, am_d, logit_lengths_d, target_lengths_d, T, U1, V, flag, d_lm_d);
}

int simple_fix_launch(const int32_t *symbols_d, const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B,
                      int T, int U1, int V, int blank, float *d_am_d, float *d_lm_d, const SimpleWs &sw, char *sws,
                      float w_am, float w_lm, bool every_arc, hipStream_t st)
{
    const float *ob = reinterpret_cast<const float *>(sws + sw.ob_off), *oe = reinterpret_cast<const float *>(sws + sw.oe_off);
    const int32_t *nxt = reinterpret_cast<const int32_t *>(sws + sw.nxt_off);
    const int32_t *head = reinterpret_cast<const int32_t *>(sws + sw.head_off);
    WR_TRY(launch("simple_fix_am_kernel", simple_fix_am_kernel, dim3((unsigned)(((long)B * T + 3) / 4)), dim3(256), 0, st,
                  ob, oe, nxt, head, symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V, blank, w_am, every_arc,
                  d_am_d));
    return launch("simple_fix_lm_kernel", simple_fix_lm_kernel, dim3((U1 + 63) / 64, B), dim3(256), 0, st, ob, oe,
                  symbols_d, logit_lengths_d, target_lengths_d, T, U1, V, blank, w_lm, every_arc, d_lm_d);
}

int smooth_check(const char *what, float ll, float la, int V)
{
    WR_REQUIRE(ll >= 0.f && la >= 0.f, WR_EINVAL, "%s: lm_only_scale %g and am_only_scale %g must not be negative", what,
               (double)ll, (double)la);
    WR_REQUIRE(ll + la <= 1.f, WR_EINVAL, "%s: lm_only_scale + am_only_scale = %g exceeds 1", what, (double)(ll + la));
    WR_REQUIRE((ll == 0.f && la == 0.f) || V <= 256 * 65535, WR_EUNSUPPORTED, "%s: V = %d exceeds %d", what, V, 256 * 65535);
    return WR_OK;
}

// The scratch a call with these scales touches: with both 0 only the simple loss's part, where SmoothWs begins.
inline size_t smooth_ws_required(const SmoothWs &mw, float ll, float la) { return ll == 0.f && la == 0.f ? mw.s.total : mw.total; }

}  // namespace
}  // namespace wr

using namespace wr;

extern "C" size_t wr_rnnt_simple_workspace_bytes(int B, int T, int U1, int V)
{
    if (B <= 0 || T <= 0 || U1 <= 0 || V <= 0) return 0;
    return simple_ws_layout(B, T, U1).total;
}

extern "C" size_t wr_rnnt_smoothed_workspace_bytes(int B, int T, int U1, int V)
{
    if (B <= 0 || T <= 0 || U1 <= 0 || V <= 0) return 0;
    return smooth_ws_layout(B, T, U1, V).total;
}

// wr_rnnt_smoothed_stats, and with both scales 0 wr_rnnt_simple_stats; `what` names the entry point in messages.
static int smoothed_stats_impl(const char *what, const float *am_d, const float *lm_d, const int32_t *symbols_d,
                               const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1, int V,
                               int blank, float lm_only_scale, float am_only_scale, void *smoothed_workspace_d,
                               size_t smoothed_workspace_bytes, void *rnnt_workspace_d, size_t rnnt_workspace_bytes,
                               void *stream)
{
    const float ll = lm_only_scale, la = am_only_scale;
    if (int rc = simple_check(what, B, T, U1, V, blank)) return rc;
    if (int rc = smooth_check(what, ll, la, V)) return rc;
    const SmoothWs mw = smooth_ws_layout(B, T, U1, V);
    const RnntWs w = rnnt_ws_layout(B, T, U1);
    const size_t need = smooth_ws_required(mw, ll, la);
    WR_REQUIRE(smoothed_workspace_bytes >= need, WR_EWORKSPACE, "%s: workspace %zu < required %zu", what,
               smoothed_workspace_bytes, need);
    WR_REQUIRE(rnnt_workspace_bytes >= w.total, WR_EWORKSPACE, "%s: rnnt workspace %zu < required %zu", what,
               rnnt_workspace_bytes, w.total);
    WR_REQUIRE(am_d && lm_d && logit_lengths_d && target_lengths_d && smoothed_workspace_d && rnnt_workspace_d, WR_EINVAL,
               "%s: null pointer argument", what);
    WR_REQUIRE(symbols_d || U1 == 1, WR_EINVAL, "%s: symbols is null", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *sws = static_cast<char *>(smoothed_workspace_d), *ws = static_cast<char *>(rnnt_workspace_d);
    if (int rc = simple_stats_launch(am_d, lm_d, symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V, blank, mw.s, w,
                                     sws, ws, st))
        return rc;
    if (ll == 0.f && la == 0.f) return WR_OK;             // rnnt_loss_simple, by the same kernels

    const float *ml = reinterpret_cast<const float *>(sws + mw.s.ml_off), *ma = reinterpret_cast<const float *>(sws + mw.s.ma_off);
    float *zl = reinterpret_cast<float *>(sws + mw.zl_off), *lb = reinterpret_cast<float *>(sws + mw.lb_off);
    float *le = reinterpret_cast<float *>(sws + mw.le_off), *nrm = reinterpret_cast<float *>(sws + mw.n_off);
    float *ab = reinterpret_cast<float *>(sws + mw.ab_off), *pbar = reinterpret_cast<float *>(sws + mw.pbar_off);
    float *lpbar = reinterpret_cast<float *>(sws + mw.lpbar_off), *part = reinterpret_cast<float *>(sws + mw.part_off);
    const long rows_lm = (long)B * U1, rows_am = (long)B * T, cells = (long)B * w.S * U1;
    const unsigned vb = (unsigned)((V + 255) / 256);
    const float c = (float)(1.0 - (double)ll - (double)la);

    WR_TRY(launch("smooth_lm_rows_kernel", smooth_lm_rows_kernel, dim3((unsigned)((rows_lm + 3) / 4)), dim3(256), 0, st,
                  lm_d, ml, symbols_d, target_lengths_d, rows_lm, U1, V, blank, zl, lb, le));
    if (la != 0.f) {
        WR_TRY(launch("smooth_colsum_kernel", smooth_colsum_kernel, dim3(mw.lm_chunks, vb), dim3(256), 0, st, lm_d, zl,
                      rows_lm, V, part));
        WR_TRY(launch("smooth_pbar_kernel", smooth_pbar_kernel, dim3(vb), dim3(256), 0, st, part, mw.lm_chunks, rows_lm, V,
                      pbar, lpbar));
        WR_TRY(launch("smooth_am_norm_kernel", smooth_am_norm_kernel, dim3((unsigned)((rows_am + 3) / 4)), dim3(256), 0, st,
                      am_d, ma, pbar, lpbar, logit_lengths_d, B, T, V, blank, nrm, ab));
        WR_TRY(launch("smooth_interp_kernel<am>", smooth_interp_kernel<true>, dim3((unsigned)((cells + 255) / 256)),
                      dim3(256), 0, st, am_d, symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V, w.S, c, ll, la, lb,
                      le, nrm, ab, lpbar, reinterpret_cast<float2 *>(ws + w.lp_off)));
    } else {
        WR_TRY(launch("smooth_interp_kernel<lm>", smooth_interp_kernel<false>, dim3((unsigned)((cells + 255) / 256)),
                      dim3(256), 0, st, (const float *)nullptr, symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V,
                      w.S, c, ll, la, lb, le, (const float *)nullptr, (const float *)nullptr, (const float *)nullptr,
                      reinterpret_cast<float2 *>(ws + w.lp_off)));
    }
    return WR_OK;
}

// wr_rnnt_smoothed_grad, wr_rnnt_smoothed_grad_lattice and, with both scales 0 and `need_grads`, wr_rnnt_simple_grad;
// `what` names the entry point in messages.  On the modified lattice every arc is subtracted at its own symbol whatever
// the scales (a label equal to the blank has both terms), as under smoothing.
static int smoothed_grad_impl(const char *what, bool need_grads, const float *am_d, const float *lm_d,
                              const int32_t *symbols_d, const int32_t *logit_lengths_d, const int32_t *target_lengths_d,
                              int B, int T, int U1, int V, int blank, float lm_only_scale, float am_only_scale,
                              const float *grad_costs_d, float *d_am_d, float *d_lm_d, float *occ_emit_d,
                              float *occ_blank_d, void *smoothed_workspace_d, size_t smoothed_workspace_bytes,
                              const void *rnnt_workspace_d, size_t rnnt_workspace_bytes, bool modified, void *stream)
{
    const float ll = lm_only_scale, la = am_only_scale;
    if (int rc = simple_check(what, B, T, U1, V, blank)) return rc;
    if (int rc = smooth_check(what, ll, la, V)) return rc;
    const SmoothWs mw = smooth_ws_layout(B, T, U1, V);
    const RnntWs w = rnnt_ws_layout(B, T, U1);
    const size_t need = smooth_ws_required(mw, ll, la);
    WR_REQUIRE(smoothed_workspace_bytes >= need, WR_EWORKSPACE, "%s: workspace %zu < required %zu", what,
               smoothed_workspace_bytes, need);
    WR_REQUIRE(rnnt_workspace_bytes >= w.total, WR_EWORKSPACE, "%s: rnnt workspace %zu < required %zu", what,
               rnnt_workspace_bytes, w.total);
    const bool occ_only = !d_am_d && !d_lm_d;
    WR_REQUIRE(am_d && lm_d && logit_lengths_d && target_lengths_d && smoothed_workspace_d && rnnt_workspace_d &&
                   (!need_grads || (d_am_d && d_lm_d)), WR_EINVAL, "%s: null pointer argument", what);
    WR_REQUIRE(occ_only ? (occ_emit_d && occ_blank_d) : (d_am_d && d_lm_d), WR_EINVAL,
               "%s: d_am and d_lm go together; without them both occupancy outputs are needed", what);
    WR_REQUIRE(symbols_d || U1 == 1, WR_EINVAL, "%s: symbols is null", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *sws = static_cast<char *>(smoothed_workspace_d);
    const bool smooth = ll != 0.f || la != 0.f;
    const float c = smooth ? (float)(1.0 - (double)ll - (double)la) : 1.f;
    if (int rc = simple_grad_launch(am_d, lm_d, symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V, grad_costs_d,
                                    d_am_d, d_lm_d, occ_emit_d, occ_blank_d, mw.s, w, sws,
                                    static_cast<const char *>(rnnt_workspace_d), c, occ_only, modified, st))
        return rc;
    if (occ_only) return WR_OK;
    if (smooth) {
        const float *ob = reinterpret_cast<const float *>(sws + mw.s.ob_off), *oe = reinterpret_cast<const float *>(sws + mw.s.oe_off);
        const float *zl = reinterpret_cast<const float *>(sws + mw.zl_off), *nrm = reinterpret_cast<const float *>(sws + mw.n_off);
        const float *pbar = reinterpret_cast<const float *>(sws + mw.pbar_off);
        const float *lpbar = reinterpret_cast<const float *>(sws + mw.lpbar_off);
        float *cg = reinterpret_cast<float *>(sws + mw.cg_off), *rb = reinterpret_cast<float *>(sws + mw.rb_off);
        float *re = reinterpret_cast<float *>(sws + mw.re_off), *h = reinterpret_cast<float *>(sws + mw.h_off);
        float *part = reinterpret_cast<float *>(sws + mw.part_off);
        const long rows_lm = (long)B * U1, rows_am = (long)B * T;
        const unsigned vb = (unsigned)((V + 255) / 256);
        WR_TRY(launch("smooth_occ_cols_kernel", smooth_occ_cols_kernel, dim3((U1 + 63) / 64, B), dim3(64 * kOccPhases), 0,
                      st, ob, oe, T, U1, rb, re));
        if (la != 0.f) {
            WR_TRY(launch("smooth_occ_rows_kernel", smooth_occ_rows_kernel, dim3((unsigned)((rows_am + 3) / 4)), dim3(256),
                          0, st, ob, oe, rows_am, U1, cg));
            WR_TRY(launch("smooth_h_part_kernel", smooth_h_part_kernel, dim3(vb, mw.t_chunks, B), dim3(256), 0, st, am_d,
                          nrm, cg, rb, re, lpbar, symbols_d, logit_lengths_d, target_lengths_d, T, U1, V, blank, part));
            WR_TRY(launch("smooth_h_kernel", smooth_h_kernel, dim3(vb), dim3(256), 0, st, part, B * mw.t_chunks, V, la, h));
            WR_TRY(launch("smooth_am_row_kernel", smooth_am_row_kernel, dim3((unsigned)((rows_am + 3) / 4)), dim3(256), 0,
                          st, am_d, nrm, cg, lpbar, logit_lengths_d, B, T, V, la, d_am_d));
            WR_TRY(launch("smooth_lm_row_kernel<unigram>", smooth_lm_row_kernel<true>, dim3((unsigned)((rows_lm + 3) / 4)),
                          dim3(256), 0, st, lm_d, zl, rb, re, h, pbar, logit_lengths_d, target_lengths_d, rows_lm, T, U1, V,
                          ll, 1.f / (float)rows_lm, d_lm_d));
        } else {
            WR_TRY(launch("smooth_lm_row_kernel<rows>", smooth_lm_row_kernel<false>, dim3((unsigned)((rows_lm + 3) / 4)),
                          dim3(256), 0, st, lm_d, zl, rb, re, (const float *)nullptr, (const float *)nullptr,
                          logit_lengths_d, target_lengths_d, rows_lm, T, U1, V, ll, 0.f, d_lm_d));
        }
    }
    return simple_fix_launch(symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V, blank, d_am_d, d_lm_d, mw.s, sws,
                             smooth ? c + la : 1.f, smooth ? c + ll : 1.f, smooth || modified, st);
}

extern "C" int wr_rnnt_smoothed_stats(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                                      const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T,
                                      int U1, int V, int blank, float lm_only_scale, float am_only_scale,
                                      void *smoothed_workspace_d, size_t smoothed_workspace_bytes, void *rnnt_workspace_d,
                                      size_t rnnt_workspace_bytes, void *stream)
{
    return smoothed_stats_impl("rnnt_smoothed_stats", am_d, lm_d, symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V,
                               blank, lm_only_scale, am_only_scale, smoothed_workspace_d, smoothed_workspace_bytes,
                               rnnt_workspace_d, rnnt_workspace_bytes, stream);
}

extern "C" int wr_rnnt_simple_stats(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                                    const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1,
                                    int V, int blank, void *simple_workspace_d, size_t simple_workspace_bytes,
                                    void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream)
{
    return smoothed_stats_impl("rnnt_simple_stats", am_d, lm_d, symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V,
                               blank, 0.f, 0.f, simple_workspace_d, simple_workspace_bytes, rnnt_workspace_d,
                               rnnt_workspace_bytes, stream);
}

extern "C" int wr_rnnt_simple_grad(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                                   const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1,
                                   int V, int blank, const float *grad_costs_d, float *d_am_d, float *d_lm_d,
                                   float *occ_emit_d, float *occ_blank_d, void *simple_workspace_d,
                                   size_t simple_workspace_bytes, const void *rnnt_workspace_d,
                                   size_t rnnt_workspace_bytes, void *stream)
{
    return smoothed_grad_impl("rnnt_simple_grad", true, am_d, lm_d, symbols_d, logit_lengths_d, target_lengths_d, B, T, U1,
                              V, blank, 0.f, 0.f, grad_costs_d, d_am_d, d_lm_d, occ_emit_d, occ_blank_d, simple_workspace_d,
                              simple_workspace_bytes, rnnt_workspace_d, rnnt_workspace_bytes, false, stream);
}

extern "C" int wr_rnnt_smoothed_grad(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                                     const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T,
                                     int U1, int V, int blank, float lm_only_scale, float am_only_scale,
                                     const float *grad_costs_d, float *d_am_d, float *d_lm_d, float *occ_emit_d,
                                     float *occ_blank_d, void *smoothed_workspace_d, size_t smoothed_workspace_bytes,
                                     const void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream)
{
    return smoothed_grad_impl("rnnt_smoothed_grad", false, am_d, lm_d, symbols_d, logit_lengths_d, target_lengths_d, B, T,
                              U1, V, blank, lm_only_scale, am_only_scale, grad_costs_d, d_am_d, d_lm_d, occ_emit_d,
                              occ_blank_d, smoothed_workspace_d, smoothed_workspace_bytes, rnnt_workspace_d,
                              rnnt_workspace_bytes, false, stream);
}

extern "C" int wr_rnnt_smoothed_grad_lattice(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                                             const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B,
                                             int T, int U1, int V, int blank, float lm_only_scale, float am_only_scale,
                                             int lattice_type, const float *grad_costs_d, float *d_am_d, float *d_lm_d,
                                             float *occ_emit_d, float *occ_blank_d, void *smoothed_workspace_d,
                                             size_t smoothed_workspace_bytes, const void *rnnt_workspace_d,
                                             size_t rnnt_workspace_bytes, void *stream)
{
    if (int rc = lattice_check("rnnt_smoothed_grad_lattice", lattice_type, 0.0)) return rc;
    return smoothed_grad_impl("rnnt_smoothed_grad_lattice", false, am_d, lm_d, symbols_d, logit_lengths_d, target_lengths_d,
                              B, T, U1, V, blank, lm_only_scale, am_only_scale, grad_costs_d, d_am_d, d_lm_d, occ_emit_d,
                              occ_blank_d, smoothed_workspace_d, smoothed_workspace_bytes, rnnt_workspace_d,
                              rnnt_workspace_bytes, lattice_type == WR_LATTICE_MODIFIED, stream);
}
