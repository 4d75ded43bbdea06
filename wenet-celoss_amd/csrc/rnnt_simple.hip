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
#include "row_stream.hpp"
#include "wr_common.hpp"

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

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

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
// direct gradient kernel's factor; e^{ma+ml-denom} may overflow there).
__global__ __launch_bounds__(256) void simple_occ_kernel(
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int B, int T, int U1, int S,
    const double *__restrict__ alpha_skew, const double *__restrict__ beta_skew, const float2 *__restrict__ lp_skew,
    const float *__restrict__ denom, const double *__restrict__ cost_ws, const float *__restrict__ ma,
    const float *__restrict__ ml, const float *__restrict__ grad_costs, const int32_t *__restrict__ flag,
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
        const double al = alpha_skew[dbase + (size_t)s * U1 + u];
        const double be = beta_skew[dbase + (size_t)s * U1 + u];
        const double ac = al + cost_ws[b];                      // cost = -ll
        const float2 lp = lp_skew[dbase + (size_t)s * U1 + u];
        const double lo = ac + be;                              // log occupancy of the node
        if (*flag != 0) gv = (float)exp(lo);
        else gv = (float)exp(lo + (((double)ma[(size_t)b * T + t] + (double)ml[(size_t)b * U1 + u]) - (double)denom[r]));
        if (t < Tb - 1) fb = (float)exp(ac + (double)lp.x + beta_skew[dbase + (size_t)(s + 1) * U1 + u]);
        else if (u == Ub) fb = (float)exp(ac + (double)lp.x);   // the final cell: beta := 0
        if (u < Ub) fe = (float)exp(ac + (double)lp.y + beta_skew[dbase + (size_t)(s + 1) * U1 + (u + 1)]);
    }
    g[r] = gv * go;
    gt[((size_t)b * U1 + u) * T + t] = gv * go;
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
__global__ __launch_bounds__(256) void simple_fix_am_kernel(
    const float *__restrict__ ob, const float *__restrict__ oe, const int32_t *__restrict__ nxt,
    const int32_t *__restrict__ head, const int32_t *__restrict__ symbols, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, int B, int T, int U1, int V, int blank, float *__restrict__ d_am)
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
        if (u < Ub && sy[u] == blank && t == Tb - 1) part += oer[u];
    }
    const float tot = wave_sum(part);
    if (lane == 0) row[blank] -= tot;
    for (int u = lane; u < Ub; u += kWave) {
        const int lab = sy[u];
        if (lab == blank || head[(size_t)b * U1 + u] == 0) continue;
        float s = oer[u];
        for (int j = nx[u]; j >= 0; j = nx[j]) s += oer[j];
        row[lab] -= s;
    }
}

// d lm[u, blank] -= sum_t occ_blank(t,u) ; d lm[u, lab_u] -= sum_t occ_emit(t,u).  One workgroup per (b, 64 columns u):
// thread (u, phase) sums t = phase, phase + 4, ... ; the four phases are added in order.
__global__ __launch_bounds__(256) void simple_fix_lm_kernel(
    const float *__restrict__ ob, const float *__restrict__ oe, const int32_t *__restrict__ symbols,
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int T, int U1, int V, int blank,
    float *__restrict__ d_lm)
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
    if (lab == blank) row[blank] -= tb + oe[((size_t)b * T + (Tb - 1)) * U1 + u];
    else {
        row[blank] -= tb;
        if (lab >= 0) row[lab] -= te;
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

}  // namespace
}  // namespace wr

using namespace wr;

extern "C" size_t wr_rnnt_simple_workspace_bytes(int B, int T, int U1, int V)
{
    if (B <= 0 || T <= 0 || U1 <= 0 || V <= 0) return 0;
    return simple_ws_layout(B, T, U1).total;
}

extern "C" int wr_rnnt_simple_stats(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                                    const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1,
                                    int V, int blank, void *simple_workspace_d, size_t simple_workspace_bytes,
                                    void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream)
{
    if (int rc = simple_check("rnnt_simple_stats", B, T, U1, V, blank)) return rc;
    WR_REQUIRE(am_d && lm_d && logit_lengths_d && target_lengths_d && simple_workspace_d && rnnt_workspace_d, WR_EINVAL,
               "rnnt_simple_stats: null pointer argument");
    WR_REQUIRE(symbols_d || U1 == 1, WR_EINVAL, "rnnt_simple_stats: symbols is null");
    const SimpleWs sw = simple_ws_layout(B, T, U1);
    const RnntWs w = rnnt_ws_layout(B, T, U1);
    WR_REQUIRE(simple_workspace_bytes >= sw.total, WR_EWORKSPACE, "rnnt_simple_stats: workspace %zu < required %zu",
               simple_workspace_bytes, sw.total);
    WR_REQUIRE(rnnt_workspace_bytes >= w.total, WR_EWORKSPACE, "rnnt_simple_stats: rnnt workspace %zu < required %zu",
               rnnt_workspace_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *sws = static_cast<char *>(simple_workspace_d), *ws = static_cast<char *>(rnnt_workspace_d);
    float *ma = reinterpret_cast<float *>(sws + sw.ma_off), *ml = reinterpret_cast<float *>(sws + sw.ml_off);
    float2 *lp = reinterpret_cast<float2 *>(ws + w.lp_off);
    float *denom = reinterpret_cast<float *>(ws + w.denom_off);
    int32_t *flag = reinterpret_cast<int32_t *>(ws + w.flag_off);

    const long rows_am = (long)B * T, rows_lm = (long)B * U1;
    hipLaunchKernelGGL(simple_rowmax_kernel, dim3((unsigned)((rows_am + rows_lm + 3) / 4)), dim3(256), 0, st, am_d, lm_d,
                       rows_am, rows_lm, V, ma, ml, flag);
    WR_CHECK_LAUNCH("simple_rowmax_kernel");
    hipLaunchKernelGGL(simple_stats_kernel, dim3((U1 + kTile - 1) / kTile, (T + kTile - 1) / kTile, B), dim3(256), 0, st,
                       am_d, lm_d, symbols_d, logit_lengths_d, target_lengths_d, T, U1, V, blank, w.S, ma, ml, lp, denom,
                       flag);
    WR_CHECK_LAUNCH("simple_stats_kernel");
    long blocks = ((long)B * T * U1 + 3) / 4;
    if (blocks > 256L * 16) blocks = 256L * 16;
    hipLaunchKernelGGL(simple_stats_direct_kernel, dim3((unsigned)blocks), dim3(256), 0, st, am_d, lm_d, symbols_d,
                       logit_lengths_d, target_lengths_d, B, T, U1, V, blank, w.S, lp, denom, flag);
    WR_CHECK_LAUNCH("simple_stats_direct_kernel");
    return WR_OK;
}

extern "C" int wr_rnnt_simple_grad(const float *am_d, const float *lm_d, const int32_t *symbols_d,
                                   const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1,
                                   int V, int blank, const float *grad_costs_d, float *d_am_d, float *d_lm_d,
                                   float *occ_emit_d, float *occ_blank_d, void *simple_workspace_d,
                                   size_t simple_workspace_bytes, const void *rnnt_workspace_d,
                                   size_t rnnt_workspace_bytes, void *stream)
{
    if (int rc = simple_check("rnnt_simple_grad", B, T, U1, V, blank)) return rc;
    WR_REQUIRE(am_d && lm_d && logit_lengths_d && target_lengths_d && d_am_d && d_lm_d && simple_workspace_d &&
                   rnnt_workspace_d, WR_EINVAL, "rnnt_simple_grad: null pointer argument");
    WR_REQUIRE(symbols_d || U1 == 1, WR_EINVAL, "rnnt_simple_grad: symbols is null");
    const SimpleWs sw = simple_ws_layout(B, T, U1);
    const RnntWs w = rnnt_ws_layout(B, T, U1);
    WR_REQUIRE(simple_workspace_bytes >= sw.total, WR_EWORKSPACE, "rnnt_simple_grad: workspace %zu < required %zu",
               simple_workspace_bytes, sw.total);
    WR_REQUIRE(rnnt_workspace_bytes >= w.total, WR_EWORKSPACE, "rnnt_simple_grad: rnnt workspace %zu < required %zu",
               rnnt_workspace_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *sws = static_cast<char *>(simple_workspace_d);
    const char *ws = static_cast<const char *>(rnnt_workspace_d);
    const float *ma = reinterpret_cast<const float *>(sws + sw.ma_off), *ml = reinterpret_cast<const float *>(sws + sw.ml_off);
    float *g = reinterpret_cast<float *>(sws + sw.g_off), *gt = reinterpret_cast<float *>(sws + sw.gt_off);
    float *ob = reinterpret_cast<float *>(sws + sw.ob_off), *oe = reinterpret_cast<float *>(sws + sw.oe_off);
    int32_t *nxt = reinterpret_cast<int32_t *>(sws + sw.nxt_off), *head = reinterpret_cast<int32_t *>(sws + sw.head_off);
    const float *denom = reinterpret_cast<const float *>(ws + w.denom_off);
    const int32_t *flag = reinterpret_cast<const int32_t *>(ws + w.flag_off);
    const long cells = (long)B * T * U1;

    hipLaunchKernelGGL(simple_occ_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, logit_lengths_d,
                       target_lengths_d, B, T, U1, w.S, reinterpret_cast<const double *>(ws + w.alpha_off),
                       reinterpret_cast<const double *>(ws + w.beta_off), reinterpret_cast<const float2 *>(ws + w.lp_off),
                       denom, reinterpret_cast<const double *>(ws + w.cost_off), ma, ml, grad_costs_d, flag, g, gt, ob, oe,
                       occ_emit_d, occ_blank_d);
    WR_CHECK_LAUNCH("simple_occ_kernel");
    hipLaunchKernelGGL(simple_chain_kernel, dim3(B), dim3(256), 0, st, symbols_d, target_lengths_d, U1, nxt, head);
    WR_CHECK_LAUNCH("simple_chain_kernel");

    const unsigned vg = (unsigned)((V + kGemmCols - 1) / kGemmCols), vd = (unsigned)((V + 255) / 256);
    hipLaunchKernelGGL((simple_grad_gemm_kernel<true>), dim3(vg, (T + kTile - 1) / kTile, B), dim3(256), 0, st, gt, am_d, ma,
                       lm_d, ml, logit_lengths_d, target_lengths_d, T, U1, V, flag, d_am_d);
    WR_CHECK_LAUNCH("simple_grad_gemm_kernel<am>");
    hipLaunchKernelGGL((simple_grad_gemm_kernel<false>), dim3(vg, (U1 + kTile - 1) / kTile, B), dim3(256), 0, st, g, lm_d, ml,
                       am_d, ma, logit_lengths_d, target_lengths_d, T, U1, V, flag, d_lm_d);
    WR_CHECK_LAUNCH("simple_grad_gemm_kernel<lm>");
    hipLaunchKernelGGL((simple_grad_direct_kernel<true>), dim3(vd, T < 64 ? T : 64, B), dim3(256), 0, st, g, denom, am_d, lm_d,
                       logit_lengths_d, target_lengths_d, T, U1, V, flag, d_am_d);
    WR_CHECK_LAUNCH("simple_grad_direct_kernel<am>");
    hipLaunchKernelGGL((simple_grad_direct_kernel<false>), dim3(vd, U1 < 64 ? U1 : 64, B), dim3(256), 0, st, g, denom, lm_d, am_d,
                       logit_lengths_d, target_lengths_d, T, U1, V, flag, d_lm_d);
    WR_CHECK_LAUNCH("simple_grad_direct_kernel<lm>");

    hipLaunchKernelGGL(simple_fix_am_kernel, dim3((unsigned)(((long)B * T + 3) / 4)), dim3(256), 0, st, ob, oe, nxt, head,
                       symbols_d, logit_lengths_d, target_lengths_d, B, T, U1, V, blank, d_am_d);
    WR_CHECK_LAUNCH("simple_fix_am_kernel");
    hipLaunchKernelGGL(simple_fix_lm_kernel, dim3((U1 + 63) / 64, B), dim3(256), 0, st, ob, oe, symbols_d, logit_lengths_d,
                       target_lengths_d, T, U1, V, blank, d_lm_d);
    WR_CHECK_LAUNCH("simple_fix_lm_kernel");
    return WR_OK;
}
