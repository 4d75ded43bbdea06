// Pruned RNN-T training for MI355X (gfx950): k2's get_rnnt_prune_ranges / do_rnnt_pruning / rnnt_loss_pruned for the
// regular lattice type.  See include/wr_api.h ("Pruned RNN-T training") for the contract.
//
//   prune_ranges_kernel   one workgroup per utterance: per frame the start s_begin of the band of R label positions
//                         with the largest occupancy score, then k2's monotonicity adjustment (two suffix minima).
//   prune_gather_kernel   am_pruned[b,t,r] = am[b,t], lm_pruned[b,t,r] = lm[b, ranges[b,t,r]] (one wave per output row).
//   prune_sum_r_kernel /  the backward of the gather: d_am = sum over r, d_lm[b,u] = sum over the (t,r) that point at u,
//   prune_scatter_kernel  one writer per output element, fixed order (ascending t; for one t at most one r matches).
//   pruned_fill_kernel    (-inf, -inf) over the skewed log-probability array of an RNN-T workspace.
//   pruned_lse_kernel     one wave per band row (b,t,r): streams the V logits once, writes denom and the blank / label
//                         log-probabilities at the cell (t, u = ranges[b,t,r]) in the conventions of rnnt_lse_kernel.
//   pruned_grad_kernel    one wave per band row again: the gradient of rnnt_grad_kernel's streamed path, lattice values
//                         read at u = ranges[b,t,r].  HBM-bound: 3 * sizeof(T) * V bytes per valid row in total.
// Between the two loss kernels the lattice sweeps of rnnt_loss.hip run unchanged: a cell outside the band carries -inf
// on both arcs, so no path crosses it.
#include "rnnt_lattice.hpp"
#include "row_stream.hpp"
#include "wr_common.hpp"
#include "wr_launch.hpp"

namespace wr {
namespace {

typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------- prune ranges --
constexpr int kRangeThreads = 1024;      // frames per chunk: one lane per frame

// Suffix minimum over the block's `n` leading threads (thread i receives min over j >= i, j < n, and `carry`, the
// minimum over everything behind the chunk); threads >= n pass INT_MAX in and get garbage out.  Wave suffix scan by
// shuffles, then the wave minima through LDS.
__device__ __forceinline__ int block_suffix_min(int v, int carry, int *sw)
{
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
        const int other = __shfl_down(v, o, kWave);
        if (lane + o < kWave) v = min(v, other);
    }
    if (lane == 0) sw[wave] = v;                 // lane 0 holds the minimum of the whole wave
    __syncthreads();
    int r = min(v, carry);
    for (int w = wave + 1; w < kRangeThreads / kWave; ++w) r = min(r, sw[w]);
    __syncthreads();
    return r;
}

// px [B, U1-1, T+1] (emit occupancies), py [B, U1, T] (blank occupancies), both t-minor: a wave reads 64 consecutive
// frames of one label row.  Frames are visited in chunks of kRangeThreads from the last chunk to the first, so both
// suffix minima carry one running value from chunk to chunk.  `px_cols` is px's row length: T + 1 (the regular lattice's
// layout) or T (the modified lattice's); only columns t < T are read either way.
__global__ __launch_bounds__(kRangeThreads) void prune_ranges_kernel(
    const float *__restrict__ px, const float *__restrict__ py, const int32_t *__restrict__ tlens_frames,
    const int32_t *__restrict__ ulens, int T, int U1, int R, int px_cols, long long *__restrict__ ranges)
{
    __shared__ int sw[kRangeThreads / kWave];
    __shared__ int s_sh[kRangeThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    int Tb = tlens_frames[b], Ub = ulens[b];
    Tb = Tb < 0 ? 0 : (Tb > T ? T : Tb);
    Ub = Ub < 0 ? 0 : (Ub > U1 - 1 ? U1 - 1 : Ub);
    const int pad = max(Ub - R + 1, 0);
    const int n0 = U1 - R;                        // window starts u0 = 0 .. n0
    const float *pyb = py + (size_t)b * U1 * T;
    const float *pxb = px + (size_t)b * (U1 - 1) * px_cols;     // never dereferenced when U1 == 1 (n0 == 0)
    int carry_s = 0x7fffffff, carry_x = 0x7fffffff;
    const int nchunks = (T + kRangeThreads - 1) / kRangeThreads;
    for (int c = nchunks - 1; c >= 0; --c) {
        const int base = c * kRangeThreads;
        const int n = min(kRangeThreads, T - base);
        const int t = base + tid;
        int s = 0x7fffffff;
        if (tid < n) {
            if (t >= Tb - 1) {
                s = pad;
            } else {
                double best = 0.0;
                s = 0;
                for (int u0 = 0; u0 <= n0; ++u0) {
                    double sc = (double)pyb[(size_t)u0 * T + t];
                    for (int r = 1; r < R; ++r) sc = sc + (double)pyb[(size_t)(u0 + r) * T + t];
                    if (u0 > 0) sc = sc - (double)pxb[(size_t)(u0 - 1) * px_cols + t];
                    if (u0 == 0 || sc > best) { best = sc; s = u0; }      // the lowest u0 wins ties
                }
            }
        }
        s = block_suffix_min(s, carry_s, sw);
        int x = tid < n ? t - s : 0x7fffffff;
        x = block_suffix_min(x, carry_x, sw);
        if (tid == 0) { sw[0] = s; sw[1] = x; }   // the chunk's first frame holds the minima over everything from it on
        x = max(x, 0);
        s_sh[tid] = t - x;
        __syncthreads();
        carry_s = sw[0];
        carry_x = sw[1];
        // ranges[b, base .. base+n, 0..R) = s_begin + r, stored as 16-byte pairs of int64 wherever a pair is whole
        const long long g0 = ((long long)b * T + base) * R, g1 = g0 + (long long)n * R;
        for (long long p = (g0 >> 1) + tid; 2 * p < g1; p += kRangeThreads) {
            const long long e0 = 2 * p, e1 = e0 + 1;
            const bool in0 = e0 >= g0, in1 = e1 < g1;
            const int i0 = in0 ? (int)((e0 - g0) / R) : 0, i1 = in1 ? (int)((e1 - g0) / R) : 0;
            const long long v0 = in0 ? s_sh[i0] + (e0 - g0 - (long long)i0 * R) : 0;
            const long long v1 = in1 ? s_sh[i1] + (e1 - g0 - (long long)i1 * R) : 0;
            if (in0 && in1) {
                i64x2 o;
                o[0] = v0; o[1] = v1;
                *reinterpret_cast<i64x2 *>(ranges + e0) = o;
            } else if (in0) {
                ranges[e0] = v0;
            } else if (in1) {
                ranges[e1] = v1;
            }
        }
        __syncthreads();
    }
}

// ----------------------------------------------------------- gather / scatter --
// Rows of C elements of E bytes are copied as 16-byte vectors when the row size and both bases allow it (vec != 0),
// element by element otherwise.
template <typename E>
__device__ __forceinline__ void copy_row(const E *__restrict__ src, E *__restrict__ dst, int C, int vec, int lane)
{
    if (vec) {
        const int nv = C / (16 / (int)sizeof(E));
        const u32x4 *s = reinterpret_cast<const u32x4 *>(src);
        u32x4 *d = reinterpret_cast<u32x4 *>(dst);
        for (int i = lane; i < nv; i += kWave) d[i] = s[i];
    } else {
        for (int i = lane; i < C; i += kWave) dst[i] = src[i];
    }
}

template <typename E>
__global__ __launch_bounds__(256) void prune_gather_kernel(
    const E *__restrict__ am, const E *__restrict__ lm, const long long *__restrict__ ranges, long nrows, int T, int U1,
    int R, int C, int vec, E *__restrict__ am_out, E *__restrict__ lm_out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long stride = (long)gridDim.x * (blockDim.x >> 6);
    for (long row = (long)blockIdx.x * (blockDim.x >> 6) + wid; row < nrows; row += stride) {
        const long bt = row / R;
        const int b = (int)(bt / T);
        long long u = ranges[row];
        u = u < 0 ? 0 : (u > U1 - 1 ? U1 - 1 : u);            // the caller checked the ranges; never read out of bounds
        copy_row(am + (size_t)bt * C, am_out + (size_t)row * C, C, vec, lane);
        copy_row(lm + ((size_t)b * U1 + (size_t)u) * C, lm_out + (size_t)row * C, C, vec, lane);
    }
}

// d_am[b,t,c] = (g[b,t,0,c] + g[b,t,1,c]) + ... in fp32, one thread per element
template <typename T>
__global__ __launch_bounds__(256) void prune_sum_r_kernel(const T *__restrict__ g, long n, int R, int C, T *__restrict__ out)
{
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long bt = i / C;
        const int c = (int)(i - bt * C);
        const T *p = g + (size_t)bt * R * C + c;
        float acc = (float)p[0];
        for (int r = 1; r < R; ++r) acc += (float)p[(size_t)r * C];
        out[i] = (T)acc;
    }
}

// d_lm[b,u,c] = sum over the frames t with ranges[b,t,0] <= u < ranges[b,t,0] + R of g[b,t,u - ranges[b,t,0],c], in
// ascending t.  One wave per (b, u, 64 columns): the lanes test 64 frames at a time, the matches are then taken in
// order from the ballot.
template <typename T>
__global__ __launch_bounds__(256) void prune_scatter_kernel(
    const T *__restrict__ g, const long long *__restrict__ ranges, long nwork, int Tn, int U1, int R, int C, int cchunks,
    T *__restrict__ out)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long stride = (long)gridDim.x * (blockDim.x >> 6);
    for (long wk = (long)blockIdx.x * (blockDim.x >> 6) + wid; wk < nwork; wk += stride) {
        const long bu = wk / cchunks;
        const int c = (int)(wk - bu * cchunks) * kWave + lane;
        const int b = (int)(bu / U1);
        const int u = (int)(bu - (long)b * U1);
        const long long *rb = ranges + (size_t)b * Tn * R;
        const T *gb = g + (size_t)b * Tn * R * C;
        float acc = 0.f;
        for (int t0 = 0; t0 < Tn; t0 += kWave) {
            const int t = t0 + lane;
            long long s = t < Tn ? rb[(size_t)t * R] : (long long)U1;        // U1 never matches
            const bool hit = s <= u && u < s + R;
            unsigned long long m = __ballot(hit);
            while (m) {
                const int k = __builtin_ctzll(m);
                m &= m - 1;
                const int r = u - (int)__shfl(s, k, kWave);
                if (c < C) acc += (float)gb[((size_t)(t0 + k) * R + r) * C + c];
            }
        }
        if (c < C) out[(size_t)bu * C + c] = (T)acc;
    }
}

// ------------------------------------------------------------------ the loss --
__global__ __launch_bounds__(256) void pruned_fill_kernel(float2 *__restrict__ lp, size_t n)
{
    // n float2 cells, the base 256-byte aligned: pairs of cells as one 16-byte store
    const size_t nv = n / 2;
    f32x4 v;
    v[0] = v[1] = v[2] = v[3] = kNegInf;
    f32x4 *p = reinterpret_cast<f32x4 *>(lp);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) lp[n - 1] = make_float2(kNegInf, kNegInf);
}

template <typename T, bool NT, int UN>
__global__ __launch_bounds__(256) void pruned_lse_kernel(
    const T *__restrict__ logits, const int32_t *__restrict__ symbols, const long long *__restrict__ ranges,
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, long nrows, int Tmax, int U1max, int R, int V,
    int blank, int S, float2 *__restrict__ lp_skew, float *__restrict__ denom)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long stride = (long)gridDim.x * (blockDim.x >> 6);
    for (long r = (long)blockIdx.x * (blockDim.x >> 6) + wid; r < nrows; r += stride) {
        const long bt = r / R;
        const int b = (int)(bt / Tmax);
        const int t = (int)(bt - (long)b * Tmax);
        const long long ul = ranges[r];
        const int T_ = llens[b], U = tlens[b];
        if (t >= T_ || ul < 0 || ul > U || ul >= U1max) continue;
        const int u = (int)ul;
        const T *row = logits + (size_t)r * V;
        const float d = wave_row_lse<T, NT, UN>(row, V, lane);
        if (lane == 0) {
            const float xb = (float)row[blank];
            float em = 0.f;
            if (u < U) {
                const int lab = symbols[(size_t)b * (U1max - 1) + u];
                em = (lab >= 0 && lab < V) ? (float)row[lab] - d : kNegInf;
            }
            denom[(size_t)bt * U1max + u] = d;
            lp_skew[((size_t)b * S + t + u) * U1max + u] = make_float2(xb - d, em);
        }
    }
}

// The streamed path of rnnt_grad_kernel (rnnt_loss.hip) on band rows.  One difference: a label equal to the blank has
// both its terms subtracted (the derivative of the loss as written, which is what k2's autograd gives) instead of the
// first match of torchaudio's case chain.
// LAT (rnnt_lattice.hpp) changes the per-row preamble only, and it is wave-uniform: where the lattice values of the cell
// and of its two successors are read, and the delay penalty `dp` inside the label term (the stored label arc has it).
template <typename T, bool NT, bool NTS, int UN, int LAT>
__global__ __launch_bounds__(256) void pruned_grad_kernel(
    const T *logits, const int32_t *__restrict__ symbols, const long long *__restrict__ ranges,
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, long nrows, int Tmax, int U1max, int R, int V,
    int blank, int S, const double *__restrict__ alpha_skew, const double *__restrict__ beta_skew,
    const float *__restrict__ denom, const double *__restrict__ cost_ws, const float *__restrict__ grad_costs, T *grads,
    double dp)
{
    typedef typename VecOf<T>::type vec_t;
    constexpr int N = VecOf<T>::N;
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long stride = (long)gridDim.x * (blockDim.x >> 6);
    for (long r = (long)blockIdx.x * (blockDim.x >> 6) + wid; r < nrows; r += stride) {
        const long bt = r / R;
        const int b = (int)(bt / Tmax);
        const int t = (int)(bt - (long)b * Tmax);
        const long long ul = ranges[r];
        const int T_ = llens[b], U = tlens[b];
        const T *row = logits + (size_t)r * V;
        T *grow = grads + (size_t)r * V;
        const RowSplit<T> sp(row, V);
        const int h = sp.h, nv = sp.nv, tail = sp.tail;
        const vec_t *body = reinterpret_cast<const vec_t *>(row + h);
        vec_t *gbody = reinterpret_cast<vec_t *>(grow + h);
        const float go = grad_costs ? grad_costs[b] : 1.f;

        const bool valid = t < T_ && ul >= 0 && ul <= U && ul < U1max;
        if (__builtin_amdgcn_readfirstlane(valid ? 0 : 1)) {          // outside the lattice: grad_costs[b] * 0, logits unread
            const T val = (T)(go * 0.f);
            vec_t z;
#pragma unroll
            for (int q = 0; q < N; ++q) z[q] = val;
            if (lane < h) grow[lane] = val;
            if (lane < tail) grow[h + N * nv + lane] = val;
            for (int i = lane; i < nv; i += kWave) stv<NTS>(z, gbody + i);
            continue;
        }
        const int u = (int)ul;
        const size_t dbase = (size_t)b * S * U1max;
        const int s = t + u;
        const bool final_cell = t == T_ - 1 && u == U;
        const bool has_b1 = t < T_ - 1;
        const bool blank_special = final_cell || has_b1;
        const size_t k = dbase + lat_idx<LAT>(t, u, U1max);
        const double al = alpha_skew[k];
        const double be = beta_skew[k];
        const double cost = cost_ws[b];
        const float d = denom[(size_t)bt * U1max + u];
        double b1;
        if (LAT == kLatModified) b1 = has_b1 ? beta_skew[k + U1max] : 0.0;
        else b1 = has_b1 ? beta_skew[dbase + (size_t)(s + 1) * U1max + u] : 0.0;
        int lab = -1;
        double b2 = 0.0;
        if (u < U) {
            lab = symbols[(size_t)b * (U1max - 1) + u];
            if (LAT == kLatModified)     // the label arc leads to (t+1, u+1); beta(T_b, .) is 0 at U_b, -inf elsewhere
                b2 = has_b1 ? beta_skew[k + U1max + 1] : (u == U - 1 ? 0.0 : (double)kNegInf);
            else
                b2 = beta_skew[dbase + (size_t)(s + 1) * U1max + (u + 1)];
        }
        const double cmd = al + cost - (double)d;      // g = logit + cm
        const float c2 = (float)(cmd + be) * kLog2e;
        const float blank_sub = final_cell ? (float)cmd : (has_b1 ? (float)(cmd + b1) : 0.f);
        const float lab_sub = LAT == kLatRegular ? (float)(cmd + b2) : (float)((cmd + b2) + delay_pen(dp, T_, t));
        const int blk = blank_special ? blank : -1;

        auto fix = [&](float val, float x, int v) -> float {
            if (v == blk) val -= fast_exp2((x + blank_sub) * kLog2e);
            if (v == lab) val -= fast_exp2((x + lab_sub) * kLog2e);
            return val;
        };
        if (lane < h) {
            const float x = (float)row[lane];
            grow[lane] = (T)(fix(fast_exp2(fmaf(x, kLog2e, c2)), x, lane) * go);
        }
        if (lane < tail) {
            const int v = h + N * nv + lane;
            const float x = (float)row[v];
            grow[v] = (T)(fix(fast_exp2(fmaf(x, kLog2e, c2)), x, v) * go);
        }
        const int iblk = (blk >= h) ? ((blk - h) / N) : -1;
        const int ilab = (lab >= h) ? ((lab - h) / N) : -1;
        auto dov = [&](int i, const vec_t x) {
            float g[N];
#pragma unroll
            for (int q = 0; q < N; ++q) g[q] = fast_exp2(fmaf((float)x[q], kLog2e, c2));
            if (i == iblk || i == ilab) {
                const int v0 = h + N * i;
#pragma unroll
                for (int q = 0; q < N; ++q) g[q] = fix(g[q], (float)x[q], v0 + q);
            }
            vec_t o;
#pragma unroll
            for (int q = 0; q < N; ++q) o[q] = (T)(g[q] * go);
            stv<NTS>(o, gbody + i);
        };
        int i = lane;
        for (; i + (UN - 1) * kWave < nv; i += UN * kWave) {
            vec_t x[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) x[q] = ldv<NT>(body + i + q * kWave);
#pragma unroll
            for (int q = 0; q < UN; ++q) dov(i + q * kWave, x[q]);
        }
        if (i < nv) {                                    // remainder (fewer than UN vectors per lane): one guarded batch
            vec_t x[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q)
                if (i + q * kWave < nv) x[q] = ldv<NT>(body + i + q * kWave);
#pragma unroll
            for (int q = 0; q < UN; ++q)
                if (i + q * kWave < nv) dov(i + q * kWave, x[q]);
        }
    }
}

// ------------------------------------------------------------------- host side --
int check_band(const char *what, int B, int T, int U1, int R)
{
    WR_REQUIRE(B > 0 && T > 0 && U1 > 0 && R > 0, WR_EINVAL, "%s: B, T, U1, R must be positive (got %d,%d,%d,%d)", what, B, T,
               U1, R);
    WR_REQUIRE(R <= U1, WR_EINVAL, "%s: R=%d exceeds the U1=%d label positions", what, R, U1);
    WR_REQUIRE((long)B * T * R < (1L << 31) && (long)B * T * U1 < (1L << 31), WR_EUNSUPPORTED, "%s: more than 2^31 rows", what);
    return WR_OK;
}

int check_loss(const char *what, int B, int T, int U1, int R, int V, int blank, int dtype)
{
    if (int rc = check_band(what, B, T, U1, R)) return rc;
    WR_REQUIRE(V > 0, WR_EINVAL, "%s: V must be positive (got %d)", what, V);
    WR_REQUIRE(blank >= 0 && blank < V, WR_EINVAL, "%s: blank %d out of range [0,%d)", what, blank, V);
    WR_REQUIRE(dtype == WR_F32 || dtype == WR_F16 || dtype == WR_BF16, WR_EINVAL, "%s: unknown dtype %d", what, dtype);
    WR_REQUIRE(U1 <= kRnntMaxCols, WR_EUNSUPPORTED, "%s: U1=%d exceeds the sweep kernel's limit of %d label columns", what,
               U1, kRnntMaxCols);
    return WR_OK;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace
}  // namespace wr

using namespace wr;

static int prune_ranges_impl(const char *what, const float *px_grad_d, int px_cols, const float *py_grad_d,
                             const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1, int R,
                             int64_t *ranges_d, void *stream)
{
    if (int rc = check_band(what, B, T, U1, R)) return rc;
    WR_REQUIRE(px_cols == T || px_cols == T + 1, WR_EINVAL, "%s: px_grad rows hold T = %d or T + 1 frames (got %d)", what, T,
               px_cols);
    WR_REQUIRE(py_grad_d && logit_lengths_d && target_lengths_d && ranges_d, WR_EINVAL, "%s: null pointer argument", what);
    WR_REQUIRE(px_grad_d || U1 == 1, WR_EINVAL, "%s: px_grad is null", what);
    WR_REQUIRE(aligned16(ranges_d), WR_EINVAL, "%s: ranges must be 16-byte aligned", what);
    return launch("prune_ranges_kernel", prune_ranges_kernel, dim3(B), dim3(kRangeThreads), 0,
                  static_cast<hipStream_t>(stream), px_grad_d, py_grad_d, logit_lengths_d, target_lengths_d, T, U1, R, px_cols,
                  reinterpret_cast<long long *>(ranges_d));
}

extern "C" int wr_rnnt_prune_ranges(const float *px_grad_d, const float *py_grad_d, const int32_t *logit_lengths_d,
                                    const int32_t *target_lengths_d, int B, int T, int U1, int R, int64_t *ranges_d,
                                    void *stream)
{
    return prune_ranges_impl("rnnt_prune_ranges", px_grad_d, T + 1, py_grad_d, logit_lengths_d, target_lengths_d, B, T, U1,
                             R, ranges_d, stream);
}

extern "C" int wr_rnnt_prune_ranges_cols(const float *px_grad_d, int px_cols, const float *py_grad_d,
                                         const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T,
                                         int U1, int R, int64_t *ranges_d, void *stream)
{
    return prune_ranges_impl("rnnt_prune_ranges_cols", px_grad_d, px_cols, py_grad_d, logit_lengths_d, target_lengths_d, B,
                             T, U1, R, ranges_d, stream);
}

extern "C" int wr_rnnt_prune_gather(const void *am_d, const void *lm_d, const int64_t *ranges_d, int dtype, int B, int T,
                                    int U1, int R, int C, void *am_pruned_d, void *lm_pruned_d, void *stream)
{
    if (int rc = check_band("rnnt_prune_gather", B, T, U1, R)) return rc;
    WR_REQUIRE(C > 0, WR_EINVAL, "rnnt_prune_gather: C must be positive (got %d)", C);
    WR_REQUIRE(dtype == WR_F32 || dtype == WR_F16 || dtype == WR_BF16, WR_EINVAL, "rnnt_prune_gather: unknown dtype %d", dtype);
    WR_REQUIRE(am_d && lm_d && ranges_d && am_pruned_d && lm_pruned_d, WR_EINVAL, "rnnt_prune_gather: null pointer argument");
    const long nrows = (long)B * T * R;
    const int esize = dtype == WR_F32 ? 4 : 2;
    const int vec = ((size_t)C * esize % 16 == 0 && aligned16(am_d) && aligned16(lm_d) && aligned16(am_pruned_d) &&
                     aligned16(lm_pruned_d)) ? 1 : 0;
    long blocks = (nrows + 3) / 4;
    if (blocks > 256L * 32) blocks = 256L * 32;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long *rg = reinterpret_cast<const long long *>(ranges_d);
    const auto gather = [&](auto e) {             // the rows are copied as 4-byte or 2-byte words, whatever they hold
        using E = decltype(e);
        return launch("prune_gather_kernel", prune_gather_kernel<E>, dim3((unsigned)blocks), dim3(256), 0, st,
                      static_cast<const E *>(am_d), static_cast<const E *>(lm_d), rg, nrows, T, U1, R, C, vec,
                      static_cast<E *>(am_pruned_d), static_cast<E *>(lm_pruned_d));
    };
    if (esize == 4) return gather(uint32_t{});
    return gather(uint16_t{});
}

extern "C" int wr_rnnt_prune_scatter(const void *g_am_pruned_d, const void *g_lm_pruned_d, const int64_t *ranges_d, int dtype,
                                     int B, int T, int U1, int R, int C, void *d_am_d, void *d_lm_d, void *stream)
{
    if (int rc = check_band("rnnt_prune_scatter", B, T, U1, R)) return rc;
    WR_REQUIRE(C > 0, WR_EINVAL, "rnnt_prune_scatter: C must be positive (got %d)", C);
    WR_REQUIRE(dtype == WR_F32 || dtype == WR_F16 || dtype == WR_BF16, WR_EINVAL, "rnnt_prune_scatter: unknown dtype %d", dtype);
    WR_REQUIRE(ranges_d && (d_am_d || d_lm_d), WR_EINVAL, "rnnt_prune_scatter: null pointer argument");
    WR_REQUIRE((!d_am_d || g_am_pruned_d) && (!d_lm_d || g_lm_pruned_d), WR_EINVAL,
               "rnnt_prune_scatter: an output without its incoming gradient");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long long *rg = reinterpret_cast<const long long *>(ranges_d);
    const long n_am = (long)B * T * C;
    long blocks_am = (n_am + 255) / 256;
    if (blocks_am > 256L * 32) blocks_am = 256L * 32;
    const int cchunks = (C + kWave - 1) / kWave;
    const long nwork = (long)B * U1 * cchunks;
    long blocks_lm = (nwork + 3) / 4;
    if (blocks_lm > 256L * 32) blocks_lm = 256L * 32;
    return with_dtype(dtype, [&](auto t) {
        using E = decltype(t);
        if (d_am_d)
            WR_TRY(launch("prune_sum_r_kernel", prune_sum_r_kernel<E>, dim3((unsigned)blocks_am), dim3(256), 0, st,
                          static_cast<const E *>(g_am_pruned_d), n_am, R, C, static_cast<E *>(d_am_d)));
        if (d_lm_d)
            WR_TRY(launch("prune_scatter_kernel", prune_scatter_kernel<E>, dim3((unsigned)blocks_lm), dim3(256), 0, st,
                          static_cast<const E *>(g_lm_pruned_d), rg, nwork, T, U1, R, C, cchunks, static_cast<E *>(d_lm_d)));
        return (int)WR_OK;
    });
}

extern "C" int wr_rnnt_pruned_stats(const void *logits_d, int dtype, const int32_t *symbols_d, const int64_t *ranges_d,
                                    const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1,
                                    int R, int V, int blank, void *rnnt_workspace_d, size_t rnnt_workspace_bytes,
                                    void *stream)
{
    if (int rc = check_loss("rnnt_pruned_stats", B, T, U1, R, V, blank, dtype)) return rc;
    WR_REQUIRE(logits_d && ranges_d && logit_lengths_d && target_lengths_d && rnnt_workspace_d, WR_EINVAL,
               "rnnt_pruned_stats: null pointer argument");
    WR_REQUIRE(symbols_d || U1 == 1, WR_EINVAL, "rnnt_pruned_stats: symbols is null");
    const RnntWs w = rnnt_ws_layout(B, T, U1);
    WR_REQUIRE(rnnt_workspace_bytes >= w.total, WR_EWORKSPACE, "rnnt_pruned_stats: workspace %zu < required %zu",
               rnnt_workspace_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(rnnt_workspace_d);
    float2 *lp = reinterpret_cast<float2 *>(ws + w.lp_off);
    const size_t ncell = (size_t)B * w.S * U1;
    size_t fill_blocks = (ncell / 2 + 255) / 256;
    if (fill_blocks > 256 * 8) fill_blocks = 256 * 8;
    if (fill_blocks < 1) fill_blocks = 1;
    WR_TRY(launch("pruned_fill_kernel", pruned_fill_kernel, dim3((unsigned)fill_blocks), dim3(256), 0, st, lp, ncell));
    const long nrows = (long)B * T * R;
    const size_t row_bytes = (size_t)V * (dtype == WR_F32 ? 4 : 2);
    // the automatic sizing of the full-lattice passes (no tuning key): about 16 KB of band logits per wave here, 68 KB in
    // the gradient pass
    const dim3 grid(stream_grid(nrows, 0, row_bytes, 16 * 1024));
    return with_dtype(dtype, [&](auto t) {
        using E = decltype(t);
        return launch("pruned_lse_kernel", pruned_lse_kernel<E, true, 16>, grid, dim3(256), 0, st,
                      static_cast<const E *>(logits_d), symbols_d, reinterpret_cast<const long long *>(ranges_d),
                      logit_lengths_d, target_lengths_d, nrows, T, U1, R, V, blank, w.S, lp,
                      reinterpret_cast<float *>(ws + w.denom_off));
    });
}

// wr_rnnt_pruned_grad (lat = kLatRegular) and wr_rnnt_pruned_grad_lattice
static int pruned_grad_impl(const char *what, const void *logits_d, int dtype, const int32_t *symbols_d,
                            const int64_t *ranges_d, const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B,
                            int T, int U1, int R, int V, int blank, int lat, double delay_penalty,
                            const float *grad_costs_d, void *grads_d, const void *rnnt_workspace_d,
                            size_t rnnt_workspace_bytes, void *stream)
{
    if (int rc = check_loss(what, B, T, U1, R, V, blank, dtype)) return rc;
    WR_REQUIRE(logits_d && ranges_d && logit_lengths_d && target_lengths_d && grads_d && rnnt_workspace_d, WR_EINVAL,
               "%s: null pointer argument", what);
    WR_REQUIRE(symbols_d || U1 == 1, WR_EINVAL, "%s: symbols is null", what);
    WR_REQUIRE(((reinterpret_cast<uintptr_t>(logits_d) ^ reinterpret_cast<uintptr_t>(grads_d)) & 15) == 0, WR_EINVAL,
               "%s: logits and grads must sit at the same offset within a 16-byte line", what);
    const RnntWs w = rnnt_ws_layout(B, T, U1);
    WR_REQUIRE(rnnt_workspace_bytes >= w.total, WR_EWORKSPACE, "%s: workspace %zu < required %zu", what,
               rnnt_workspace_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const char *ws = static_cast<const char *>(rnnt_workspace_d);
    const long nrows = (long)B * T * R;
    const size_t row_bytes = (size_t)V * (dtype == WR_F32 ? 4 : 2);
    const dim3 grid(stream_grid(nrows, 0, row_bytes, 68 * 1024));
    const LatView lv = lattice_view(w, ws, lat == kLatModified);
    return with_dtype(dtype, [&](auto t) {
        using E = decltype(t);
        return with_int<kLatModified, kLatRegularPen, kLatRegular>(lat, [&](auto lat_c) {
            return launch("pruned_grad_kernel", pruned_grad_kernel<E, true, true, 16, lat_c.value>, grid, dim3(256), 0, st,
                          static_cast<const E *>(logits_d), symbols_d, reinterpret_cast<const long long *>(ranges_d),
                          logit_lengths_d, target_lengths_d, nrows, T, U1, R, V, blank, w.S, lv.alpha, lv.beta,
                          reinterpret_cast<const float *>(ws + w.denom_off),
                          reinterpret_cast<const double *>(ws + w.cost_off), grad_costs_d, static_cast<E *>(grads_d),
                          delay_penalty);
        });
    });
}

extern "C" int wr_rnnt_pruned_grad(const void *logits_d, int dtype, const int32_t *symbols_d, const int64_t *ranges_d,
                                   const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T, int U1,
                                   int R, int V, int blank, const float *grad_costs_d, void *grads_d,
                                   const void *rnnt_workspace_d, size_t rnnt_workspace_bytes, void *stream)
{
    return pruned_grad_impl("rnnt_pruned_grad", logits_d, dtype, symbols_d, ranges_d, logit_lengths_d, target_lengths_d, B,
                            T, U1, R, V, blank, kLatRegular, 0.0, grad_costs_d, grads_d, rnnt_workspace_d,
                            rnnt_workspace_bytes, stream);
}

extern "C" int wr_rnnt_pruned_grad_lattice(const void *logits_d, int dtype, const int32_t *symbols_d,
                                           const int64_t *ranges_d, const int32_t *logit_lengths_d,
                                           const int32_t *target_lengths_d, int B, int T, int U1, int R, int V, int blank,
                                           int lattice_type, double delay_penalty, const float *grad_costs_d,
                                           void *grads_d, const void *rnnt_workspace_d, size_t rnnt_workspace_bytes,
                                           void *stream)
{
    if (int rc = lattice_check("rnnt_pruned_grad_lattice", lattice_type, delay_penalty)) return rc;
    const int lat = lattice_type == WR_LATTICE_MODIFIED ? kLatModified : (delay_penalty > 0.0 ? kLatRegularPen : kLatRegular);
    return pruned_grad_impl("rnnt_pruned_grad_lattice", logits_d, dtype, symbols_d, ranges_d, logit_lengths_d,
                            target_lengths_d, B, T, U1, R, V, blank, lat, delay_penalty, grad_costs_d, grads_d,
                            rnnt_workspace_d, rnnt_workspace_bytes, stream);
}
