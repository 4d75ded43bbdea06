// Lattice types of the k2 RNN-T losses for MI355X (gfx950): the modified lattice (k2's rnnt_type = "modified": a label
// consumes a frame) and the delay penalty, for the simple, smoothed and pruned losses alike.  See include/wr_api.h
// ("Lattice types and the delay penalty") for the contract and rnnt_lattice.hpp for where the arrays live.
//
// The statistics pass of any of the three losses leaves (blank, emit) log-probabilities in the anti-diagonal array of an
// RNN-T workspace.  wr_rnnt_lattice_sweeps then runs
//   lattice_prepare_kernel    one thread per stored position of that array: adds pen(b,t) to the label log-probability
//                             (float64, rounded once) and, for the modified lattice, lays the pairs out as plain
//                             [b][t][u] rows.  Regular lattice + penalty: in place, and rnnt_loss.hip's sweeps follow.
//   lattice_mod_sweep_kernel  one workgroup per (utterance, direction), one lane per label column, T_b dependent steps
//                             (+ 1 forward, for the terminal node).  Every lane is on the same frame, so a step reads and
//                             writes one contiguous row.  The exchange is rnnt_sweep_kernel's: the lane's own previous
//                             value and its neighbour's previous value (+ arc), by DPP rotate inside a wave and a
//                             double-buffered LDS slot plus one barrier across waves.  fp64 state, PF rows in flight.
//   lattice_export_kernel     alpha / beta of either lattice as plain (B, T, U1) floats, for the tests.
#include "rnnt_lattice.hpp"
#include "wr_launch.hpp"

namespace wr {
namespace {

__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// rnnt_loss.hip's log-add: fp64 state, the bounded log1p(exp(-|a-b|)) term in fp32; -inf safe
__device__ __forceinline__ double log_add_exp_d(double a, double b)
{
    const double m = fmax(a, b);
    const float d = (float)(-fabs(a - b));          // NaN when both are -inf
    const float r = kLn2 * fast_log2(1.0f + fast_exp2(d * kLog2e));
    return (m == (double)kNegInf) ? (double)kNegInf : m + (double)r;
}

// One thread per position (b, s = t + u, u) of the anti-diagonal array: whole lines of it are read.  MOD: the pair goes
// to row t of the plain array `lp_plain` (another region of the workspace); otherwise the label term is rewritten in
// place (launched only with a penalty).
template <bool MOD>
__global__ __launch_bounds__(256) void lattice_prepare_kernel(
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int B, int T, int U1, int S, double dp,
    float2 *lp_skew, float2 *lp_plain)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)B * S * U1) return;
    const long diag = (long)S * U1;
    const int b = (int)(r / diag);
    const long cc = r - b * diag;
    const int sd = (int)(cc / U1), u = (int)(cc - (long)sd * U1), t = sd - u;
    const int Tb = clampi(llens[b], 0, T), Ub = clampi(tlens[b], 0, U1 - 1);
    if (t < 0 || t >= Tb || u > Ub) return;
    float2 lp = lp_skew[r];
    if (dp > 0.0 && u < Ub) lp.y = (float)((double)lp.y + delay_pen(dp, Tb, t));
    if (MOD) lp_plain[(size_t)b * diag + (size_t)t * U1 + u] = lp;
    else lp_skew[r] = lp;
}

// alpha(t,u) = logadd(alpha(t-1,u) + blank(t-1,u), alpha(t-1,u-1) + emit'(t-1,u-1)), alpha(0,0) = 0; ll = alpha(T,U)
// beta(t,u)  = logadd(blank(t,u) + beta(t+1,u),   emit'(t,u) + beta(t+1,u+1)),       beta(T,U) = 0, beta(T,u != U) = -inf
// Rows 0 .. T-1 are stored; row T of alpha is the terminal node alone (ll), row T of beta is the constant above.
template <int PF>
__global__ __launch_bounds__(kRnntMaxCols) void lattice_mod_sweep_kernel(
    const float2 *__restrict__ lp_plain, const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int Tmax,
    int U1max, int S, double *__restrict__ alpha_plain, double *__restrict__ beta_plain, double *__restrict__ ll_out,
    double *__restrict__ cost_ws, float *__restrict__ costs_out,
    double *__restrict__ dump /* [2*B*kRnntMaxCols] scratch that absorbs the stores of idle lanes */)
{
    constexpr double NEG = (double)kNegInf;
    __shared__ double xch[2][kRnntMaxCols / kWave];
    const int b = blockIdx.x;
    const bool backward = blockIdx.y != 0;
    const int u = threadIdx.x;
    const int lane = u & (kWave - 1), wave = u >> 6;
    const int nw = blockDim.x >> 6;
    const int T = clampi(llens[b], 0, Tmax), U = clampi(tlens[b], 0, U1max - 1);

    if (T == 0) {
        if (u == 0) {
            if (backward) { cost_ws[b] = 0.0; costs_out[b] = 0.f; } else ll_out[b] = 0.0;
        }
        return;
    }
    const bool in_row = u < U1max;
    const int col = in_row ? u : U1max - 1;
    const float2 *__restrict__ lp = lp_plain + (size_t)b * S * U1max + col;
    double *__restrict__ out = (backward ? beta_plain : alpha_plain) + (size_t)b * S * U1max + col;
    double *__restrict__ sink = dump + ((size_t)b * 2 + (backward ? 1 : 0)) * kRnntMaxCols + u;
    const bool ucol = in_row && u <= U;

    auto load_row = [&](int t) -> float2 {
        const int tc = t < 0 ? 0 : (t >= T ? T - 1 : t);
        return lp[(size_t)tc * U1max];
    };

    float2 ring[PF];
    double result = NEG;

    if (!backward) {
        double st = NEG;      // alpha(t-1, u)
        float skp = 0.f;      // blank(t-1, u)
        double send = NEG;    // alpha(t-1, u) + emit'(t-1, u): what lane u+1 needs
#pragma unroll
        for (int i = 0; i < PF; ++i) ring[i] = load_row(i);
        for (int base = 0; base <= T; base += PF) {              // frames 0 .. T-1 and the terminal row T
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int t = base + i;                          // rows t > T have no active lane
                const float2 cur = ring[i];
                ring[i] = load_row(t + PF);
                double recv = lane_rotate_up_d(send);
                if (lane == 0)       // row 0 has no left neighbour yet (the LDS slots are still unwritten)
                    recv = (t == 0) ? ((wave == 0) ? 0.0 : NEG) : ((wave == 0) ? NEG : xch[(t + 1) & 1][wave - 1]);
                const bool active = (t < T) & ucol;
                const float sk = active ? cur.x : 0.f;
                const float em = active ? cur.y : 0.f;
                const double top = (t >= 1) ? st + (double)skp : NEG;
                double v = log_add_exp_d(top, recv);             // the origin sees recv = 0, top = -inf  ->  0
                result = (t == T && u == U) ? v : result;        // the terminal node (T, U)
                v = active ? v : NEG;
                double *dst = active ? out + (size_t)t * U1max : sink;
                *dst = v;
                send = v + (double)em;
                if (lane == kWave - 1) xch[t & 1][wave] = send;
                st = v;
                skp = sk;
                if (nw > 1) __syncthreads();
            }
        }
        if (u == U) ll_out[b] = result;
    } else {
        double st = (u == U) ? 0.0 : NEG;     // beta(t+1, u); row T is the terminal condition
        double send = st;                     // what lane u-1 needs
        if (lane == 0) xch[T & 1][wave] = send;
        if (nw > 1) __syncthreads();
#pragma unroll
        for (int i = 0; i < PF; ++i) ring[i] = load_row(T - 1 - i);
        for (int base = 0; base < T; base += PF) {
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int t = T - 1 - (base + i);                // rows t < 0 have no active lane
                const float2 cur = ring[i];
                ring[i] = load_row(t - PF);
                double recv = lane_rotate_down_d(send);
                if (lane == kWave - 1) recv = (wave == nw - 1) ? NEG : xch[(t + 1) & 1][wave + 1];
                const bool active = (t >= 0) & ucol;
                const float sk = active ? cur.x : 0.f;
                const float em = active ? cur.y : 0.f;
                const double down = st + (double)sk;
                const double diag = (u < U) ? recv + (double)em : NEG;
                double v = log_add_exp_d(down, diag);
                v = active ? v : NEG;
                double *dst = active ? out + (size_t)t * U1max : sink;
                *dst = v;
                result = (t == 0 && u == 0) ? v : result;
                send = v;
                if (lane == 0) xch[t & 1][wave] = send;
                st = v;
                if (nw > 1) __syncthreads();
            }
        }
        if (u == 0) { cost_ws[b] = -result; costs_out[b] = (float)(-result); }
    }
}

template <int LAT>
__global__ __launch_bounds__(256) void lattice_export_kernel(
    const double *__restrict__ alpha_ws, const double *__restrict__ beta_ws, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, int B, int T, int U1, int S, float *__restrict__ alpha, float *__restrict__ beta)
{
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)B * T * U1) return;
    const int cells = T * U1;
    const int b = (int)(r / cells);
    const int c = (int)(r - (long)b * cells);
    const int t = c / U1, u = c - t * U1;
    float a = 0.f, be = 0.f;
    if (t < clampi(llens[b], 0, T) && u <= clampi(tlens[b], 0, U1 - 1)) {
        const size_t k = (size_t)b * S * U1 + lat_idx<LAT>(t, u, U1);
        a = (float)alpha_ws[k];
        be = (float)beta_ws[k];
    }
    alpha[r] = a;
    beta[r] = be;
}

// `rows`: a kernel of this file runs (it indexes B * (T + U1 - 1) * U1 positions); without one the limits are those of
// wr_rnnt_loss_sweeps.
int lattice_shape(const char *what, int B, int T, int U1, bool rows)
{
    WR_REQUIRE(B > 0 && T > 0 && U1 > 0, WR_EINVAL, "%s: B, T, U1 must be positive (got %d,%d,%d)", what, B, T, U1);
    WR_REQUIRE(U1 <= kRnntMaxCols, WR_EUNSUPPORTED, "%s: U1=%d exceeds the sweep kernel's limit of %d label columns", what,
               U1, kRnntMaxCols);
    WR_REQUIRE((long)B * T * U1 < (1L << 31) && (!rows || (long)B * (T + U1 - 1) * U1 < (1L << 31)), WR_EUNSUPPORTED,
               "%s: more than 2^31 lattice positions", what);
    return WR_OK;
}

}  // namespace

int lattice_check(const char *what, int lattice_type, double delay_penalty)
{
    WR_REQUIRE(lattice_type == WR_LATTICE_REGULAR || lattice_type == WR_LATTICE_MODIFIED, WR_EINVAL,
               "%s: unknown lattice type %d", what, lattice_type);
    WR_REQUIRE(delay_penalty >= 0.0 && delay_penalty < (double)__builtin_huge_valf(), WR_EINVAL,
               "%s: delay_penalty %g must be finite and not negative", what, delay_penalty);
    return WR_OK;
}

}  // namespace wr

using namespace wr;

extern "C" int wr_rnnt_lattice_sweeps(const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int T,
                                      int U1, int lattice_type, double delay_penalty, float *costs_d, void *workspace_d,
                                      size_t workspace_bytes, void *stream)
{
    if (int rc = lattice_shape("rnnt_lattice_sweeps", B, T, U1, lattice_type != WR_LATTICE_REGULAR || !(delay_penalty == 0.0)))
        return rc;
    if (int rc = lattice_check("rnnt_lattice_sweeps", lattice_type, delay_penalty)) return rc;
    WR_REQUIRE(logit_lengths_d && target_lengths_d && costs_d && workspace_d, WR_EINVAL,
               "rnnt_lattice_sweeps: null pointer argument");
    const RnntWs w = rnnt_ws_layout(B, T, U1);
    WR_REQUIRE(workspace_bytes >= w.total, WR_EWORKSPACE, "rnnt_lattice_sweeps: workspace %zu < required %zu",
               workspace_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace_d);
    const bool modified = lattice_type == WR_LATTICE_MODIFIED;
    const long cells = (long)B * w.S * U1;
    float2 *lp_skew = reinterpret_cast<float2 *>(ws + w.lp_off);
    if (modified) {
        WR_TRY(launch("lattice_prepare_kernel<modified>", lattice_prepare_kernel<true>,
                      dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, logit_lengths_d, target_lengths_d, B, T, U1,
                      w.S, delay_penalty, lp_skew, reinterpret_cast<float2 *>(ws + w.alpha_off)));
        const LatView v = lattice_view(w, ws, true);
        return launch("lattice_mod_sweep_kernel", lattice_mod_sweep_kernel<8>, dim3(B, 2), dim3(64 * w.K), 0, st, v.lp,
                      logit_lengths_d, target_lengths_d, T, U1, w.S, const_cast<double *>(v.alpha),
                      const_cast<double *>(v.beta), reinterpret_cast<double *>(ws + w.ll_off),
                      reinterpret_cast<double *>(ws + w.cost_off), costs_d, reinterpret_cast<double *>(ws + w.dump_off));
    }
    if (delay_penalty > 0.0)
        WR_TRY(launch("lattice_prepare_kernel<regular>", lattice_prepare_kernel<false>,
                      dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, logit_lengths_d, target_lengths_d, B, T, U1,
                      w.S, delay_penalty, lp_skew, nullptr));
    return rnnt_launch_sweep(w, ws, logit_lengths_d, target_lengths_d, B, T, U1, costs_d, st);
}

extern "C" int wr_rnnt_lattice_export(const void *workspace_d, size_t workspace_bytes, const int32_t *logit_lengths_d,
                                      const int32_t *target_lengths_d, int B, int T, int U1, int lattice_type,
                                      float *alpha_d, float *beta_d, void *stream)
{
    if (int rc = lattice_shape("rnnt_lattice_export", B, T, U1, true)) return rc;
    if (int rc = lattice_check("rnnt_lattice_export", lattice_type, 0.0)) return rc;
    WR_REQUIRE(workspace_d && alpha_d && beta_d && logit_lengths_d && target_lengths_d, WR_EINVAL,
               "rnnt_lattice_export: null pointer argument");
    const RnntWs w = rnnt_ws_layout(B, T, U1);
    WR_REQUIRE(workspace_bytes >= w.total, WR_EWORKSPACE, "rnnt_lattice_export: workspace too small");
    const bool modified = lattice_type == WR_LATTICE_MODIFIED;
    const LatView v = lattice_view(w, static_cast<const char *>(workspace_d), modified);
    const unsigned blocks = (unsigned)(((long)B * T * U1 + 255) / 256);
    hipStream_t st = static_cast<hipStream_t>(stream);
    // (the modified arm comes first, as it always has: the order of the arms is the order of the kernels in the code
    // object, which a host-only change leaves byte-identical)
    return with_bool(modified, [&](auto mod) {
        constexpr int LAT = mod.value ? kLatModified : kLatRegular;
        return launch("lattice_export_kernel", lattice_export_kernel<LAT>, dim3(blocks), dim3(256), 0, st, v.alpha, v.beta,
                      logit_lengths_d, target_lengths_d, B, T, U1, w.S, alpha_d, beta_d);
    });
}
