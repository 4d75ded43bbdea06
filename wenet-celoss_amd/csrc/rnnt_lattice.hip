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
//                             writes one contiguous row.  The exchange, the ring of PF rows in flight and the fp64 state
//                             are lattice_wavefront.hpp's, as for rnnt_sweep_kernel.
//   lattice_export_kernel     alpha / beta of either lattice as plain (B, T, U1) floats, for the tests.
//
// The token-and-duration transducer (TDT) loss and its forced alignment follow at the end of the file: a lattice of its
// own, whose cells have 2 * D arcs that jump up to 8 frames (include/wr_api.h, "Token-and-duration transducer";
// rnnt_tdt.hpp for the arrays).
#include "lattice_wavefront.hpp"
#include "rnnt_lattice.hpp"
#include "rnnt_tdt.hpp"
#include "row_stream.hpp"
#include "wr_launch.hpp"

namespace wr {
namespace {

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
    __shared__ SweepSlots<double> xch;
    const SweepLane L = sweep_lane(llens, tlens, Tmax, U1max);
    const bool backward = blockIdx.y != 0;
    const int u = L.u, T = L.T, U = L.U;

    if (T == 0) {
        sweep_store_empty(L, backward, ll_out, cost_ws, costs_out);
        return;
    }
    const float2 *__restrict__ lp = lp_plain + (size_t)L.b * S * U1max + L.col;
    double *__restrict__ out = sweep_out(L, backward, alpha_plain, beta_plain, S, U1max);
    double *__restrict__ sink = sweep_sink(L, backward, dump);
    const bool ucol = L.ucol;

    auto load_row = [&](int t) -> float2 {
        const int tc = t < 0 ? 0 : (t >= T ? T - 1 : t);
        return lp[(size_t)tc * U1max];
    };

    double result = NEG;

    if (!backward) {
        double st = NEG;      // alpha(t-1, u)
        float skp = 0.f;      // blank(t-1, u)
        double send = NEG;    // alpha(t-1, u) + emit'(t-1, u): what lane u+1 needs
        // frames 0 .. T-1 and the terminal row T; rows t > T have no active lane
        sweep_steps<PF, true>(0, T + 1, load_row, [&](int t, const float2 cur) {
            // every lane is live on row 0, before any slot is written
            const double recv = sweep_recv<true>(L, xch, send, t, (t == 0) ? 0.0 : NEG, t == 0);
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
            st = v;
            skp = sk;
            sweep_post<true>(L, xch, send, t);
        });
        sweep_store_ll(L, ll_out, result);
    } else {
        double st = (u == U) ? 0.0 : NEG;     // beta(t+1, u); row T is the terminal condition
        double send = st;                     // what lane u-1 needs
        sweep_post<false>(L, xch, send, T);
        sweep_steps<PF, false>(T - 1, T, load_row, [&](int t, const float2 cur) {    // rows t < 0 have no active lane
            const double recv = sweep_recv<false>(L, xch, send, t, NEG);     // never unwritten: row T was posted above
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
            st = v;
            sweep_post<false>(L, xch, send, t);
        });
        sweep_store_cost(L, cost_ws, costs_out, result);
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

// ---------------------------------------------------------------- token-and-duration transducer (TDT) --
// Cell (t,u), t < T_b, u <= U_b, of a row of V token logits and D duration logits:
//   tok_k = log_softmax(row[0 .. V))_k - sigma,   dur_n = log_softmax(row[V .. V + D))_n,   d = durations[n]
//   blank arc, d >= 1:         (t,u) -> (t + d, u)       tok_blank + dur_n   (t + d == T_b only at u == U_b: the terminal)
//   label arc, d >= 0, u < U:  (t,u) -> (t + d, u + 1)   tok_label + dur_n   (t + d <= T_b - 1)
//
//   tdt_stats_kernel    one wave per row: both log-sum-exps, {tok_blank, tok_label} and the D duration log-probabilities
//                       into the anti-diagonal arrays.
//   tdt_sweep_kernel    one workgroup per (utterance, direction), one lane per label column, one anti-diagonal per step
//                       (a label arc with d = 0 stays on its frame).  fp64 state in two register rings per lane, one
//                       value exchanged per step (DPP rotate; LDS slot + barrier across waves).
//   tdt_record_kernel   one thread per cell: the gradient's row constants as 3 + D contiguous floats.
//   tdt_grad_kernel     one wave per row: pruned_grad_kernel's streamed loop over the token columns, lanes 0 .. D-1 then
//                       write the duration columns.
//   tdt_export_kernel   alpha / beta as plain (B, T, U1) floats, for the tests.
//   tdt_viterbi_kernel  forced alignment: the forward sweep with max for log-add and one decision byte per cell, then the
//                       backtrace by the same workgroup (include/wr_api.h, "TDT forced alignment").
namespace wr {
namespace {

template <typename T, bool NT, int UN>
__global__ __launch_bounds__(256) void tdt_stats_kernel(
    const T *__restrict__ logits, const int32_t *__restrict__ targets, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, long nrows, int Tmax, int U1max, int V, int D, int blank, float sigma, int S,
    float2 *__restrict__ tok, float *__restrict__ dur, float *__restrict__ denom)
{
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long stride = (long)gridDim.x * (blockDim.x >> 6);
    const int cells = Tmax * U1max;
    for (long r = (long)blockIdx.x * (blockDim.x >> 6) + wid; r < nrows; r += stride) {
        const int b = (int)(r / cells);
        const int c = (int)(r - (long)b * cells);
        const int t = c / U1max, u = c - t * U1max;
        const int Tb = clampi(llens[b], 0, Tmax), Ub = clampi(tlens[b], 0, U1max - 1);
        if (t >= Tb || u > Ub) continue;                      // padding is never read
        const T *row = logits + (size_t)r * (V + D);
        const float d = wave_row_lse<T, NT, UN>(row, V, lane);
        // the D <= 9 duration logits: one per lane
        float x = kNegInf;
        if (lane < D) x = (float)row[V + lane];
        const float y = x * kLog2e;
        const float M = wave_max(y);
        const float s = wave_sum(lane < D ? fast_exp2(y - M) : 0.f);
        const float dd = (M + fast_log2(s)) * kLn2;
        const size_t k = ((size_t)b * S + t + u) * U1max + u;
        if (lane < D) dur[k * D + lane] = x - dd;
        if (lane == 0) {
            const float xb = (float)row[blank];
            float em = kNegInf;
            if (u < Ub) {
                const int lab = targets[(size_t)b * (U1max - 1) + u];
                if (lab >= 0 && lab < V) em = ((float)row[lab] - d) - sigma;
            }
            denom[r] = d;
            tok[k] = make_float2((xb - d) - sigma, em);
        }
    }
}

// the arcs of one cell as a sweep lane holds them: the duration log-probabilities by jump d (slots of absent jumps unused)
struct TdtArc {
    float tb, tl;
    float w[kTdtMaxD];
};

// the arcs of column `col`'s cell on anti-diagonal s of utterance `ub`, its frame clamped into [0, T): always a position
// of the arrays
__device__ __forceinline__ TdtArc tdt_load_arc(const float2 *__restrict__ tok, const float *__restrict__ dur,
                                               const TdtDur &dd, size_t ub, int col, int T, int U1max, int s)
{
    int t = s - col;
    t = t < 0 ? 0 : (t >= T ? T - 1 : t);
    const size_t k = ub + (size_t)(t + col) * U1max + col;
    TdtArc a;
    const float2 p = tok[k];
    a.tb = p.x;
    a.tl = p.y;
#pragma unroll
    for (int d = 0; d < kTdtMaxD; ++d) a.w[d] = dd.slot[d] >= 0 ? dur[k * dd.D + dd.slot[d]] : 0.f;
    return a;
}

// Forward, lane u on anti-diagonal s at cell (t = s - u, u): own[j] / nbr[j] collect the mass that arcs of finished cells
// of this column send into (t + j, u) / (t + j, u + 1).  alpha(t,u) = logadd(own[0], what lane u-1 sent a step ago); the
// cell then pushes its 2 * D arcs into the rings, hands nbr[0] -- complete, every (t' <= t, u) is done -- to lane u + 1, and
// both rings shift by one frame.  The terminal is own[0] of lane U_b at t = T_b: blank arcs only, exactly at T_b.
// Backward: own[j] = beta(t + j, u) with beta(T_b, U_b) = 0 and -inf beyond, nb[j] = beta(t + j, u + 1) as received (an
// idle lane sends -inf, so no label arc reaches frame T_b).  Ring positions are compile-time: the loops over d = 0 .. 8
// unroll against the wave-uniform table `dd`.
template <int PF>
__global__ __launch_bounds__(kRnntMaxCols) void tdt_sweep_kernel(
    const float2 *__restrict__ tok, const float *__restrict__ dur, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, int Tmax, int U1max, int S, const TdtDur dd, double *__restrict__ alpha_skew,
    double *__restrict__ beta_skew, double *__restrict__ ll_out, double *__restrict__ cost_ws,
    float *__restrict__ costs_out, double *__restrict__ dump)
{
    constexpr double NEG = (double)kNegInf;
    __shared__ SweepSlots<double> xch;
    const SweepLane L = sweep_lane(llens, tlens, Tmax, U1max);
    const bool backward = blockIdx.y != 0;
    const int u = L.u, T = L.T, U = L.U;

    if (T == 0) {
        sweep_store_empty(L, backward, ll_out, cost_ws, costs_out);
        return;
    }
    const bool ucol = L.ucol;
    const size_t ub = (size_t)L.b * S * U1max;
    const int nsteps = T + U;                // anti-diagonals 0 .. T + U - 1 hold this utterance's cells
    double *__restrict__ out = sweep_out(L, backward, alpha_skew, beta_skew, S, U1max);
    double *__restrict__ sink = sweep_sink(L, backward, dump);
    auto load_arc = [&](int s) -> TdtArc { return tdt_load_arc(tok, dur, dd, ub, L.col, T, U1max, s); };

    double own[kTdtMaxD], nbr[kTdtMaxD];
#pragma unroll
    for (int j = 0; j < kTdtMaxD; ++j) own[j] = nbr[j] = NEG;
    double send = NEG, result = NEG;

    if (!backward) {
        // the cells' anti-diagonals and the terminal's; steps s > T + U have no active lane
        sweep_steps<PF, true>(0, nsteps + 1, load_arc, [&](int s, const TdtArc &cur) {
            const int t = s - u;
            const double recv = sweep_recv<true>(L, xch, send, s, NEG, s == 0);    // step 0 has nothing to receive
            const bool active = ucol & (t >= 0) & (t < T);
            const double own0 = own[0];
            double v = log_add_exp_d(own0, recv);
            v = (s == 0 && u == 0) ? 0.0 : v;                 // the origin
            result = (t == T && u == U) ? own0 : result;      // the terminal: blank arcs that end exactly at T
            v = active ? v : NEG;
            double *dst = active ? out + (size_t)s * U1max : sink;
            *dst = v;
            const double ab = v + (double)(active ? cur.tb : 0.f);
            const double al = (u < U) ? v + (double)(active ? cur.tl : 0.f) : NEG;
#pragma unroll
            for (int d = 0; d < kTdtMaxD; ++d) {
                if (dd.slot[d] >= 0) {
                    const double w = (double)(active ? cur.w[d] : 0.f);
                    if (d >= 1) own[d] = log_add_exp_d(own[d], ab + w);
                    nbr[d] = log_add_exp_d(nbr[d], al + w);
                }
            }
            send = nbr[0];
#pragma unroll
            for (int j = 0; j + 1 < kTdtMaxD; ++j) { own[j] = own[j + 1]; nbr[j] = nbr[j + 1]; }
            own[kTdtMaxD - 1] = nbr[kTdtMaxD - 1] = NEG;
            sweep_post<true>(L, xch, send, s);
        });
        sweep_store_ll(L, ll_out, result);
    } else {
        const int s0 = nsteps - 1;                // lane U starts at (T - 1, U), below the terminal
        own[1] = (u == U) ? 0.0 : NEG;            // beta(T, U) = 0
        sweep_post<false>(L, xch, NEG, s0 + 1);
        sweep_steps<PF, false>(s0, nsteps, load_arc, [&](int s, const TdtArc &cur) {     // steps s < 0 have no active lane
            const int t = s - u;
            const double recv = sweep_recv<false>(L, xch, send, s, NEG);     // never unwritten: s0 + 1 was posted above
#pragma unroll
            for (int j = kTdtMaxD - 1; j >= 1; --j) nbr[j] = nbr[j - 1];
            nbr[0] = recv;                                    // beta(t, u + 1)
            const bool active = ucol & (t >= 0) & (t < T);
            const float tb = active ? cur.tb : 0.f;
            const float tl = (active && u < U) ? cur.tl : kNegInf;
            double acc = NEG;
#pragma unroll
            for (int d = 0; d < kTdtMaxD; ++d) {
                if (dd.slot[d] >= 0) {
                    const float w = active ? cur.w[d] : 0.f;
                    if (d >= 1) acc = log_add_exp_d(acc, ((double)tb + (double)w) + own[d]);
                    acc = log_add_exp_d(acc, ((double)tl + (double)w) + nbr[d]);
                }
            }
            const double v = active ? acc : NEG;
            double *dst = active ? out + (size_t)s * U1max : sink;
            *dst = v;
            result = (s == 0 && u == 0) ? v : result;
            send = v;
#pragma unroll
            for (int j = kTdtMaxD - 1; j >= 2; --j) own[j] = own[j - 1];
            own[1] = v;
            sweep_post<false>(L, xch, send, s);
        });
        sweep_store_cost(L, cost_ws, costs_out, result);
    }
}

// One thread per cell.  With ll = -cost, a = alpha(t,u):
//   ob_n = exp(a + tok_blank + dur_n + beta(t + d, u) - ll),   ol_n = exp(a + tok_label + dur_n + beta(t + d, u + 1) - ll)
// where the arc exists, 0 elsewhere;  O = exp(a + beta(t,u) - ll).
//   rec[0] = a + beta(t,u) - ll - denom    softmax_k * O = exp(logit_k + rec[0])
//   rec[1] = sum ob_n,  rec[2] = sum ol_n  what the blank / label column subtracts
//   rec[3 + n] = exp(dur_n) * O - (ob_n + ol_n)     d cost / d duration logit n
// Everything in fp64, rounded once.  A cell no path crosses has a or beta = -inf against a finite ll: exact zeros.
__global__ __launch_bounds__(256) void tdt_record_kernel(
    const float2 *__restrict__ tok, const float *__restrict__ dur, const float *__restrict__ denom,
    const double *__restrict__ alpha_skew, const double *__restrict__ beta_skew, const double *__restrict__ cost_ws,
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens, int B, int Tmax, int U1max, int S,
    const TdtDur dd, float *__restrict__ rec)
{
    constexpr double NEG = (double)kNegInf;
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= (long)B * Tmax * U1max) return;
    const int cells = Tmax * U1max;
    const int b = (int)(r / cells);
    const int c = (int)(r - (long)b * cells);
    const int t = c / U1max, u = c - t * U1max;
    const int T = clampi(llens[b], 0, Tmax), U = clampi(tlens[b], 0, U1max - 1);
    if (t >= T || u > U) return;
    const int D = dd.D;
    const size_t ub = (size_t)b * S * U1max;
    const size_t k = ub + (size_t)(t + u) * U1max + u;
    const double a = alpha_skew[k], be = beta_skew[k], ll = -cost_ws[b];
    const float2 p = tok[k];
    const double base = a - ll;
    const double O = exp(base + be);
    float *o = rec + (size_t)r * (kTdtRec + D);
    double Ob = 0.0, Ol = 0.0;
#pragma unroll
    for (int d = 0; d < kTdtMaxD; ++d) {
        const int n = dd.slot[d];
        if (n < 0) continue;
        const double w = (double)dur[k * D + n];
        double bb = NEG, bl = NEG;
        if (d >= 1) {
            if (t + d < T) bb = beta_skew[ub + (size_t)(t + d + u) * U1max + u];
            else if (t + d == T && u == U) bb = 0.0;
        }
        if (u < U && t + d < T) bl = beta_skew[ub + (size_t)(t + d + u + 1) * U1max + (u + 1)];
        const double ob = bb == NEG ? 0.0 : exp(((base + (double)p.x) + w) + bb);
        const double ol = bl == NEG ? 0.0 : exp(((base + (double)p.y) + w) + bl);
        Ob += ob;
        Ol += ol;
        o[kTdtRec + n] = (float)(exp(w) * O - (ob + ol));
    }
    o[0] = (float)((base + be) - (double)denom[r]);
    o[1] = (float)Ob;
    o[2] = (float)Ol;
}

// pruned_grad_kernel's streamed loop on rows of V + D logits: g_k = exp(logit_k + rec[0]) over the V token columns, the
// blank and the label column minus rec[1] / rec[2] (both when they coincide), then lanes 0 .. D-1 write rec[3 + n] into the
// duration columns.  No clamp, no dead-row skip.  In place: a lane stores an element only after loading it, and the
// duration columns are not read at all.
template <typename T, bool NT, bool NTS, int UN>
__global__ __launch_bounds__(256) void tdt_grad_kernel(
    const T *logits, const int32_t *__restrict__ targets, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, long nrows, int Tmax, int U1max, int V, int D, int blank,
    const float *__restrict__ rec, const float *__restrict__ grad_costs, T *grads)
{
    typedef typename VecOf<T>::type vec_t;
    constexpr int N = VecOf<T>::N;
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long stride = (long)gridDim.x * (blockDim.x >> 6);
    const int cells = Tmax * U1max;
    const int W = V + D;
    for (long r = (long)blockIdx.x * (blockDim.x >> 6) + wid; r < nrows; r += stride) {
        const int b = (int)(r / cells);
        const int c = (int)(r - (long)b * cells);
        const int t = c / U1max, u = c - t * U1max;
        const int T_ = clampi(llens[b], 0, Tmax), U = clampi(tlens[b], 0, U1max - 1);
        const T *row = logits + (size_t)r * W;
        T *grow = grads + (size_t)r * W;
        const float go = grad_costs ? grad_costs[b] : 1.f;

        const bool valid = t < T_ && u <= U;
        if (__builtin_amdgcn_readfirstlane(valid ? 0 : 1)) {          // outside the lattice: grad_costs[b] * 0, logits unread
            const RowSplit<T> sp(row, W);
            vec_t *gbody = reinterpret_cast<vec_t *>(grow + sp.h);
            const T val = (T)(go * 0.f);
            vec_t z;
#pragma unroll
            for (int q = 0; q < N; ++q) z[q] = val;
            if (lane < sp.h) grow[lane] = val;
            if (lane < sp.tail) grow[sp.h + N * sp.nv + lane] = val;
            for (int i = lane; i < sp.nv; i += kWave) stv<NTS>(z, gbody + i);
            continue;
        }
        const RowSplit<T> sp(row, V);
        const int h = sp.h, nv = sp.nv, tail = sp.tail;
        const vec_t *body = reinterpret_cast<const vec_t *>(row + h);
        vec_t *gbody = reinterpret_cast<vec_t *>(grow + h);
        const float *rc = rec + (size_t)r * (kTdtRec + D);            // one contiguous record
        const float c2 = rc[0] * kLog2e;
        const float blank_sub = rc[1], lab_sub = rc[2];
        const float dval = lane < D ? rc[kTdtRec + lane] : 0.f;
        const int lab = u < U ? targets[(size_t)b * (U1max - 1) + u] : -1;

        auto fix = [&](float val, int v) -> float {
            if (v == blank) val -= blank_sub;
            if (v == lab) val -= lab_sub;
            return val;
        };
        if (lane < h) {
            const float x = (float)row[lane];
            grow[lane] = (T)(fix(fast_exp2(fmaf(x, kLog2e, c2)), lane) * go);
        }
        if (lane < tail) {
            const int v = h + N * nv + lane;
            const float x = (float)row[v];
            grow[v] = (T)(fix(fast_exp2(fmaf(x, kLog2e, c2)), v) * go);
        }
        const int iblk = (blank >= h) ? ((blank - h) / N) : -1;
        const int ilab = (lab >= h) ? ((lab - h) / N) : -1;
        auto dov = [&](int i, const vec_t x) {
            float g[N];
#pragma unroll
            for (int q = 0; q < N; ++q) g[q] = fast_exp2(fmaf((float)x[q], kLog2e, c2));
            if (i == iblk || i == ilab) {
                const int v0 = h + N * i;
#pragma unroll
                for (int q = 0; q < N; ++q) g[q] = fix(g[q], v0 + q);
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
        if (lane < D) grow[V + lane] = (T)(dval * go);
    }
}

__global__ __launch_bounds__(256) void tdt_export_kernel(
    const double *__restrict__ alpha_skew, const double *__restrict__ beta_skew, const int32_t *__restrict__ llens,
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
        const size_t k = (size_t)b * S * U1 + (size_t)(t + u) * U1 + u;
        a = (float)alpha_skew[k];
        be = (float)beta_skew[k];
    }
    alpha[r] = a;
    beta[r] = be;
}

// ---- TDT forced alignment (include/wr_api.h, "TDT forced alignment"): the best path of the lattice above.
constexpr int kTdtStageBytes = 32768;      // decision bytes staged in LDS per backtrace block ...
constexpr int kTdtStageDiags = 256;        // ... of at most this many anti-diagonals (at least 32: U1max <= 1024)
constexpr int kTdtJumpWindow = 2048;       // frames whose blank jumps collect in LDS between two coalesced flushes
// decision byte of a cell: the winning arc's d in the low nibble, kTdtDecLabel set if it is a label arc; kTdtDecNone where
// no arc won (the cell is unreachable)
constexpr unsigned kTdtDecLabel = 0x10;
constexpr unsigned kTdtDecNone = 0xFF;

// The forward branch of tdt_sweep_kernel with max for log-add: own[j] / nbr[j] hold the best blank / label candidate into
// (t + j, u) / (t + j, u + 1) and, in nibble j of otags / ntags, the jump d of the arc that holds it.  A push replaces on
// >=: within one ring entry later pushes come from later frames, so the smaller d wins a tie, and a NaN candidate never
// replaces anything.  The two rings merge as "label only if strictly greater"; the terminal is own[0] of lane U_b at
// t = T_b.  Every cell's decision goes out as one byte in anti-diagonal order (`decisions`: the workspace's beta region).
//
// Backtrace, same workgroup: rounds of (stage a block of anti-diagonals into LDS, coalesced; thread 0 walks it; all
// threads flush the blank jumps of the frames walked, coalesced).  Every step lowers t + u, the walk is bounded by
// T_b + U_b + 1 arcs all the same, and a decision byte that names no arc of this lattice ends it with the no-path outputs.
template <int PF>
__global__ __launch_bounds__(kRnntMaxCols) void tdt_viterbi_kernel(
    const float2 *__restrict__ tok, const float *__restrict__ dur, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, int Tmax, int U1max, int S, const TdtDur dd, uint8_t *decisions,
    int32_t *__restrict__ label_frames, int32_t *__restrict__ label_durations, int32_t *__restrict__ blank_jumps,
    double *__restrict__ scores)
{
    constexpr double NEG = (double)kNegInf;
    __shared__ SweepSlots<double> xch;
    __shared__ SweepSlots<int> xtag;
    __shared__ uint32_t stage[kTdtStageBytes / 4 + 1];
    __shared__ int lfr[kRnntMaxCols], ldu[kRnntMaxCols];
    __shared__ uint8_t jl[kTdtJumpWindow];
    __shared__ int cur[4];      // the backtrace cursor: t, u, state (0 walking, 1 at the origin, 2 no path), terminal's d
    const SweepLane L = sweep_lane(llens, tlens, Tmax, U1max);
    const int b = L.b, u = L.u, T = L.T, U = L.U;
    int32_t *frames_out = label_frames + (size_t)b * (U1max - 1);
    int32_t *durs_out = label_durations + (size_t)b * (U1max - 1);
    int32_t *jumps_out = blank_jumps ? blank_jumps + (size_t)b * Tmax : nullptr;

    const bool ucol = L.ucol;
    const size_t ub = (size_t)b * S * U1max;
    const int nsteps = T + U;                // anti-diagonals 0 .. T + U - 1 hold this utterance's cells
    uint8_t *dec = decisions + ub;

    auto load_arc = [&](int s) -> TdtArc { return tdt_load_arc(tok, dur, dd, ub, L.col, T, U1max, s); };

    double result = NEG;
    int rdec = 0;
    if (T > 0) {                             // T_b = 0 has no cell to read: no path (the Python layer refuses it)
        double own[kTdtMaxD], nbr[kTdtMaxD];
#pragma unroll
        for (int j = 0; j < kTdtMaxD; ++j) own[j] = nbr[j] = NEG;
        uint64_t otags = 0, ntags = 0;
        double send = NEG;
        int stag = 0;
        // the cells' anti-diagonals and the terminal's; steps s > T + U have no active lane
        sweep_steps<PF, true>(0, nsteps + 1, load_arc, [&](int s, const TdtArc &cur_arc) {
            const int t = s - u;
            // step 0 has nothing to receive; the candidate's tag travels with it (the same wave rotate)
            const double recv = sweep_recv<true>(L, xch, send, s, NEG, s == 0);
            const int rtag = sweep_recv_slot<true, int>(L, xtag, __builtin_amdgcn_update_dpp(0, stag, 0x13C, 0xf, 0xf, false),
                                                        s, 0, s == 0, 0);
            const bool active = ucol & (t >= 0) & (t < T);
            const double own0 = own[0];
            const int otag0 = (int)(otags & 15);
            const bool lab = recv > own0;                     // strict: a tie goes to the blank arc
            double v = lab ? recv : own0;
            unsigned by = lab ? (kTdtDecLabel | (unsigned)rtag) : (unsigned)otag0;
            if (s == 0 && u == 0) { v = 0.0; by = 0; }        // the origin
            if (t == T && u == U) { result = own0; rdec = otag0; }   // the terminal: blank arcs that end exactly at T
            v = active ? v : NEG;
            by = (v == NEG) ? kTdtDecNone : by;
            if (active) dec[(size_t)s * U1max + u] = (uint8_t)by;
            const double ab = v + (double)(active ? cur_arc.tb : 0.f);
            const double al = (u < U) ? v + (double)(active ? cur_arc.tl : 0.f) : NEG;
#pragma unroll
            for (int d = 0; d < kTdtMaxD; ++d) {
                if (dd.slot[d] >= 0) {
                    const double w = (double)(active ? cur_arc.w[d] : 0.f);
                    const uint64_t clr = ~((uint64_t)15 << (4 * d)), tag = (uint64_t)d << (4 * d);
                    if (d >= 1) {
                        const double c = ab + w;
                        const bool win = c >= own[d];
                        own[d] = win ? c : own[d];
                        otags = win ? ((otags & clr) | tag) : otags;
                    }
                    const double c = al + w;
                    const bool win = c >= nbr[d];
                    nbr[d] = win ? c : nbr[d];
                    ntags = win ? ((ntags & clr) | tag) : ntags;
                }
            }
            send = nbr[0];
            stag = (int)(ntags & 15);
#pragma unroll
            for (int j = 0; j + 1 < kTdtMaxD; ++j) { own[j] = own[j + 1]; nbr[j] = nbr[j + 1]; }
            own[kTdtMaxD - 1] = nbr[kTdtMaxD - 1] = NEG;
            otags >>= 4;
            ntags >>= 4;
            sweep_put<true>(L, xtag, stag, s);
            sweep_post<true>(L, xch, send, s);
        });
    }
    if (u == U) {
        scores[b] = result;
        cur[0] = T;
        cur[1] = U;
        cur[2] = (result > NEG) ? 0 : 2;
        cur[3] = rdec;
    }
    // every lane stored decision bytes: drain them and drop this CU's cached lines before the workgroup reads them back
    __threadfence();
    __syncthreads();

    unsigned dmask = 0;
#pragma unroll
    for (int d = 0; d < kTdtMaxD; ++d) dmask |= dd.slot[d] >= 0 ? 1u << d : 0u;
    const int nd = min(kTdtStageDiags, kTdtStageBytes / U1max);
    int budget = T + U + 1;                  // thread 0's: arcs of the longest path, the terminal's included
    while (cur[2] == 0) {
        const int ct = cur[0], cu = cur[1];  // the cursor (t, u): on diagonal ct + cu, or the terminal (T, U)
        const int hi = min(ct + cu, nsteps - 1), lo = max(hi - nd + 1, 0);
        const size_t g0 = ub + (size_t)lo * U1max, a0 = g0 & ~(size_t)3;     // whole words, from the one that holds g0
        const int nwords = ((hi - lo + 1) * U1max + (int)(g0 - a0) + 3) >> 2;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(decisions + a0);
        for (int i = u; i < nwords; i += blockDim.x) stage[i] = src[i];
        const int fhi = ct - 1, flo = max(fhi - kTdtJumpWindow + 1, 0);      // frames >= ct are final already
        for (int i = u; i < kTdtJumpWindow; i += blockDim.x) jl[i] = 0;
        __syncthreads();
        if (u == 0) {
            const uint8_t *sb = reinterpret_cast<const uint8_t *>(stage) + (g0 - a0);
            int t = ct, uu = cu, state = 0;
            while (true) {
                if (t == 0 && uu == 0) { state = 1; break; }
                const int s = t + uu;
                if (t < T && s < lo) break;                       // the next block
                const unsigned by = (t == T) ? (unsigned)cur[3] : sb[(s - lo) * U1max + uu];
                const int d = by & 15, f = t - d;
                const bool lab = (by & kTdtDecLabel) != 0;
                const bool arc = (by >> 5) == 0 && ((dmask >> d) & 1) != 0 && f >= 0 && (lab ? uu >= 1 : d >= 1);
                if (!arc || --budget < 0) { state = 2; break; }
                if (f < flo) break;                               // the next window of frames
                if (lab) { --uu; lfr[uu] = f; ldu[uu] = d; } else jl[fhi - f] = (uint8_t)d;
                t = f;
            }
            if (state == 0 && t == ct && uu == cu) state = 2;     // a round always takes a step: nd > 9, the window > 8
            cur[0] = t;
            cur[1] = uu;
            cur[2] = state;
        }
        __syncthreads();
        if (jumps_out)
            for (int f = cur[0] + u; f <= fhi; f += blockDim.x) jumps_out[f] = jl[fhi - f];
        __syncthreads();
    }
    const bool found = cur[2] == 1;
    if (!found && u == 0) scores[b] = NEG;
    for (int i = u; i < U1max - 1; i += blockDim.x) {
        const bool in = found && i < U;
        frames_out[i] = in ? lfr[i] : -1;
        durs_out[i] = in ? ldu[i] : -1;
    }
    if (jumps_out)
        for (int f = (found ? T : 0) + u; f < Tmax; f += blockDim.x) jumps_out[f] = 0;
}

}  // namespace

// pass 1 of the loss and of the alignment: {tok_blank, tok_label}, the D duration log-probabilities and the token
// log-sum-exp of every cell
static int tdt_launch_stats(const TdtWs &w, char *ws, const void *logits_d, int dtype, const int32_t *targets_d,
                            const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                            int V, int D, int blank, double sigma, hipStream_t st)
{
    float2 *tok = reinterpret_cast<float2 *>(ws + w.tok_off);
    float *durp = reinterpret_cast<float *>(ws + w.dur_off);
    float *denom = reinterpret_cast<float *>(ws + w.denom_off);
    const long nrows = (long)B * Tmax * U1max;
    const size_t row_bytes = (size_t)(V + D) * (dtype == WR_F32 ? 4 : 2);
    const dim3 grid1(stream_grid(nrows, tune_get(kTuneLseBlocksPerCu), row_bytes, 16 * 1024));
    const bool nt = (tune_get(kTuneNonTemporal) & 4) != 0;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_bool(nt, [&](auto nt_c) {
            return with_int<16, 8, 4>(unroll_of(kTuneLseUnroll), [&](auto un) {
                return launch("tdt_stats_kernel", tdt_stats_kernel<T, nt_c.value, un.value>, grid1, dim3(256), 0, st,
                              static_cast<const T *>(logits_d), targets_d, logit_lengths_d, target_lengths_d, nrows, Tmax,
                              U1max, V, D, blank, (float)sigma, w.S, tok, durp, denom);
            });
        });
    });
}

int tdt_loss_fwd_body(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                      const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank, const TdtDur &dur,
                      double sigma, float *costs_d, void *workspace_d, hipStream_t st)
{
    const TdtWs w = tdt_ws_layout(B, Tmax, U1max, dur.D);
    WR_TRY(tdt_launch_stats(w, static_cast<char *>(workspace_d), logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d,
                            B, Tmax, U1max, V, dur.D, blank, sigma, st));
    return tdt_sweeps_body(logit_lengths_d, target_lengths_d, B, Tmax, U1max, dur, costs_d, workspace_d, st);
}

int tdt_sweeps_body(const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                    const TdtDur &dur, float *costs_d, void *workspace_d, hipStream_t st)
{
    const TdtWs w = tdt_ws_layout(B, Tmax, U1max, dur.D);
    char *ws = static_cast<char *>(workspace_d);
    float2 *tok = reinterpret_cast<float2 *>(ws + w.tok_off);
    float *durp = reinterpret_cast<float *>(ws + w.dur_off);
    float *denom = reinterpret_cast<float *>(ws + w.denom_off);
    double *alpha = reinterpret_cast<double *>(ws + w.alpha_off), *beta = reinterpret_cast<double *>(ws + w.beta_off);
    double *cost = reinterpret_cast<double *>(ws + w.cost_off);
    const long nrows = (long)B * Tmax * U1max;
    WR_TRY(launch("tdt_sweep_kernel", tdt_sweep_kernel<4>, dim3(B, 2), dim3(64 * w.K), 0, st, tok, durp, logit_lengths_d,
                  target_lengths_d, Tmax, U1max, w.S, dur, alpha, beta, reinterpret_cast<double *>(ws + w.ll_off), cost,
                  costs_d, reinterpret_cast<double *>(ws + w.dump_off)));
    return launch("tdt_record_kernel", tdt_record_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, tok, durp,
                  denom, alpha, beta, cost, logit_lengths_d, target_lengths_d, B, Tmax, U1max, w.S, dur,
                  reinterpret_cast<float *>(ws + w.rec_off));
}

int tdt_loss_bwd_body(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                      const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank, int D,
                      const float *grad_costs_d, void *grads_d, const void *workspace_d, hipStream_t st)
{
    const TdtWs w = tdt_ws_layout(B, Tmax, U1max, D);
    const char *ws = static_cast<const char *>(workspace_d);
    const long nrows = (long)B * Tmax * U1max;
    const size_t row_bytes = (size_t)(V + D) * (dtype == WR_F32 ? 4 : 2);
    const dim3 grid3(stream_grid(nrows, tune_get(kTuneGradBlocksPerCu), row_bytes, 68 * 1024));
    const bool nt = (tune_get(kTuneNonTemporal) & 1) != 0;
    const bool nts = (tune_get(kTuneNonTemporal) & 2) != 0;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_bool(nt, [&](auto nt_c) {
            return with_int<16, 8, 4>(unroll_of(kTuneGradUnroll), [&](auto un) {
                return with_bool(nts, [&](auto nts_c) {
                    return launch("tdt_grad_kernel", tdt_grad_kernel<T, nt_c.value, nts_c.value, un.value>, grid3, dim3(256),
                                  0, st, static_cast<const T *>(logits_d), targets_d, logit_lengths_d, target_lengths_d,
                                  nrows, Tmax, U1max, V, D, blank, reinterpret_cast<const float *>(ws + w.rec_off),
                                  grad_costs_d, static_cast<T *>(grads_d));
                });
            });
        });
    });
}

int tdt_export_body(const void *workspace_d, const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B,
                    int Tmax, int U1max, int D, float *alpha_d, float *beta_d, hipStream_t st)
{
    const TdtWs w = tdt_ws_layout(B, Tmax, U1max, D);
    const char *ws = static_cast<const char *>(workspace_d);
    return launch("tdt_export_kernel", tdt_export_kernel, dim3((unsigned)(((long)B * Tmax * U1max + 255) / 256)), dim3(256),
                  0, st, reinterpret_cast<const double *>(ws + w.alpha_off),
                  reinterpret_cast<const double *>(ws + w.beta_off), logit_lengths_d, target_lengths_d, B, Tmax, U1max, w.S,
                  alpha_d, beta_d);
}

int tdt_align_body(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                   const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank, const TdtDur &dur,
                   double sigma, int32_t *label_frames_d, int32_t *label_durations_d, int32_t *blank_jumps_d,
                   double *scores_d, void *workspace_d, hipStream_t st)
{
    const TdtWs w = tdt_ws_layout(B, Tmax, U1max, dur.D);
    char *ws = static_cast<char *>(workspace_d);
    WR_TRY(tdt_launch_stats(w, ws, logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V, dur.D,
                            blank, sigma, st));
    // one decision byte per cell, in the beta region (8 bytes per cell), which alignment does not use otherwise
    // (three rows in flight: with the sweep's four the rings and their tags no longer fit 128 VGPRs)
    return launch("tdt_viterbi_kernel", tdt_viterbi_kernel<3>, dim3(B), dim3(64 * w.K), 0, st,
                  reinterpret_cast<const float2 *>(ws + w.tok_off), reinterpret_cast<const float *>(ws + w.dur_off),
                  logit_lengths_d, target_lengths_d, Tmax, U1max, w.S, dur, reinterpret_cast<uint8_t *>(ws + w.beta_off),
                  label_frames_d, label_durations_d, blank_jumps_d, scores_d);
}

}  // namespace wr
