// RNN-T loss + gradient for MI355X (gfx950), replacing the
// torchaudio.functional.rnnt_loss call sites of the reference
// (wenet/transducer/transducer.py:142-147 and :296-301).  See include/wr_api.h.
//
// Three device passes over a batch of variable-length utterances packed into
// one grid (mathematics: SURVEY.md App. A.1):
//
//   pass 1  rnnt_lse_kernel    one wave per lattice cell (b,t,u): streams the
//           V logits of the cell once (16-B loads, online max/sum), writes
//           denom(t,u) and the two log-probs the lattice needs
//           (skip = blank, emit = label) into a *diagonal-skewed* array.
//           HBM-bound: 4*V bytes read per cell.
//   pass 2  rnnt_sweep_kernel  one workgroup per (utterance, direction), one lane per label column, one anti-diagonal
//           per dependent step (the wavefront scheme: lattice_wavefront.hpp).  Latency-bound.
//   pass 3  rnnt_grad_kernel   one wave per cell again: re-reads the V logits,
//           writes grad = g_b * (exp(logit + alpha + beta + cost - denom) with
//           the blank / label corrections), zero in the padded region.  A dead
//           cell (every exponential provably +0, kDeadThr) is written as
//           g_b * 0 without reading its logits; a faint cell (the main
//           exponential provably +0, the blank or label term not) the same
//           way except that element, for which that one logit is read.
//           HBM-bound: 4*V read (live cells only) + 4*V written per cell.
//
// Algorithmic traffic: 3 * 4 * V bytes per live valid cell, 2 * 4 * V per dead
// cell, 2 * 4 * V + two sectors read per faint cell (+ 4*V per padded cell).
// Dead and faint cells are about 38 % of the BASELINE batch (iid N(0,1)
// logits; 2 % faint); the share depends on the data.
#include "lattice_wavefront.hpp"
#include "rnnt_latency.hpp"
#include "row_stream.hpp"
#include "wr_common.hpp"
#include "wr_launch.hpp"

namespace wr {
namespace {

// ------------------------------------------------------------------ pass 1 --
// (row streaming helpers: row_stream.hpp)
template <typename T, bool NT, int UN>
__global__ __launch_bounds__(256) void rnnt_lse_kernel(
    const T *__restrict__ logits, const int32_t *__restrict__ targets,
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens,
    int B, int Tmax, int U1max, int V, int blank, int K, int S,
    float2 *__restrict__ lp_skew, float *__restrict__ denom, const int32_t *__restrict__ run_if,
    int order, int order_run /* logical_block's mode and c */)
{
    if (run_if != nullptr && *run_if == 0) return;     // repair pass behind the joiner's fused epilogue: usually nothing to do
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    const long nrows = (long)B * Tmax * U1max;
    const long stride = (long)gridDim.x * waves_per_block;
    const int cells = Tmax * U1max;
    const long first = (long)logical_block(blockIdx.x, gridDim.x, order, (unsigned)order_run);
    for (long r = first * waves_per_block + wid; r < nrows; r += stride) {
        const int b = (int)(r / cells);
        const int c = (int)(r - (long)b * cells);
        const int t = c / U1max;
        const int u = c - t * U1max;
        const int T_ = llens[b], U = tlens[b];
        if (t >= T_ || u > U) continue;
        const T *row = logits + (size_t)r * V;
        const float d = wave_row_lse<T, NT, UN>(row, V, lane);
        if (lane == 0) {
            const float xb = (float)row[blank];
            float em = 0.f;
            if (u < U) {
                const int lab = targets[(size_t)b * (U1max - 1) + u];
                em = (float)row[lab] - d;
            }
            denom[r] = d;
            const int s = t + u;
            lp_skew[((size_t)b * S + s) * U1max + u] = make_float2(xb - d, em);
        }
    }
}

// ------------------------------------------------------------------ pass 2 --
// The wavefront scheme (lanes, neighbour exchange, PF-deep ring, fp64 state and why) is lattice_wavefront.hpp's; the
// forward step is its rnnt_forward_step, shared with rnnt_viterbi_kernel.  Step s: cell (t = s - u, u) of anti-diagonal s.
template <int PF>
__global__ __launch_bounds__(kRnntMaxCols) void rnnt_sweep_kernel(
    const float2 *__restrict__ lp_skew, const int32_t *__restrict__ llens,
    const int32_t *__restrict__ tlens, int Tmax, int U1max, int S,
    double *__restrict__ alpha_skew, double *__restrict__ beta_skew,
    double *__restrict__ ll_out, double *__restrict__ cost_ws, float *__restrict__ costs_out,
    double *__restrict__ dump /* [2*B*kRnntMaxCols] scratch that absorbs the stores of idle lanes */)
{
    constexpr double NEG = (double)kNegInf;
    __shared__ SweepSlots<double> xch;
    const SweepLane L = sweep_lane(llens, tlens, Tmax, U1max);
    const bool backward = blockIdx.y != 0;
    const int u = L.u, T = L.T, U = L.U;
    const int nsteps = (T > 0) ? T + U : 0;       // anti-diagonals that hold a valid cell

    if (nsteps == 0) {
        sweep_store_empty(L, backward, ll_out, cost_ws, costs_out);
        return;
    }
    const float2 *__restrict__ lp = lp_skew + (size_t)L.b * S * U1max + L.col;
    double *__restrict__ out = sweep_out(L, backward, alpha_skew, beta_skew, S, U1max);
    double *__restrict__ sink = sweep_sink(L, backward, dump);

    auto load_row = [&](int s) -> float2 {
        const int sc = s < 0 ? 0 : (s >= nsteps ? nsteps - 1 : s);
        return lp[(size_t)sc * U1max];
    };

    if (!backward) {
        RnntFwd f;
        sweep_steps<PF, true>(0, nsteps, load_row, [&](int s, const float2 cur) {     // steps s >= nsteps have no active lane
            rnnt_forward_step(L, xch, s, cur, f, [&](bool active, int, double top, double recv) {
                double v = log_add_exp_d(top, recv);     // the origin sees recv = 0, top = -inf  ->  0
                v = active ? v : NEG;
                double *dst = active ? out + (size_t)s * U1max : sink;
                *dst = v;
                return v;
            });
        });
        sweep_store_ll(L, ll_out, f.result);
    } else {
        double st = NEG;      // beta(t+1, u): this lane's value on the previous diagonal
        double send = NEG;    // beta(t, u): what the lane to the left needs on the next step
        double result = 0.0;
        // This branch keeps its own ring loop and its own receive: with sweep_steps or sweep_recv the kernel compiles to
        // 66 VGPRs (7 waves per SIMD) against 62 (8) as written here (profiles/lattice_wavefront.md).
        float2 ring[PF];
#pragma unroll
        for (int i = 0; i < PF; ++i) ring[i] = load_row(nsteps - 1 - i);
        for (int base = 0; base < nsteps; base += PF) {
#pragma unroll
            for (int i = 0; i < PF; ++i) {
                const int s = nsteps - 1 - (base + i);   // steps s < 0 have no active lane
                const float2 cur = ring[i];
                ring[i] = load_row(s - PF);
                // beta(t, u+1) from the lane to the right (on the first step the lanes at a wave boundary are idle)
                double recv = lane_rotate_down_d(send);
                if (L.lane == kWave - 1) recv = (L.wave == L.nw - 1) ? NEG : xch[(s + 1) & 1][L.wave + 1];
                const int t = s - u;
                const bool active = (t >= 0) & (t < T) & (u <= U);
                const float sk = active ? cur.x : 0.f;
                const float em = active ? cur.y : 0.f;
                const double down = (t < T - 1) ? st + (double)sk : NEG;
                const double right = (u < U) ? recv + (double)em : NEG;
                double v = log_add_exp_d(down, right);
                v = (t == T - 1 && u == U) ? (double)sk : v;
                v = active ? v : NEG;
                double *dst = active ? out + (size_t)s * U1max : sink;
                *dst = v;
                result = (active && t == 0 && u == 0) ? v : result;
                send = v;
                st = v;
                sweep_post<false>(L, xch, send, s);
            }
        }
        sweep_store_cost(L, cost_ws, costs_out, result);
    }
}

// ------------------------------------------------------------------ pass 3 --
// Dead and faint cells.  Every exponential of a cell's gradient is bounded without its logits: x <= denom for every
// logit x of the row, so the main term's exponent x + alpha + beta + cost - denom is at most lo = alpha + beta + cost
// (the cell's log-occupancy), the blank term's at most alpha + cost + beta(t+1,u) (alpha + cost at the final cell) and
// the label term's at most alpha + cost + beta(t,u+1).  A term whose bound is below kDeadThr has a fast_exp2 that
// returns +0 whatever the logits hold.  Main term below it: every element of the row is finish(+0 - its case-chain
// term), and only the blank and the label element have such a term.  If those bounds are below the threshold too
// (or do not apply) the subtraction gives 0 - 0 = +0 and the row is finish(0) everywhere: a dead row, written without
// being read.  Otherwise it is a faint row: finish(0) everywhere except the blank and / or label element, for which
// that one logit is read.  The side bounds exceed lo by about one step's log-probability, so faint rows are a rim
// around the dead region.
//
// Bound on what the kernel itself evaluates (log2 units; u = 2^-24 is the fp32 unit roundoff):
//   - denom >= max x up to its own rounding: pass 1 takes M = fl(max x * log2e) (fmaxf of rounded products is the
//     rounded maximum), adds fast_log2(s) >= 0 (s >= 1: the maximum's own term is 2^0) and rounds (M + l) * ln2;
//     the joiner epilogue (joint_lse.hpp) bounds a lane's ref + log2(s) the same way.  So x - denom <= 4u |denom|.
//   - main term: c2 = fl(fl(cmd + be) * log2e) rounds a quantity of magnitude |lo - denom| twice and fmaf rounds
//     once more.  Blank / label terms: blank_sub (lab_sub) = fl(cmd + beta') once, then the sum with x and the
//     product with log2e once each.  For a negative bound every argument is therefore at most
//     log2e * ((1 - 4u) * bound + 12u * |denom|).
//   - |denom| < kDeadDenomMax = 2^16 caps the last term at 0.05 nats.  It is also the test that denom is finite: a
//     +inf or NaN logit makes denom +inf or NaN, and such rows keep the streaming path and their NaN pattern.
// The cut-off: __builtin_amdgcn_exp2f (v_exp_f32) flushes denormal results on gfx950.  Measured over every float in
// [-152, -125] with the library's compile flags (tests/test_rnnt_faint_rows_gpu.py::test_exp2_cutoff): +0 for every
// float <= x0 = -126.00000763 (0xC2FC0001, the float below -126), 2^-126 at -126.  kDeadThr = (x0 - 8.6) / log2e
// rounded down to one decimal keeps the margin of 8.6 log2 units this threshold has always had (-110 nats against the
// -150 of an exp2 that keeps denormals): bound < -93.3 nats gives log2e * bound < -134.60, and with the roundings
// above every argument is below log2e * (-93.3 * (1 - 4u) + 0.047) = -134.53.  The same test checks +0 for every float
// <= x0 down to -inf.  Every comparison is written so that a NaN operand makes the row live / the element read.
constexpr double kDeadThr = -93.3;
constexpr float kDeadDenomMax = 65536.f;

// Element v of a row whose main term is +0: the blank / label element that was read, or the row's finish(0).
template <typename T>
__device__ __forceinline__ T faint_pick(int v, int sblk, T vblk, int slab, T vlab, T val)
{
    return v == sblk ? vblk : (v == slab ? vlab : val);
}

// The regularised form of the pass (REG: FastEmit and the delay penalty, include/wr_api.h "FastEmit and the delay penalty
// for the full-lattice loss") is a second instantiation of rnnt_grad_kernel with one more argument; the plain one keeps
// its code.  The regularisers change three per-row constants and nothing per element:
//   be_eff  = logadd(beta, log lambda + emit' + beta(t,u+1)) replaces beta in the main term (fp64; emit' is the stored,
//             already penalised label arc of the workspace, so no logit is read for it and grads may alias logits),
//   lab_sub = cmd + beta(t,u+1) + pen(b,t) + log1p(lambda), both only where the label term exists; blank_sub is unchanged.
// Dead / faint rows with them.  The three bounds are the same quantities: main alpha + cost + be_eff, label alpha + cost +
// beta(t,u+1) + pen + log1p(lambda) (pen can be positive: the bound is still what is compared), blank unchanged.  The
// rounding argument above kDeadThr carries over term by term: be_eff and pen + log1p(lambda) are formed and added in
// fp64 before the one rounding to fp32 that c2 / lab_sub always had, so the main argument is again fl(fl(cmd + be_eff)
// log2e) fma'd with x log2e (three roundings of a quantity of magnitude <= |bound| + |denom|) and the label argument
// fl(fl(x + lab_sub) log2e) with lab_sub = fl(bound - denom) (three again), and x - denom <= 4u |denom| does not involve
// them.  For a negative bound every argument is therefore at most log2e * ((1 - 4u) * bound + 12u * |denom|), as before,
// and bound < kDeadThr gives +0.  A NaN in be_eff or the penalised bound makes the comparison false: live / read.
// `Reg`: empty (the plain pass: the kernel and its arguments are what they always were) or one RnntRegArgs.
template <typename T, bool NT /* loads */, bool NTS /* stores */, int UN, typename... Reg>
__global__ __launch_bounds__(256) void rnnt_grad_kernel(
    const T *logits, const int32_t *__restrict__ targets,
    const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens,
    int B, int Tmax, int U1max, int V, int blank, float clamp, int K, int S,
    const double *__restrict__ alpha_skew, const double *__restrict__ beta_skew,
    const float *__restrict__ denom, const double *__restrict__ cost_ws,
    const float *__restrict__ grad_costs, T *grads, int skip_dead, int order, int order_run /* logical_block's mode and c */,
    Reg... reg_args)
{
    constexpr bool REG = sizeof...(Reg) != 0;
    typedef typename VecOf<T>::type vec_t;
    constexpr int N = VecOf<T>::N;
    const int lane = threadIdx.x & (kWave - 1);
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int waves_per_block = blockDim.x >> 6;
    const long nrows = (long)B * Tmax * U1max;
    const long stride = (long)gridDim.x * waves_per_block;
    const int cells = Tmax * U1max;
    const long first = (long)logical_block(blockIdx.x, gridDim.x, order, (unsigned)order_run);
    for (long r = first * waves_per_block + wid; r < nrows; r += stride) {
        const int b = (int)(r / cells);
        const int c = (int)(r - (long)b * cells);
        const int t = c / U1max;
        const int u = c - t * U1max;
        const int T_ = llens[b], U = tlens[b];
        const T *row = logits + (size_t)r * V;
        T *grow = grads + (size_t)r * V;

        const RowSplit<T> sp(row, V);
        const int h = sp.h, nv = sp.nv, tail = sp.tail;
        const vec_t *body = reinterpret_cast<const vec_t *>(row + h);
        vec_t *gbody = reinterpret_cast<vec_t *>(grow + h);

        // Lattice state is fp64; the combinations below are small in magnitude
        // (log-occupancies), so they are formed in fp64 and only then rounded.
        // Special entries (SURVEY.md App. A.1 case chain; first match wins): the blank term at the final cell and
        // wherever t < T-1 (with beta(t+1,u): b1), the label term (with beta(t,u+1): b2) unless it is the blank.
        const size_t dbase = (size_t)b * S * U1max;
        const int s = t + u;
        const bool valid = t < T_ && u <= U;
        const bool final_cell = t == T_ - 1 && u == U;
        const bool has_b1 = t < T_ - 1;
        const bool blank_special = final_cell || has_b1;
        double al = 0.0, be = 0.0, cost = 0.0, b1 = 0.0, b2 = 0.0;
        double be_eff = 0.0, lpen = 0.0;                 // REG: see above
        float go = 1.f, d = 0.f;
        int lab = -1;
        bool has_lab = false;
        if (valid) {
            al = alpha_skew[dbase + (size_t)s * U1max + u];
            be = beta_skew[dbase + (size_t)s * U1max + u];
            cost = cost_ws[b];
            if (grad_costs) go = grad_costs[b];
            d = denom[r];
            if (has_b1) b1 = beta_skew[dbase + (size_t)(s + 1) * U1max + u];
            if (u < U) {
                lab = targets[(size_t)b * (U1max - 1) + u];
                if (lab == blank && blank_special) lab = -1;
                else has_lab = true;
            }
            if (has_lab) b2 = beta_skew[dbase + (size_t)(s + 1) * U1max + (u + 1)];
            if constexpr (REG) {
                const RnntRegArgs &ra = only_arg(reg_args...);
                be_eff = be;
                if (has_lab) {
                    lpen = delay_pen(ra.reg.delay_penalty, T_ > Tmax ? Tmax : T_, t) + ra.reg.log1p_lambda;
                    if (ra.reg.log_lambda > (double)kNegInf)
                        be_eff = log_add_d(be, ra.reg.log_lambda + (double)ra.lp_skew[dbase + (size_t)s * U1max + u].y + b2);
                }
            }
        }
        const double bm = REG ? be_eff : be;             // beta of the main term
        auto lab_of = [&](double x) -> double {          // exponent of the label term from the one without regularisers
            if constexpr (REG) return x + lpen;
            else return x;
        };
        const double ac = al + cost;
        auto finish = [&](float val) -> float {
            if (clamp > 0.f) val = fminf(fmaxf(val, -clamp), clamp);
            return val * go;
        };

        // A padded cell's gradient is exactly zero.  A valid cell whose main bound is below kDeadThr (a NaN anywhere
        // makes the cell live) has a main term of +0 in every element, so the row is finish(0) except where a blank /
        // label term with a bound of its own at or above the threshold is subtracted: none in a dead row, one or two
        // in a faint row.  Those logits are the only ones read, before anything is stored (grads may alias logits),
        // and their elements are computed by the expressions of c2 / blank_sub / lab_sub / fix() below.
        // A label outside [0, V) matches no element on either path.
        const bool main_dead = skip_dead != 0 && fabsf(d) < kDeadDenomMax && ac + bm < kDeadThr;
        if (__builtin_amdgcn_readfirstlane((!valid || main_dead) ? 1 : 0)) {
            const T val = valid ? (T)finish(0.f) : (T)0.f;
            const bool blank_dead = !blank_special || (has_b1 ? ac + b1 : ac) < kDeadThr;
            const bool label_dead = !has_lab || lab_of(ac + b2) < kDeadThr || lab >= V;
            const int sblk = (valid && !blank_dead) ? blank : -1;
            const int slab = (valid && !label_dead) ? lab : -1;
            // The main term is evaluated for these elements as the streamed row evaluates it (it is +0): written as a
            // literal 0 the compiler folds 0 - e into -e under the clamp, and -0 is not what the streamed row gives.
            const double cmd = ac - (double)d;
            const float c2 = (float)(cmd + bm) * kLog2e;
            T vblk = val, vlab = val;
            if (sblk >= 0) {
                const float x = (float)row[sblk];
                const float sub = final_cell ? (float)cmd : (float)(cmd + b1);
                float g = fast_exp2(fmaf(x, kLog2e, c2));
                g -= fast_exp2((x + sub) * kLog2e);
                vblk = (T)finish(g);
            }
            if (slab >= 0) {
                const float x = (float)row[slab];
                const float sub = (float)lab_of(cmd + b2);
                float g = fast_exp2(fmaf(x, kLog2e, c2));
                g -= fast_exp2((x + sub) * kLog2e);
                vlab = (T)finish(g);
            }
            vec_t z;
#pragma unroll
            for (int q = 0; q < N; ++q) z[q] = val;
            if (lane < h) grow[lane] = faint_pick(lane, sblk, vblk, slab, vlab, val);
            if (lane < tail) grow[h + N * nv + lane] = faint_pick(h + N * nv + lane, sblk, vblk, slab, vlab, val);
            const int iblk = (sblk >= h) ? ((sblk - h) / N) : -1;
            const int ilab = (slab >= h) ? ((slab - h) / N) : -1;
            // the one or two body vectors that hold a read element, made up front: the store loop only selects
            vec_t oblk = z, olab = z;
#pragma unroll
            for (int q = 0; q < N; ++q) {
                oblk[q] = faint_pick(h + N * iblk + q, sblk, vblk, slab, vlab, val);
                olab[q] = faint_pick(h + N * ilab + q, sblk, vblk, slab, vlab, val);
            }
            for (int i = lane; i < nv; i += kWave) {
                vec_t o = z;
#pragma unroll
                for (int q = 0; q < N; ++q) o[q] = i == iblk ? oblk[q] : (i == ilab ? olab[q] : z[q]);
                stv<NTS>(o, gbody + i);
            }
            continue;
        }

        const double cmd = ac - (double)d;          // g = logit + cm
        const float c2 = (float)(cmd + bm) * kLog2e;
        // exponents (natural log) of the subtracted terms, minus the logit
        const float blank_sub = final_cell ? (float)cmd : (has_b1 ? (float)(cmd + b1) : 0.f);
        const float lab_sub = has_lab ? (float)lab_of(cmd + b2) : 0.f;
        const int blk = blank_special ? blank : -1;

        auto fix = [&](float val, float x, int v) -> float {
            // val = exp(x + cm + be) already; subtract the case-chain term.
            if (v == blk) val -= fast_exp2((x + blank_sub) * kLog2e);
            else if (v == lab) val -= fast_exp2((x + lab_sub) * kLog2e);
            return val;
        };

        if (lane < h) {
            const float x = (float)row[lane];
            grow[lane] = (T)finish(fix(fast_exp2(fmaf(x, kLog2e, c2)), x, lane));
        }
        if (lane < tail) {
            const int v = h + N * nv + lane;
            const float x = (float)row[v];
            grow[v] = (T)finish(fix(fast_exp2(fmaf(x, kLog2e, c2)), x, v));
        }
        // body vector i covers elements v = h + N*i .. h + N*i + N-1
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
            for (int q = 0; q < N; ++q) o[q] = (T)finish(g[q]);
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

// ----------------------------------------------------- diagnostics export --
__global__ void rnnt_export_kernel(const double *__restrict__ alpha_skew, const double *__restrict__ beta_skew,
                                   const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens,
                                   int B, int Tmax, int U1max, int K, int S,
                                   float *__restrict__ alpha, float *__restrict__ beta)
{
    const long n = (long)B * Tmax * U1max;
    for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (long)gridDim.x * blockDim.x) {
        const int cells = Tmax * U1max;
        const int b = (int)(r / cells);
        const int c = (int)(r - (long)b * cells);
        const int t = c / U1max, u = c - t * U1max;
        float a = 0.f, be = 0.f;
        if (t < llens[b] && u <= tlens[b]) {
            const size_t k = ((size_t)b * S + t + u) * U1max + u;
            a = (float)alpha_skew[k];
            be = (float)beta_skew[k];
        }
        alpha[r] = a;
        beta[r] = be;
    }
}

int check_shape(int B, int Tmax, int U1max, int V, int blank)
{
    WR_REQUIRE(B > 0 && Tmax > 0 && U1max > 0 && V > 0, WR_EINVAL,
               "rnnt: B, Tmax, U1max, V must be positive (got %d,%d,%d,%d)", B, Tmax, U1max, V);
    WR_REQUIRE(blank >= 0 && blank < V, WR_EINVAL, "rnnt: blank %d out of range [0,%d)", blank, V);
    WR_REQUIRE(U1max <= kRnntMaxCols, WR_EUNSUPPORTED,
               "rnnt: U1max=%d exceeds the sweep kernel's limit of %d label columns", U1max, kRnntMaxCols);
    WR_REQUIRE((long)B * Tmax * U1max < (1L << 31), WR_EUNSUPPORTED, "rnnt: more than 2^31 lattice cells");
    return WR_OK;
}

constexpr size_t kLseBytesPerWave = 16 * 1024;     // one row of 5 000 fp32 logits
constexpr size_t kGradBytesPerWave = 104 * 1024;   // 5.2 such rows on average

}  // namespace

// Grid of a streaming pass: 4-wave workgroups, each wave visits rows r, r + G, r + 2G, ... (G = waves of the grid).
// Round 1 ran persistent grids (12 workgroups per CU, ~390 rows per wave at the BASELINE shape).  Measured in round 2
// (tools/tune_rnnt.py SWEEP=grid, sustained fwd + bwd sequence): many short-lived workgroups are faster -- the hardware
// dispatches them in index order as slots free up, so what is in flight at any moment is a tight window of adjacent rows
// (a few short-lived windows for k rows per wave) instead of 12 288 persistent waves that drift apart:
//     read-only row pass:         15.71 ms at 12 per CU -> 14.64 ms with one row per wave (monotonic in between);
//     read + write gradient pass: 34.49 ms at 16 per CU -> 33.65 (128) -> 33.35 (512) -> 33.18 (1 024) -> 32.96 ms at
//                                 1 400 per CU (3.4 rows per wave); one or two rows per wave lose again (2 048 per CU =
//                                 2.3 rows per wave: +2 %).
// Workgroup order (logical_block, wr_common.hpp; profiles/xcd_row_order.md has every row of what was measured, B = 32 at
// the BASELINE shape, sustained fwd + bwd, tools/tune_rnnt.py SWEEP=order / order2, two boxes, spread within a box
// under 0.05 ms).  Consecutive workgroups run on consecutive XCDs; with XCD runs of c blocks (mode 2) the rows one XCD
// streams are contiguous:
//     read-only row pass:         identity 14.98 / 15.01 ms -> runs of c = 302: 13.86 / 13.84, 604: 13.79, 1 208 and
//                                 longer: 13.76 ms; eight contiguous regions (the removed mode 1): 14.66 ms.
//     read + write gradient pass: identity 25.24 / 25.66 ms at 1 355 per CU (68 KB per wave) -> runs: 25.30 on the second
//                                 box; the run length (64 ... 1 208) moves it by less than the spread.  Runs gain
//                                 0.35 - 0.41 ms at every grid measured (512 ... 1 355 per CU), and with them fewer
//                                 rows in flight win: 24.78 (512) / 24.82 (768, 896) / 25.13 (1 024) / 25.39 ms (1 200)
//                                 on one box, 24.64 (1 024) against 25.30 (1 355) on the other.  104 KB per wave is
//                                 886 per CU.  Mode 1 reached 24.58 / 24.74 ms, but only with exactly one row per wave
//                                 (27.8 ms at 2 048 per CU, 33.4 ms at 4 096) and is not kept.
//     PMC bytes of the gradient pass: 60.86 GB read -> 60.11 (c = 302) / 60.04 (604); written 99.00 -> 99.04 GB.
// Defaults: mode 2 for both passes (keys 15 and 16), c = 8 * U1max (order_run below).
// `knob` > 0 forces that many workgroups per CU (the round-1 meaning of tuning keys 0 and 1); 0 = automatic: every wave
// gets about `bytes_per_wave` of logits.
int stream_grid(long nrows, int knob, size_t row_bytes, size_t bytes_per_wave)
{
    long blocks = (nrows + 3) / 4;
    if (knob > 0) {
        const long cap = 256L * knob;
        if (blocks > cap) blocks = cap;
    } else {
        const long all = blocks;                                  // one row per wave
        blocks = (long)(((double)nrows * (double)row_bytes) / (4.0 * (double)bytes_per_wave)) + 1;
        if (blocks > all) blocks = all;
        const long floor_blocks = 256L * 12 < (nrows + 3) / 4 ? 256L * 12 : (nrows + 3) / 4;   // never fewer than a persistent grid
        if (blocks < floor_blocks) blocks = floor_blocks;
    }
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

// logical_block's run length c for mode 2.  The 64-byte sector of alpha_skew / beta_skew that holds cell (t, u) also
// holds (t-1, u+1) ... (t-7, u+7), rows U1max apart, so a run has to cover several frames of 4-row workgroups before
// the gradient pass can share a sector inside one L2; that pass is flat from 2 to 8 frames' worth and the row pass
// still gains up to c = 8 * U1max (1 208 at the BASELINE shape: 32 frames, 97 MB of logits per run).  Key 17 > 0
// overrides it.
static int order_run(int U1max)
{
    const int forced = tune_get(kTuneOrderRun);
    const int c = forced > 0 ? forced : 8 * U1max;
    return c < (1 << 24) ? c : (1 << 24);
}

int rnnt_launch_sweep(const RnntWs &w, char *ws, const int32_t *llens, const int32_t *tlens, int B, int Tmax,
                      int U1max, float *costs, hipStream_t st)
{
    return launch("rnnt_sweep_kernel", rnnt_sweep_kernel<8>, dim3(B, 2), dim3(64 * w.K), 0, st,
                  reinterpret_cast<const float2 *>(ws + w.lp_off), llens, tlens, Tmax, U1max, w.S,
                  reinterpret_cast<double *>(ws + w.alpha_off), reinterpret_cast<double *>(ws + w.beta_off),
                  reinterpret_cast<double *>(ws + w.ll_off), reinterpret_cast<double *>(ws + w.cost_off), costs,
                  reinterpret_cast<double *>(ws + w.dump_off));
}

int rnnt_launch_lse(const RnntWs &w, char *ws, const void *logits_d, int dtype, const int32_t *targets_d,
                    const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V,
                    int blank, hipStream_t st)
{
    const long nrows = (long)B * Tmax * U1max;
    const size_t row_bytes = (size_t)V * (dtype == WR_F32 ? 4 : 2);
    const dim3 grid1(stream_grid(nrows, tune_get(kTuneLseBlocksPerCu), row_bytes, kLseBytesPerWave));
    const bool nt = (tune_get(kTuneNonTemporal) & 4) != 0;
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_bool(nt, [&](auto nt_c) {
            return with_int<16, 8, 4>(unroll_of(kTuneLseUnroll), [&](auto un) {
                return launch("rnnt_lse_kernel", rnnt_lse_kernel<T, nt_c.value, un.value>, grid1,
                              dim3(256), 0, st, static_cast<const T *>(logits_d), targets_d, logit_lengths_d,
                              target_lengths_d, B, Tmax, U1max, V, blank, w.K, w.S,
                              reinterpret_cast<float2 *>(ws + w.lp_off), reinterpret_cast<float *>(ws + w.denom_off),
                              nullptr, tune_get(kTuneLseOrder), order_run(U1max));
            });
        });
    });
}

}  // namespace wr

using namespace wr;

extern "C" size_t wr_rnnt_workspace_bytes(int B, int Tmax, int U1max)
{
    if (B <= 0 || Tmax <= 0 || U1max <= 0) return 0;
    return rnnt_ws_layout(B, Tmax, U1max).total;
}

namespace wr {

int rnnt_loss_fwd_body(const char *what, const void *logits_d, int dtype, const int32_t *targets_d,
                       const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V,
                       int blank, double delay_penalty, float *costs_d, void *workspace_d, size_t workspace_bytes,
                       void *stream)
{
    if (int rc = check_shape(B, Tmax, U1max, V, blank)) return rc;
    WR_REQUIRE(logits_d && logit_lengths_d && target_lengths_d && costs_d && workspace_d, WR_EINVAL,
               "%s: null pointer argument", what);
    WR_REQUIRE(targets_d || U1max == 1, WR_EINVAL, "%s: targets is null", what);
    WR_REQUIRE(dtype == WR_F32 || dtype == WR_F16 || dtype == WR_BF16, WR_EINVAL, "%s: unknown dtype %d", what, dtype);
    const RnntWs w = rnnt_ws_layout(B, Tmax, U1max);
    WR_REQUIRE(workspace_bytes >= w.total, WR_EWORKSPACE, "%s: workspace %zu < required %zu", what, workspace_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace_d);
    WR_TRY(rnnt_launch_lse(w, ws, logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V, blank,
                           st));
    if (delay_penalty > 0.0)
        return wr_rnnt_lattice_sweeps(logit_lengths_d, target_lengths_d, B, Tmax, U1max, WR_LATTICE_REGULAR, delay_penalty,
                                      costs_d, workspace_d, workspace_bytes, stream);
    return rnnt_launch_sweep(w, ws, logit_lengths_d, target_lengths_d, B, Tmax, U1max, costs_d, st);
}

int rnnt_loss_fwd_from_lse_body(const char *what, const float *logits_d, const int32_t *targets_d,
                                const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                                int V, int blank, double delay_penalty, float *costs_d, void *workspace_d,
                                size_t workspace_bytes, void *stream)
{
    if (int rc = check_shape(B, Tmax, U1max, V, blank)) return rc;
    WR_REQUIRE(logits_d && logit_lengths_d && target_lengths_d && costs_d && workspace_d, WR_EINVAL,
               "%s: null pointer argument", what);
    WR_REQUIRE(targets_d || U1max == 1, WR_EINVAL, "%s: targets is null", what);
    const RnntWs w = rnnt_ws_layout(B, Tmax, U1max);
    WR_REQUIRE(workspace_bytes >= w.total, WR_EWORKSPACE, "%s: workspace %zu < required %zu", what, workspace_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace_d);
    // repair pass: the stand-alone row statistics, executed only if the joiner's epilogue raised the flag (a partial
    // sum overflowed: more than 88 nats of spread inside one row); otherwise every workgroup leaves at once
    const long nrows = (long)B * Tmax * U1max;
    WR_TRY(launch("rnnt_lse_kernel (repair)", rnnt_lse_kernel<float, false, 8>,
                  dim3(stream_grid(nrows, tune_get(kTuneLseBlocksPerCu), (size_t)V * 4, kLseBytesPerWave)), dim3(256), 0, st,
                  logits_d, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V, blank, w.K, w.S,
                  reinterpret_cast<float2 *>(ws + w.lp_off), reinterpret_cast<float *>(ws + w.denom_off),
                  reinterpret_cast<const int32_t *>(ws + w.flag_off), tune_get(kTuneLseOrder), order_run(U1max)));
    if (delay_penalty > 0.0)
        return wr_rnnt_lattice_sweeps(logit_lengths_d, target_lengths_d, B, Tmax, U1max, WR_LATTICE_REGULAR, delay_penalty,
                                      costs_d, workspace_d, workspace_bytes, stream);
    return rnnt_launch_sweep(w, ws, logit_lengths_d, target_lengths_d, B, Tmax, U1max, costs_d, st);
}

}  // namespace wr

extern "C" int wr_rnnt_loss_fwd(const void *logits_d, int dtype, const int32_t *targets_d,
                                const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax,
                                int U1max, int V, int blank, float *costs_d, void *workspace_d,
                                size_t workspace_bytes, void *stream)
{
    return rnnt_loss_fwd_body("rnnt_loss_fwd", logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V,
                              blank, 0.0, costs_d, workspace_d, workspace_bytes, stream);
}

extern "C" int wr_rnnt_loss_fwd_from_lse(const float *logits_d, const int32_t *targets_d, const int32_t *logit_lengths_d,
                                         const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank,
                                         float *costs_d, void *workspace_d, size_t workspace_bytes, void *stream)
{
    return rnnt_loss_fwd_from_lse_body("rnnt_loss_fwd_from_lse", logits_d, targets_d, logit_lengths_d, target_lengths_d, B, Tmax,
                                       U1max, V, blank, 0.0, costs_d, workspace_d, workspace_bytes, stream);
}

extern "C" int wr_rnnt_loss_sweeps(const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax,
                                   int U1max, float *costs_d, void *workspace_d, size_t workspace_bytes, void *stream)
{
    if (int rc = check_shape(B, Tmax, U1max, 1, 0)) return rc;
    WR_REQUIRE(logit_lengths_d && target_lengths_d && costs_d && workspace_d, WR_EINVAL,
               "rnnt_loss_sweeps: null pointer argument");
    const RnntWs w = rnnt_ws_layout(B, Tmax, U1max);
    WR_REQUIRE(workspace_bytes >= w.total, WR_EWORKSPACE, "rnnt_loss_sweeps: workspace %zu < required %zu",
               workspace_bytes, w.total);
    return rnnt_launch_sweep(w, static_cast<char *>(workspace_d), logit_lengths_d, target_lengths_d, B, Tmax, U1max, costs_d,
                             static_cast<hipStream_t>(stream));
}

namespace wr {

// (defined at the end of the file: the regularised instantiations then follow every kernel the file had before them
// in the code object, and those keep their places)
int rnnt_launch_grad_reg(const RnntWs &w, const char *ws, const void *logits_d, int dtype, const int32_t *targets_d,
                         const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V,
                         int blank, float clamp, const float *grad_costs_d, void *grads_d, const RnntReg &reg, dim3 grid,
                         bool nt, bool nts, int skip, hipStream_t st);

int rnnt_loss_bwd_body(const char *what, const void *logits_d, int dtype, const int32_t *targets_d,
                       const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V,
                       int blank, float clamp, const float *grad_costs_d, void *grads_d, const void *workspace_d,
                       size_t workspace_bytes, const RnntReg *reg, void *stream)
{
    if (int rc = check_shape(B, Tmax, U1max, V, blank)) return rc;
    WR_REQUIRE(logits_d && logit_lengths_d && target_lengths_d && grads_d && workspace_d, WR_EINVAL,
               "%s: null pointer argument", what);
    WR_REQUIRE(targets_d || U1max == 1, WR_EINVAL, "%s: targets is null", what);
    WR_REQUIRE(dtype == WR_F32 || dtype == WR_F16 || dtype == WR_BF16, WR_EINVAL, "%s: unknown dtype %d", what, dtype);
    const RnntWs w = rnnt_ws_layout(B, Tmax, U1max);
    WR_REQUIRE(workspace_bytes >= w.total, WR_EWORKSPACE, "%s: workspace %zu < required %zu", what, workspace_bytes, w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const char *ws = static_cast<const char *>(workspace_d);
    const long nrows = (long)B * Tmax * U1max;
    const size_t row_bytes = (size_t)V * (dtype == WR_F32 ? 4 : 2);
    const dim3 grid3(stream_grid(nrows, tune_get(kTuneGradBlocksPerCu), row_bytes, kGradBytesPerWave));
    const bool nt = (tune_get(kTuneNonTemporal) & 1) != 0;
    const bool nts = (tune_get(kTuneNonTemporal) & 2) != 0;
    const int skip = tune_get(kTuneGradSkip) != 0 ? 1 : 0;
    if (reg != nullptr)
        return rnnt_launch_grad_reg(w, ws, logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V,
                                    blank, clamp, grad_costs_d, grads_d, *reg, grid3, nt, nts, skip, st);
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_bool(nt, [&](auto nt_c) {
            return with_int<16, 8, 4>(unroll_of(kTuneGradUnroll), [&](auto un) {
                return with_bool(nts, [&](auto nts_c) {
                    return launch("rnnt_grad_kernel", rnnt_grad_kernel<T, nt_c.value, nts_c.value, un.value>, grid3,
                                  dim3(256), 0, st, static_cast<const T *>(logits_d), targets_d, logit_lengths_d,
                                  target_lengths_d, B, Tmax, U1max, V, blank, clamp, w.K, w.S,
                                  reinterpret_cast<const double *>(ws + w.alpha_off),
                                  reinterpret_cast<const double *>(ws + w.beta_off),
                                  reinterpret_cast<const float *>(ws + w.denom_off),
                                  reinterpret_cast<const double *>(ws + w.cost_off), grad_costs_d,
                                  static_cast<T *>(grads_d), skip, tune_get(kTuneGradOrder), order_run(U1max));
                });
            });
        });
    });
}

}  // namespace wr

extern "C" int wr_rnnt_loss_bwd(const void *logits_d, int dtype, const int32_t *targets_d,
                                const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax,
                                int U1max, int V, int blank, float clamp, const float *grad_costs_d, void *grads_d,
                                const void *workspace_d, size_t workspace_bytes, void *stream)
{
    return rnnt_loss_bwd_body("rnnt_loss_bwd", logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V,
                              blank, clamp, grad_costs_d, grads_d, workspace_d, workspace_bytes, nullptr, stream);
}

extern "C" int wr_rnnt_export_lattice(const void *workspace_d, size_t workspace_bytes,
                                      const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B,
                                      int Tmax, int U1max, float *alpha_d, float *beta_d, void *stream)
{
    if (int rc = check_shape(B, Tmax, U1max, 1, 0)) return rc;
    WR_REQUIRE(workspace_d && alpha_d && beta_d && logit_lengths_d && target_lengths_d, WR_EINVAL,
               "rnnt_export_lattice: null pointer argument");
    const RnntWs w = rnnt_ws_layout(B, Tmax, U1max);
    WR_REQUIRE(workspace_bytes >= w.total, WR_EWORKSPACE, "rnnt_export_lattice: workspace too small");
    const char *ws = static_cast<const char *>(workspace_d);
    return launch("rnnt_export_kernel", rnnt_export_kernel, dim3(256), dim3(256), 0, static_cast<hipStream_t>(stream),
                  reinterpret_cast<const double *>(ws + w.alpha_off), reinterpret_cast<const double *>(ws + w.beta_off),
                  logit_lengths_d, target_lengths_d, B, Tmax, U1max, w.K, w.S, alpha_d, beta_d);
}

// the gradient pass with FastEmit and / or the delay penalty: rnnt_loss_bwd_body's launch, regularised instantiation
int wr::rnnt_launch_grad_reg(const RnntWs &w, const char *ws, const void *logits_d, int dtype, const int32_t *targets_d,
                             const int32_t *logit_lengths_d, const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                             int V, int blank, float clamp, const float *grad_costs_d, void *grads_d, const RnntReg &reg,
                             dim3 grid, bool nt, bool nts, int skip, hipStream_t st)
{
    const RnntRegArgs ra{reinterpret_cast<const float2 *>(ws + w.lp_off), reg};
    return with_dtype(dtype, [&](auto t) {
        using T = decltype(t);
        return with_bool(nt, [&](auto nt_c) {
            return with_int<16, 8, 4>(unroll_of(kTuneGradUnroll), [&](auto un) {
                return with_bool(nts, [&](auto nts_c) {
                    return launch("rnnt_grad_kernel (regularised)",
                                  rnnt_grad_kernel<T, nt_c.value, nts_c.value, un.value, RnntRegArgs>, grid, dim3(256), 0, st,
                                  static_cast<const T *>(logits_d), targets_d, logit_lengths_d, target_lengths_d, B, Tmax,
                                  U1max, V, blank, clamp, w.K, w.S, reinterpret_cast<const double *>(ws + w.alpha_off),
                                  reinterpret_cast<const double *>(ws + w.beta_off),
                                  reinterpret_cast<const float *>(ws + w.denom_off),
                                  reinterpret_cast<const double *>(ws + w.cost_off), grad_costs_d, static_cast<T *>(grads_d),
                                  skip, tune_get(kTuneGradOrder), order_run(U1max), ra);
                });
            });
        });
    });
}
