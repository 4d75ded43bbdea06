// The wavefront skeleton under the five kernels that walk a transducer lattice one dependent step at a time:
// rnnt_sweep_kernel (rnnt_loss.hip), rnnt_viterbi_kernel (rnnt_align.hip), lattice_mod_sweep_kernel, tdt_sweep_kernel and
// tdt_viterbi_kernel (rnnt_lattice.hip).  Each kernel keeps its recurrence; what they share is here, once.
//
// One workgroup per (utterance, direction), one lane per label column u (NW = ceil(U1max/64) waves).  At every step a lane
// works on one cell of its column (the cell (t = s - u, u) of anti-diagonal s, or row t of the modified lattice).  What a
// cell needs from the step before is the lane's own previous value and its neighbouring lane's previous value: inside a
// wave that is one DPP wave rotate; across the wave boundary (lane 63 -> lane 0 of the next wave, or back) it goes through
// an 8-byte LDS slot, double buffered, with one s_barrier per step.  The loop body is straight-line: loads are
// unconditional (clamped rows, values masked afterwards) and idle lanes store to a sink, so PF rows of log-probs stay in
// flight under counted s_waitcnt.  State in fp64, the bounded log1p(exp(-|a-b|)) term in fp32.  Latency-bound: T + U
// dependent steps of ~0.26 us each (0.30 ms for rnnt_sweep_kernel at the BASELINE shape).
#pragma once
#include "wr_common.hpp"

namespace wr {

// Precision: alpha/beta reach magnitudes ~ (T+U)*log(V) (1e4 at the BASELINE shape), where an fp32 ulp is 1e-3.  The
// lattice state is therefore carried in fp64 (adds, max) while the transcendental part log1p(exp(-|a-b|)) in [0, ln 2]
// is evaluated in fp32: absolute error ~1e-7 per step instead of ~5e-4.  -inf safe.
__device__ __forceinline__ double log_add_exp_d(double a, double b)
{
    const double m = fmax(a, b);
    const float d = (float)(-fabs(a - b));          // NaN when both are -inf
    const float r = kLn2 * fast_log2(1.0f + fast_exp2(d * kLog2e));
    return (m == (double)kNegInf) ? (double)kNegInf : m + (double)r;
}

// The cross-wave slots: [step parity][wave].  A kernel declares one in LDS and hands it to the exchange below.
template <typename V>
using SweepSlots = V[2][kRnntMaxCols / kWave];

// Where a thread of a sweep workgroup stands: blockIdx.x is the utterance, threadIdx.x the label column.
struct SweepLane {
    int b, u;          // utterance, label column (may lie beyond the row: 64 * NW >= U1max)
    int lane, wave;    // u % 64, u / 64
    int nw;            // waves of the workgroup
    int T, U;          // the utterance's frames and labels, clamped into [0, Tmax] x [0, U1max - 1]
    int col;           // u clamped into the row: always a position of the arrays
    bool ucol;         // u is a column of this utterance's lattice (u <= U)
};

__device__ __forceinline__ SweepLane sweep_lane(const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens,
                                                int Tmax, int U1max)
{
    SweepLane L;
    L.b = blockIdx.x, L.u = threadIdx.x;
    L.lane = L.u & (kWave - 1), L.wave = L.u >> 6;
    L.nw = blockDim.x >> 6;
    L.T = clampi(llens[L.b], 0, Tmax), L.U = clampi(tlens[L.b], 0, U1max - 1);
    const bool in_row = L.u < U1max;
    L.col = in_row ? L.u : U1max - 1;
    L.ucol = in_row && L.u <= L.U;
    return L;
}

// alpha / beta column of this lane in a [B][S][U1max] array; its slot of `dump` ([2*B*kRnntMaxCols]) for idle steps' stores
__device__ __forceinline__ double *sweep_out(const SweepLane &L, bool backward, double *alpha, double *beta, int S, int U1max)
{
    return (backward ? beta : alpha) + (size_t)L.b * S * U1max + L.col;
}

__device__ __forceinline__ double *sweep_sink(const SweepLane &L, bool backward, double *dump)
{
    return dump + ((size_t)L.b * 2 + (backward ? 1 : 0)) * kRnntMaxCols + L.u;
}

// What this lane's neighbour sent on the previous step: lane u-1's value (FWD) or lane u+1's (!FWD).  The lane at the end
// of the whole row has no neighbour and sees `edge`.  `unwritten`: no step has posted yet, so a lane at a wave boundary
// sees -inf instead of the slot (a kernel whose boundary lanes are idle on its first step may leave it false).
template <bool FWD, typename V>
__device__ __forceinline__ V sweep_recv_slot(const SweepLane &L, const SweepSlots<V> &xch, V rotated, int step, V edge,
                                             bool unwritten, V none)
{
    if (FWD && L.lane == 0) rotated = (L.wave == 0) ? edge : (unwritten ? none : xch[(step + 1) & 1][L.wave - 1]);
    if (!FWD && L.lane == kWave - 1) rotated = (L.wave == L.nw - 1) ? edge : (unwritten ? none : xch[(step + 1) & 1][L.wave + 1]);
    return rotated;
}

template <bool FWD>
__device__ __forceinline__ double sweep_recv(const SweepLane &L, const SweepSlots<double> &xch, double send, int step,
                                             double edge, bool unwritten = false)
{
    return sweep_recv_slot<FWD, double>(L, xch, FWD ? lane_rotate_up_d(send) : lane_rotate_down_d(send), step, edge,
                                        unwritten, (double)kNegInf);
}

// The lane at the wave boundary leaves `send` for the next wave's step; sweep_post adds the step's one barrier.
template <bool FWD, typename V>
__device__ __forceinline__ void sweep_put(const SweepLane &L, SweepSlots<V> &xch, V send, int step)
{
    if (L.lane == (FWD ? kWave - 1 : 0)) xch[step & 1][L.wave] = send;
}

template <bool FWD>
__device__ __forceinline__ void sweep_post(const SweepLane &L, SweepSlots<double> &xch, double send, int step)
{
    sweep_put<FWD>(L, xch, send, step);
    if (L.nw > 1) __syncthreads();
}

// The step loop with PF rows in flight: `count` dependent steps from `first`, upwards (FWD) or downwards.  load(s) fetches
// what step s reads (it must accept any s: the ring runs PF steps ahead and the count is rounded up to PF; clamp there,
// mask in the step); step(s, row) is the recurrence.
template <int PF, bool FWD, typename Load, typename Step>
__device__ __forceinline__ void sweep_steps(int first, int count, const Load &load, const Step &step)
{
    decltype(load(0)) ring[PF];
#pragma unroll
    for (int i = 0; i < PF; ++i) ring[i] = load(FWD ? first + i : first - i);
    for (int base = 0; base < count; base += PF) {
#pragma unroll
        for (int i = 0; i < PF; ++i) {
            const int s = FWD ? first + (base + i) : first - (base + i);
            const auto cur = ring[i];
            ring[i] = load(FWD ? s + PF : s - PF);
            step(s, cur);
        }
    }
}

// ---- the forward step of the regular lattice: rnnt_sweep_kernel (log-add) and rnnt_viterbi_kernel (max) differ in `cell`
struct RnntFwd {
    double down = (double)kNegInf;    // A(t-1, u) + blank(t-1, u): the next cell's blank candidate; at (T-1, U) the result
    double send = (double)kNegInf;    // A(t, u) + emit(t, u): what the lane to the right needs on the next diagonal
    double result = 0.0;              // A(T-1, U) + blank(T-1, U), on the one lane that sees the terminal cell
};

// Lane u on anti-diagonal s at cell (t = s - u, u); `cur` = {blank, emit} of that cell.  cell(active, t, top, recv) merges
// the blank predecessor's candidate `top` with the emit predecessor's `recv` (the origin sees recv = 0, top = -inf), records
// what its kernel keeps of the cell and returns the cell's value, -inf on an idle lane.  (On diagonal 0 the lanes at a wave
// boundary are idle: what they read from the unwritten slots is masked.)
template <typename Cell>
__device__ __forceinline__ void rnnt_forward_step(const SweepLane &L, SweepSlots<double> &xch, int s, const float2 cur,
                                                  RnntFwd &f, const Cell &cell)
{
    constexpr double NEG = (double)kNegInf;
    const double recv = sweep_recv<true>(L, xch, f.send, s, (s == 0) ? 0.0 : NEG);
    const int t = s - L.u;
    const bool active = (t >= 0) & (t < L.T) & (L.u <= L.U);
    const float sk = active ? cur.x : 0.f;
    const float em = active ? cur.y : 0.f;
    const double top = (t >= 1) ? f.down : NEG;
    const double v = cell(active, t, top, recv);
    f.down = v + (double)sk;
    f.result = (active && t == L.T - 1 && L.u == L.U) ? f.down : f.result;
    f.send = v + (double)em;
    sweep_post<true>(L, xch, f.send, s);
}

// ---- tails.  An utterance without frames: cost 0, log-likelihood 0.
__device__ __forceinline__ void sweep_store_empty(const SweepLane &L, bool backward, double *ll_out, double *cost_ws,
                                                  float *costs_out)
{
    if (L.u != 0) return;
    if (backward) { cost_ws[L.b] = 0.0; costs_out[L.b] = 0.f; } else ll_out[L.b] = 0.0;
}

// Forward: exactly one lane (u = U) saw the terminal cell.
__device__ __forceinline__ void sweep_store_ll(const SweepLane &L, double *ll_out, double result)
{
    if (L.u == L.U) ll_out[L.b] = result;
}

// Backward: lane 0 holds beta(0, 0) = the log-likelihood; the cost is its negative.
__device__ __forceinline__ void sweep_store_cost(const SweepLane &L, double *cost_ws, float *costs_out, double result)
{
    if (L.u == 0) { cost_ws[L.b] = -result; costs_out[L.b] = (float)(-result); }
}

}  // namespace wr
