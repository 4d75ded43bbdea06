// Lattice types of the k2 RNN-T losses (rnnt_lattice.hip; include/wr_api.h, "Lattice types and the delay penalty").
//
// Where the lattice arrays of an RNN-T workspace live, by lattice type (every region holds B * S * U1 8-byte elements,
// utterance b at element b * S * U1):
//   regular    arcs (float2) at lp_off, alpha at alpha_off, beta at beta_off, element (t + u) * U1 + u (anti-diagonals)
//   modified   arcs (float2) at alpha_off, alpha at lp_off, beta at beta_off, element t * U1 + u (plain rows; S >= T).
//              The statistics kernels always write the anti-diagonal array at lp_off; lattice_prepare_kernel copies it
//              into plain rows at alpha_off, and the forward sweep then writes alpha over the array it no longer needs.
#pragma once

#include "wr_common.hpp"

namespace wr {

// template modes of the kernels that read a lattice
constexpr int kLatRegular = 0;       // today's path: regular lattice, no penalty (bit-identical to what it was)
constexpr int kLatRegularPen = 1;    // regular lattice, delay penalty inside the stored label arcs
constexpr int kLatModified = 2;      // modified lattice (with or without penalty)

struct LatView {
    const float2 *lp;
    const double *alpha, *beta;
};

inline LatView lattice_view(const RnntWs &w, const char *ws, bool modified)
{
    LatView v;
    v.lp = reinterpret_cast<const float2 *>(ws + (modified ? w.alpha_off : w.lp_off));
    v.alpha = reinterpret_cast<const double *>(ws + (modified ? w.lp_off : w.alpha_off));
    v.beta = reinterpret_cast<const double *>(ws + w.beta_off);
    return v;
}

template <int LAT>
__device__ __forceinline__ size_t lat_idx(int t, int u, int U1)
{
    return LAT == kLatModified ? (size_t)t * U1 + u : (size_t)(t + u) * U1 + u;
}

// pen(b,t) = delay_penalty * ((T_b - 1) / 2 - t), in float64
__device__ __forceinline__ double delay_pen(double dp, int Tb, int t) { return dp * (0.5 * (double)(Tb - 1) - (double)t); }

// rnnt_lattice.hip: WR_OK, or the error of a lattice type / penalty the library does not have
int lattice_check(const char *what, int lattice_type, double delay_penalty);

}  // namespace wr
