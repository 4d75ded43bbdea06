// RNN-T forced alignment for MI355X (gfx950): the single best path through the transducer lattice of the RNN-T loss
// (torchaudio's lattice, log-softmax fused).  See include/wr_api.h.
//
//   A(0,0) = 0,  A(t,u) = max(A(t-1,u) + blank(t-1,u), A(t,u-1) + emit(t,u-1)),  score = A(T-1,U) + blank(T-1,U).
//
// Two device passes:
//   pass 1  rnnt_lse_kernel (rnnt_loss.hip, unchanged) -- or the joiner's statistics epilogue (wr_joint_rnnt_stats) --
//           writes the {blank, emit} log-probs of every cell into the diagonal-skewed `lp_skew` of the RNN-T workspace.
//   pass 2  rnnt_viterbi_kernel: the forward branch of rnnt_sweep_kernel with max in place of log-add-exp: the same
//           rnnt_forward_step of lattice_wavefront.hpp (one workgroup per utterance, one lane per label column u, one
//           step per anti-diagonal s = t + u; the scheme is described there) with another merge of the two candidates.
//           Each step's decision bits ("the emit predecessor won") form one 64-bit ballot word per (diagonal, wave),
//           stored by lane 0 of the wave into the workspace's beta region, which alignment never uses otherwise
//           (B*S*ceil(U1/64) words against B*S*U1 doubles).  Then the same workgroup walks back from (T-1, U) to (0, 0),
//           one diagonal per step: the whole workgroup stages blocks of decision words into LDS with coalesced loads,
//           one lane walks each block and records the frame of every emit step; the frames leave coalesced at the end.
//
// Tie rule (shared with tests/rnnt_align_ref.py): the emit predecessor wins only if its candidate is strictly greater;
// on equality or when a comparison involves a NaN the blank predecessor wins.  The value is NaN if either candidate is
// NaN, so a NaN anywhere on the reachable lattice reaches the score, while the decisions still form a monotone path.
#include "lattice_wavefront.hpp"
#include "wr_launch.hpp"

namespace wr {
namespace {

constexpr int kAlignStageWords = 4096;     // decision words staged in LDS per backtrace block (32 KB)

template <int PF>
__global__ __launch_bounds__(kRnntMaxCols) void rnnt_viterbi_kernel(
    const float2 *__restrict__ lp_skew, const int32_t *__restrict__ llens, const int32_t *__restrict__ tlens,
    int Tmax, int U1max, int S, uint64_t *decisions /* [B, S, nw] */, int32_t *__restrict__ label_frames,
    double *__restrict__ scores)
{
    constexpr double NEG = (double)kNegInf;
    __shared__ SweepSlots<double> xch;
    __shared__ uint64_t stage[kAlignStageWords];
    __shared__ int frames[kRnntMaxCols];
    const SweepLane L = sweep_lane(llens, tlens, Tmax, U1max);
    const int b = L.b, u = L.u, nw = L.nw, T = L.T, U = L.U;
    const int nsteps = (T > 0) ? T + U : 0;       // anti-diagonals that hold a valid cell
    int32_t *frames_out = label_frames + (size_t)b * (U1max - 1);

    if (nsteps == 0) {                             // no frame: no path (the host refuses T_b = 0)
        if (u == 0) scores[b] = NEG;
        for (int i = u; i < U1max - 1; i += blockDim.x) frames_out[i] = -1;
        return;
    }
    const float2 *__restrict__ lp = lp_skew + (size_t)b * S * U1max + L.col;
    uint64_t *dec = decisions + (size_t)b * S * nw;

    auto load_row = [&](int s) -> float2 {
        const int sc = s < 0 ? 0 : (s >= nsteps ? nsteps - 1 : s);
        return lp[(size_t)sc * U1max];
    };

    RnntFwd f;
    sweep_steps<PF, true>(0, nsteps, load_row, [&](int s, const float2 cur) {         // steps s >= nsteps have no active lane
        rnnt_forward_step(L, xch, s, cur, f, [&](bool active, int t, double top, double recv) {
            const bool emit = (t == 0) | (recv > top);   // strict: ties and NaN comparisons go to the blank predecessor
            double v = emit ? recv : top;
            v = (recv != recv) ? recv : v;                // a NaN candidate makes the value NaN (top's NaN is kept above)
            v = active ? v : NEG;
            const uint64_t word = __ballot(active & emit);
            if (L.lane == 0 && s < nsteps) dec[(size_t)s * nw + L.wave] = word;
            return v;
        });
    });
    sweep_store_ll(L, scores, f.result);

    // The decision words were written by lane 0 of every wave: drain them and drop this CU's cached lines before the
    // workgroup reads them back.
    __threadfence();
    __syncthreads();

    // Backtrace from (T-1, U) on diagonal T-1+U to the origin.  Thread 0 owns the cursor (bt, bu), bt + bu = s.
    const int D = kAlignStageWords / nw;          // diagonals per staged block (>= 256)
    int bt = T - 1, bu = U;
    for (int hi = T - 1 + U; hi > 0;) {
        const int lo = hi - D + 1 > 1 ? hi - D + 1 : 1;
        const int n = (hi - lo + 1) * nw;
        for (int i = u; i < n; i += blockDim.x) stage[i] = dec[(size_t)lo * nw + i];
        __syncthreads();
        if (u == 0) {
            for (int s = hi; s >= lo; --s) {
                const uint64_t wd = stage[(s - lo) * nw + (bu >> 6)];
                // on the top row only the emit predecessor exists; column 0 has no emit predecessor
                const bool e = bu > 0 && (bt == 0 || ((wd >> (bu & (kWave - 1))) & 1) != 0);
                if (e) { --bu; frames[bu] = bt; } else { --bt; }
            }
        }
        __syncthreads();
        hi = lo - 1;
    }
    for (int i = u; i < U1max - 1; i += blockDim.x) frames_out[i] = i < U ? frames[i] : -1;
}

int check_align(const char *what, int B, int Tmax, int U1max)
{
    WR_REQUIRE(B > 0 && Tmax > 0 && U1max > 0, WR_EINVAL, "%s: B, Tmax, U1max must be positive (got %d,%d,%d)", what, B,
               Tmax, U1max);
    WR_REQUIRE(U1max <= kRnntMaxCols, WR_EUNSUPPORTED,
               "%s: U1max=%d exceeds the Viterbi kernel's limit of %d label columns", what, U1max, kRnntMaxCols);
    WR_REQUIRE((long)B * Tmax * U1max < (1L << 31), WR_EUNSUPPORTED, "%s: more than 2^31 lattice cells", what);
    return WR_OK;
}

int launch_viterbi(const RnntWs &w, char *ws, const int32_t *llens, const int32_t *tlens, int B, int Tmax, int U1max,
                   int32_t *label_frames, double *scores, hipStream_t st)
{
    return launch("rnnt_viterbi_kernel", rnnt_viterbi_kernel<8>, dim3(B), dim3(64 * w.K), 0, st,
                  reinterpret_cast<const float2 *>(ws + w.lp_off), llens, tlens, Tmax, U1max, w.S,
                  reinterpret_cast<uint64_t *>(ws + w.beta_off), label_frames, scores);
}

}  // namespace
}  // namespace wr

using namespace wr;

extern "C" int wr_rnnt_align(const void *logits_d, int dtype, const int32_t *targets_d, const int32_t *logit_lengths_d,
                             const int32_t *target_lengths_d, int B, int Tmax, int U1max, int V, int blank,
                             int32_t *label_frames_d, double *scores_d, void *workspace_d, size_t workspace_bytes,
                             void *stream)
{
    if (int rc = check_align("rnnt_align", B, Tmax, U1max)) return rc;
    WR_REQUIRE(V > 0, WR_EINVAL, "rnnt_align: V must be positive (got %d)", V);
    WR_REQUIRE(blank >= 0 && blank < V, WR_EINVAL, "rnnt_align: blank %d out of range [0,%d)", blank, V);
    WR_REQUIRE(logits_d && logit_lengths_d && target_lengths_d && scores_d && workspace_d, WR_EINVAL,
               "rnnt_align: null pointer argument");
    WR_REQUIRE((targets_d && label_frames_d) || U1max == 1, WR_EINVAL, "rnnt_align: targets or label_frames is null");
    WR_REQUIRE(dtype == WR_F32 || dtype == WR_F16 || dtype == WR_BF16, WR_EINVAL, "rnnt_align: unknown dtype %d", dtype);
    const RnntWs w = rnnt_ws_layout(B, Tmax, U1max);
    WR_REQUIRE(workspace_bytes >= w.total, WR_EWORKSPACE, "rnnt_align: workspace %zu < required %zu", workspace_bytes,
               w.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace_d);
    if (int rc = rnnt_launch_lse(w, ws, logits_d, dtype, targets_d, logit_lengths_d, target_lengths_d, B, Tmax, U1max, V,
                                 blank, st))
        return rc;
    return launch_viterbi(w, ws, logit_lengths_d, target_lengths_d, B, Tmax, U1max, label_frames_d, scores_d, st);
}

extern "C" int wr_rnnt_align_from_stats(const int32_t *targets_d, const int32_t *logit_lengths_d,
                                        const int32_t *target_lengths_d, int B, int Tmax, int U1max,
                                        int32_t *label_frames_d, double *scores_d, void *rnnt_workspace_d,
                                        size_t rnnt_workspace_bytes, void *stream)
{
    if (int rc = check_align("rnnt_align_from_stats", B, Tmax, U1max)) return rc;
    WR_REQUIRE(logit_lengths_d && target_lengths_d && scores_d && rnnt_workspace_d, WR_EINVAL,
               "rnnt_align_from_stats: null pointer argument");
    WR_REQUIRE((targets_d && label_frames_d) || U1max == 1, WR_EINVAL,
               "rnnt_align_from_stats: targets or label_frames is null");
    const RnntWs w = rnnt_ws_layout(B, Tmax, U1max);
    WR_REQUIRE(rnnt_workspace_bytes >= w.total, WR_EWORKSPACE, "rnnt_align_from_stats: workspace %zu < required %zu",
               rnnt_workspace_bytes, w.total);
    return launch_viterbi(w, static_cast<char *>(rnnt_workspace_d), logit_lengths_d, target_lengths_d, B, Tmax, U1max,
                          label_frames_d, scores_d, static_cast<hipStream_t>(stream));
}
