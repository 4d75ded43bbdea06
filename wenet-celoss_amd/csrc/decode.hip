// Transducer decoding on MI355X (gfx950): batched greedy search and batched
// prefix beam search with every per-step operation on the device.
//
// Replaces (semantics: SURVEY.md App. A.3 / A.4)
//   greedy   wenet/transducer/search/greedy_search copy.py:6-63  (the upstream core loop that
//            Transducer.greedy_search dispatches to, transducer.py:515-598)
//   beam     wenet/transducer/search/prefix_beam_search.py:42-148 (PrefixBeamSearch)
//   step API wenet/transducer/predictor.py:160-200 (RNNPredictor.forward_step, LSTM cell x L +
//            projection) and wenet/transducer/joint.py:45-70 for step shapes.
//
// The reference runs ONE utterance at a time from Python with a host<->device
// sync on every step (.item()).  Here `lanes` (independent streams for greedy;
// utterances x beam hypotheses for beam search) advance together with all control
// state in device memory.  Every activation that feeds a contraction is kept
// K-MAJOR ([feature][lane], lanes padded to 32) so that the exact-fp32 MFMA
// (v_mfma_f32_32x32x2_f32) fragments of both operands are plain coalesced 128-byte
// reads from L2 -- no LDS staging, no transposes between stages:
//
//   lane_gemm_kernel        C^T = A^T-segments x k-major weights (+bias), 32 output columns per
//                           workgroup, K split over the 4 waves, register ping-pong on the L2
//                           fragment loads, LDS only for the final 4-way reduction.  Five launches
//                           per micro-step, the elementwise stages fused as epilogues:
//                             LSTM layer l   gates = x W_ih^T + h W_hh^T -> cell update (c, h),
//                                            predicated per lane ("predictor steps only after a
//                                            non-blank"); gate columns permuted so one tile holds
//                                            i,f,g,o of 8 hidden units
//                             projection     k-major store
//                             pred_ffn       -> joiner activation tanh(enc_ffn(enc)[utt,t] + .)
//                             ffn_out        row-major logits
//                           (the embedding of a lane's next token is written by the kernel that
//                           decides the token)
//   greedy_update_kernel    log-softmax + argmax (first index on ties) + the
//                           frame/emission state machine + cache commit
//   beam_topk_kernel /      log-softmax, CTC mixture, top-k from registers; per-utterance
//   beam_update_kernel      expansion, prefix fusion (float64 log_add), stable prune --
//                           one candidate per thread
//   tdt_beam_topk_kernel /  the same for a token-and-duration model: token and duration log-softmax, the best
//   tdt_beam_update_kernel  (token, duration) pairs of the hypotheses at the utterance's earliest frame; the
//                           others wait; equal tokens at an equal frame fuse
//                           What a twin does as the plain kernel does exists once: topk_row_max / _log_sum / _mix_select,
//                           topk_merge, the beam_* phases over one BeamUpdLds, ResolveLane (both look-ahead resolve kernels)
//   beam_chunk_begin_kernel /   the streaming form of both beam searches (wr_prefix_beam_search_chunk): the update kernels'
//   beam_stream_export_kernel   <TIMES> instantiations carry a Viterbi score and the frame of every token, the begin kernel
//                           continues each stream from the state its previous chunk left (and clamps, fuses and re-sorts
//                           for a final call), the export kernel writes the n-best with times after every chunk
//
// Micro-steps are replayed from a hipGraph (captured once per decoder handle) so
// the host only checks a "lanes still active" word every 16 steps.
#include "decode_stream.hpp"
#include "decode_tdt.hpp"
#include "wr_common.hpp"
#include "wr_launch.hpp"

#include <math.h>
#include <string.h>

#include <new>
#include <vector>

namespace wr {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---- diagnostic build only (-DWR_STAMPS, tools/decode_stamps.py): per-wave s_memtime / s_memrealtime stamps of the
// micro-step kernels into a device array, to attribute a kernel's microseconds to load latency / MFMA / reduction /
// epilogue and to measure start skew and inter-kernel gaps.  In the product library none of this exists.
#ifdef WR_STAMPS
constexpr int kStampSlots = 12, kStampWgs = 1024, kStampWaves = 8, kStampPts = 10;
__device__ unsigned long long g_stamps[kStampSlots * kStampWgs * kStampWaves * kStampPts];
#define WR_STAMP_DECL unsigned long long st_[::wr::kStampPts] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define WR_STAMP(i) do { __builtin_amdgcn_sched_barrier(0); st_[i] = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define WR_STAMP_RT(i) do { __builtin_amdgcn_sched_barrier(0); st_[i] = __builtin_amdgcn_s_memrealtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define WR_STAMP_DRAIN() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
#define WR_STAMP_FLUSH(slot)                                                                                              \
    do {                                                                                                                  \
        const int wg_ = blockIdx.y * gridDim.x + blockIdx.x, wv_ = threadIdx.x >> 6;                                      \
        if ((threadIdx.x & 63) == 0 && (slot) >= 0 && (slot) < ::wr::kStampSlots && wg_ < ::wr::kStampWgs && wv_ < ::wr::kStampWaves) \
            for (int i_ = 0; i_ < ::wr::kStampPts; ++i_)                                                                  \
                ::wr::g_stamps[((size_t)((slot) * ::wr::kStampWgs + wg_) * ::wr::kStampWaves + wv_) * ::wr::kStampPts + i_] = st_[i_]; \
    } while (0)
#else
#define WR_STAMP_DECL
#define WR_STAMP(i)
#define WR_STAMP_RT(i)
#define WR_STAMP_DRAIN()
#define WR_STAMP_FLUSH(slot)
#endif

constexpr int kMaxLayers = WR_MAX_LSTM_LAYERS;
enum PredictorType { kPredLstm = 0, kPredEmbedding = 1, kPredConv = 2 };
constexpr int kMaxLanes = 1024;      // streams (greedy) or utterances x beam decoded together
constexpr int kMaxBeam = 16;
constexpr int kMaxLook = 4;          // greedy look-ahead: encoder frames evaluated per micro-step against one predictor state
#ifndef WR_STEPS_PER_GRAPH
#define WR_STEPS_PER_GRAPH 16
#endif
constexpr int kStepsPerGraph = WR_STEPS_PER_GRAPH;
constexpr int kStageSlots = 4;

struct Dims {
    int V, E, P, D, H, L, J;      // vocab, encoder dim, predictor out dim, embed dim, hidden, layers, join dim
    int Ve;                       // rows of the embedding table (= V unless the caller says otherwise)
    int Dp, Hp, Pp, Jp;           // K dimensions padded to a multiple of 8 (zero rows)
    int G4p, Vp;                  // N dimensions: 4H padded to 32, V padded to 256
    int NL, NLp;                  // lanes, lanes padded to 32
    int act;                      // joiner activation (wr_activation)
    int ptype, ctx, heads, pact;  // predictor: 0 LSTM / 1 embedding / 2 conv; context size, heads, activation (types 1, 2)
    float ln_eps;
};

// Device-resident decoder state; all pointers are carved from the caller's workspace.
// "T" suffix = k-major ([feature][NLp]).
struct DevState {
    Dims d;
    // k-major (transposed, zero padded) weights
    const float *embed;
    float *wt_ih[kMaxLayers], *wt_hh[kMaxLayers], *bsum[kMaxLayers];
    float *proj_wt, *predffn_wt, *encffn_wt, *out_wt;
    const float *proj_b, *predffn_b, *encffn_b, *out_b;
    // stateless predictors (predictor.py:203-481): the LSTM slots above stay empty; the "LSTM state" cache_hT[l] holds
    // the embedding of history slot l (l = 0 oldest), L = ctx - 1, H = D
    const float *pos_w, *pffn_b, *pnorm_w, *pnorm_b, *conv_w, *conv_b;
    float *pffn_wt;               // [Dp][up(D,32)] k-major ffn weight (type 1)
    // LSTM predictor: projection followed by pred_ffn is ONE linear map (nothing non-linear sits between predictor.py:198
    // and joint.py:57): pred_ffn(projection(h)) = (Wf Wp) h + (Wf bp + bf), composed once per handle
    float *projffn_wt, *projffn_b;   // [Hp][up(J,32)], [up(J,32)]
    float *combT, *ffnT;          // [Dp][NLp] head-weighted context sum / ffn output (type 1)
    // per-call inputs
    const float *enc;             // [n_utt, T, E]
    const int32_t *enc_lens;      // [n_utt]
    const float *ctc_logp;        // [n_utt, T, V] (beam only)
    int n_utt, T, lanes_per_utt, n_lanes;
    // lane state
    float *ep_all;                // [n_utt, T, J]
    int32_t *token, *lane_t, *noblk, *need_pred, *lane_active;
    int32_t *new_is_cache;        // streaming quirk: the pending predictor state equals the committed one
    float *xT;                    // [Dp][NLp]     embedding of each lane's token
    float *cache_hT, *cache_cT;   // [L][Hp][NLp]  committed LSTM state
    float *new_hT, *new_cT;       // [L][Hp][NLp]  output of the last predictor step
    // LSTM predictor in its hoisted form (see "LSTM predictor step" below): state lives in a pool of 2 * NLp slots
    float *etab;                  // [V][G4p]          W_ih(layer 0) . embed[v], gate columns permuted like the weights
    float *pool_c;                // [L][2 NLp][Hp]    cell state of a slot
    float *pool_g;                // [L][2 NLp][G4p]   W_hh . h + b_ih + b_hh of the slot's hidden state
    int32_t *comm_slot, *new_slot;   // [NLp] slot of a lane's committed state / slot its next predictor step writes
    float *outT;                  // [Pp][NLp]     projected predictor output
    float *ht;                    // [Jp][kMaxLook * NLp]  joiner activation, column f * NLp + n
    float *logits;                // [kMaxLook * NLp, V]   row f * NLp + n: lane n, frame t_n + f
    int32_t *row_tok;             // [kMaxLook * NLp]      argmax of each logits row (look-ahead greedy)
    float4 *row_part;             // [NLp][Vp / 32]        per-block row statistics written by the ffn_out epilogue
    int n_cb;                     // Vp / 32
    int32_t *active_count;        // lanes still decoding
    // greedy outputs / params
    int32_t *hyps;                // [NL, max_hyp]
    int32_t *hyp_lens;
    int max_hyp, n_steps, blank;
    // beam state
    int beam;
    float ctc_weight, tr_weight;
    float *topv;                  // [NL, beam]
    int32_t *topi;
    int32_t *bhyps;               // [2, n_utt, beam, Lmax]
    int32_t *bhyp_lens;           // [2, n_utt, beam]
    double *bscores;              // [n_utt, beam]
    unsigned long long *bhash;    // [n_utt, beam]   running hash of each hypothesis' tokens
    int32_t *n_hyps;              // [n_utt]
    int32_t *frame;               // [n_utt]
    int32_t *hyp_sel;             // [n_utt]
    int Lmax;
    // hot-word greedy (wr_greedy_search_hotword): the state machine of greedy_search.py:297-430 on the device
    int hw_on, hw_filter;         // mode flag; context_filter_state == 'on'
    int hw_nctx[2];               // entries of the empty list (0) and of the hot-word list (1)
    const int32_t *gate_tab;      // [n_utt, T]   top-1 of the hot-word gate per frame (hw_gate_table_kernel)
    int32_t *cur_gate;            // [NLp] result[-1]: 1 = hot-word biasing, 0 = empty-list biasing
    int32_t *gb_flag, *gb_end, *last_t;   // [NLp] go_back_flag, go_back_end, last_t
    int32_t *trace, *trace_len;   // [NL, trace_cap] / [NL]: `result`, the gate trace
    int trace_cap;
    float *biasT;                 // [Pp][NLp] biased predictor output (input of pred_ffn in hot-word mode)
    // token-and-duration greedy (wr_greedy_search_tdt).  The durations travel here, in the state block every call uploads,
    // and never as a kernel argument: those are baked into the captured graphs
    unsigned long long tdt_durs;  // durations[j] in bits [4j, 4j + 4)
    int tdt_D;                    // the logits row is V - tdt_D token columns followed by tdt_D duration columns
    int32_t *hyp_frames;          // [NL, max_hyp] frame of each emission, or null
    // streaming prefix beam search (wr_prefix_beam_search_chunk): the block wr_decoder_attach_beam_stream was given, which
    // also holds bhyps / bhyp_lens / bscores while a chunk call runs; null in every other search.  lane_t and frame[] count
    // from the first frame of the stream's latest chunk, bs_base[b] is that frame's absolute number
    int32_t *btimes;              // [2, n_utt, beam, Lmax]  frame of each token of a hypothesis (slot 0, the seed: -1)
    double *bvscores;             // [n_utt, beam]           Viterbi score
    int32_t *bs_base, *bs_F;      // [n_utt] absolute frame of the latest chunk's first frame / frames received (F_b)
    int32_t *bs_state;            // [n_utt] bit 1: the stream has had its final call
    const int32_t *bs_flags;      // [n_utt] this call: bit 0 reset the stream first, bit 1 final
    // context-graph biasing in that search (wr_prefix_beam_search_context_chunk; bs_flags bit 2: export the stream finalised);
    // null / 0 in every other search.  The table is the caller's, S states and A arcs
    double *bctx_score;           // [n_utt, beam]           bonus of the entry
    int32_t *bctx_state;          // [n_utt, beam]           graph state of the entry
    int32_t *btags;               // [2, n_utt, beam, Lmax]  tag of each token of a hypothesis (slot 0, the seed: -1)
    ContextGraph cg;
};

struct GemmArgs {
    const float *A0, *B0;         // segment 0: A^T [K0][lda], B [K0][ldb]   (K multiples of 8)
    const float *A1, *B1;         // optional segment 1
    int K0, K1, lda, ldb;
    const float *bias;            // [N] or null
    float *C;
    int ldc, N, n_lanes;
    // epilogues that need lane state (LSTM cell, joiner activation): workspace pointers by value, so that the
    // kernel reads them from its argument segment instead of chasing them through the device-side state
    const DevState *st;           // per-call scalars (T, lanes_per_utt)
    const int32_t *lane_active, *need_pred, *lane_t;
    float *new_hT;                // this layer's new hidden state [Hp][NLp] (lane-indexed: the next GEMM's A operand)
    const float *ep_all;          // [n_utt, T, J]
    int H, J;
    int act;                      // joiner activation (wr_activation)
    int look, lane_stride;        // joiner activation: frames per lane and the column stride between frames (NLp)
    float4 *row_part;             // kEpiRowStats: per (row, 32-column block) {max, sum exp(x - max), runner-up, first index of max}
    int row_part_ld;              // blocks per row
    const int32_t *ep_gate;       // hot-word mode: per-lane selector of the encoder stream (ep_all + gate * ep_gate_stride)
    size_t ep_gate_stride;
    // LSTM layers >= 1 (kEpiLstmCell) and the recurrent products (kEpiSlotRow): state pool of this layer, row-major per slot
    float *pool_g;                // [2 NLp][G4p]  W_hh . h + b of the slot's hidden state
    float *pool_c;                // [2 NLp][Hp]   cell state
    const int32_t *comm_slot, *new_slot;   // [NLp]
    const int32_t *slot_idx;      // kEpiSlotRow: the slot each lane's row goes to
    int Hp, G4p;
#ifdef WR_STAMPS
    int dbg_slot;
#endif
};

// Handle-constant pointers of the per-lane state, passed to the deciding kernels BY VALUE: the kernel-argument segment
// is in the scalar registers within 0.06 us of the wave's start, so the lane's flags, slots and row records are requested
// at once instead of behind the load of the state block (one memory round trip, ~0.5 us, off the critical path of every
// micro-step).  Everything that changes from call to call (buffers of the caller, T, n_steps ...) stays in DevState.
struct LaneArgs {
    int32_t *lane_active, *lane_t, *noblk, *need_pred, *new_is_cache, *comm_slot, *new_slot;
    const float4 *row_part;
    int n_cb, V;
};

enum GemmEpilogue { kEpiKMajor = 0, kEpiRowMajor = 1, kEpiLstmCell = 2, kEpiJointAct = 3, kEpiRowStats = 4, kEpiSlotRow = 5 };

// ----------------------------------------------------------------- setup --
// src [R][C] row-major -> dst [C][Rp] (zero padded columns R..Rp-1 and rows C..Cp-1)
__global__ void transpose_pad_kernel(const float *__restrict__ src, int R, int C, int Rp, int Cp, float *__restrict__ dst)
{
    __shared__ float tile[32][33];
    const int r0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < R && c < C) ? src[(size_t)r * C + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, r = r0 + tx;
        if (c < Cp && r < Rp) dst[(size_t)c * Rp + r] = tile[tx][i];
    }
}

__global__ void add_bias_kernel(const float *a, const float *b, int n, float *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = a[i] + b[i];
}

// ep_all[row, :] = enc[row, :] @ enc_ffn^T + b     (rows = n_utt * T)
__global__ __launch_bounds__(256) void ep_all_kernel(DevState *s, const float *__restrict__ enc, float *__restrict__ ep_out)
{
    extern __shared__ float xs[];              // [8][E]
    const Dims &d = s->d;
    const long rows = (long)s->n_utt * s->T;
    const long r0 = (long)blockIdx.x * 8;
    for (int i = threadIdx.x; i < 8 * d.E; i += blockDim.x) {
        const long r = r0 + i / d.E;
        xs[i] = (r < rows) ? enc[(size_t)r * d.E + i % d.E] : 0.f;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < d.J; j += blockDim.x) {
        float acc[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[r] = 0.f;
        for (int k = 0; k < d.E; ++k) {
            const float w = s->encffn_wt[(size_t)k * d.J + j];
#pragma unroll
            for (int r = 0; r < 8; ++r) acc[r] = fmaf(w, xs[r * d.E + k], acc[r]);
        }
        const float b = s->encffn_b[j];
#pragma unroll
        for (int r = 0; r < 8; ++r)
            if (r0 + r < rows) ep_out[(size_t)(r0 + r) * d.J + j] = acc[r] + b;
    }
}

// --------------------------------------------------------- predictor step --
__device__ __forceinline__ float sigmoidf_(float x) { return 1.f / (1.f + __expf(-x)); }

// LSTM weights: w [4H][K] (nn.LSTM layout, gate-major rows i,f,g,o) -> k-major [Kp][4*Hp] with the gate
// columns permuted so that every 32-column tile holds i,f,g,o of 8 consecutive hidden units
// (column c' -> unit (c'/32)*8 + c'%8, gate (c'%32)/8); padded rows/columns are zero.
__global__ void lstm_weight_prep_kernel(const float *__restrict__ w, int H, int Hp, int K, int Kp, float *__restrict__ dst)
{
    const int G4p = 4 * Hp;
    const long total = (long)Kp * G4p;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i / G4p), c = (int)(i % G4p);
        const int unit = (c >> 5) * 8 + (c & 7), gate = (c & 31) >> 3;
        dst[i] = (k < K && unit < H) ? w[(size_t)(gate * H + unit) * K + k] : 0.f;
    }
}
__global__ void lstm_bias_prep_kernel(const float *__restrict__ b_ih, const float *__restrict__ b_hh, int H, int Hp,
                                      float *__restrict__ dst)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= 4 * Hp) return;
    const int unit = (c >> 5) * 8 + (c & 7), gate = (c & 31) >> 3;
    dst[c] = unit < H ? b_ih[gate * H + unit] + b_hh[gate * H + unit] : 0.f;
}

// C = sum over segments of A^T B (+ bias).  grid = (column tiles of 32, lane tiles of 32*MT); 512 threads = 8
// waves, each takes an eighth of every segment's K.  Both operands come straight from L2 / Infinity Cache
// (k-major, coalesced 128-byte fragments) through a register ping-pong of CH k-steps; with the shipped sizes
// (K <= 512 per segment) the whole K slice of a wave is in flight before its first MFMA, so a launch pays one
// memory latency.  Loads are unconditional (clamped rows, masked by a 0/1 factor) so the waits stay counted.
// Epilogues: k-major store, row-major store (logits), LSTM cell (gate columns are permuted at create time so a
// 32-column tile holds i,f,g,o of 8 hidden units), joiner activation tanh(enc_ffn(enc)[t] + pred_ffn(pred)).
// VW ("virtual waves" per wave): with VW = 2 a workgroup has 4 waves (256 threads) and every wave works through two of
// the eight K slices one after the other, each into accumulators of its own -- the same eight partial tiles, summed in the
// same order, so the results are BIT-IDENTICAL to the 8-wave form, but four workgroups fit a CU instead of two (the
// 640-workgroup joiner GEMM of a 128-lane beam search then runs in one round instead of two).
constexpr int kGemmWaves = 8;
template <int MT, int EPI, int VW = 1>
__device__ __forceinline__ void lane_gemm_body(const GemmArgs &g, const int bx, float (&red)[kGemmWaves][MT][32 * 32])
{
    WR_STAMP_DECL;
    WR_STAMP_RT(7);
    WR_STAMP(0);
    const int n0 = bx * 32;
    const int lane0 = blockIdx.y * (32 * MT);                          // first decode lane of this workgroup
    const int tid = threadIdx.x, lane = tid & 63, wave_phys = tid >> 6;
    const int half = lane >> 5, l31 = lane & 31;
    constexpr int CH = (VW == 2 || MT >= 4) ? 8 : 16;                   // k-pairs per chunk (NBUF chunks in flight)
    constexpr int NT = 64 * kGemmWaves / VW;
#ifdef WR_STAMPS
    asm volatile("" ::"s"(g.K0), "s"(g.ldb));      // the kernel-argument segment has arrived
    WR_STAMP(9);
#endif
    const int kq0 = g.K0 / kGemmWaves, kq1 = (g.A1 != nullptr) ? g.K1 / kGemmWaves : 0;
    const int nch0 = (kq0 + 2 * CH - 1) / (2 * CH), nch1 = (kq1 + 2 * CH - 1) / (2 * CH);
    const int nch = nch0 + nch1;
    int wave = wave_phys * VW;                                          // the K slice being worked on
    f32x16 acc[MT];

    auto load_chunk = [&](int ci, float (&bv)[CH], float (&av)[MT][CH], int slice_ahead = 0) {
        const bool s1 = ci >= nch0;
        const int cj = s1 ? ci - nch0 : ci;
        const int kq = s1 ? kq1 : kq0;
        const float *__restrict__ As = s1 ? g.A1 : g.A0;
        const float *__restrict__ Bs = s1 ? g.B1 : g.B0;
        const int kb = (wave + slice_ahead) * kq;
        const float *__restrict__ A = As + (size_t)(kb + half) * g.lda + lane0 + l31;
        const float *__restrict__ Bm = Bs + (size_t)(kb + half) * g.ldb + n0 + l31;
#pragma unroll
        for (int i = 0; i < CH; ++i) {
            const int k = cj * 2 * CH + 2 * i;
            const int kc = k < kq ? k : kq - 2;                         // K >= 16: kq - 2 is a valid row pair
            bv[i] = Bm[(size_t)kc * g.ldb];                             // nothing consumes the value here: the load stays
#pragma unroll                                                          // in flight until its MFMA (round 2 multiplied by a
            for (int m = 0; m < MT; ++m) av[m][i] = A[(size_t)kc * g.lda + m * 32];   // 0/1 mask here and so WAITED here)
        }
    };
    // chunk `ci`: its k-pairs beyond the slice's end (only when the slice is not a multiple of the chunk) are masked
    // at use; the test is wave-uniform and false for the shipped sizes
    auto mfma_chunk = [&](int ci, const float (&bv)[CH], const float (&av)[MT][CH]) {
        const bool s1 = ci >= nch0;
        const int valid = (s1 ? kq1 : kq0) - (s1 ? ci - nch0 : ci) * 2 * CH;   // k rows of this chunk inside the slice
        if (valid >= 2 * CH) {
#pragma unroll
            for (int i = 0; i < CH; ++i)
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][i], bv[i], acc[m], 0, 0, 0);
        } else {
#pragma unroll
            for (int i = 0; i < CH; ++i) {
                const float b = 2 * i < valid ? bv[i] : 0.f;
#pragma unroll
                for (int m = 0; m < MT; ++m) acc[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[m][i], b, acc[m], 0, 0, 0);
            }
        }
    };
    // Loads in three groups.  (1) The few per-lane indices that later loads depend on (state slots, flags, the lane's
    // frame) go out FIRST, so that they come back with the operands; (2) the first two operand chunks; (3) behind them
    // the epilogue operands (bias, pool rows, enc_ffn rows), whose addresses need (1): by then (1) has long arrived, and
    // (3) is consumed only after the K loop.  (Round 2 issued (1) after (2) and paid a second memory round trip.)
    constexpr int kItems = MT * 1024 / NT;                                // outputs per thread of the 32 x 32*MT tile
    float bias_v[kItems > 4 ? kItems : 4];
    bool cell_on = false, cell_in = false;
    int cell_j = 0, cell_n = 0, cell_unit = 0, cell_sn = 0, cell_sc = 0, cell_la = 0, cell_np = 0;
    float cell_c = 0.f, cell_g[4];
    int slot_v[kItems];
    bool act_on[kItems], act_in[kItems];
    int act_la[kItems], act_tt[kItems], act_gate[kItems];
    float act_ep[kMaxLook][kItems];
    int act_T = 1, act_lpu = 1;
    if (EPI == kEpiLstmCell) {
        const int q = tid & 255;
        cell_j = q >> 5;
        cell_n = lane0 + ((tid >> 8) % MT) * 32 + l31;
        cell_unit = (n0 >> 5) * 8 + cell_j;
        cell_in = tid < MT * 256 && cell_n < g.n_lanes && cell_unit < g.H;
        const int nn = cell_in ? cell_n : 0;
        cell_la = g.lane_active[nn]; cell_np = g.need_pred[nn];
        cell_sc = g.comm_slot[nn];
        cell_sn = g.new_slot[nn];
    } else if (EPI == kEpiSlotRow) {
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int i = tid + it * NT;
            const int n = lane0 + (i >> 10) * 32 + ((i & 1023) >> 5);
            slot_v[it] = g.slot_idx[n < g.n_lanes ? n : 0];
        }
    } else if (EPI == kEpiJointAct) {
        act_T = g.st->T; act_lpu = g.st->lanes_per_utt;
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int i = tid + it * NT;
            const int v = n0 + ((i & 1023) >> 5), n = lane0 + (i >> 10) * 32 + (i & 31);
            act_in[it] = n < g.n_lanes && v < g.N;
            const int nn = act_in[it] ? n : 0;
            act_la[it] = g.lane_active[nn];
            act_tt[it] = g.lane_t[nn];
            act_gate[it] = g.ep_gate ? g.ep_gate[nn] : 0;
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    // The wave works through its VW slices one after the other as ONE sequence of chunks with NBUF chunk buffers in
    // flight (a ring: the MFMAs of chunk c are followed by the request for chunk c + NBUF, across slice boundaries too);
    // at the end of a slice the accumulators go to LDS and start again from zero.  What bounds these kernels is how
    // many loads a CU has in flight (~2 us of memory latency): two buffers for the 8- and 4-wave forms, four where a
    // wave is alone on its SIMD (VW >= 4).
    constexpr int NBUF = VW >= 4 ? 4 : 2;
    float bb[NBUF][CH], ba[NBUF][MT][CH];
    const int n_chunks = VW * nch;
    int ld_cc = 0, ld_slice = 0;                                        // next chunk to request: (slice, chunk in slice)
    auto request = [&](float (&bv)[CH], float (&av)[MT][CH]) {
        wave = wave_phys * VW + ld_slice;
        load_chunk(ld_cc, bv, av);
        const bool last = ld_slice == VW - 1 && ld_cc == nch - 1;       // past the end: the last chunk again (counted waits)
        if (!last) { if (++ld_cc == nch) { ld_cc = 0; ++ld_slice; } }
    };
#pragma unroll
    for (int j = 0; j < NBUF; ++j) request(bb[j], ba[j]);
    __builtin_amdgcn_sched_barrier(0);

    if (EPI == kEpiRowMajor || EPI == kEpiRowStats || EPI == kEpiSlotRow) {
        const int v = n0 + l31;                                          // the column of every item of this thread
        bias_v[0] = g.bias ? g.bias[v < g.N ? v : g.N - 1] : 0.f;
    } else if (EPI == kEpiKMajor || EPI == kEpiJointAct) {
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int v = n0 + (((tid + it * NT) & 1023) >> 5);
            bias_v[it] = g.bias ? g.bias[v < g.N ? v : g.N - 1] : 0.f;
        }
    }
    if (EPI == kEpiLstmCell) {
        // gates = (W_ih . h_below: this GEMM) + (W_hh . h + b: pool_g of the lane's committed slot); one (lane, unit) per thread
        const float *__restrict__ gp = g.pool_g + (size_t)cell_sc * g.G4p + n0 + cell_j;
#pragma unroll
        for (int gt = 0; gt < 4; ++gt) cell_g[gt] = gp[gt * 8];
        cell_c = g.pool_c[(size_t)cell_sc * g.Hp + (cell_in ? cell_unit : 0)];
        cell_on = cell_in && cell_la && cell_np;
    } else if (EPI == kEpiJointAct) {
#pragma unroll
        for (int it = 0; it < kItems; ++it) act_on[it] = act_in[it] && act_la[it];
#pragma unroll
        for (int f = 0; f < kMaxLook; ++f)
#pragma unroll
            for (int it = 0; it < kItems; ++it) {
                const int i = tid + it * NT;
                const int v = n0 + ((i & 1023) >> 5), n = lane0 + (i >> 10) * 32 + (i & 31);
                const int t = act_tt[it] + f < act_T ? act_tt[it] + f : act_T - 1;
                const size_t sel = (size_t)(act_on[it] ? act_gate[it] : 0) * g.ep_gate_stride;
                act_ep[f][it] = (act_on[it] && f < g.look) ? g.ep_all[sel + ((size_t)(n / act_lpu) * act_T + t) * g.J + v] : 0.f;
            }
    }
    __builtin_amdgcn_sched_barrier(0);
    WR_STAMP(1);                                   // every load of the launch issued
#if defined(WR_STAMPS) && WR_STAMPS >= 2
    WR_STAMP_DRAIN();                              // level 2: wait for them, so that point 2 is the pure load latency
    WR_STAMP(2);
#endif

#pragma unroll
    for (int m = 0; m < MT; ++m) acc[m] = (f32x16){0};
    int mm_cc = 0, mm_slice = 0;
    for (int c0 = 0; c0 < n_chunks; c0 += NBUF) {
#pragma unroll
        for (int j = 0; j < NBUF; ++j) {
            if (c0 + j < n_chunks) {
                mfma_chunk(mm_cc, bb[j], ba[j]);
                __builtin_amdgcn_sched_barrier(0);
#if defined(WR_STAMPS) && WR_STAMPS < 2
                if (c0 + j == 0) WR_STAMP(2);      // first chunk's operands arrived and its MFMAs issued
#endif
                if (mm_cc == nch - 1) {            // slice complete: its partial tile to LDS
                    const int wslice = wave_phys * VW + mm_slice;
#pragma unroll
                    for (int m = 0; m < MT; ++m) {
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = (r & 3) + 8 * (r >> 2) + 4 * half;       // C/D layout of the 32x32 MFMA
                            red[wslice][m][row * 32 + (l31 ^ row)] = acc[m][r];    // XOR swizzle: both epilogue orders are conflict-free
                        }
                        acc[m] = (f32x16){0};
                    }
                    mm_cc = 0; ++mm_slice;
                } else {
                    ++mm_cc;
                }
                if (c0 + j + NBUF < n_chunks) {
                    request(bb[j], ba[j]);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    }
    WR_STAMP(3);                                   // MFMAs retired (accumulators read), partial tiles on their way to LDS
    __syncthreads();
    WR_STAMP(4);
    auto total = [&](int m, int ln, int col) {
        const int rc = ln * 32 + (col ^ ln);
        return ((red[0][m][rc] + red[1][m][rc]) + (red[2][m][rc] + red[3][m][rc])) +
               ((red[4][m][rc] + red[5][m][rc]) + (red[6][m][rc] + red[7][m][rc]));
    };
    if (EPI == kEpiRowMajor) {
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int i = tid + it * NT;
            const int m = i >> 10, ln = (i & 1023) >> 5, col = i & 31;
            const int n = lane0 + m * 32 + ln, v = n0 + col;
            if (n < g.n_lanes && v < g.N) g.C[(size_t)n * g.ldc + v] = total(m, ln, col) + bias_v[0];
        }
    } else if (EPI == kEpiRowStats) {
        // the logits leave as above, and with them the statistics of this workgroup's 32 columns of every row: the
        // update kernel then resolves log-softmax and argmax of a row from V / 32 records instead of V logits.  The 32
        // columns of a row sit in the 32 lanes of a half-wave: butterflies inside the half.
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int i = tid + it * NT;
            const int m = i >> 10, ln = (i & 1023) >> 5, col = i & 31;
            const int n = lane0 + m * 32 + ln, v = n0 + col;
            const bool in = v < g.N;
            const float x = total(m, ln, col) + bias_v[0];
            if (n < g.n_lanes && in) g.C[(size_t)n * g.ldc + v] = x;
            const float xs = in ? x : -3.0e38f;
            auto fmx = [](float a, float b) { return fmaxf(a, b); };
            const float mx = half_allreduce_f(xs, fmx);
            // first column holding the maximum
            const int first = half_allreduce_i((xs == mx) ? col : 32, [](int a, int b) { return a < b ? a : b; });
            const float second = half_allreduce_f((col == first) ? -3.0e38f : xs, fmx);     // the largest of the others
            // the sum: every lane ends with the same value only if the additions pair up identically in both halves of
            // each butterfly -- they do (a + b == b + a), so the record does not depend on the lane that stores it
            const float se = half_allreduce_f(in ? expf(x - mx) : 0.f, [](float a, float b) { return a + b; });
            if (col == 0 && n < g.n_lanes)
                g.row_part[(size_t)n * g.row_part_ld + bx] = make_float4(mx, se, second, __builtin_bit_cast(float, n0 + first));
        }
    } else if (EPI == kEpiKMajor) {
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int i = tid + it * NT;
            const int m = i >> 10, col = (i & 1023) >> 5, ln = i & 31;   // consecutive threads -> consecutive lanes
            const int v = n0 + col, n = lane0 + m * 32 + ln;
            if (v < g.N) g.C[(size_t)v * g.ldc + n] = total(m, ln, col) + bias_v[it];
        }
    } else if (EPI == kEpiLstmCell) {
        // tile columns: [i x8 | f x8 | g x8 | o x8] of hidden units u0 .. u0+7; only lanes whose predictor steps are
        // written.  One (lane, unit) per thread.
        if (cell_on) {
            const int j = cell_j, ln = l31;
            const int m = (tid >> 8) % MT;
            const float ig = sigmoidf_(total(m, ln, j) + cell_g[0]);
            const float fg = sigmoidf_(total(m, ln, 8 + j) + cell_g[1]);
            const float gg = tanhf(total(m, ln, 16 + j) + cell_g[2]);
            const float og = sigmoidf_(total(m, ln, 24 + j) + cell_g[3]);
            const float c = fg * cell_c + ig * gg;
            g.pool_c[(size_t)cell_sn * g.Hp + cell_unit] = c;
            g.new_hT[(size_t)cell_unit * g.lda + cell_n] = og * tanhf(c);       // lda = NLp
        }
    } else if (EPI == kEpiSlotRow) {
        // row-major rows addressed through a per-lane slot: pool_g[slot(n)][v] = W_hh[v] . h_n + b[v]
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int i = tid + it * NT;
            const int m = i >> 10, ln = (i & 1023) >> 5, col = i & 31;
            const int n = lane0 + m * 32 + ln, v = n0 + col;
            if (n < g.n_lanes && v < g.N) g.C[(size_t)slot_v[it] * g.ldc + v] = total(m, ln, col) + bias_v[0];
        }
    } else {   // kEpiJointAct: ht[j][f * stride + lane] = tanh(ep_all[utt, t_lane + f, j] + pp[j][lane]); zero for idle lanes
#pragma unroll
        for (int it = 0; it < kItems; ++it) {
            const int i = tid + it * NT;
            const int m = i >> 10, col = (i & 1023) >> 5, ln = i & 31;
            const int v = n0 + col, n = lane0 + m * 32 + ln;
            if (v >= g.N) continue;
            const float pp = total(m, ln, col) + bias_v[it];
#pragma unroll
            for (int f = 0; f < kMaxLook; ++f)
                if (f < g.look) g.C[(size_t)v * g.ldc + f * g.lane_stride + n] = act_on[it] ? act_value(g.act, act_ep[f][it] + pp) : 0.f;
        }
    }
    WR_STAMP(5);                                   // epilogue stores issued
    WR_STAMP_DRAIN();
    WR_STAMP(6);
    WR_STAMP_RT(8);
    WR_STAMP_FLUSH(g.dbg_slot);
}

template <int MT, int EPI>
__global__ __launch_bounds__(64 * kGemmWaves) void lane_gemm_kernel(GemmArgs g)
{
    __shared__ float red[kGemmWaves][MT][32 * 32];
    lane_gemm_body<MT, EPI>(g, blockIdx.x, red);
}

// the 1-wave form (VW = 8): ONE wave works through all eight K slices of a 32 x 32 tile.  For the 640 tiles of a 128-lane
// beam search's joiner GEMM this is the fastest shape: 640 independent waves on the chip's 1024 SIMDs, no barrier, each
// MFMA-bound for K / 2 * 64 cycles (7 us at K = 512) with its loads hidden behind them, where the 8-wave form needs two
// rounds of workgroups (20 us).  Same eight partial tiles summed in the same order: bit-identical.
template <int EPI>
__global__ __launch_bounds__(64) void lane_gemm1_kernel(GemmArgs g)
{
    __shared__ float red[kGemmWaves][1][32 * 32];
    lane_gemm_body<1, EPI, 8>(g, blockIdx.x, red);
}

// the 4-wave form (VW = 2, 32-lane tiles): same results, four workgroups per CU
template <int EPI>
__global__ __launch_bounds__(64 * kGemmWaves / 2, 4) void lane_gemm4_kernel(GemmArgs g)
{
    __shared__ float red[kGemmWaves][1][32 * 32];
    lane_gemm_body<1, EPI, 2>(g, blockIdx.x, red);
}

// Two independent GEMMs over the same lanes in ONE launch (column tiles [0, ct0) belong to the first): the small
// predictor GEMMs leave most of the chip idle, so the recurrent product of the layer below rides along for free.
template <int MT, int EPI0, int EPI1>
__global__ __launch_bounds__(64 * kGemmWaves) void lane_gemm_pair_kernel(GemmArgs g0, GemmArgs g1, int ct0)
{
    __shared__ float red[kGemmWaves][MT][32 * 32];
    if ((int)blockIdx.x < ct0) lane_gemm_body<MT, EPI0>(g0, blockIdx.x, red);
    else lane_gemm_body<MT, EPI1>(g1, (int)blockIdx.x - ct0, red);
}

// ---- LSTM predictor step, hoisted form -------------------------------------------------------------------------
// gates_l = W_ih_l . in_l + W_hh_l . h_l + b_l.  Two of the three terms do not have to wait for the step:
//   * layer 0's input is an embedding row, so W_ih_0 . embed[v] is a table (etab, built once per handle);
//   * W_hh_l . h_l + b_l depends only on the state the step starts from, and that state was itself produced by an
//     earlier step: it is computed right behind that step (kEpiSlotRow jobs riding in the launches of the next stage,
//     which leave most of the chip idle) and kept with the state (pool_g).
// Layer 0 is then elementwise and runs in the tail of the kernel that decides the token (update / resolve / beam
// update / init): one launch per micro-step less, and the layer >= 1 GEMMs have half the depth.  State lives in a pool
// of 2 * NLp slots addressed through comm_slot / new_slot: committing a step swaps two integers (greedy) and the beam
// search's survivors inherit slot numbers instead of copied caches.  Lane-indexed are only the hidden outputs of the
// last step (new_hT), which the next GEMM reads as its k-major A operand.
__device__ __forceinline__ void lstm_layer0_cell(const DevState &S, int n, int tok, int sc, int sn)
{
    const Dims &d = S.d;
    const float *__restrict__ e = S.etab + (size_t)tok * d.G4p;
    const float *__restrict__ g = S.pool_g + (size_t)sc * d.G4p;
    const float *__restrict__ c0 = S.pool_c + (size_t)sc * d.Hp;
    float *__restrict__ c1 = S.pool_c + (size_t)sn * d.Hp;
    for (int u = threadIdx.x; u < d.H; u += blockDim.x) {
        const int col = (u >> 3) * 32 + (u & 7);              // tile of 32 columns = i,f,g,o of 8 units
        const float ig = sigmoidf_(e[col] + g[col]);
        const float fg = sigmoidf_(e[col + 8] + g[col + 8]);
        const float gg = tanhf(e[col + 16] + g[col + 16]);
        const float og = sigmoidf_(e[col + 24] + g[col + 24]);
        const float c = fg * c0[u] + ig * gg;
        c1[u] = c;
        S.new_hT[(size_t)u * d.NLp + n] = og * tanhf(c);
    }
}

// A lane's two slots hold the zero state (h = 0, so W_hh . h + b = b), comm_slot = n, new_slot = NLp + n.
__device__ __forceinline__ void lstm_reset_lane(const DevState &S, int n)
{
    const Dims &d = S.d;
    const size_t S2 = 2 * (size_t)d.NLp;
    for (int l = 0; l < d.L; ++l) {
        float *pc = S.pool_c + ((size_t)l * S2 + n) * d.Hp;
        float *pg = S.pool_g + ((size_t)l * S2 + n) * d.G4p;
        for (int i = threadIdx.x; i < d.Hp; i += blockDim.x) pc[i] = 0.f;
        for (int i = threadIdx.x; i < d.G4p; i += blockDim.x) pg[i] = S.bsum[l][i];
    }
    if (threadIdx.x == 0) { S.comm_slot[n] = n; S.new_slot[n] = d.NLp + n; }
}

// etab[v][c'] = sum_k w_ih0[gate * H + unit][k] * embed[v][k]  (c' <-> (unit, gate) as in lstm_weight_prep_kernel); float64
// sums rounded once (setup, once per handle)
__global__ void lstm_etab_kernel(const float *__restrict__ embed, const float *__restrict__ w_ih, int V, int D, int H, int Hp,
                                 float *__restrict__ etab)
{
    const int G4p = 4 * Hp;
    const long total = (long)V * G4p;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int v = (int)(i / G4p), c = (int)(i % G4p);
        const int unit = (c >> 5) * 8 + (c & 7), gate = (c & 31) >> 3;
        double a = 0.0;
        if (unit < H) {
            const float *__restrict__ wr = w_ih + (size_t)(gate * H + unit) * D;
            const float *__restrict__ er = embed + (size_t)v * D;
            for (int k = 0; k < D; ++k) a += (double)wr[k] * (double)er[k];
        }
        etab[i] = (float)a;
    }
}

// step API: layer 0 for every lane as a kernel of its own
__global__ void lstm_layer0_kernel(DevState *sp)
{
    const DevState &S = *sp;
    const int n = blockIdx.x;
    if (!(S.lane_active[n] && S.need_pred[n])) return;
    lstm_layer0_cell(S, n, S.token[n], S.comm_slot[n], S.new_slot[n]);
}

// xT[:, n] = embed[tok] for one lane (called by the kernels that decide a lane's next token)
__device__ __forceinline__ void write_embedding_column(DevState *s, int n, int tok)
{
    const Dims &d = s->d;
    for (int k = threadIdx.x; k < d.D; k += blockDim.x) s->xT[(size_t)k * d.NLp + n] = s->embed[(size_t)tok * d.D + k];
}

// A lane starts from the zero state with the blank as its first predictor input
__device__ __forceinline__ void first_predictor_input(DevState *s, int n)
{
    if (s->d.ptype == kPredLstm) {
        lstm_reset_lane(*s, n);
        __syncthreads();                                      // the slot rows written above are read below
        lstm_layer0_cell(*s, n, s->blank, n, s->d.NLp + n);
    } else {
        write_embedding_column(s, n, s->blank);
    }
}

// wt[k][j] = sum_p wf[j][p] * wp[p][k]  (k-major, as lane_gemm reads it),  bias[j] = bf[j] + sum_p wf[j][p] * bp[p];
// products and sums in float64, rounded to fp32 once (setup, once per handle)
__global__ void compose_proj_ffn_kernel(const float *__restrict__ wf /* [J][P] */, const float *__restrict__ bf,
                                        const float *__restrict__ wp /* [P][H] */, const float *__restrict__ bp, int J, int P,
                                        int H, int Jn, float *__restrict__ wt /* [Hp][Jn] */, float *__restrict__ bias)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (long)H * J) {
        const int k = (int)(idx / J), j = (int)(idx - (long)k * J);
        double a = 0.0;
        for (int p = 0; p < P; ++p) a += (double)wf[(size_t)j * P + p] * (double)wp[(size_t)p * H + k];
        wt[(size_t)k * Jn + j] = (float)a;
    } else if (idx < (long)H * J + J) {
        const int j = (int)(idx - (long)H * J);
        double a = (double)bf[j];
        for (int p = 0; p < P; ++p) a += (double)wf[(size_t)j * P + p] * (double)bp[p];
        bias[j] = (float)a;
    }
}

// ---------------------------------------------------- stateless predictors --
// EmbeddingPredictor.forward_step (predictor.py:325-372) and ConvPredictor.forward_step (:455-481), one lane per
// workgroup.  context = [history slots 0 .. ctx-2 (cache_hT), embedding of the lane's token (xT)];
//   embedding:  weight[h][c] = sum_e context[c][e] * pos[h][e][c]        (pos = pos_embed.weight viewed [heads, D, ctx])
//               comb[e] = sum_h sum_c weight[h][c] * context[c][e] / (heads * ctx)   -> ffn -> LayerNorm -> activation
//   conv:       comb[e] = sum_c context[c][e] * conv_w[e][c] (+ conv_b[e])            -> LayerNorm -> activation
// The new history is context[1 ..] (new_hT): the search kernels commit it on an emission exactly like an LSTM state.
// STAGE 0: embedding predictor, context weighting -> combT (+ new history); the ffn runs as a lane GEMM in between;
// STAGE 1: LayerNorm + activation of ffnT -> outT;  STAGE 2: conv predictor, all of it.
constexpr int kCtxThreads = 256;
constexpr int kCtxPer = 4;                    // embedding width <= 1024
constexpr int kMaxCtx = WR_MAX_LSTM_LAYERS + 1;

__device__ __forceinline__ float ctx_block_sum(float v, float *red)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// LayerNorm (biased variance, as torch.nn.LayerNorm) + activation of this thread's elements e = tid + 256 j
__device__ __forceinline__ void ctx_norm_act_store(const DevState &S, const float (&x)[kCtxPer], int n, float *red)
{
    const Dims &d = S.d;
    const int tid = threadIdx.x;
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < kCtxPer; ++j) part += (tid + kCtxThreads * j < d.D) ? x[j] : 0.f;
    const float mean = ctx_block_sum(part, red) / (float)d.D;
    part = 0.f;
#pragma unroll
    for (int j = 0; j < kCtxPer; ++j) {
        const float t = x[j] - mean;
        part += (tid + kCtxThreads * j < d.D) ? t * t : 0.f;
    }
    const float rstd = 1.f / sqrtf(ctx_block_sum(part, red) / (float)d.D + d.ln_eps);
#pragma unroll
    for (int j = 0; j < kCtxPer; ++j) {
        const int e = tid + kCtxThreads * j;
        if (e < d.D) S.outT[(size_t)e * d.NLp + n] = act_value(d.pact, (x[j] - mean) * rstd * S.pnorm_w[e] + S.pnorm_b[e]);
    }
}

template <int STAGE>
__global__ __launch_bounds__(kCtxThreads) void ctx_predictor_kernel(DevState *sp)
{
    const DevState &S = *sp;
    const Dims &d = S.d;
    const int n = blockIdx.x, tid = threadIdx.x;
    if (!(S.lane_active[n] && S.need_pred[n])) return;      // predicated per lane, like the LSTM cell epilogue
    __shared__ float red[4];
    __shared__ float part[64 * 4];
    const int D = d.D, ctx = d.ctx;
    const size_t ls = (size_t)d.Hp * d.NLp;
    if (STAGE == 1) {
        float x[kCtxPer];
#pragma unroll
        for (int j = 0; j < kCtxPer; ++j) {
            const int e = tid + kCtxThreads * j;
            x[j] = e < D ? S.ffnT[(size_t)e * d.NLp + n] : 0.f;
        }
        ctx_norm_act_store(S, x, n, red);
        return;
    }
    float cin[kMaxCtx][kCtxPer];
#pragma unroll
    for (int c = 0; c < kMaxCtx; ++c)
#pragma unroll
        for (int j = 0; j < kCtxPer; ++j) {
            const int e = tid + kCtxThreads * j;
            float v = 0.f;
            if (c < ctx && e < D) v = c < ctx - 1 ? S.cache_hT[(size_t)c * ls + (size_t)e * d.NLp + n] : S.xT[(size_t)e * d.NLp + n];
            cin[c][j] = v;
        }
    // new history = context[1 ..]
#pragma unroll
    for (int c = 1; c < kMaxCtx; ++c)
#pragma unroll
        for (int j = 0; j < kCtxPer; ++j) {
            const int e = tid + kCtxThreads * j;
            if (c < ctx && e < D) S.new_hT[(size_t)(c - 1) * ls + (size_t)e * d.NLp + n] = cin[c][j];
        }
    float o[kCtxPer];
    if (STAGE == 0) {
        const int heads = d.heads;
#pragma unroll
        for (int c = 0; c < kMaxCtx; ++c) {
            if (c >= ctx) continue;
            for (int h = 0; h < heads; ++h) {
                float p = 0.f;
#pragma unroll
                for (int j = 0; j < kCtxPer; ++j) {
                    const int e = tid + kCtxThreads * j;
                    if (e < D) p += cin[c][j] * S.pos_w[((size_t)h * D + e) * ctx + c];
                }
                p = wave_sum(p);
                if ((tid & 63) == 0) part[(h * ctx + c) * 4 + (tid >> 6)] = p;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kCtxPer; ++j) o[j] = 0.f;
        for (int h = 0; h < heads; ++h) {                     // per head: weight[h] @ context, then the sum over heads
            float t[kCtxPer];
#pragma unroll
            for (int j = 0; j < kCtxPer; ++j) t[j] = 0.f;
#pragma unroll
            for (int c = 0; c < kMaxCtx; ++c) {
                if (c >= ctx) continue;
                const float *q = part + (h * ctx + c) * 4;
                const float w = q[0] + q[1] + q[2] + q[3];
#pragma unroll
                for (int j = 0; j < kCtxPer; ++j) t[j] += w * cin[c][j];
            }
#pragma unroll
            for (int j = 0; j < kCtxPer; ++j) o[j] += t[j];
        }
        const float inv = 1.f / (float)(heads * ctx);
#pragma unroll
        for (int j = 0; j < kCtxPer; ++j) {
            const int e = tid + kCtxThreads * j;
            if (e < D) S.combT[(size_t)e * d.NLp + n] = o[j] * inv;
        }
    } else {
#pragma unroll
        for (int j = 0; j < kCtxPer; ++j) {
            const int e = tid + kCtxThreads * j;
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < kMaxCtx; ++c)
                if (c < ctx && e < D) a += cin[c][j] * S.conv_w[(size_t)e * ctx + c];
            o[j] = (e < D && S.conv_b) ? a + S.conv_b[e] : a;
        }
        ctx_norm_act_store(S, o, n, red);
    }
}

// Tail of the kernels that decide a lane's token: the commit (greedy_search copy.py:52 `cache = new_cache`) and the
// next predictor input.  LSTM predictor: a commit swaps the lane's two slot numbers, and layer 0 of the predictor step
// the emission causes is evaluated here (lstm_layer0_cell) from the committed slot; stateless predictors copy their token
// history and leave the new token's embedding column for ctx_predictor_kernel.  `sc` / `sn`: the lane's slots as
// loaded at the top of the kernel.
__device__ __forceinline__ void commit_and_feed(const DevState &S, int n, bool feed, bool commit, int tok, int sc, int sn)
{
    const Dims &d = S.d;
    const int tid = threadIdx.x;
    if (d.ptype == kPredLstm) {
        if (commit) {
            const int t = sc; sc = sn; sn = t;
            if (tid == 0) { S.comm_slot[n] = sc; S.new_slot[n] = sn; }
        }
        if (feed) lstm_layer0_cell(S, n, tok, sc, sn);
        return;
    }
    if (feed) {
        for (int q = tid; q < d.D; q += blockDim.x) S.xT[(size_t)q * d.NLp + n] = S.embed[(size_t)tok * d.D + q];
    }
    if (commit) {
        for (int i = tid; i < d.L * d.Hp; i += blockDim.x) {
            const size_t o = (size_t)i * d.NLp + n;
            S.cache_hT[o] = S.new_hT[o];
            S.cache_cT[o] = S.new_cT[o];
        }
    }
}

// ---------------------------------------------------------------- greedy --
__global__ void greedy_init_kernel(DevState *s)
{
    const Dims &d = s->d;
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    for (int i = tid; i < d.L * d.Hp; i += blockDim.x) {
        const size_t o = (size_t)i * d.NLp + n;
        s->cache_hT[o] = 0.f; s->cache_cT[o] = 0.f; s->new_hT[o] = 0.f; s->new_cT[o] = 0.f;
    }
    if (tid == 0) {
        const int T = s->enc_lens[n] < s->T ? s->enc_lens[n] : s->T;
        s->token[n] = s->blank;
        s->lane_t[n] = 0;
        s->noblk[n] = 0;
        s->need_pred[n] = 1;
        s->new_is_cache[n] = 0;
        s->hyp_lens[n] = 0;
        const int act = T > 0;
        s->lane_active[n] = act;
        if (act) atomicAdd(s->active_count, 1);
    }
    first_predictor_input(s, n);
}

// Streaming: start the next chunk of every stream with the state the previous chunk left behind
// (reset_cache / forward_greedy_search of "transducer ref.py":541-606).  `ref_new_cache` reproduces the
// reference's `new_cache = self.cache` at the top of each chunk (the not-yet-committed predictor state of the
// previous chunk is dropped); 0 keeps it, so that chunked decoding equals decoding the concatenation.
__global__ void greedy_chunk_init_kernel(DevState *s, int ref_new_cache)
{
    const Dims &d = s->d;
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    (void)d;
    if (tid == 0) {
        const int T = s->enc_lens[n] < s->T ? s->enc_lens[n] : s->T;
        s->lane_t[n] = 0;
        s->hyp_lens[n] = 0;
        // `new_cache = self.cache` at the top of a chunk: until the predictor steps again, committing is a no-op.
        // (The pending state itself is left alone -- the predictor OUTPUT of the last step stays valid, as
        // self.pred_out_step does in the reference.)
        s->new_is_cache[n] = ref_new_cache ? 1 : 0;
        const int act = T > 0;
        s->lane_active[n] = act;
        if (act) atomicAdd(s->active_count, 1);
    }
}

// The lane's scalars and its row records are fetched up front and the state machine runs redundantly in every thread
// (thread 0 stores), so the kernel has one memory round trip before the reductions and one after.
// HW = true: the hot-word variant (greedy_search.py:297-430).  The gate decision of the NEXT predictor step is made
// here, right after the emission that causes that step -- the gate is a function of the frame alone (see
// hw_gate_table_kernel), so it does not have to wait for the predictor.  A "go-back" (:369-385) withdraws exactly
// the emission this kernel has just decided on (the reference pops the last token, predictor output, cache and
// input and steps the predictor again from the popped state), so it costs nothing to undo: the token is not
// appended, the cache not committed, the next input not replaced.
template <bool HW, int PP>
__global__ __launch_bounds__(256) void greedy_update_kernel(DevState *sp, LaneArgs a)
{
    WR_STAMP_DECL;
    WR_STAMP_RT(7);
    WR_STAMP(0);
    const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    // no branch before the loads: everything this lane needs is requested in one batch, the per-lane state through the
    // kernel-argument pointers (no dependence on the state block), idle lanes leave after the first reduction
    const int act = a.lane_active[n];
    int t = a.lane_t[n], nb = a.noblk[n];
    const int need = a.need_pred[n];
    int nic = a.new_is_cache[n];
    const int sc = a.comm_slot[n], sn = a.new_slot[n];     // LSTM predictor: state slots (unused otherwise)
    // The row is resolved from the per-block records the ffn_out epilogue left (kEpiRowStats): {block max, sum of
    // exp(x - block max), runner-up, first index of the block max} for every 32 columns -- V / 32 records instead of V
    // logits.  log_softmax as the reference evaluates it, lp = (x - max) - log(sum(exp(x - max))), and its argmax with
    // the first index on ties: lp is a monotone function of x, so the maximum of lp is (max - max) - ls and the
    // winner is the first column whose lp equals it.  A block takes part if its maximum does; if its runner-up does too
    // (two logits that lp cannot tell apart: they differ by less than half an ulp of ls), its 32 logits are re-read and
    // scanned in order -- otherwise the recorded first index is the answer.
    // Every WAVE resolves the row on its own from all the records (PP per lane; they are a few KB and come from L2 once
    // per CU): the three reductions are register butterflies, no LDS and no workgroup barrier on the way to the token.
    const float4 *__restrict__ rp = a.row_part + (size_t)n * a.n_cb;
    const int ncb = (a.V + 31) / 32;
    float4 rec[PP];
#pragma unroll
    for (int i = 0; i < PP; ++i) {
        const int bq = lane + i * 64;
        rec[i] = rp[bq < ncb ? bq : ncb - 1];
    }
    const DevState S = *sp;                         // by value: no reloads of the pointers after the stores below
    const Dims &d = S.d;
    const int len = S.hyp_lens[n];
    const int enc_len = S.enc_lens[n];
    int gate_cur = 1, gb_flag = 0, gb_end = 0, last_t = 0, tlen = 0, gate_t0 = 1, gate_t1 = 1, last_gate = 1;
    if (HW) {
        gate_cur = S.cur_gate[n]; gb_flag = S.gb_flag[n]; gb_end = S.gb_end[n]; last_t = S.last_t[n];
        tlen = S.trace_len[n];
        const int tc = t < S.T ? t : S.T - 1, tn = t + 1 < S.T ? t + 1 : S.T - 1;
        gate_t0 = S.gate_tab[(size_t)n * S.T + tc];                  // the next predictor step sees frame t or t + 1
        gate_t1 = S.gate_tab[(size_t)n * S.T + tn];
        last_gate = S.trace[(size_t)n * S.trace_cap + (tlen > 0 ? (tlen <= S.trace_cap ? tlen - 1 : S.trace_cap - 1) : 0)];
    }
    float m = -3.0e38f;
#pragma unroll
    for (int i = 0; i < PP; ++i) m = fmaxf(m, (lane + i * 64 < ncb) ? rec[i].x : -3.0e38f);
    m = wave_allmax_dpp(m);
    WR_STAMP(1);                                   // state and records arrived, first reduction done
    if (!act) return;
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < PP; ++i) sum += (lane + i * 64 < ncb) ? rec[i].y * expf(rec[i].x - m) : 0.f;
    sum = wave_allsum_dpp(sum);
    const float ls = logf(sum);
    const float top = (m - m) - ls;                 // log-probability of the maximum, exactly as the elementwise formula gives it
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < PP; ++i) {
        const int bq = lane + i * 64;
        if (bq >= ncb) continue;
        if (((rec[i].x - m) - ls) != top) continue;
        int idx = __builtin_bit_cast(int, rec[i].w);
        if (((rec[i].z - m) - ls) == top) {          // runner-up indistinguishable from the block maximum: scan the block
            const float *__restrict__ x = S.logits + (size_t)n * d.V;
            idx = 0x7fffffff;
            for (int c = 31; c >= 0; --c) {
                const int v = bq * 32 + c;
                if (v < d.V && ((x[v] - m) - ls) == top) idx = v;
            }
        }
        if (idx < bi) bi = idx;
    }
    bi = wave_allmin_dpp(bi);
    WR_STAMP(2);                                   // token decided
    const int k = bi;
    const bool emit = (k != S.blank);
    if (need) nic = 0;                             // the predictor stepped in this micro-step
    bool commit = emit && !nic;
    int need_next = need;
    const int t_dec = t;                           // the frame this decision was made on
    if (emit) { need_next = 1; nb += 1; }
    if (!emit || nb >= S.n_steps) {
        if (!emit) need_next = 0;
        t += 1;
        nb = 0;
    }
    const int T = enc_len < S.T ? enc_len : S.T;
    // hot-word gate of the predictor step this emission leads to (greedy_search.py:357-392)
    bool withdraw = false;
    int push0 = -1, push1 = -1;                    // values appended to the trace (after an optional pop)
    bool pop = false;
    if (HW && emit && t < T) {
        const int gt = (t == t_dec) ? gate_t0 : gate_t1;
        if (S.hw_filter) {
            if (!gb_flag) {
                if (gt == 0) { push0 = 0; last_t = t; gate_cur = 0; }
                else if (tlen > 0 && last_gate == 0) {
                    // go-back: forget the gate-0 step and the token it produced, resume from its frame with biasing on
                    withdraw = true;
                    gb_end = t; t = last_t; gb_flag = 1;
                    pop = true;
                    nb -= 1;
                    push0 = 1;                     // the re-run step is recorded with the gate forced to 1 (:388-391)
                    if (t >= gb_end) gb_flag = 0;
                    gate_cur = 1;
                } else { push0 = 1; gate_cur = 1; }
            } else {
                push0 = 1;
                if (t >= gb_end) gb_flag = 0;
                gate_cur = 1;
            }
        } else { push0 = 1; gate_cur = 1; }
    }
    (void)push1;
    if (withdraw) commit = false;
    if (tid == 0) {
        atomicAdd(S.active_count + (emit ? 2 : 1), 1);               // decision statistics for the look-ahead policy
        if (need) S.new_is_cache[n] = 0;
        if (emit && !withdraw) {
            if (len < S.max_hyp) S.hyps[(size_t)n * S.max_hyp + len] = k;
            S.hyp_lens[n] = len + 1;
            S.token[n] = k;
        }
        S.need_pred[n] = need_next;
        S.lane_t[n] = t;
        S.noblk[n] = nb;
        if (HW) {
            int tl = tlen - (pop ? 1 : 0);
            if (push0 >= 0) {
                if (tl < S.trace_cap) S.trace[(size_t)n * S.trace_cap + tl] = push0;
                tl += 1;
            }
            S.trace_len[n] = tl;
            S.cur_gate[n] = gate_cur;
            S.gb_flag[n] = gb_flag;
            S.gb_end[n] = gb_end;
            S.last_t[n] = last_t;
        }
        if (t >= T) {
            S.lane_active[n] = 0;
            atomicSub(S.active_count, 1);
        }
    }
    commit_and_feed(S, n, emit && !withdraw, commit, k, sc, sn);
    WR_STAMP(5);
    WR_STAMP_DRAIN();
    WR_STAMP(6);
    WR_STAMP_RT(8);
    WR_STAMP_FLUSH(HW ? 5 : 4);
}

// ---- look-ahead greedy: `look` encoder frames per micro-step against one predictor state -------------------
// While a lane keeps answering blank its predictor output does not change, so the joiner rows of frames t, t+1, ...
// can be evaluated together: greedy_rows_kernel takes the argmax of every (frame, lane) row in parallel,
// greedy_resolve_kernel then walks a lane's rows in order through the same state machine as greedy_update_kernel
// and stops at the first emission (the predictor must step before the next decision).  Token sequences are
// identical to the one-frame-per-step loop; a run of blanks costs one micro-step instead of `look`.
template <int NV>
__global__ __launch_bounds__(256) void greedy_rows_kernel(DevState *sp)
{
    __shared__ float sv[4];
    __shared__ int si[4];
    const DevState S = *sp;
    const Dims &d = S.d;
    const int n = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int act = S.lane_active[n];
    const int t = S.lane_t[n];
    const int enc_len = S.enc_lens[n];
    const float *__restrict__ x = S.logits + ((size_t)f * d.NLp + n) * d.V;
    float xv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * 256;
        xv[i] = x[v < d.V ? v : d.V - 1];
    }
    float m = -3.0e38f;
#pragma unroll
    for (int i = 0; i < NV; ++i) m = fmaxf(m, (tid + i * 256 < d.V) ? xv[i] : -3.0e38f);
    m = block_max(m, sv);
    const int T = enc_len < S.T ? enc_len : S.T;
    if (!act || t + f >= T) return;                // frames past the end are never consulted
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) sum += (tid + i * 256 < d.V) ? expf(xv[i] - m) : 0.f;
    sum = block_sum(sum, sv);
    const float ls = logf(sum);
    float best = -3.0e38f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * 256;
        const float lp = (xv[i] - m) - ls;
        if (v < d.V && lp > best) { best = lp; bi = v; }   // strided ascending scan keeps the lowest index per thread
    }
    block_argmax(best, bi, sv, si);
    if (tid == 0) S.row_tok[(size_t)f * d.NLp + n] = bi;
}

// What both look-ahead resolve kernels start from and end with.  The constructor requests the lane's scalars and its
// `look` row decisions in one batch, before the caller's `!act` return; T = the lane's frame count; nic = whether the pending
// predictor state still equals the committed one.  The kernel's walk advances t / nb / len / need and notes n_blank (rows
// answered blank), `emitted` (the one label, or -1) and `commit`.  store: thread 0 writes that back, then commit_and_feed.
struct ResolveLane {
    int act, t, nb, need0, nic, len, T, sc, sn, rows[kMaxLook];
    int need, emitted = -1, n_blank = 0;
    bool commit = false;
    __device__ __forceinline__ ResolveLane(const DevState &S, int n, int look)
    {
        act = S.lane_active[n];
        t = S.lane_t[n], nb = S.noblk[n];
        need = need0 = S.need_pred[n];
        nic = S.new_is_cache[n];
        len = S.hyp_lens[n];
        const int enc_len = S.enc_lens[n];
        sc = S.comm_slot[n], sn = S.new_slot[n];
#pragma unroll
        for (int f = 0; f < kMaxLook; ++f) rows[f] = S.row_tok[(size_t)(f < look ? f : 0) * S.d.NLp + n];
        T = enc_len < S.T ? enc_len : S.T;
        if (need0) nic = 0;                        // the predictor stepped in this micro-step
    }
    __device__ __forceinline__ void store(const DevState &S, int n, int tid) const
    {
        if (tid == 0) {
            if (n_blank) atomicAdd(S.active_count + 1, n_blank);     // decision statistics for the look-ahead policy
            if (emitted >= 0) atomicAdd(S.active_count + 2, 1);      // (consulted rows only)
            if (need0) S.new_is_cache[n] = 0;
            S.hyp_lens[n] = len;
            if (emitted >= 0) S.token[n] = emitted;
            S.need_pred[n] = need;
            S.lane_t[n] = t;
            S.noblk[n] = nb;
            if (t >= T) {
                S.lane_active[n] = 0;
                atomicSub(S.active_count, 1);
            }
        }
        commit_and_feed(S, n, emitted >= 0, commit, emitted, sc, sn);
    }
};

__global__ __launch_bounds__(256) void greedy_resolve_kernel(DevState *sp, int look)
{
    const DevState S = *sp;
    const int n = blockIdx.x, tid = threadIdx.x;
    ResolveLane ln(S, n, look);
    if (!ln.act) return;
    bool done = false;
#pragma unroll
    for (int f = 0; f < kMaxLook; ++f) {
        if (f >= look || done) continue;
        const int k = ln.rows[f];
        const bool emit = (k != S.blank);
        ln.n_blank += emit ? 0 : 1;
        if (emit) {
            if (tid == 0 && ln.len < S.max_hyp) S.hyps[(size_t)n * S.max_hyp + ln.len] = k;
            ln.len += 1;
            ln.need = 1;
            ln.nb += 1;
            ln.commit = !ln.nic;
            ln.emitted = k;
        }
        if (!emit || ln.nb >= S.n_steps) {
            if (!emit) ln.need = 0;
            ln.t += 1;
            ln.nb = 0;
        }
        done = emit || ln.t >= ln.T;               // after an emission the remaining rows belong to a stale predictor state
    }
    ln.store(S, n, tid);
}

// ---- token-and-duration (TDT) greedy: the two look-ahead kernels with the TDT decision rule ------------------
// The logits row is Vt = V - tdt_D token columns followed by tdt_D duration columns.  tdt_rows_kernel takes the argmax
// of each part of every (frame, lane) row on the raw fp32 logits (a log-softmax is monotone within a part), lowest
// index on exact ties, and packs them as k | j << 16 into row_tok (V <= 16384).  A part without a finite maximum (NaN
// logits) decides blank / duration 0 rather than an index outside the tables.
template <int NV>
__global__ __launch_bounds__(256) void tdt_rows_kernel(DevState *sp)
{
    __shared__ float sv[4];
    __shared__ int si[4];
    const DevState S = *sp;
    const Dims &d = S.d;
    const int n = blockIdx.x, f = blockIdx.y, tid = threadIdx.x;
    const int act = S.lane_active[n];
    const int t = S.lane_t[n];
    const int enc_len = S.enc_lens[n];
    const int Vt = d.V - S.tdt_D;
    const float *__restrict__ x = S.logits + ((size_t)f * d.NLp + n) * d.V;
    float xv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * 256;
        xv[i] = x[v < Vt ? v : Vt - 1];
    }
    const float xd = x[Vt + (tid < S.tdt_D ? tid : 0)];       // the duration columns: at most 9, one per lane of a wave
    const int T = enc_len < S.T ? enc_len : S.T;
    if (!act || t + f >= T) return;                // frames past the end are never consulted
    float best = -3.0e38f;
    int bi = 0x7fffffff;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * 256;
        if (v < Vt && xv[i] > best) { best = xv[i]; bi = v; }   // strided ascending scan keeps the lowest index per thread
    }
    block_argmax(best, bi, sv, si);
    float dbest = tid < S.tdt_D ? xd : -3.0e38f;
    int dj = tid < S.tdt_D && xd > -3.0e38f ? tid : 0x7fffffff;
    wave_argmax_dpp(dbest, dj);                    // every wave holds lanes 0 .. 63 of its own threads: wave 0 has the columns
    if (tid == 0) {
        const int k = bi < Vt ? bi : S.blank, j = dj < S.tdt_D ? dj : 0;
        S.row_tok[(size_t)f * d.NLp + n] = k | (j << 16);
    }
}

// One workgroup per lane walks the lane's rows against the one predictor state of this micro-step (t0: the lane's frame
// at entry; row f belongs to frame t0 + f):
//   blank:  t += max(d, 1), the emission counter restarts, the walk goes on at row t - t0 (a jump skips rows)
//   label:  emitted at frame t; the counter restarts if d > 0, else counts; t += d; after n_steps labels without a frame
//           advance t += 1; the walk stops (the remaining rows belong to a stale predictor state)
// A lane is done when t >= T_n; a jump may overshoot T_n.  Every micro-step consults row 0, which emits or advances.
__global__ __launch_bounds__(256) void tdt_resolve_kernel(DevState *sp, int look)
{
    const DevState S = *sp;
    const int n = blockIdx.x, tid = threadIdx.x;
    ResolveLane ln(S, n, look);
    if (!ln.act) return;
    const int t0 = ln.t;
#pragma unroll
    for (int f = 0; f < kMaxLook; ++f) {
        if (f >= look || ln.emitted >= 0 || ln.t >= ln.T || ln.t - t0 != f) continue;   // consulted: the row of the lane's current frame
        const int k = ln.rows[f] & 0xffff;
        const int dur = (int)((S.tdt_durs >> (4 * (ln.rows[f] >> 16))) & 15);
        if (k == S.blank) {
            ln.n_blank += 1;
            ln.t += dur > 1 ? dur : 1;
            ln.nb = 0;
            ln.need = 0;
            continue;
        }
        if (tid == 0 && ln.len < S.max_hyp) {
            S.hyps[(size_t)n * S.max_hyp + ln.len] = k;
            if (S.hyp_frames) S.hyp_frames[(size_t)n * S.max_hyp + ln.len] = ln.t;
        }
        ln.len += 1;
        ln.need = 1;
        ln.commit = !ln.nic;
        ln.emitted = k;
        ln.nb = dur > 0 ? 0 : ln.nb + 1;
        ln.t += dur;
        if (ln.nb >= S.n_steps) {
            ln.t += 1;
            ln.nb = 0;
        }
    }
    ln.store(S, n, tid);
}

// ------------------------------------------------------- hot-word greedy --
// Device copy of the ContextBias weights the greedy loop uses (wenet/transformer/context_bias.py:375-394), re-laid
// k-major where a thread block streams them (see wr_decoder_attach_hotword).
struct HwDev {
    int D, heads, HW, NLAB, max_ctx;
    const float *q_wt, *q_b;          // [D][D] k-major
    const float *k_w, *k_b, *v_w, *v_b;   // row-major (nn.Linear), used once per call for the list projections
    const float *o_wt, *o_b;          // [D][D] k-major
    const float *bn_w, *bn_b;         // predictor_bias_bias_norm
    const float *c_wt, *c_b;          // [2D][D] k-major
    const float *on_w, *on_b;         // predictor_bias_out_norm
    const float *he_w, *he_b, *hv_w, *hv_b, *ho_w, *ho_b, *hn_w, *hn_b, *hl_w, *hl_b;   // gate chain, row-major
    float *kbuf[2], *vbuf[2];         // [max_ctx][D]: K / V of the empty list (0) and of the hot-word list (1)
    float *cold_c;                    // [D] one-entry empty list: combine(second half) of its constant bias feature + bias
    int32_t *gate_tab;                // [max_utt * Tmax]
    // attention folded over a short list (heads * entries <= D), built once per call by hw_fold_kernel:
    //   scores = mqT^T x + mq_c      mqT[k][r] = sum_{j in head h} Wq[j][k] K[c][j] / sqrt(d_k),  r = h * n_ctx + c
    //   out    = noT^T p + b_o       noT[r][j] = sum_{i in head h} Wo[j][i] V[c][i]
    float *mqT[2], *mq_c[2], *noT[2]; // [D][D], [D], [D][D] per list (used when 1 < entries and heads * entries <= D)
    // the predictor's projection (predictor.py:198) is evaluated here too: x = proj_wt^T h + proj_b, from the LSTM's last
    // layer output (k-major [Hp][NLp]) -- one launch per decision less than a projection GEMM of its own
    const float *proj_wt, *proj_b, *h_lastT;
    int Hp, P, proj_ld, NLp;
    // ... and where the hidden size allows (Hp <= D) it is composed into what consumes x: nothing non-linear sits between
    // the projection and the query / combine Linears, so  combine[:, :D] (Wp h + bp) = c1p_wt^T h + c1p_b  (per handle,
    // float64 sums) and  scores = mqpT^T h + mqp_c  (per call, short lists) -- one dependent matrix-vector stage less
    float *c1p_wt, *c1p_b;            // [Hp][D], [D]
    float *cold_cp;                   // [D] cold_c with the composed bias: the one-entry empty list's whole constant
    float *mqpT[2], *mqp_c[2];        // [Hp][D], [D] per list
    // handle-constant pointers of the lane state the bias kernel starts from (kernel arguments: no wait for the state block)
    const int32_t *lane_active, *need_pred, *cur_gate;
};

// K / V projections of an encoded context list: out[c][j] = b[j] + sum_k hidden[c][k] * W[j][k].
// grid (n_ctx, 2): y = 0 -> K, 1 -> V.  A wave per output, lanes over k (row-major weights: coalesced), wave_sum.
__global__ __launch_bounds__(256) void hw_kv_kernel(HwDev hw, const float *__restrict__ hidden, int list)
{
    const int c = blockIdx.x, which = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float *__restrict__ W = which ? hw.v_w : hw.k_w;
    const float *__restrict__ bb = which ? hw.v_b : hw.k_b;
    float *__restrict__ out = (which ? hw.vbuf[list] : hw.kbuf[list]) + (size_t)c * hw.D;
    const float *__restrict__ x = hidden + (size_t)c * hw.D;
    for (int j = wave; j < hw.D; j += 4) {
        float acc = 0.f;
        for (int k = lane; k < hw.D; k += 64) acc = fmaf(W[(size_t)j * hw.D + k], x[k], acc);
        acc = wave_sum(acc);
        if (lane == 0) out[j] = acc + bb[j];
    }
}

// y[j] = b[j] + sum_k W[j][k] * x[k] for a small row-major Linear inside one workgroup (x, y in LDS): a wave per output
__device__ __forceinline__ void block_linear_rowmajor(const float *__restrict__ W, const float *__restrict__ b, const float *x,
                                                      int K, int N, float *y)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int j = wave; j < N; j += nw) {
        float acc = 0.f;
        for (int k = lane; k < K; k += 64) acc = fmaf(W[(size_t)j * K + k], x[k], acc);
        acc = wave_sum(acc);
        if (lane == 0) y[j] = acc + b[j];
    }
    __syncthreads();
}

// LayerNorm over v[0..N) (LDS) as torch.nn.LayerNorm: biased variance, eps = 1e-5.  Result through `emit(j, value)`.
template <typename F>
__device__ __forceinline__ void block_layer_norm(const float *v, int N, const float *__restrict__ w, const float *__restrict__ b,
                                                 float *sv, F emit)
{
    float s = 0.f;
    for (int j = threadIdx.x; j < N; j += blockDim.x) s += v[j];
    const float mean = block_sum(s, sv) / (float)N;
    float q = 0.f;
    for (int j = threadIdx.x; j < N; j += blockDim.x) { const float dlt = v[j] - mean; q += dlt * dlt; }
    const float var = block_sum(q, sv) / (float)N;
    const float rstd = 1.0f / sqrtf(var + 1e-5f);
    for (int j = threadIdx.x; j < N; j += blockDim.x) emit(j, (v[j] - mean) * rstd * w[j] + b[j]);
    __syncthreads();
}

// The hot-word gate of every frame (ContextBias.forward_hw_pred_both, context_bias.py:388-394, then topk(1) as
// greedy_search.py:359-364).  hw_bias attends from one query (the predictor-side feature) to ONE key / value (the
// encoder-side feature of frame t): softmax over a single score is exactly 1.0, so the attention output is exactly
// linear_out(linear_v(hw_output_layer_enc(enc_feat[t]))) whatever the query is -- the gate depends on the frame
// alone and is evaluated for all frames before the loop.  One workgroup per frame.
__global__ __launch_bounds__(256) void hw_gate_table_kernel(HwDev hw, const float *__restrict__ enc_feat, long rows)
{
    extern __shared__ float sm[];                   // x[D] | a[HW] | b[HW]
    __shared__ float sv[4];
    float *x = sm, *a = sm + hw.D, *bq = a + hw.HW;
    const long r = blockIdx.x;
    if (r >= rows) return;
    for (int k = threadIdx.x; k < hw.D; k += blockDim.x) x[k] = enc_feat[(size_t)r * hw.D + k];
    __syncthreads();
    block_linear_rowmajor(hw.he_w, hw.he_b, x, hw.D, hw.HW, a);         // hw_output_layer_enc
    block_linear_rowmajor(hw.hv_w, hw.hv_b, a, hw.HW, hw.HW, bq);       // hw_bias.linear_v  (attention weight == 1)
    block_linear_rowmajor(hw.ho_w, hw.ho_b, bq, hw.HW, hw.HW, a);       // hw_bias.linear_out
    block_layer_norm(a, hw.HW, hw.hn_w, hw.hn_b, sv, [&](int j, float v) { bq[j] = v; });   // hw_bias_norm
    block_linear_rowmajor(hw.hl_w, hw.hl_b, bq, hw.HW, hw.NLAB, a);     // hw_output_layer
    if (threadIdx.x == 0) {
        int best = 0;
        for (int j = 1; j < hw.NLAB; ++j)
            if (a[j] > a[best]) best = j;            // topk(1): the largest, first index on ties
        hw.gate_tab[r] = best;
    }
}

// y[j] = b[j] + sum_k WT[k][j] * x[k] with the K range split over the 16 waves of the workgroup (every wave has its
// whole share of the k-major weight rows in flight at once), partial sums through LDS.  x, y, part in LDS.
constexpr int kHwThreads = 1024;
__device__ __forceinline__ void block_gemv_kmajor(const float *__restrict__ WT, int ldw, const float *__restrict__ b, const float *x,
                                                  int K, int N, float *part, float *y)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NW = kHwThreads / 64;
    const int kper = (K + NW - 1) / NW;
    const int k0 = wave * kper;
    int k1 = k0 + kper;
    k1 = k1 < K ? k1 : K;
    for (int j0 = 0; j0 < N; j0 += 256) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k = k0; k < k1; ++k) {
            const float xv = x[k];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int j = j0 + lane + 64 * i;
                acc[i] = fmaf(WT[(size_t)k * ldw + (j < N ? j : N - 1)], xv, acc[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = j0 + lane + 64 * i;
            if (j < N) part[wave * N + j] = acc[i];
        }
    }
    __syncthreads();
    for (int j = threadIdx.x; j < N; j += kHwThreads) {
        float sacc = b[j];
#pragma unroll
        for (int w = 0; w < NW; ++w) sacc += part[w * N + j];
        y[j] = sacc;
    }
    __syncthreads();
}

// c1p_wt[i][j] = sum_p combine_w[j][p] * Wp[p][i],  c1p_b[j] = combine_b[j] + sum_p combine_w[j][p] * bp[p]   (p < P = D: the
// first half of the combine Linear's input); float64 sums rounded once.  proj_wt is the handle's k-major projection weight.
__global__ void hw_compose_kernel(const float *__restrict__ cw /* [D][2D] */, const float *__restrict__ cb,
                                  const float *__restrict__ proj_wt /* [Hp][Pn] */, const float *__restrict__ proj_b, int D, int P,
                                  int H, int Hp, int Pn, float *__restrict__ wt /* [Hp][D] */, float *__restrict__ bias)
{
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < (long)Hp * D) {
        const int i = (int)(idx / D), j = (int)(idx - (long)i * D);
        double a = 0.0;
        if (i < H)
            for (int p = 0; p < P; ++p) a += (double)cw[(size_t)j * 2 * D + p] * (double)proj_wt[(size_t)i * Pn + p];
        wt[idx] = (float)a;
    } else if (idx < (long)Hp * D + D) {
        const int j = (int)(idx - (long)Hp * D);
        double a = (double)cb[j];
        for (int p = 0; p < P; ++p) a += (double)cw[(size_t)j * 2 * D + p] * (double)proj_b[p];
        bias[j] = (float)a;
    }
}

// Per call, per list with heads * entries <= D: the query projection folded into the keys and the output projection folded
// into the values (see HwDev).  One workgroup per (head, entry) row r.
__global__ __launch_bounds__(256) void hw_fold_kernel(HwDev hw, int list, int nctx)
{
    const int r = blockIdx.x, tid = threadIdx.x;
    const int D = hw.D, dk = D / hw.heads;
    const int hh = r / nctx, c = r - hh * nctx;
    const float *__restrict__ kr = hw.kbuf[list] + (size_t)c * D + hh * dk;
    const float *__restrict__ vr = hw.vbuf[list] + (size_t)c * D + hh * dk;
    const float inv = 1.f / sqrtf((float)dk);
    const int R = hw.heads * nctx;
    for (int k = tid; k < D; k += 256) {
        const float *__restrict__ wq = hw.q_wt + (size_t)k * D + hh * dk;      // q_wt is k-major: [in k][out j]
        float a = 0.f;
        for (int j = 0; j < dk; ++j) a = fmaf(wq[j], kr[j], a);
        hw.mqT[list][(size_t)k * R + r] = a * inv;
        float o = 0.f;
        for (int i = 0; i < dk; ++i) o = fmaf(hw.o_wt[(size_t)(hh * dk + i) * D + k], vr[i], o);   // o_wt: [in i][out j = k here]
        hw.noT[list][(size_t)r * D + k] = o;
    }
    if (tid == 0) {
        float a = 0.f;
        for (int j = 0; j < dk; ++j) a = fmaf(hw.q_b[hh * dk + j], kr[j], a);
        hw.mq_c[list][r] = a * inv;
    }
    if (hw.proj_wt == nullptr || hw.Hp > D) return;
    // ... and the predictor's projection composed in front: mqpT[i][r] = sum_k Wp[k][i] mqT[k][r]
    __syncthreads();                                          // this workgroup's column of mqT is complete
    __shared__ float mcol[1024];
    for (int k = tid; k < D; k += 256) mcol[k] = hw.mqT[list][(size_t)k * R + r];
    __syncthreads();
    for (int i = tid; i < hw.Hp; i += 256) {
        const float *__restrict__ wp = hw.proj_wt + (size_t)i * hw.proj_ld;
        float a = 0.f;
        for (int k = 0; k < D; ++k) a = fmaf(wp[k], mcol[k], a);
        hw.mqpT[list][(size_t)i * R + r] = a;
    }
    if (tid == 0) {
        float a = hw.mq_c[list][r];
        for (int k = 0; k < D; ++k) a = fmaf(hw.proj_b[k], mcol[k], a);
        hw.mqp_c[list][r] = a;
    }
}

// ContextBias.forward_predictor_bias (context_bias.py:375-381) for the lanes whose predictor has just stepped, with
// the list the gate selected (cur_gate: 1 = hot words, 0 = empty list -- greedy_search.py:357,394-395 evaluate the hot
// variant first and replace it when the gate says 0; only the one that reaches the joiner is computed here):
//   pb  = predictor_bias_bias_norm(MultiHeadedAttention(query = pred, key = value = bias_hidden))
//   out = predictor_bias_out_norm(predictor_bias_combine(cat(pred, pb)))
// One workgroup per lane; K / V of both lists were projected once per call (hw_kv_kernel).
__global__ __launch_bounds__(kHwThreads) void hw_bias_kernel(DevState *sp, HwDev hw)
{
    extern __shared__ float sm[];                   // x[D] q[D] ctx[D] o[D] pb[D] | part[16][D] | p[heads * max_ctx]
    __shared__ float sv[kHwThreads / 64];
    const int n = blockIdx.x, tid = threadIdx.x;
    // the lane's flags and (below) its LSTM output are requested through the kernel-argument pointers, beside the load of
    // the state block instead of behind it
    const int la = hw.lane_active[n], np = hw.need_pred[n], gate = hw.cur_gate[n];
    const float h_early = (hw.proj_wt != nullptr && tid < hw.Hp) ? hw.h_lastT[(size_t)tid * hw.NLp + n] : 0.f;   // Hp <= 1024 = threads
    const DevState S = *sp;
    const Dims &d = S.d;
    if (!la || !np) return;                                       // after a blank the predictor output is kept
    const int D = hw.D, g = gate ? 1 : 0;
    const int nctx = S.hw_nctx[g];
    const float *__restrict__ Kb = hw.kbuf[g];
    const float *__restrict__ Vb = hw.vbuf[g];
    float *x = sm, *q = sm + D, *ctx = sm + 2 * D, *o = sm + 3 * D, *pb = sm + 4 * D;
    float *part = sm + 5 * D, *p = part + (kHwThreads / 64) * D;
    // x = projection(h_last) (predictor.py:198): the lane's column of the k-major LSTM output through LDS
    // (stateless predictors have no projection: their kernels leave the output in outT)
    const bool short_list = nctx > 1 && hw.heads * nctx <= D;     // (a function of the call's list length: hw_fold_kernel ran)
    const bool composed = hw.proj_wt != nullptr && hw.Hp <= D && (short_list || (g == 0 && nctx == 1));
    float *hcol = pb;                                             // the lane's LSTM output (pb is free until the first LayerNorm)
    if (composed) {
        if (tid < hw.Hp) hcol[tid] = h_early;
        __syncthreads();
    } else if (hw.proj_wt != nullptr) {
        if (tid < hw.Hp) q[tid] = h_early;
        __syncthreads();
        block_gemv_kmajor(hw.proj_wt, hw.proj_ld, hw.proj_b, q, hw.Hp, hw.P, part, x);
    } else {
        for (int j = tid; j < D; j += kHwThreads) x[j] = S.outT[(size_t)j * d.NLp + n];
        __syncthreads();
    }
    if (g == 0 && nctx == 1) {
        // The empty list has ONE entry: softmax over one score is exactly 1, the context is exactly that entry's value
        // row, so the bias feature -- and the second half of the combine Linear applied to it -- is the same vector
        // for every step of the call (hw_cold_kernel computed it once).  Only the first half depends on the predictor.
        if (composed) block_gemv_kmajor(hw.c1p_wt, D, hw.cold_cp, hcol, hw.Hp, D, part, ctx);
        else block_gemv_kmajor(hw.c_wt, D, hw.cold_c, x, D, D, part, ctx);
        block_layer_norm(ctx, D, hw.on_w, hw.on_b, sv, [&](int j, float v) { S.biasT[(size_t)j * d.NLp + n] = v; });
        return;
    }
    if (short_list) {
        // short list: scores and the attention output as ONE matrix-vector product each (folded projections, HwDev)
        const int R = hw.heads * nctx;
        if (composed) {
            block_gemv_kmajor(hw.mqpT[g], R, hw.mqp_c[g], hcol, hw.Hp, R, part, p);
            block_gemv_kmajor(hw.c1p_wt, D, hw.c1p_b, hcol, hw.Hp, D, part, q);   // first half of the combine Linear
        } else {
            block_gemv_kmajor(hw.mqT[g], R, hw.mq_c[g], x, D, R, part, p);
            block_gemv_kmajor(hw.c_wt, D, hw.c_b, x, D, D, part, q);        // first half of the combine Linear (needs x only)
        }
        {   // softmax over the list, one wave per head (torch.softmax: exp(x - max) / sum)
            const int lane = tid & 63, wave = tid >> 6;
            for (int hh = wave; hh < hw.heads; hh += kHwThreads / 64) {
                float mx = -3.0e38f;
                for (int c = lane; c < nctx; c += 64) mx = fmaxf(mx, p[hh * nctx + c]);
                mx = wave_max(mx);
                float ssum = 0.f;
                for (int c = lane; c < nctx; c += 64) { const float e = expf(p[hh * nctx + c] - mx); p[hh * nctx + c] = e; ssum += e; }
                ssum = wave_sum(ssum);
                for (int c = lane; c < nctx; c += 64) p[hh * nctx + c] = p[hh * nctx + c] / ssum;
            }
        }
        __syncthreads();
        block_gemv_kmajor(hw.noT[g], D, hw.o_b, p, R, D, part, o);
        block_layer_norm(o, D, hw.bn_w, hw.bn_b, sv, [&](int j, float v) { pb[j] = v; });
        block_gemv_kmajor(hw.c_wt + (size_t)D * D, D, q, pb, D, D, part, ctx);
        block_layer_norm(ctx, D, hw.on_w, hw.on_b, sv, [&](int j, float v) { S.biasT[(size_t)j * d.NLp + n] = v; });
        return;
    }
    block_gemv_kmajor(hw.q_wt, D, hw.q_b, x, D, D, part, q);         // linear_q
    // scores[h][c] = q_h . k_{c,h} / sqrt(d_k)   (attention.py:185): four threads per (head, entry) pair, each a
    // quarter of the head's d_k elements with its loads in flight together, summed across the quad by DPP
    const int dk = D / hw.heads;
    const float sq = sqrtf((float)dk);
    {
        const int quarter = (dk + 3) / 4, sub = tid & 3;
        for (int pr0 = 0; pr0 < hw.heads * nctx; pr0 += kHwThreads / 4) {
            const int idx = pr0 + (tid >> 2);
            const bool on = idx < hw.heads * nctx;
            const int hh = on ? idx / nctx : 0, c = on ? idx - hh * nctx : 0;
            const float *__restrict__ kr = Kb + (size_t)c * D + hh * dk;
            const float *qh = q + hh * dk;
            float acc = 0.f;
#pragma unroll 16
            for (int i = 0; i < quarter; ++i) {
                const int e = sub * quarter + i;
                const float kv = kr[e < dk ? e : dk - 1];
                acc = fmaf(e < dk ? qh[e] : 0.f, kv, acc);
            }
            acc += __shfl_xor(acc, 1, kWave);
            acc += __shfl_xor(acc, 2, kWave);
            if (on && sub == 0) p[idx] = acc / sq;
        }
    }
    __syncthreads();
    {   // softmax over the list, one wave per head (torch.softmax: exp(x - max) / sum)
        const int lane = tid & 63, wave = tid >> 6;
        for (int hh = wave; hh < hw.heads; hh += kHwThreads / 64) {
            float mx = -3.0e38f;
            for (int c = lane; c < nctx; c += 64) mx = fmaxf(mx, p[hh * nctx + c]);
            mx = wave_max(mx);
            float ssum = 0.f;
            for (int c = lane; c < nctx; c += 64) { const float e = expf(p[hh * nctx + c] - mx); p[hh * nctx + c] = e; ssum += e; }
            ssum = wave_sum(ssum);
            for (int c = lane; c < nctx; c += 64) p[hh * nctx + c] = p[hh * nctx + c] / ssum;
        }
    }
    __syncthreads();
    {   // context = attn @ v: the list split four ways over the thread block, partial sums through LDS
        constexpr int SPL = 4;
        const int per = kHwThreads / SPL;                            // 256 columns per pass
        const int sgrp = tid / per, jj = tid - sgrp * per;
        for (int j0 = 0; j0 < D; j0 += per) {
            const int j = j0 + jj;
            const int jc = j < D ? j : D - 1, hh = jc / dk;
            float acc = 0.f;
#pragma unroll 8
            for (int c = sgrp; c < nctx; c += SPL) acc = fmaf(p[hh * nctx + c], Vb[(size_t)c * D + jc], acc);
            if (j < D) part[sgrp * D + j] = acc;
        }
        __syncthreads();
        for (int j = tid; j < D; j += kHwThreads) ctx[j] = (part[j] + part[D + j]) + (part[2 * D + j] + part[3 * D + j]);
    }
    __syncthreads();
    block_gemv_kmajor(hw.o_wt, D, hw.o_b, ctx, D, D, part, o);       // linear_out
    block_layer_norm(o, D, hw.bn_w, hw.bn_b, sv, [&](int j, float v) { pb[j] = v; });
    // combine over cat(pred, pb): two K segments of the k-major [2D][D] weight; q / ctx are free again
    block_gemv_kmajor(hw.c_wt, D, hw.c_b, x, D, D, part, q);
    block_gemv_kmajor(hw.c_wt + (size_t)D * D, D, q, pb, D, D, part, ctx);   // "bias" = the first segment's sums
    block_layer_norm(ctx, D, hw.on_w, hw.on_b, sv, [&](int j, float v) { S.biasT[(size_t)j * d.NLp + n] = v; });
}

// One-entry empty list (the reference's `context_list_empty`, greedy_search.py:328-333): its attention output does not
// depend on the query, so   cold_c = predictor_bias_combine[:, D:] . predictor_bias_bias_norm(linear_out(v_0)) + bias
// is computed once per call.
__global__ __launch_bounds__(kHwThreads) void hw_cold_kernel(HwDev hw)
{
    extern __shared__ float sm[];                   // v[D] o[D] pb[D] | part[16][D]
    __shared__ float sv[kHwThreads / 64];
    const int D = hw.D, tid = threadIdx.x;
    float *v = sm, *o = sm + D, *pb = sm + 2 * D, *part = sm + 3 * D;
    for (int j = tid; j < D; j += kHwThreads) v[j] = hw.vbuf[0][j];
    __syncthreads();
    block_gemv_kmajor(hw.o_wt, D, hw.o_b, v, D, D, part, o);
    block_layer_norm(o, D, hw.bn_w, hw.bn_b, sv, [&](int j, float val) { pb[j] = val; });
    block_gemv_kmajor(hw.c_wt + (size_t)D * D, D, hw.c_b, pb, D, D, part, o);
    for (int j = tid; j < D; j += kHwThreads) {
        hw.cold_c[j] = o[j];
        if (hw.proj_wt != nullptr && hw.Hp <= D) hw.cold_cp[j] = o[j] + (hw.c1p_b[j] - hw.c_b[j]);   // + combine[:, :D] . bp
    }
}

__global__ void greedy_hw_init_kernel(DevState *s)
{
    const Dims &d = s->d;
    const int n = blockIdx.x;
    const int tid = threadIdx.x;
    for (int i = tid; i < d.L * d.Hp; i += blockDim.x) {
        const size_t o = (size_t)i * d.NLp + n;
        s->cache_hT[o] = 0.f; s->cache_cT[o] = 0.f; s->new_hT[o] = 0.f; s->new_cT[o] = 0.f;
    }
    if (tid == 0) {
        const int T = s->enc_lens[n] < s->T ? s->enc_lens[n] : s->T;
        s->token[n] = s->blank;
        s->lane_t[n] = 0;
        s->noblk[n] = 0;
        s->need_pred[n] = 1;
        s->new_is_cache[n] = 0;
        s->hyp_lens[n] = 0;
        const int act = T > 0;
        s->lane_active[n] = act;
        if (act) atomicAdd(s->active_count, 1);
        // gate of the first predictor step (frame 0): nothing to go back to yet (greedy_search.py:365-368,386)
        int gate = 1;
        if (act && s->hw_filter && s->gate_tab[(size_t)n * s->T] == 0) gate = 0;
        s->cur_gate[n] = gate;
        s->gb_flag[n] = 0; s->gb_end[n] = -1; s->last_t[n] = 0;
        if (act && s->trace_cap > 0) s->trace[(size_t)n * s->trace_cap] = gate;
        s->trace_len[n] = act ? 1 : 0;
    }
    first_predictor_input(s, n);
}

// ------------------------------------------------------------------ beam --
// 64-bit running hash of a hypothesis' token sequence (kept per hypothesis, extended by one token per emission)
__device__ __forceinline__ unsigned long long hyp_hash_push(unsigned long long h, int tok)
{
    return (h ^ (unsigned long long)(unsigned)(tok + 1)) * 0x100000001b3ull + 0x9e3779b97f4a7c15ull;
}

__global__ void beam_init_kernel(DevState *s)
{
    const Dims &d = s->d;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int b = n / s->beam, j = n % s->beam;
    if (s->bs_flags && !(s->bs_flags[b] & 1)) return;      // a chunk call starts only the streams it resets
    for (int i = tid; i < d.L * d.Hp; i += blockDim.x) {
        const size_t o = (size_t)i * d.NLp + n;
        s->cache_hT[o] = 0.f; s->cache_cT[o] = 0.f;
        s->new_hT[o] = 0.f; s->new_cT[o] = 0.f;
    }
    if (tid == 0) {
        const int T = s->enc_lens[b] < s->T ? s->enc_lens[b] : s->T;
        s->token[n] = s->blank;
        s->lane_t[n] = 0;
        s->need_pred[n] = 1;
        s->lane_active[n] = (j == 0 && T > 0);
        s->bhyp_lens[(size_t)b * s->beam + j] = (j == 0) ? 1 : 0;
        s->bhyps[((size_t)b * s->beam + j) * s->Lmax] = s->blank;
        s->bhash[n] = hyp_hash_push(0ull, s->blank);
        if (s->btags) {                            // a biased stream: at the root, no bonus, the seed's tag slot
            s->bctx_state[(size_t)b * s->beam + j] = 0;
            s->bctx_score[(size_t)b * s->beam + j] = 0.0;
            s->btags[((size_t)b * s->beam + j) * s->Lmax] = -1;
        }
        if (j == 0) {
            s->n_hyps[b] = 1;
            s->frame[b] = 0;
            s->hyp_sel[b] = 0;
            s->bscores[(size_t)b * s->beam] = 0.0;
        }
    }
    first_predictor_input(s, n);
}

// per lane: log-softmax, mixture with the CTC posterior of this frame, top-`beam`.  One 512-thread workgroup per lane
// (round 2: 256 threads with 24 classes each; 1 024 threads were tried too: the transcendentals shrink with the classes
// per thread, the fixed cost of a selection round -- two DPP reductions per wave -- grows with the waves per SIMD).  The row lives in registers; every wave extracts the top-`beam` of its part with
// wave-local argmax rounds (DPP, no barriers), wave 0 merges the 16 x beam survivors.  Ties go to the lowest index
// throughout.
constexpr int kTopkThreads = 512;
// What both top-k kernels do with a row in registers (xv: the Vn token columns, strided over the workgroup; cv: the CTC
// posterior's row beside it): its block maximum m, ls = log sum exp(x - m), then the mixture (CTC_OPT = false: always; true:
// only if has_ctc) and `beam` wave-local argmax rounds (DPP, no barriers): wave w's k-th best into wv / wi[w * beam + k].
// The loads stay in the kernels: issued from a helper of any form they cost the <32> instantiations 26 to 33 VGPRs and a
// wave per SIMD (profiles/decode_twins_ab.md).
template <int NV>
__device__ __forceinline__ float topk_row_max(const float (&xv)[NV], int Vn, int tid, float *sv)
{
    float m = -3.0e38f;
#pragma unroll
    for (int i = 0; i < NV; ++i) m = fmaxf(m, (tid + i * kTopkThreads < Vn) ? xv[i] : -3.0e38f);
    return block_max(m, sv);
}
template <int NV>
__device__ __forceinline__ float topk_row_log_sum(const float (&xv)[NV], float m, int Vn, int tid, float *sv)
{
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) sum += (tid + i * kTopkThreads < Vn) ? expf(xv[i] - m) : 0.f;
    return logf(block_sum(sum, sv));
}
template <int NV, bool CTC_OPT>
__device__ __forceinline__ void topk_mix_select(const DevState &S, float (&xv)[NV], const float (&cv)[NV], float m, float ls, bool has_ctc,
                                                int Vn, int tid, float *wv, int *wi)
{
    const float ninf = -__builtin_huge_valf();
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const float l = (xv[i] - m) - ls;
        // prefix_beam_search.py:99-101: log(tw * exp(logp) + cw * exp(ctc[i]))
        const float mix = (!CTC_OPT || has_ctc) ? logf(S.tr_weight * expf(l) + S.ctc_weight * expf(cv[i])) : l;
        xv[i] = (tid + i * kTopkThreads < Vn) ? mix : ninf;
    }
    const int lane = tid & 63, wave = tid >> 6;
    for (int k = 0; k < S.beam; ++k) {
        float best = ninf;
        int bi = 0x7fffffff;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (xv[i] > best) { best = xv[i]; bi = tid + i * kTopkThreads; }   // ascending scan: lowest index wins ties
        wave_argmax_dpp(best, bi);
        if (lane == 0) { wv[wave * S.beam + k] = best; wi[wave * S.beam + k] = bi; }
        if (bi != 0x7fffffff && (bi % kTopkThreads) == tid) {                     // taken
#pragma unroll
            for (int i = 0; i < NV; ++i)
                if (i == bi / kTopkThreads) xv[i] = ninf;
        }
    }
}

// wave 0 merges the waves' survivors (wv / wi, after a barrier): kth(k, best, bi) for k = 0 .. beam-1 in descending order,
// every lane of the wave holding the k-th best value and its index; ties go to the lower index
template <typename F>
__device__ __forceinline__ void topk_merge(const float *wv, const int *wi, int beam, int lane, F &&kth)
{
    constexpr int NW = kTopkThreads / 64;
    constexpr int PM = NW * kMaxBeam / 64;          // survivors per lane of wave 0
    const float ninf = -__builtin_huge_valf();
    const int total = NW * beam;
    float c0[PM];
    int ci[PM];
#pragma unroll
    for (int q = 0; q < PM; ++q) {
        const int j = lane + q * 64;
        c0[q] = j < total ? wv[j] : ninf;
        ci[q] = j < total ? wi[j] : 0x7fffffff;
    }
    for (int k = 0; k < beam; ++k) {
        float best = ninf;
        int bi = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < PM; ++q)
            if (c0[q] > best || (c0[q] == best && ci[q] < bi)) { best = c0[q]; bi = ci[q]; }
        wave_argmax_dpp(best, bi);
        kth(k, best, bi);
#pragma unroll
        for (int q = 0; q < PM; ++q)
            if (ci[q] == bi) c0[q] = ninf;
    }
}

template <int NV>
__global__ __launch_bounds__(kTopkThreads) void beam_topk_kernel(DevState *sp)
{
    constexpr int NW = kTopkThreads / 64;
    __shared__ float sv[NW], wv[NW * kMaxBeam];
    __shared__ int wi[NW * kMaxBeam];
    WR_STAMP_DECL;
    WR_STAMP_RT(7);
    WR_STAMP(0);
    const DevState S = *sp;
    const Dims &d = S.d;
    const int n = blockIdx.x, tid = threadIdx.x;
    // no branch before the loads: the lane's scalars and both rows are requested in one batch (idle lanes leave
    // after the first reduction)
    const int act = S.lane_active[n];
    const int b = n / S.beam;
    int fr = S.frame[b];
    fr = fr < S.T ? fr : S.T - 1;
    const float *__restrict__ x = S.logits + (size_t)n * d.V;
    const float *__restrict__ cp = S.ctc_logp + ((size_t)b * S.T + fr) * d.V;
    float xv[NV], cv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * kTopkThreads;
        xv[i] = x[v < d.V ? v : d.V - 1];
        cv[i] = cp[v < d.V ? v : d.V - 1];
    }
    const float m = topk_row_max(xv, d.V, tid, sv);
    WR_STAMP(1);                                   // rows arrived, first reduction done
    if (!act) return;
    const float ls = topk_row_log_sum(xv, m, d.V, tid, sv);
    WR_STAMP(2);
    topk_mix_select<NV, false>(S, xv, cv, m, ls, true, d.V, tid, wv, wi);
    // touch the next frame's CTC row (one word per 128-byte line) so that it is already in the Infinity Cache and
    // its translation cached when the next micro-step asks for it
    if (fr + 1 < S.T && tid * 32 < d.V) {
        const float touch = cp[(size_t)d.V + tid * 32];
        asm volatile("" ::"v"(touch));
    }
    WR_STAMP(3);                                   // per-wave selection rounds done
    __syncthreads();
    WR_STAMP(4);
    if (tid < 64)
        topk_merge(wv, wi, S.beam, tid, [&](int k, float best, int bi) {
            if (tid == 0) {
                S.topv[(size_t)n * S.beam + k] = best;
                S.topi[(size_t)n * S.beam + k] = (bi < d.V) ? bi : 0;
            }
        });
    WR_STAMP(5);
    WR_STAMP_DRAIN();
    WR_STAMP(6);
    WR_STAMP_RT(8);
    WR_STAMP_FLUSH(6);
}

__device__ __forceinline__ double log_add2(double a, double b)
{
    // wenet/utils/common.py:268-276 for two arguments, float64
    const double ninf = -__builtin_huge_val();
    if (a == ninf && b == ninf) return ninf;
    // mx + log(exp(a - mx) + exp(b - mx)): the larger argument contributes exp(0.0) = 1.0 exactly, so one exp suffices
    // (the sum is the same two addends in either order)
    const double mx = a > b ? a : b, mn = a > b ? b : a;
    return mx + log(1.0 + exp(mn - mx));
}

// one workgroup per utterance: expansion, prefix fusion, stable prune (prefix_beam_search.py:107-146).
// One candidate (hypothesis j, rank t) per thread; the all-pairs steps (which candidates spell the same token
// sequence, where a class ranks) run pair-per-thread.  Sequences are compared through their running hashes and
// verified token by token only when the hashes agree, so fusion is exact.  Then the survivors' hypotheses,
// predictor caches and next input embeddings are moved into place (rows of the k-major caches are independent,
// so each batch of rows is read into registers, synchronised and written back in place).
constexpr int kBeamUpdThreads = 1024;   // one workgroup per utterance; 256 threads in round 2 (the all-pairs steps and the
                                        // layer-0 cells of the survivors are 4 x as parallel now)
// The workgroup's LDS record of the candidates (c_*, f_score) and of the pruned beam (order, e_*) that the shared phases
// below work on; both update kernels fill c_* and e_lb in their own phase 1.
struct BeamUpdLds {
    static constexpr int MC = kMaxBeam * kMaxBeam;
    double c_score[MC], f_score[MC];
    unsigned long long c_hash[MC];
    int c_base[MC], c_tok[MC], c_len[MC], c_last[MC], c_rep[MC], c_rank[MC], order[kMaxBeam];
    int e_src[kMaxBeam], e_blank[kMaxBeam], e_tok[kMaxBeam], e_last[kMaxBeam], e_lb[kMaxBeam];
    // TIMES (the streaming search) only: a candidate's Viterbi score -- after beam_fuse_scores a representative's is its
    // class's maximum and c_vbest the member that holds it -- and, per survivor, that member's base hypothesis (whose times
    // it takes) and whether the member appended a token
    double c_vscore[MC];
    int c_vbest[MC], e_vsrc[kMaxBeam], e_vapp[kMaxBeam];
};

// CTX (include/wr_api.h, "Context-graph biasing in the streaming transducer prefix beam search"): the record of the biased
// instantiations, which alone carry these arrays in their LDS.  A candidate's graph state, bonus and the tag of the token it
// appended; all members of a class agree on them (they are a function of the tokens), so the representative's are the
// class's.  e_ctag: the tag a survivor appends.
struct BeamCtxLds : BeamUpdLds {
    double c_cscore[MC];
    int c_cstate[MC], c_ctag[MC], e_ctag[kMaxBeam];
};
template <bool CTX>
using BeamLds = std::conditional_t<CTX, BeamCtxLds, BeamUpdLds>;

// The graph state, bonus and tag of candidate `c`, which extends entry `entry` of the beam by `tok` (context_graph.hpp); a
// negative `tok` appends nothing and copies the entry's fields.
//
// The walk is context_graph_next of context_graph.hpp (same clamps, same search) with the float64 add done inside each
// branch.  It stays a body of its own here: with the shared one the biased stream measured slower at equal registers,
// LDS and occupancy (profiles/context_twins_ab.md, "Time against the parent").
__device__ __forceinline__ void ctx_graph_next(const ContextGraph &g, int state, double score, int tok, int *st_out,
                                               double *sc_out, int *tag_out)
{
    const int ns = g.S, na = g.A;
    state = state < 0 ? 0 : (state < ns ? state : ns - 1);
    int lo = g.arc_begin[state], hi = g.arc_begin[state + 1];
    lo = lo < 0 ? 0 : (lo < na ? lo : na);
    hi = hi < lo ? lo : (hi < na ? hi : na);
    const int end = hi;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (g.arc_token[mid] < tok) lo = mid + 1; else hi = mid;
    }
    if (lo < end && g.arc_token[lo] == tok) {
        int nx = g.arc_next[lo];
        nx = nx < 0 ? 0 : (nx < ns ? nx : ns - 1);
        *st_out = nx;
        *sc_out = score + (double)g.arc_score[lo];
        *tag_out = (state == 0 ? 1 : 0) | (g.final_[nx] != 0 ? 2 : 0);
    } else {
        *st_out = 0;
        *sc_out = score + (double)g.escape[state];
        *tag_out = 0;
    }
}

__device__ __forceinline__ void beam_ctx_candidate(const DevState &S, BeamCtxLds &L, int c, size_t entry, int tok)
{
    int cst = S.bctx_state[entry], ctag = 0;
    double csc = S.bctx_score[entry];
    if (tok >= 0) ctx_graph_next(S.cg, cst, csc, tok, &cst, &csc, &ctag);
    L.c_cstate[c] = cst;
    L.c_cscore[c] = csc;
    L.c_ctag[c] = ctag;
}

// phase 2: class representative = the first candidate with the same token sequence (:130-142) -- and, WITH_FRAME, the same
// frame c_t (c_t is not read otherwise)
template <bool WITH_FRAME>
__device__ __forceinline__ void beam_find_classes(BeamUpdLds &L, const int *c_t, const int32_t *__restrict__ hy, int Lmax, int C, int tid)
{
    for (int p = tid; p < C * C; p += kBeamUpdThreads) {
        const int i = p / C, f = p - i * C;
        if (f >= i || (WITH_FRAME && c_t[f] != c_t[i]) || L.c_hash[f] != L.c_hash[i] || L.c_len[f] != L.c_len[i] || L.c_last[f] != L.c_last[i]) continue;
        // equal hashes, lengths and last tokens: the sequences are equal iff the first len-1 tokens of the two base
        // hypotheses are (both bases hold at least that many); compared in batches of independent loads
        const int32_t *__restrict__ pi = hy + (size_t)L.c_base[i] * Lmax;
        const int32_t *__restrict__ pf = hy + (size_t)L.c_base[f] * Lmax;
        const int ncmp = L.c_len[i] - 1;
        bool same = true;
        constexpr int UC = 16;
        for (int q0 = 0; q0 < ncmp && same; q0 += UC) {
            int xa[UC], ya[UC];
#pragma unroll
            for (int u = 0; u < UC; ++u) {
                const int q = q0 + u < ncmp ? q0 + u : ncmp - 1;
                xa[u] = pi[q];
                ya[u] = pf[q];
            }
#pragma unroll
            for (int u = 0; u < UC; ++u) same = same && (xa[u] == ya[u]);
        }
        if (same) atomicMin(&L.c_rep[i], f);
    }
    __syncthreads();
}

// phase 3: a representative accumulates its duplicates' scores in candidate order with float64 log_add
// (a float64 exp + log is ~2 us of dependent instructions and a wave runs it for one lane at a time: consecutive
// candidates sit in different waves, so that the few duplicates of a frame are summed side by side)
// Most frames have no duplicate at all: then the fused scores are the candidates' own (one count over the workgroup
// instead of every candidate scanning all later ones).
// TIMES: beside the sum, the class's Viterbi score -- the maximum of its members' c_vscore, an exact tie to the first in
// pool order -- and the member holding it (c_vbest); only a representative's own c_vscore is rewritten, which no other
// thread reads.
template <bool TIMES>
__device__ __forceinline__ void beam_fuse_scores(BeamUpdLds &L, int C, int tid)
{
    const int n_dup = __syncthreads_count(tid < C && L.c_rep[tid] != tid);
    if (n_dup == 0) {
        if (tid < C) {
            L.f_score[tid] = L.c_score[tid];
            if (TIMES) L.c_vbest[tid] = tid;
        }
    } else {
        const int c = (tid & 63) * (kBeamUpdThreads / 64) + (tid >> 6);
        if (c < C) {
            double sc = L.c_score[c];
            double vb = TIMES ? L.c_vscore[c] : 0.0;
            int vi = c;
            if (L.c_rep[c] == c) {
#pragma unroll 8
                for (int f = c + 1; f < C; ++f)
                    if (L.c_rep[f] == c) {
                        sc = log_add2(sc, L.c_score[f]);
                        if (TIMES && L.c_vscore[f] > vb) { vb = L.c_vscore[f]; vi = f; }
                    }
                if (TIMES) { L.c_vscore[c] = vb; L.c_vbest[c] = vi; }
            }
            L.f_score[c] = sc;
        }
    }
    __syncthreads();
}

// phase 4: stable descending sort position among representatives (list.sort(reverse=True) keeps order on ties), the prune
// to `beam`, and the survivors' record: e_* in LDS, length / score / hash / next predictor input of lane b * beam + rank.
// not_appended(c_tok) says whether a candidate added no token to its base.  Returns the survivor count; the caller
// synchronises before anyone reads e_*.  Called once per kernel: the count lives in s_keep, zeroed here behind the barrier.
// TIMES: also the survivor's Viterbi score, and whose times it takes (e_vsrc, e_vapp).
// CTX (implies TIMES): the rank is by total = fused score + bonus, one float64 add; the stored score stays the fused one, and
// the survivor's graph state, bonus and the tag it appends (e_ctag) are the representative's.
template <bool TIMES, bool CTX = false, typename F>
__device__ __forceinline__ int beam_rank_prune(const DevState &S, BeamLds<CTX> &L, int32_t *__restrict__ hl2, int b, int C, int tid, F &&not_appended)
{
    static_assert(!CTX || TIMES, "the biased search is a streaming search");
    __shared__ int s_keep;
    const int beam = S.beam;
    if (tid == 0) s_keep = 0;
    for (int p = tid; p < C * C; p += kBeamUpdThreads) {
        const int i = p / C, f = p - i * C;
        if (L.c_rep[i] != i || L.c_rep[f] != f) continue;
        double me = L.f_score[i], ot = L.f_score[f];
        if constexpr (CTX) { me += L.c_cscore[i]; ot += L.c_cscore[f]; }
        if (ot > me || (ot == me && f < i)) atomicAdd(&L.c_rank[i], 1);
    }
    __syncthreads();
    if (tid < C && L.c_rep[tid] == tid) {
        if (L.c_rank[tid] < beam) L.order[L.c_rank[tid]] = tid;
        atomicAdd(&s_keep, 1);
    }
    __syncthreads();
    const int keep = s_keep < beam ? s_keep : beam;
    if (tid < keep) {
        const int f = L.order[tid];
        L.e_src[tid] = L.c_base[f];
        L.e_tok[tid] = L.c_tok[f];
        L.e_blank[tid] = not_appended(L.c_tok[f]);
        L.e_last[tid] = L.c_last[f];
        hl2[tid] = L.c_len[f];
        S.bscores[(size_t)b * beam + tid] = L.f_score[f];
        S.bhash[b * beam + tid] = L.c_hash[f];
        S.token[b * beam + tid] = L.c_last[f];     // next frame's predictor input: last token of the hypothesis (:78-80)
        if (TIMES) {
            const int vb = L.c_vbest[f];
            L.e_vsrc[tid] = L.c_base[vb];
            L.e_vapp[tid] = !not_appended(L.c_tok[vb]);
            S.bvscores[(size_t)b * beam + tid] = L.c_vscore[f];
        }
        if constexpr (CTX) {
            S.bctx_state[(size_t)b * beam + tid] = L.c_cstate[f];
            S.bctx_score[(size_t)b * beam + tid] = L.c_cscore[f];
            L.e_ctag[tid] = L.c_ctag[f];
        }
    }
    return keep;
}

// phase 5: the pruned beam -- hypotheses into the other buffer, (survivor, position) pairs in flight together.
// TIMES: and each survivor's times (tm -> tm2, laid out like the hypotheses) from the base of its class's Viterbi-best
// member, which need not be e_src; a member that appended a token appends `frame`, the frame it was expanded at.
// CTX: and each survivor's tags (tg -> tg2, laid out likewise) from e_src, the representative's base -- the tags are a function
// of the tokens, so they travel with the hypothesis, not with the Viterbi-best member; a survivor that appended a token
// appends e_ctag.
template <bool TIMES, bool CTX = false>
__device__ __forceinline__ void beam_move_hyps(const BeamLds<CTX> &L, const int32_t *__restrict__ hy, int32_t *__restrict__ hy2, int Lmax, int keep, int tid,
                                               const int32_t *__restrict__ tm = nullptr, int32_t *__restrict__ tm2 = nullptr, int frame = 0,
                                               const int32_t *__restrict__ tg = nullptr, int32_t *__restrict__ tg2 = nullptr)
{
    constexpr int NT = kBeamUpdThreads;
    int maxlb = 0;
    for (int e = 0; e < keep; ++e) maxlb = L.e_lb[L.e_src[e]] > maxlb ? L.e_lb[L.e_src[e]] : maxlb;
    constexpr int UN = 4;
    for (int i0 = 0; i0 < keep * maxlb; i0 += NT * UN) {
        int val[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int i = i0 + u * NT + tid;
            const int e = i / maxlb, q = i - e * maxlb;
            const bool in = e < keep && q < L.e_lb[L.e_src[e < keep ? e : 0]];
            val[u] = in ? hy[(size_t)L.e_src[e] * Lmax + q] : 0;
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int i = i0 + u * NT + tid;
            const int e = i / maxlb, q = i - e * maxlb;
            if (e < keep && q < L.e_lb[L.e_src[e]]) hy2[(size_t)e * Lmax + q] = val[u];
        }
    }
    if (tid < keep) {
        const int lb = L.e_lb[L.e_src[tid]];
        if (!L.e_blank[tid] && lb < Lmax) hy2[(size_t)tid * Lmax + lb] = L.e_tok[tid];
    }
    if (TIMES) {
        int maxlv = 0;
        for (int e = 0; e < keep; ++e) maxlv = L.e_lb[L.e_vsrc[e]] > maxlv ? L.e_lb[L.e_vsrc[e]] : maxlv;
        for (int i = tid; i < keep * maxlv; i += NT) {
            const int e = i / maxlv, q = i - e * maxlv;
            if (q < L.e_lb[L.e_vsrc[e]]) tm2[(size_t)e * Lmax + q] = tm[(size_t)L.e_vsrc[e] * Lmax + q];
        }
        if (tid < keep) {
            const int lv = L.e_lb[L.e_vsrc[tid]];
            if (L.e_vapp[tid] && lv < Lmax) tm2[(size_t)tid * Lmax + lv] = frame;
        }
    }
    if constexpr (CTX) {
        for (int i = tid; i < keep * maxlb; i += NT) {
            const int e = i / maxlb, q = i - e * maxlb;
            if (q < L.e_lb[L.e_src[e]]) tg2[(size_t)e * Lmax + q] = tg[(size_t)L.e_src[e] * Lmax + q];
        }
        if (tid < keep) {
            const int lb = L.e_lb[L.e_src[tid]];
            if (!L.e_blank[tid] && lb < Lmax) tg2[(size_t)tid * Lmax + lb] = L.e_ctag[tid];
        }
    }
}

// the survivors' predictor state and next predictor input.  A survivor that appended nothing (e_blank: a blank extension,
// or a hypothesis that waited) inherits its base hypothesis' committed state, a label the state the predictor stepped to.
__device__ __forceinline__ void beam_move_predictor(const DevState &S, const BeamUpdLds &L, int b, int keep, int tid)
{
    constexpr int NT = kBeamUpdThreads;
    const Dims &d = S.d;
    const int beam = S.beam;
    if (d.ptype == kPredLstm) {
        // LSTM predictor: a survivor inherits a slot NUMBER -- its base hypothesis' committed slot for a blank extension,
        // the slot of the base's new state for a label (:111-124; several survivors may share one; only an expanded base
        // has one) -- and gets a free slot of the utterance's 2 * beam for its own next step; then layer 0 of that step
        // (lstm_layer0_cell), whenever that step will be consulted.  Nothing is copied.  Slots of utterance b: lanes'
        // numbers b * beam + j and NLp + b * beam + j.
        __shared__ int s_comm[kMaxBeam], s_new[kMaxBeam], s_oc[kMaxBeam], s_on[kMaxBeam];
        if (tid < beam) { s_oc[tid] = S.comm_slot[b * beam + tid]; s_on[tid] = S.new_slot[b * beam + tid]; }
        __syncthreads();
        if (tid == 0) {
            unsigned used = 0;                                   // bit j: slot b*beam + j, bit beam + j: slot NLp + b*beam + j
            for (int e = 0; e < keep; ++e) {
                const int sl = L.e_blank[e] ? s_oc[L.e_src[e]] : s_on[L.e_src[e]];
                s_comm[e] = sl;
                used |= 1u << (sl >= d.NLp ? beam + (sl - d.NLp - b * beam) : sl - b * beam);
            }
            // every lane of the utterance, idle ones too, gets a free slot of its own: the recurrent-product jobs write
            // pool_g[new_slot[n]] for all lanes and must never land in a slot that is in use
            int bit = 0;
            for (int e = 0; e < beam; ++e) {
                while (used & (1u << bit)) ++bit;
                s_new[e] = bit < beam ? b * beam + bit : d.NLp + b * beam + (bit - beam);
                if (e >= keep) s_comm[e] = s_new[e];
                ++bit;
            }
        }
        __syncthreads();
        if (tid < beam) { S.comm_slot[b * beam + tid] = s_comm[tid]; S.new_slot[b * beam + tid] = s_new[tid]; }
        // layer 0 of every survivor's next step (lstm_layer0_cell), (survivor, unit) pairs spread over the workgroup with
        // the loads of two pairs per thread in flight together
        constexpr int UN = 2;
        const int items = keep * d.H;
        for (int i0 = 0; i0 < items; i0 += NT * UN) {
            float ev[UN][4], gv[UN][4], cv[UN];
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                const int i = i0 + q * NT + tid;
                const int e = i < items ? i / d.H : 0, u = i < items ? i - e * d.H : 0;
                const int col = (u >> 3) * 32 + (u & 7);
                const float *__restrict__ er = S.etab + (size_t)L.e_last[e] * d.G4p + col;
                const float *__restrict__ gr = S.pool_g + (size_t)s_comm[e] * d.G4p + col;
#pragma unroll
                for (int gt = 0; gt < 4; ++gt) { ev[q][gt] = er[gt * 8]; gv[q][gt] = gr[gt * 8]; }
                cv[q] = S.pool_c[(size_t)s_comm[e] * d.Hp + u];
            }
#pragma unroll
            for (int q = 0; q < UN; ++q) {
                const int i = i0 + q * NT + tid;
                if (i >= items) continue;
                const int e = i / d.H, u = i - e * d.H;
                const float ig = sigmoidf_(ev[q][0] + gv[q][0]);
                const float fg = sigmoidf_(ev[q][1] + gv[q][1]);
                const float gg = tanhf(ev[q][2] + gv[q][2]);
                const float og = sigmoidf_(ev[q][3] + gv[q][3]);
                const float c = __builtin_fmaf(ig, gg, fg * cv[q]);    // ig * gg fused, fg * c rounded: stated, not left to -ffp-contract
                S.pool_c[(size_t)s_new[e] * d.Hp + u] = c;
                S.new_hT[(size_t)u * d.NLp + b * beam + e] = og * tanhf(c);
            }
        }
        return;
    }
    // next predictor inputs
    constexpr int UI = 4;
    const float *__restrict__ emb = S.embed;
    for (int i0 = 0; i0 < keep * d.D; i0 += NT * UI) {
        float val[UI];
#pragma unroll
        for (int u = 0; u < UI; ++u) {
            const int i = i0 + u * NT + tid;
            const int e = i / d.D, k = i - e * d.D;
            val[u] = e < keep ? emb[(size_t)L.e_last[e] * d.D + k] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UI; ++u) {
            const int i = i0 + u * NT + tid;
            const int e = i / d.D, k = i - e * d.D;
            if (e < keep) S.xT[(size_t)k * d.NLp + b * beam + e] = val[u];
        }
    }
    // predictor caches (token histories): a blank extension keeps the base hypothesis' cache, a label takes the predictor's
    // new cache (:111-124).  Rows i of [L*Hp][NLp]; a thread owns (row, survivor) pairs, `beam` survivors per row; each
    // batch of rows is read into registers, synchronised and written back in place.
    constexpr int UN = 8;
    const int rows = d.L * d.Hp, per_it = NT / beam;           // rows per pass of the workgroup
    const int e = tid % beam, r0 = tid / beam;
    const bool on = e < keep && r0 < per_it;
    const int src = b * beam + (on ? L.e_src[e] : 0), dst = b * beam + e;
    const bool bl = on ? L.e_blank[e] != 0 : true;
    const float *hsrc = bl ? S.cache_hT : S.new_hT;
    const float *csrc = bl ? S.cache_cT : S.new_cT;
    for (int rb = 0; rb < rows; rb += per_it * UN) {
        float hv[UN], cw[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int r = rb + u * per_it + r0;
            const size_t so = (size_t)(r < rows ? r : 0) * d.NLp + src;
            hv[u] = hsrc[so];
            cw[u] = csrc[so];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int r = rb + u * per_it + r0;
            if (on && r < rows) {
                const size_t dst_o = (size_t)r * d.NLp + dst;
                S.cache_hT[dst_o] = hv[u];
                S.cache_cT[dst_o] = cw[u];
            }
        }
    }
}

// TIMES: the streaming form (wr_prefix_beam_search_chunk).  The frames of this chunk are T_b = F_b - base_b, frame[b] counts
// from the chunk's first frame, and every candidate carries a Viterbi score and its class the times of its best member.
// CTX: the biased form of it (wr_prefix_beam_search_context_chunk): a candidate that appends a token walks the context graph.
template <bool TIMES, bool CTX = false>
__global__ __launch_bounds__(kBeamUpdThreads) void beam_update_kernel(DevState *sp)
{
    __shared__ BeamLds<CTX> L;
    WR_STAMP_DECL;
    WR_STAMP_RT(7);
    WR_STAMP(0);
    const DevState S = *sp;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int beam = S.beam;
    const int T = TIMES ? S.bs_F[b] - S.bs_base[b] : (S.enc_lens[b] < S.T ? S.enc_lens[b] : S.T);
    const int fr = S.frame[b];
    if (fr >= T) return;
    const int N = S.n_hyps[b], C = N * beam;
    const int sel = S.hyp_sel[b];
    const size_t hstride = (size_t)S.n_utt * beam * S.Lmax;
    const int32_t *__restrict__ hy = S.bhyps + sel * hstride + (size_t)b * beam * S.Lmax;
    int32_t *__restrict__ hy2 = S.bhyps + (1 - sel) * hstride + (size_t)b * beam * S.Lmax;
    const int32_t *__restrict__ hl = S.bhyp_lens + (size_t)sel * S.n_utt * beam + (size_t)b * beam;
    int32_t *__restrict__ hl2 = S.bhyp_lens + (size_t)(1 - sel) * S.n_utt * beam + (size_t)b * beam;
    // phase 1: candidates in the reference's order (hypothesis-major, then top-k rank; :109-127)
    if (tid < kMaxBeam) L.e_lb[tid] = tid < N ? hl[tid] : 0;
    if (tid < C) {
        const int j = tid / beam, t = tid - j * beam;
        const int n = b * beam + j;
        const int tok = S.topi[(size_t)n * beam + t];
        // scores tensor is fp32 built from Python floats (:86); add in fp32 (:105); .item() -> float64 (:116)
        const float sj = (float)S.bscores[(size_t)b * beam + j];
        const float tv = S.topv[(size_t)n * beam + t];
        const int lb = hl[j];
        const int last = S.token[n];               // last token of hypothesis j (this frame's predictor input)
        const unsigned long long hh = S.bhash[n];
        L.c_score[tid] = (double)(sj + tv);
        if (TIMES) L.c_vscore[tid] = (double)((float)S.bvscores[(size_t)b * beam + j] + tv);
        L.c_base[tid] = j;
        L.c_tok[tid] = tok;
        L.c_len[tid] = lb + (tok != S.blank ? 1 : 0);
        L.c_last[tid] = (tok != S.blank) ? tok : last;
        L.c_hash[tid] = (tok != S.blank) ? hyp_hash_push(hh, tok) : hh;
        L.c_rep[tid] = tid;
        L.c_rank[tid] = 0;
        if constexpr (CTX) beam_ctx_candidate(S, L, tid, (size_t)b * beam + j, tok != S.blank ? tok : -1);   // a blank copies
    }
    __syncthreads();
    WR_STAMP(1);                                   // candidates built
    beam_find_classes<false>(L, nullptr, hy, S.Lmax, C, tid);
    WR_STAMP(2);                                   // classes known
    beam_fuse_scores<TIMES>(L, C, tid);
    WR_STAMP(9);                                   // duplicates' scores summed
    const int keep = beam_rank_prune<TIMES, CTX>(S, L, hl2, b, C, tid, [&](int tok) { return tok == S.blank; });
    __syncthreads();
    WR_STAMP(3);                                   // fused, ranked, pruned
    if constexpr (CTX)
        beam_move_hyps<true, true>(L, hy, hy2, S.Lmax, keep, tid, S.btimes + sel * hstride + (size_t)b * beam * S.Lmax,
                                   S.btimes + (1 - sel) * hstride + (size_t)b * beam * S.Lmax, S.bs_base[b] + fr,
                                   S.btags + sel * hstride + (size_t)b * beam * S.Lmax,
                                   S.btags + (1 - sel) * hstride + (size_t)b * beam * S.Lmax);
    else if (TIMES)
        beam_move_hyps<true>(L, hy, hy2, S.Lmax, keep, tid, S.btimes + sel * hstride + (size_t)b * beam * S.Lmax,
                             S.btimes + (1 - sel) * hstride + (size_t)b * beam * S.Lmax, S.bs_base[b] + fr);
    else
        beam_move_hyps<false>(L, hy, hy2, S.Lmax, keep, tid);
    WR_STAMP(4);                                   // hypotheses moved
    beam_move_predictor(S, L, b, keep, tid);
    if (tid < beam) {
        const int nfr = fr + 1;
        const int n = b * beam + tid;
        S.lane_active[n] = (tid < keep) && (nfr < T);
        S.lane_t[n] = nfr;
        S.need_pred[n] = 1;
        if (tid == 0) {
            S.n_hyps[b] = keep;
            S.frame[b] = nfr;
            S.hyp_sel[b] = 1 - sel;
        }
    }
    WR_STAMP(5);
    WR_STAMP_DRAIN();
    WR_STAMP(6);
    WR_STAMP_RT(8);
    WR_STAMP_FLUSH(7);
}

// -------------------------------------------------- token-and-duration beam --
// include/wr_api.h, "TDT prefix beam search".  The hypotheses of one utterance stand at different frames (lane_t[n]); only
// those at the earliest frame f = frame[b] are expanded in a step (lane_active), the others wait in the beam as they are.
// beam_init_kernel starts the lanes; this kernel counts the utterances that have a frame to decode and clears the
// statistics: active_count = {utterances running, utterance-steps taken, hypotheses expanded}.
__global__ void tdt_beam_begin_kernel(DevState *s)
{
    __shared__ int cnt;
    if (threadIdx.x == 0) cnt = 0;
    __syncthreads();
    int mine = 0;
    for (int b = threadIdx.x; b < s->n_utt; b += blockDim.x) mine += (s->enc_lens[b] > 0 && s->T > 0) ? 1 : 0;
    if (mine) atomicAdd(&cnt, mine);
    __syncthreads();
    if (threadIdx.x == 0) { s->active_count[0] = cnt; s->active_count[1] = 0; s->active_count[2] = 0; }
}

// per active lane: log-softmax of the V token columns of the row (stride Dims.V = V + D), mixture with the CTC posterior of
// the LANE's frame, top-`beam` tokens as in beam_topk_kernel; then the log-softmax of the D <= 9 duration columns in one
// wave and the best `beam` of the beam x D pairs (rank r, duration j) by mix[k_r] + ld[j], ties to the lower r, then the
// lower j.  Out: topv = the pair's value, topi = k | j << 16 (as tdt_rows_kernel packs a decision).
template <int NV>
__global__ __launch_bounds__(kTopkThreads) void tdt_beam_topk_kernel(DevState *sp)
{
    constexpr int NW = kTopkThreads / 64;
    __shared__ float sv[NW], wv[NW * kMaxBeam];
    __shared__ int wi[NW * kMaxBeam];
    const DevState S = *sp;
    const Dims &d = S.d;
    const int n = blockIdx.x, tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    // no branch before the loads (idle lanes leave after the first reduction)
    const int act = S.lane_active[n];
    const int b = n / S.beam;
    int fr = S.lane_t[n];
    fr = fr < S.T ? fr : S.T - 1;
    fr = fr > 0 ? fr : 0;
    const int D = S.tdt_D, Vt = d.V - D;
    const bool has_ctc = S.ctc_logp != nullptr;
    const float *__restrict__ x = S.logits + (size_t)n * d.V;
    const float *__restrict__ cp = has_ctc ? S.ctc_logp + ((size_t)b * S.T + fr) * Vt : x;
    const float ninf = -__builtin_huge_valf();
    float xv[NV], cv[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = tid + i * kTopkThreads;
        xv[i] = x[v < Vt ? v : Vt - 1];
        cv[i] = 0.f;
    }
    if (has_ctc) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = tid + i * kTopkThreads;
            cv[i] = cp[v < Vt ? v : Vt - 1];
        }
    }
    const float xd = x[Vt + (lane < D ? lane : 0)];           // the duration columns, one per lane of every wave
    const float m = topk_row_max(xv, Vt, tid, sv);
    if (!act) return;
    const float ls = topk_row_log_sum(xv, m, Vt, tid, sv);
    topk_mix_select<NV, true>(S, xv, cv, m, ls, has_ctc, Vt, tid, wv, wi);
    __syncthreads();
    if (wave != 0) return;
    // duration log-softmax: lanes 0 .. D-1 of this wave hold the columns
    const float dm = wave_allmax_dpp(lane < D ? xd : -3.0e38f);
    const float ds = wave_allsum_dpp(lane < D ? expf(xd - dm) : 0.f);
    const float ldv = (xd - dm) - logf(ds);
    constexpr int PP = (kMaxBeam * kTdtMaxD + 63) / 64;   // (rank, duration) pairs per lane: pair p = r * D + j at lane p % 64
    const int npair = S.beam * D;
    float pv[PP], pl[PP];
    int pk[PP];
#pragma unroll
    for (int q = 0; q < PP; ++q) {
        pl[q] = __shfl(ldv, (lane + q * 64) % D, kWave);
        pv[q] = ninf;
        pk[q] = 0;
    }
    topk_merge(wv, wi, S.beam, lane, [&](int k, float best, int bi) {
#pragma unroll
        for (int q = 0; q < PP; ++q) {
            const int p = lane + q * 64;
            if (p < npair && p / D == k) { pv[q] = best + pl[q]; pk[q] = bi < Vt ? bi : 0; }   // one fp32 add
        }
    });
    for (int c = 0; c < S.beam; ++c) {
        float best = ninf;
        int bp = 0x7fffffff;
#pragma unroll
        for (int q = 0; q < PP; ++q)
            if (pv[q] > best) { best = pv[q]; bp = lane + q * 64; }              // ascending p: lower r, then lower j
        wave_argmax_dpp(best, bp);
        if (bp == 0x7fffffff) {                    // nothing finite is left
            if (lane == 0) { S.topv[(size_t)n * S.beam + c] = ninf; S.topi[(size_t)n * S.beam + c] = 0; }
            continue;
        }
        if ((bp & 63) == lane) {
#pragma unroll
            for (int q = 0; q < PP; ++q)
                if (q == (bp >> 6)) {
                    S.topv[(size_t)n * S.beam + c] = best;
                    S.topi[(size_t)n * S.beam + c] = pk[q] | ((bp % D) << 16);
                    pv[q] = ninf;
                }
        }
    }
}

// one workgroup per utterance: the pool (a waiting hypothesis as it is, an active one's `beam` pairs), then the phases of
// beam_update_kernel with the frame as part of a class's key -- the first pool entry with the same tokens and the same frame
// represents the class and accumulates it in pool order (float64 log_add), stable prune, the survivors moved by
// beam_move_hyps / beam_move_predictor (a waiting survivor and a blank extension inherit the committed predictor state, a
// label the stepped one) -- then each survivor's frame, and which of them stand at the new earliest frame.
// MODE kTdtWhole: a step of wr_prefix_beam_search_tdt.  The streaming search (include/wr_api.h, "Streaming transducer prefix
// beam search"; frames count from the chunk's first, T = F_b - base_b, Viterbi scores and times are carried):
// kTdtStream, a step -- arcs are clamped to T only once the stream has had its final call; kTdtFinal, what a final call does
// before its first step -- nothing is expanded, every frame beyond T is clamped to T, and the beam is fused and re-sorted.
enum TdtUpdateMode { kTdtWhole = 0, kTdtStream = 1, kTdtFinal = 2 };
// CTX: the biased form of the two streaming modes; a label arc walks the context graph once, whatever its duration.
template <int MODE, bool CTX = false>
__device__ __forceinline__ void tdt_beam_update(const DevState &S, BeamLds<CTX> &L, int b)
{
    constexpr bool TIMES = MODE != kTdtWhole;
    __shared__ int c_t[BeamUpdLds::MC], e_t[kMaxBeam], p_t[kMaxBeam], p_off[kMaxBeam + 1], s_nact, s_fnext;
    const int tid = threadIdx.x;
    const int beam = S.beam;
    const int T = TIMES ? S.bs_F[b] - S.bs_base[b] : (S.enc_lens[b] < S.T ? S.enc_lens[b] : S.T);
    const bool clamp = !TIMES || (S.bs_state[b] & 2);
    const int fr = S.frame[b];                     // the earliest frame of the beam
    if (MODE != kTdtFinal && fr >= T) return;      // every hypothesis has reached T_b
    const int N = S.n_hyps[b];
    const int sel = S.hyp_sel[b];
    const size_t hstride = (size_t)S.n_utt * beam * S.Lmax;
    const int32_t *__restrict__ hy = S.bhyps + sel * hstride + (size_t)b * beam * S.Lmax;
    int32_t *__restrict__ hy2 = S.bhyps + (1 - sel) * hstride + (size_t)b * beam * S.Lmax;
    const int32_t *__restrict__ hl = S.bhyp_lens + (size_t)sel * S.n_utt * beam + (size_t)b * beam;
    int32_t *__restrict__ hl2 = S.bhyp_lens + (size_t)(1 - sel) * S.n_utt * beam + (size_t)b * beam;
    // phase 1: the pool in the order of the beam
    if (tid < kMaxBeam) {                          // the entries' lengths and frames, requested side by side
        L.e_lb[tid] = tid < N ? hl[tid] : 0;
        p_t[tid] = tid < N ? S.lane_t[b * beam + tid] : 0;
    }
    __syncthreads();
    if (tid == 0) {
        int off = 0, na = 0;
        for (int e = 0; e < N; ++e) {
            const int t = p_t[e];
            p_off[e] = off;
            const bool expand = MODE != kTdtFinal && t == fr;
            off += expand ? beam : 1;
            na += expand ? 1 : 0;
        }
        p_off[N] = off;
        s_nact = na;
    }
    __syncthreads();
    const int C = p_off[N];                        // <= beam * beam: a waiting hypothesis takes the place of `beam` pairs
    if (tid < C) {
        int e = 0;
        while (e + 1 < N && p_off[e + 1] <= tid) ++e;
        const int r = tid - p_off[e];
        const int n = b * beam + e;
        const int te = p_t[e];
        const int lb = hl[e];
        const int last = S.token[n];               // last token of hypothesis e (its predictor input)
        const unsigned long long hh = S.bhash[n];
        const double se = S.bscores[(size_t)b * beam + e];
        int tok = -1, tn = te;                     // tok < 0: nothing appended (a waiting hypothesis or a blank arc)
        double sc = se, vs = TIMES ? S.bvscores[(size_t)b * beam + e] : 0.0;
        if (MODE != kTdtFinal && te == fr) {
            const int pair = S.topi[(size_t)n * beam + r];
            const int k = pair & 0xffff;
            const int dur = (int)((S.tdt_durs >> (4 * (pair >> 16))) & 15);
            const float v = S.topv[(size_t)n * beam + r];
            sc = (double)((float)se + v);          // the reference's fp32 add of a float-cast score
            if (TIMES) vs = (double)((float)vs + v);
            tn = te + (dur > 1 ? dur : 1);
            if (clamp) tn = tn < T ? tn : T;
            if (k != S.blank) tok = k;
        }
        if (MODE == kTdtFinal) tn = tn < T ? tn : T;
        L.c_score[tid] = sc;
        if (TIMES) L.c_vscore[tid] = vs;
        L.c_base[tid] = e;
        L.c_tok[tid] = tok;
        c_t[tid] = tn;
        L.c_len[tid] = lb + (tok >= 0 ? 1 : 0);
        L.c_last[tid] = tok >= 0 ? tok : last;
        L.c_hash[tid] = tok >= 0 ? hyp_hash_push(hh, tok) : hh;
        L.c_rep[tid] = tid;
        L.c_rank[tid] = 0;
        if constexpr (CTX) beam_ctx_candidate(S, L, tid, (size_t)b * beam + e, tok);   // a waiting entry, a blank arc: tok < 0
    }
    __syncthreads();
    beam_find_classes<true>(L, c_t, hy, S.Lmax, C, tid);
    beam_fuse_scores<TIMES>(L, C, tid);
    const int keep = beam_rank_prune<TIMES, CTX>(S, L, hl2, b, C, tid, [](int tok) { return tok < 0; });
    if (tid < keep) e_t[tid] = c_t[L.order[tid]];
    __syncthreads();
    if (tid == 0) {
        int fn = e_t[0];
        for (int e = 1; e < keep; ++e) fn = e_t[e] < fn ? e_t[e] : fn;
        s_fnext = fn;
    }
    if constexpr (CTX)
        beam_move_hyps<true, true>(L, hy, hy2, S.Lmax, keep, tid, S.btimes + sel * hstride + (size_t)b * beam * S.Lmax,
                                   S.btimes + (1 - sel) * hstride + (size_t)b * beam * S.Lmax, S.bs_base[b] + fr,
                                   S.btags + sel * hstride + (size_t)b * beam * S.Lmax,
                                   S.btags + (1 - sel) * hstride + (size_t)b * beam * S.Lmax);
    else if (TIMES)
        beam_move_hyps<true>(L, hy, hy2, S.Lmax, keep, tid, S.btimes + sel * hstride + (size_t)b * beam * S.Lmax,
                             S.btimes + (1 - sel) * hstride + (size_t)b * beam * S.Lmax, S.bs_base[b] + fr);
    else
        beam_move_hyps<false>(L, hy, hy2, S.Lmax, keep, tid);
    beam_move_predictor(S, L, b, keep, tid);
    __syncthreads();
    const int fnext = s_fnext;                     // f strictly increases: every arc advances
    if (tid < beam) {
        const int n = b * beam + tid;
        const int t = tid < keep ? e_t[tid] : fnext;
        S.lane_active[n] = (tid < keep) && t == fnext && t < T;
        S.lane_t[n] = t;
        S.need_pred[n] = 1;
        if (tid == 0) {
            S.n_hyps[b] = keep;
            S.frame[b] = fnext;
            S.hyp_sel[b] = 1 - sel;
            if (MODE == kTdtFinal) {               // the call's begin: the utterance is counted here if it has a frame to decode
                if (fnext < T) atomicAdd(S.active_count, 1);
            } else {
                atomicAdd(S.active_count + 1, 1);
                atomicAdd(S.active_count + 2, s_nact);
                if (fnext >= T) atomicSub(S.active_count, 1);
            }
        }
    }
}

template <bool TIMES, bool CTX = false>
__global__ __launch_bounds__(kBeamUpdThreads) void tdt_beam_update_kernel(DevState *sp)
{
    __shared__ BeamLds<CTX> L;
    const DevState S = *sp;
    tdt_beam_update<TIMES ? kTdtStream : kTdtWhole, CTX>(S, L, blockIdx.x);
}

// The begin of a chunk call (wr_prefix_beam_search_chunk), one workgroup per stream, after beam_init_kernel has started the
// streams the call resets.  A stream that has had its final call, or gets no frame and no flag, is left as it is.  Otherwise:
// the chunk's lens[b] frames are added (base_b = the old F_b, F_b += lens[b]) and the entries' frames, which count from the
// chunk's first frame, are moved to the new base; a reset starts the seed's Viterbi score and times slot; a final call of a
// token-and-duration stream clamps, fuses and re-sorts (tdt_beam_update<kTdtFinal>); then the lanes at the earliest frame
// that have a frame of the chunk to decode are active, and active_count[0] counts the streams with such a lane.
// CTX: the biased streams; flag bit 2 concerns the export alone and is masked here (beam_init_kernel has seeded the graph
// state, the bonus and the tag slot of a stream that is reset).
template <bool TDT, bool CTX = false>
__global__ __launch_bounds__(kBeamUpdThreads) void beam_chunk_begin_kernel(DevState *sp)
{
    __shared__ BeamLds<CTX> L;
    const DevState S = *sp;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int beam = S.beam;
    const int flags = CTX ? S.bs_flags[b] & 3 : S.bs_flags[b];
    const bool reset = flags & 1;
    int len = S.enc_lens[b];
    len = len > 0 ? len : 0;
    len = len < S.T ? len : S.T;
    if (!reset && ((S.bs_state[b] & 2) || (flags == 0 && len == 0))) return;
    const int F0 = reset ? 0 : S.bs_F[b];
    const int shift = reset ? 0 : F0 - S.bs_base[b];      // the frames of the stream's previous chunk
    const int fr = S.frame[b] - shift;
    const int N = S.n_hyps[b];
    const int lt = tid < beam ? S.lane_t[b * beam + tid] - shift : 0;
    __syncthreads();                               // everything above is read before anything below is written
    if (tid < beam) S.lane_t[b * beam + tid] = lt;
    if (tid == 0) {
        S.bs_base[b] = F0;
        S.bs_F[b] = F0 + len;
        S.bs_state[b] = flags & 2;
        S.frame[b] = fr;
        if (reset) {                               // beam_init_kernel left the seed in buffer 0
            S.bvscores[(size_t)b * beam] = 0.0;
            S.btimes[(size_t)b * beam * S.Lmax] = -1;
        }
    }
    if (TDT && (flags & 2)) {
        __syncthreads();                           // the state written above is read through global memory
        tdt_beam_update<kTdtFinal, CTX>(S, L, b);
        return;
    }
    if (tid < beam) S.lane_active[b * beam + tid] = tid < N && lt == fr && lt < len;
    if (tid == 0 && fr < len) atomicAdd(S.active_count, 1);
}

__global__ void beam_export_kernel(DevState *s, int32_t *hyps_out, int32_t *lens_out, double *scores_out, int32_t *n_out)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int beam = s->beam;
    const int sel = s->hyp_sel[b];
    const size_t hstride = (size_t)s->n_utt * beam * s->Lmax;
    const int32_t *hy = s->bhyps + sel * hstride + (size_t)b * beam * s->Lmax;
    const int32_t *hl = s->bhyp_lens + (size_t)sel * s->n_utt * beam + (size_t)b * beam;
    const int N = s->n_hyps[b];
    for (int i = tid; i < beam * s->Lmax; i += blockDim.x) {
        const int e = i / s->Lmax, q = i % s->Lmax;
        hyps_out[((size_t)b * beam + e) * s->Lmax + q] = (e < N && q < hl[e]) ? hy[(size_t)e * s->Lmax + q] : -1;
    }
    if (tid < beam) {
        lens_out[(size_t)b * beam + tid] = (tid < N) ? hl[tid] : 0;
        scores_out[(size_t)b * beam + tid] = (tid < N) ? s->bscores[(size_t)b * beam + tid] : -__builtin_huge_val();
    }
    if (tid == 0) n_out[b] = N;
}

// the same for the streaming search, with each hypothesis' times (absolute frames; the seed's slot and the padding -1) and
// Viterbi score
__global__ void beam_stream_export_kernel(DevState *s, int32_t *hyps_out, int32_t *times_out, int32_t *lens_out, double *scores_out,
                                          double *vscores_out, int32_t *n_out)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const int beam = s->beam;
    const int sel = s->hyp_sel[b];
    const size_t hstride = (size_t)s->n_utt * beam * s->Lmax;
    const int32_t *hy = s->bhyps + sel * hstride + (size_t)b * beam * s->Lmax;
    const int32_t *tm = s->btimes + sel * hstride + (size_t)b * beam * s->Lmax;
    const int32_t *hl = s->bhyp_lens + (size_t)sel * s->n_utt * beam + (size_t)b * beam;
    const int N = s->n_hyps[b];
    for (int i = tid; i < beam * s->Lmax; i += blockDim.x) {
        const int e = i / s->Lmax, q = i % s->Lmax;
        const bool in = e < N && q < hl[e];
        hyps_out[((size_t)b * beam + e) * s->Lmax + q] = in ? hy[(size_t)e * s->Lmax + q] : -1;
        times_out[((size_t)b * beam + e) * s->Lmax + q] = in ? tm[(size_t)e * s->Lmax + q] : -1;
    }
    if (tid < beam) {
        lens_out[(size_t)b * beam + tid] = (tid < N) ? hl[tid] : 0;
        scores_out[(size_t)b * beam + tid] = (tid < N) ? s->bscores[(size_t)b * beam + tid] : -__builtin_huge_val();
        vscores_out[(size_t)b * beam + tid] = (tid < N) ? s->bvscores[(size_t)b * beam + tid] : -__builtin_huge_val();
    }
    if (tid == 0) n_out[b] = N;
}

// the same for the biased streaming search: beside the above the pure fused score, the bonus, the tags and the graph state of
// every hypothesis; scores = trans_scores + context_scores, the add of the prune.  A stream flagged bit 2 is exported "as if
// it ended here": an entry away from the root gains (double)escape[state] in the exported bonus and the exported list is
// sorted again, stable and descending, by the new totals.  The state block is only read.
__global__ void beam_context_export_kernel(DevState *s, int32_t *hyps_out, int32_t *times_out, int32_t *lens_out, double *scores_out,
                                           double *vscores_out, int32_t *n_out, double *trans_out, double *ctx_out, int32_t *tags_out,
                                           int32_t *states_out)
{
    __shared__ double s_ctx[kMaxBeam], s_tot[kMaxBeam];
    __shared__ int s_row[kMaxBeam];                // the exported row of entry e
    const int b = blockIdx.x, tid = threadIdx.x;
    const int beam = s->beam;
    const int sel = s->hyp_sel[b];
    const size_t hstride = (size_t)s->n_utt * beam * s->Lmax;
    const int32_t *hy = s->bhyps + sel * hstride + (size_t)b * beam * s->Lmax;
    const int32_t *tm = s->btimes + sel * hstride + (size_t)b * beam * s->Lmax;
    const int32_t *tg = s->btags + sel * hstride + (size_t)b * beam * s->Lmax;
    const int32_t *hl = s->bhyp_lens + (size_t)sel * s->n_utt * beam + (size_t)b * beam;
    const int N = s->n_hyps[b];
    const bool fin = s->bs_flags[b] & 4;
    if (tid < beam) {
        double cx = 0.0, tot = -__builtin_huge_val();
        if (tid < N) {
            int st = s->bctx_state[(size_t)b * beam + tid];
            st = st < 0 ? 0 : (st < s->cg.S ? st : s->cg.S - 1);
            cx = s->bctx_score[(size_t)b * beam + tid];
            if (fin && st != 0) cx += (double)s->cg.escape[st];
            tot = s->bscores[(size_t)b * beam + tid] + cx;
        }
        s_ctx[tid] = cx;
        s_tot[tid] = tot;
    }
    __syncthreads();
    if (tid < beam) {
        int r = tid;
        if (fin && tid < N) {
            r = 0;
            for (int f = 0; f < N; ++f) r += (s_tot[f] > s_tot[tid] || (s_tot[f] == s_tot[tid] && f < tid)) ? 1 : 0;
        }
        s_row[tid] = r;
    }
    __syncthreads();
    for (int i = tid; i < beam * s->Lmax; i += blockDim.x) {
        const int e = i / s->Lmax, q = i % s->Lmax;
        const bool in = e < N && q < hl[e];
        const size_t o = ((size_t)b * beam + s_row[e]) * s->Lmax + q;
        hyps_out[o] = in ? hy[(size_t)e * s->Lmax + q] : -1;
        times_out[o] = in ? tm[(size_t)e * s->Lmax + q] : -1;
        tags_out[o] = in ? tg[(size_t)e * s->Lmax + q] : -1;
    }
    if (tid < beam) {
        const size_t o = (size_t)b * beam + s_row[tid];
        const bool in = tid < N;
        lens_out[o] = in ? hl[tid] : 0;
        scores_out[o] = s_tot[tid];
        trans_out[o] = in ? s->bscores[(size_t)b * beam + tid] : -__builtin_huge_val();
        vscores_out[o] = in ? s->bvscores[(size_t)b * beam + tid] : -__builtin_huge_val();
        ctx_out[o] = s_ctx[tid];
        states_out[o] = in ? s->bctx_state[(size_t)b * beam + tid] : 0;
    }
    if (tid == 0) n_out[b] = N;
}

}  // namespace
}  // namespace wr

using namespace wr;

// ------------------------------------------------------------ host handle --
// an executable graph of kStepsPerGraph steps and the shape it was captured for (-1: none, or dropped by a failed call)
struct GraphSlot {
    hipGraphExec_t exec = nullptr;
    int key = -1;
};

// The streams of wr_prefix_beam_search_chunk: the caller's block, and what the host knows of each stream.  The lanes'
// predictor state lives in the handle's workspace, so the streams are live only while wr_decoder::stream_lanes says so
// (kBeamStreamLanes: the last search on the handle was a chunk call).
constexpr int kBeamStreamLanes = -2;
constexpr int kBeamCtxStreamLanes = -3;       // the same for the biased form: neither form continues the other's streams
struct BeamStreams {
    bool attached = false;
    bool ctx = false;             // attached by wr_decoder_attach_beam_context_stream: the block also holds the three below
    double *ctx_score = nullptr;
    int32_t *ctx_state = nullptr, *btags = nullptr;
    int n = 0, beam = 0, max_frames = 0;
    int32_t *bhyps = nullptr, *btimes = nullptr, *bhyp_lens = nullptr, *base = nullptr, *F = nullptr, *state = nullptr,
            *flags = nullptr;                      // device, carved from the caller's block
    double *bscores = nullptr, *bvscores = nullptr;
    int32_t *h_flags = nullptr;   // pinned, [kStageSlots][n]: the flags of a call on their way to `flags`
    std::vector<int> phase;       // per stream: 0 never reset (or overwritten by another search), 1 running, 2 had its final call
    std::vector<long> frames;     // per stream: chunk widths summed since its reset
    bool overwritten = false;     // the streams were live when another search took the lanes (for the refusal's text)
    int blank = 0, D = 0;         // what the running streams are searched with
    unsigned long long durs = 0;
};

struct wr_decoder {
    Dims d{};
    DevState host{};              // host copy of the device state block
    DevState *dev = nullptr;      // device copy (first bytes of the workspace)
    char *ws = nullptr;
    size_t ws_bytes = 0;
    int max_utt = 0, Tmax = 0, max_hyp = 0, max_beam = 0;
    size_t zero_range[2] = {0, 0};
    int32_t *h_active = nullptr;  // pinned host word
    DevState *h_stage = nullptr;  // pinned staging slots for the state block (kStageSlots), so that the upload is a
    hipEvent_t stage_ev[kStageSlots] = {};   // true async copy: a slot is reused only after the copy that read it has completed
    int stage_next = 0;
    hipStream_t work = nullptr;   // decode work runs here (graph capture is illegal on the legacy default stream)
    hipEvent_t ev_in = nullptr, ev_out = nullptr;   // ordering against the caller's stream, no device-wide sync
    GraphSlot greedy[kMaxLook + 1];   // one per look-ahead setting, keyed by the lanes
    GraphSlot greedy_tdt[kMaxLook + 1];   // the same for the token-and-duration micro-step
    GraphSlot beam;               // keyed by lanes and beam
    GraphSlot beam_tdt;           // the token-and-duration beam step, keyed likewise
    GraphSlot hotword;            // keyed by the lanes
    int stream_lanes = -1;        // lanes whose streaming state (cache, token, flags) is live; -1: none
    int look = 0;                 // greedy look-ahead: frames per micro-step (1..kMaxLook), 0: chosen per replay
    // hot-word greedy (wr_decoder_attach_hotword)
    bool hw_attached = false;
    HwDev hw{};
    float *hw_ep2 = nullptr;      // [2][max_utt * Tmax * J] enc_ffn of the empty-list (0) / hot-word (1) encoder stream
    int32_t *hw_state = nullptr;  // cur_gate | gb_flag | gb_end | last_t, NLp each
    float *hw_biasT = nullptr;    // [Pp][NLp]
    // streaming prefix beam search (wr_decoder_attach_beam_stream)
    GraphSlot beam_stream, beam_tdt_stream;   // the streaming forms of `beam` / `beam_tdt`, keyed likewise
    GraphSlot beam_ctx_stream, beam_tdt_ctx_stream;   // and their biased forms (wr_prefix_beam_search_context_chunk)
    BeamStreams bs;
    bool use_graph = true;        // greedy micro-steps replayed from a hipGraph (default on)
    bool use_graph_beam = false;  // beam frames: plain launches measured faster (no host polling to amortise), default off
};

namespace {

template <typename F>
void for_each_graph(wr_decoder *h, F f)
{
    for (GraphSlot &g : h->greedy) f(g);
    for (GraphSlot &g : h->greedy_tdt) f(g);
    f(h->beam);
    f(h->beam_tdt);
    f(h->beam_stream);
    f(h->beam_tdt_stream);
    f(h->beam_ctx_stream);
    f(h->beam_tdt_ctx_stream);
    f(h->hotword);
}

struct Carver {
    char *base;
    size_t off;
    template <typename T>
    T *take(size_t n)
    {
        off = align_up(off, 256);
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += n * sizeof(T);
        return p;
    }
};

size_t carve(const wr_transducer_weights *w, int max_lanes, int max_utt, int Tmax, int max_hyp, int max_beam, char *base,
             DevState *st, DevState **dev, size_t *zero_range = nullptr)
{
    Carver c{base, 0};
    Dims d;
    d.V = w->vocab_size; d.E = w->enc_dim; d.P = w->pred_dim; d.D = w->embed_dim; d.H = w->hidden; d.L = w->n_layers;
    d.J = w->join_dim;
    d.Ve = w->embed_rows > 0 ? w->embed_rows : w->vocab_size;
    d.act = w->activation;
    d.ptype = w->predictor_type; d.ctx = w->context_size; d.heads = w->n_head; d.pact = w->pred_activation;
    d.ln_eps = w->ln_eps;
    d.Dp = round_up(d.D, 16); d.Hp = round_up(d.H, 16); d.Pp = round_up(d.P, 16); d.Jp = round_up(d.J, 16);   // K: 8 waves x k-pairs
    d.G4p = 4 * d.Hp;                                      // 32-column tiles = i,f,g,o of 8 hidden units
    d.Vp = round_up(d.V, 256);
    d.NL = max_lanes;
    d.NLp = max_lanes <= 32 ? 32 : round_up(max_lanes, 64);   // lane tiles of the GEMM: 32, or pairs of 32
    DevState s;
    memset(&s, 0, sizeof(s));
    s.d = d;
    DevState *devp = c.take<DevState>(1);
    const size_t zero_begin = align_up(c.off, 256);       // everything from here to zero_end is zero-filled at create
    for (int l = 0; l < d.L && d.ptype == kPredLstm; ++l) {
        if (l > 0) s.wt_ih[l] = c.take<float>((size_t)d.Hp * d.G4p);     // layer 0's input product is the table `etab`
        s.wt_hh[l] = c.take<float>((size_t)d.Hp * d.G4p);
        s.bsum[l] = c.take<float>((size_t)d.G4p);
    }
    const int Pn = round_up(d.P, 32), Jn = round_up(d.J, 32);
    if (d.ptype == kPredLstm) {
        s.proj_wt = c.take<float>((size_t)d.Hp * Pn);
        s.projffn_wt = c.take<float>((size_t)d.Hp * Jn);
        s.projffn_b = c.take<float>((size_t)Jn);
    }
    if (d.ptype == kPredEmbedding) {
        s.pffn_wt = c.take<float>((size_t)d.Dp * round_up(d.D, 32));
        s.combT = c.take<float>((size_t)d.Dp * d.NLp);
        s.ffnT = c.take<float>((size_t)d.Dp * d.NLp);
    }
    s.predffn_wt = c.take<float>((size_t)d.Pp * Jn);
    s.encffn_wt = c.take<float>((size_t)d.E * d.J);
    s.out_wt = c.take<float>((size_t)d.Jp * d.Vp);
    s.xT = c.take<float>((size_t)d.Dp * d.NLp);
    const size_t cs = (size_t)d.L * d.Hp * d.NLp;
    s.cache_hT = c.take<float>(cs); s.cache_cT = c.take<float>(cs);
    s.new_hT = c.take<float>(cs); s.new_cT = c.take<float>(cs);
    s.outT = c.take<float>((size_t)d.Pp * d.NLp);
    s.ht = c.take<float>((size_t)d.Jp * kMaxLook * d.NLp);
    s.comm_slot = c.take<int32_t>(d.NLp); s.new_slot = c.take<int32_t>(d.NLp);
    if (d.ptype == kPredLstm) {
        s.pool_c = c.take<float>((size_t)d.L * 2 * d.NLp * d.Hp);
        s.pool_g = c.take<float>((size_t)d.L * 2 * d.NLp * d.G4p);
    }
    const size_t zero_end = align_up(c.off, 256);
    if (d.ptype == kPredLstm) s.etab = c.take<float>((size_t)d.Ve * d.G4p);
    s.ep_all = c.take<float>((size_t)max_utt * Tmax * d.J);
    s.token = c.take<int32_t>(d.NLp); s.lane_t = c.take<int32_t>(d.NLp); s.noblk = c.take<int32_t>(d.NLp);
    s.need_pred = c.take<int32_t>(d.NLp); s.lane_active = c.take<int32_t>(d.NLp);
    s.new_is_cache = c.take<int32_t>(d.NLp);
    s.logits = c.take<float>((size_t)kMaxLook * d.NLp * d.V);
    s.row_tok = c.take<int32_t>((size_t)kMaxLook * d.NLp);
    s.n_cb = d.Vp / 32;
    s.row_part = c.take<float4>((size_t)d.NLp * s.n_cb);
    s.active_count = c.take<int32_t>(64);
    s.topv = c.take<float>((size_t)d.NL * kMaxBeam); s.topi = c.take<int32_t>((size_t)d.NL * kMaxBeam);
    s.n_hyps = c.take<int32_t>(max_utt); s.frame = c.take<int32_t>(max_utt);
    s.hyp_sel = c.take<int32_t>(max_utt);
    const int Lmax = Tmax + 1;
    s.bhyps = c.take<int32_t>((size_t)2 * max_utt * max_beam * Lmax);
    s.bhyp_lens = c.take<int32_t>((size_t)2 * max_utt * max_beam);
    s.bscores = c.take<double>((size_t)max_utt * max_beam);
    s.bhash = c.take<unsigned long long>((size_t)max_utt * max_beam);
    s.Lmax = Lmax;
    s.max_hyp = max_hyp;
    if (zero_range) { zero_range[0] = zero_begin; zero_range[1] = zero_end; }
    if (st) *st = s;
    if (dev) *dev = devp;
    return align_up(c.off, 256);
}

int check_weights(const wr_transducer_weights *w)
{
    WR_REQUIRE(w != nullptr, WR_EINVAL, "decoder: weights is null");
    WR_REQUIRE(w->vocab_size > 1 && w->enc_dim > 0 && w->pred_dim > 0 && w->embed_dim > 0 && w->hidden > 0 && w->join_dim > 0,
               WR_EINVAL, "decoder: non-positive dimension");
    WR_REQUIRE(w->n_layers >= 1 && w->n_layers <= kMaxLayers, WR_EUNSUPPORTED, "decoder: n_layers=%d (max %d)", w->n_layers,
               kMaxLayers);
    WR_REQUIRE(w->activation >= WR_ACT_TANH && w->activation <= WR_ACT_GELU, WR_EINVAL,
               "decoder: activation code %d is not a wr_activation", w->activation);
    WR_REQUIRE(w->join_dim <= 1024 && w->pred_dim <= 1024 && w->hidden <= 1024 && w->embed_dim <= 1024 && w->enc_dim <= 1024,
               WR_EUNSUPPORTED, "decoder: a layer dimension exceeds 1024");
    WR_REQUIRE(w->vocab_size * sizeof(float) <= 64 * 1024, WR_EUNSUPPORTED, "decoder: vocab_size=%d exceeds 16384",
               w->vocab_size);
    WR_REQUIRE(w->embed && w->enc_ffn_w && w->enc_ffn_b && w->pred_ffn_w && w->pred_ffn_b && w->out_w && w->out_b, WR_EINVAL,
               "decoder: null weight pointer");
    WR_REQUIRE(w->predictor_type >= kPredLstm && w->predictor_type <= kPredConv, WR_EINVAL, "decoder: predictor_type %d",
               w->predictor_type);
    if (w->predictor_type == kPredLstm) {
        WR_REQUIRE(w->proj_w && w->proj_b, WR_EINVAL, "decoder: null weight pointer");
        for (int l = 0; l < w->n_layers; ++l)
            WR_REQUIRE(w->w_ih[l] && w->w_hh[l] && w->b_ih[l] && w->b_hh[l], WR_EINVAL, "decoder: null LSTM weight (layer %d)", l);
        return WR_OK;
    }
    // stateless predictors: the token history rides in the LSTM-state slots
    WR_REQUIRE(w->context_size >= 2 && w->context_size <= kMaxCtx && w->n_layers == w->context_size - 1, WR_EUNSUPPORTED,
               "decoder: context_size=%d (history_size + 1) must be 2..%d with n_layers = context_size - 1 (got %d)",
               w->context_size, kMaxCtx, w->n_layers);
    WR_REQUIRE(w->hidden == w->embed_dim && w->pred_dim == w->embed_dim, WR_EINVAL,
               "decoder: a stateless predictor has hidden = pred_dim = embed_dim");
    WR_REQUIRE(w->pred_activation >= WR_ACT_TANH && w->pred_activation <= WR_ACT_GELU, WR_EINVAL,
               "decoder: pred_activation code %d is not a wr_activation", w->pred_activation);
    WR_REQUIRE(w->ln_eps > 0.f && w->norm_w && w->norm_b, WR_EINVAL, "decoder: LayerNorm weights / epsilon missing");
    if (w->predictor_type == kPredEmbedding) {
        WR_REQUIRE(w->n_head >= 1 && w->n_head * w->context_size <= 64, WR_EUNSUPPORTED,
                   "decoder: n_head * context_size = %d exceeds 64", w->n_head * w->context_size);
        WR_REQUIRE(w->pos_w && w->ffn_w && w->ffn_b, WR_EINVAL, "decoder: null EmbeddingPredictor weight");
    } else {
        WR_REQUIRE(w->conv_w, WR_EINVAL, "decoder: null ConvPredictor weight");
    }
    return WR_OK;
}

int launch_transpose(const float *src, int R, int C, int Rp, int Cp, float *dst, hipStream_t st)
{
    return launch("transpose_pad_kernel", transpose_pad_kernel, dim3((Rp + 31) / 32, (Cp + 31) / 32), dim3(256), 0, st, src, R, C,
                  Rp, Cp, dst);
}

// a 128-lane workgroup reads A columns lane0 .. lane0 + 127: the k-major arrays must be that wide
inline bool d_nlp_lt128(const GemmArgs &g) { return (g.lda % 128) != 0; }

// Exact-fp32 MFMA runs at 256 flop/clk/CU, so a 64-lane x 32-column x 512-deep tile already costs 3.4 us on its
// CU: lane tiles of 32 (more, smaller workgroups) whenever they all fit on the chip at once.
template <int EPI>
int launch_gemm(const GemmArgs &g, int n_cols_padded, int n_lanes, hipStream_t st)
{
    const int mt = (n_lanes + 31) / 32, ct = n_cols_padded / 32;
    const int policy = tune_get(kTuneLaneGemmTile);               // 0: by occupancy, 1: 32-lane tiles, 2: 64-lane tiles
    const dim3 block(64 * kGemmWaves);
    if (mt == 1 || policy == 1 || (policy == 0 && ct * mt <= 256))
        return launch("lane_gemm_kernel", lane_gemm_kernel<1, EPI>, dim3(ct, mt), block, 0, st, g);
    if (policy == 2 || (policy == 0 && ct * ((mt + 1) / 2) <= 256) || !(EPI == kEpiRowMajor || EPI == kEpiRowStats) || d_nlp_lt128(g))
        return launch("lane_gemm_kernel", lane_gemm_kernel<2, EPI>, dim3(ct, (mt + 1) / 2), block, 0, st, g);
    // more tiles than one round of 64-lane workgroups (bit-identical results in every form): 128-lane workgroups
    // (knob 6 = 3: 4-wave workgroups of 32 lanes, four per CU; 4: one wave per tile)
    if constexpr (EPI == kEpiRowMajor || EPI == kEpiRowStats) {
        if (policy == 3)
            return launch("lane_gemm4_kernel", lane_gemm4_kernel<EPI>, dim3(ct, mt), dim3(64 * kGemmWaves / 2), 0, st, g);
        if (policy == 4 && EPI == kEpiRowMajor)
            return launch("lane_gemm1_kernel", lane_gemm1_kernel<kEpiRowMajor>, dim3(ct, mt), dim3(64), 0, st, g);
        return launch("lane_gemm_kernel", lane_gemm_kernel<4, EPI>, dim3(ct, (mt + 3) / 4), block, 0, st, g);
    }
    return WR_OK;
}

// two GEMMs over the same lanes in one launch (lane_gemm_pair_kernel)
template <int EPI0, int EPI1>
int launch_gemm_pair(const GemmArgs &g0, int cols0, const GemmArgs &g1, int cols1, int n_lanes, hipStream_t st)
{
    const int mt = (n_lanes + 31) / 32, ct0 = cols0 / 32, ct = ct0 + cols1 / 32;
    const int policy = tune_get(kTuneLaneGemmTile);
    if (mt == 1 || policy == 1 || (policy == 0 && ct * mt <= 256))
        return launch("lane_gemm_pair_kernel", lane_gemm_pair_kernel<1, EPI0, EPI1>, dim3(ct, mt), dim3(64 * kGemmWaves), 0, st, g0,
                      g1, ct0);
    return launch("lane_gemm_pair_kernel", lane_gemm_pair_kernel<2, EPI0, EPI1>, dim3(ct, (mt + 1) / 2), dim3(64 * kGemmWaves), 0,
                  st, g0, g1, ct0);
}

// The fields every GEMM job sets.  `stamp` is the job's slot in the stamp array of the diagnostic build (-1: none).
GemmArgs gemm_job(const float *A0, int lda, int K0, const float *B0, int ldb, const float *bias, float *C, int ldc, int N,
                  int n_lanes, int stamp = -1)
{
    GemmArgs g{};
    g.A0 = A0; g.lda = lda; g.K0 = K0; g.B0 = B0; g.ldb = ldb; g.bias = bias;
    g.C = C; g.ldc = ldc; g.N = N; g.n_lanes = n_lanes;
#ifdef WR_STAMPS
    g.dbg_slot = stamp;
#endif
    return g;
}

// pool_g[l][new_slot[n]] = W_hh_l . new_h_l[n] + b_l: the recurrent product of the state a lane's step has just produced,
// for whichever later step starts from that state (see "LSTM predictor step").  Rides in the launch of the next stage.
GemmArgs recurrent_job(const wr_decoder *h, int l, int n_lanes, const int32_t *slot_idx)
{
    const Dims &d = h->d;
    const DevState &s = h->host;
    GemmArgs g = gemm_job(s.new_hT + (size_t)l * d.Hp * d.NLp, d.NLp, d.Hp, s.wt_hh[l], d.G4p, s.bsum[l],
                          s.pool_g + (size_t)l * 2 * d.NLp * d.G4p, d.G4p, d.G4p, n_lanes);
    g.slot_idx = slot_idx;
    return g;
}

// predictor step (predicated per lane).  LSTM: layer 0 was evaluated by the kernel that decided the token (or by the init
// kernel); here layers 1 .. L-1, each one GEMM of depth H with the recurrent product of the layer below in the same
// launch, and -- unless the caller folds it into pred_ffn -- the projection (with the last layer's recurrent product).
// `*recurrent_pending` is set if the last layer's recurrent product is still to be launched (the caller pairs it with its
// next GEMM).
int launch_predictor(wr_decoder *h, int n_lanes, hipStream_t st, bool with_projection = true, bool *recurrent_pending = nullptr)
{
    const Dims &d = h->d;
    const DevState &s = h->host;
    const size_t ls = (size_t)d.Hp * d.NLp;
    if (recurrent_pending) *recurrent_pending = false;
    if (d.ptype == kPredEmbedding) {            // context weighting -> ffn (lane GEMM) -> LayerNorm + activation
        WR_TRY(launch("ctx_predictor_kernel", ctx_predictor_kernel<0>, dim3(n_lanes), dim3(kCtxThreads), 0, st, h->dev));
        const int Dn = round_up(d.D, 32);
        WR_TRY(launch_gemm<kEpiKMajor>(gemm_job(s.combT, d.NLp, d.Dp, s.pffn_wt, Dn, s.pffn_b, s.ffnT, d.NLp, d.D, n_lanes), Dn,
                                       n_lanes, st));
        return launch("ctx_predictor_kernel", ctx_predictor_kernel<1>, dim3(n_lanes), dim3(kCtxThreads), 0, st, h->dev);
    }
    if (d.ptype == kPredConv)
        return launch("ctx_predictor_kernel", ctx_predictor_kernel<2>, dim3(n_lanes), dim3(kCtxThreads), 0, st, h->dev);
    for (int l = 1; l < d.L; ++l) {
        GemmArgs g = gemm_job(s.new_hT + (size_t)(l - 1) * ls, d.NLp, d.Hp, s.wt_ih[l], d.G4p, nullptr, nullptr, 0, d.G4p, n_lanes,
                              l < 2 ? l : -1);
        g.lane_active = s.lane_active; g.need_pred = s.need_pred; g.H = d.H; g.Hp = d.Hp; g.G4p = d.G4p;
        g.pool_g = s.pool_g + (size_t)l * 2 * d.NLp * d.G4p; g.pool_c = s.pool_c + (size_t)l * 2 * d.NLp * d.Hp;
        g.comm_slot = s.comm_slot; g.new_slot = s.new_slot; g.new_hT = s.new_hT + (size_t)l * ls;
        WR_TRY(launch_gemm_pair<kEpiLstmCell, kEpiSlotRow>(g, d.G4p, recurrent_job(h, l - 1, n_lanes, s.new_slot), d.G4p, n_lanes, st));
    }
    if (!with_projection) {                       // the caller applies the composed projection + pred_ffn
        if (recurrent_pending) *recurrent_pending = true;
        return WR_OK;
    }
    const int Pn = round_up(d.P, 32);
    return launch_gemm_pair<kEpiKMajor, kEpiSlotRow>(
        gemm_job(s.new_hT + (size_t)(d.L - 1) * ls, d.NLp, d.Hp, s.proj_wt, Pn, s.proj_b, s.outT, d.NLp, d.P, n_lanes, 8), Pn,
        recurrent_job(h, d.L - 1, n_lanes, s.new_slot), d.G4p, n_lanes, st);
}

// pred_ffn over the k-major operand A with the joiner activation as epilogue.  `fold`: A is the last LSTM layer's hidden
// state and the weight is the composed projection + pred_ffn.  The activation adds enc_ffn of `look` frames from `ep_all`;
// with `ep_gate` (hot-word search) each lane picks one of the two encoder streams stored behind each other there.
GemmArgs pred_ffn_job(const wr_decoder *h, const float *A, bool fold, int n_lanes, int look, const float *ep_all,
                      const int32_t *ep_gate = nullptr)
{
    const Dims &d = h->d;
    const DevState &s = h->host;
    GemmArgs g = gemm_job(A, d.NLp, fold ? d.Hp : d.Pp, fold ? s.projffn_wt : s.predffn_wt, round_up(d.J, 32),
                          fold ? s.projffn_b : s.predffn_b, s.ht, kMaxLook * d.NLp, d.J, n_lanes, 2);
    g.st = h->dev; g.lane_active = s.lane_active; g.lane_t = s.lane_t; g.ep_all = ep_all; g.J = d.J;
    g.look = look; g.lane_stride = d.NLp; g.act = d.act;
    if (ep_gate) { g.ep_gate = ep_gate; g.ep_gate_stride = (size_t)h->max_utt * h->Tmax * d.J; }
    return g;
}

// launch it, together with the last layer's recurrent product where launch_predictor left that pending
int launch_pred_ffn(const wr_decoder *h, const GemmArgs &g, bool recurrent_pending, int n_lanes, hipStream_t st)
{
    const Dims &d = h->d;
    if (recurrent_pending)
        return launch_gemm_pair<kEpiJointAct, kEpiSlotRow>(g, round_up(d.J, 32), recurrent_job(h, d.L - 1, n_lanes, h->host.new_slot),
                                                           d.G4p, n_lanes, st);
    return launch_gemm<kEpiJointAct>(g, round_up(d.J, 32), n_lanes, st);
}

// the joiner output for `rows` (frame, lane) columns of ht: rows f * NLp + n of the logits; `row_stats` adds the records
// the greedy update kernel reads (kEpiRowStats)
GemmArgs joint_out_job(const wr_decoder *h, int rows, bool row_stats)
{
    const Dims &d = h->d;
    const DevState &s = h->host;
    GemmArgs g = gemm_job(s.ht, kMaxLook * d.NLp, d.Jp, s.out_wt, d.Vp, s.out_b, s.logits, d.V, d.V, rows, 3);
    if (row_stats) { g.row_part = s.row_part; g.row_part_ld = s.n_cb; }
    return g;
}

int launch_predictor_and_joint(wr_decoder *h, int n_lanes, hipStream_t st, int look = 1, bool row_stats = false)
{
    const Dims &d = h->d;
    const DevState &s = h->host;
    // LSTM predictor: the projection is folded into pred_ffn (one launch less per micro-step; wr_tune_set(11, 1) keeps
    // them apart).  The hot-word search and wr_predictor_step need the projected output itself and keep the two stages.
    const bool fold = d.ptype == kPredLstm && tune_get(kTuneFoldProj) != 1;
    bool recurrent_pending = false;
    WR_TRY(launch_predictor(h, n_lanes, st, !fold, &recurrent_pending));
    const float *A = fold ? s.new_hT + (size_t)(d.L - 1) * d.Hp * d.NLp : s.outT;
    WR_TRY(launch_pred_ffn(h, pred_ffn_job(h, A, fold, n_lanes, look, s.ep_all), recurrent_pending, n_lanes, st));
    const int rows = (look - 1) * d.NLp + n_lanes;
    const GemmArgs g = joint_out_job(h, rows, row_stats);
    if (row_stats) return launch_gemm<kEpiRowStats>(g, d.Vp, rows, st);   // greedy, one frame per micro-step
    return launch_gemm<kEpiRowMajor>(g, d.Vp, rows, st);
}

// enc_ffn of `rows` encoder frames: 8 frames per workgroup
int launch_ep_all(wr_decoder *h, hipStream_t st, long rows, const float *enc, float *out)
{
    return launch("ep_all_kernel", ep_all_kernel, dim3((unsigned)((rows + 7) / 8)), dim3(256), (size_t)8 * h->d.E * sizeof(float), st,
                  h->dev, enc, out);
}

// the k-major, padded and composed forms of the weights, into the workspace
int prepare_weights(wr_decoder *h, const wr_transducer_weights *w, hipStream_t st)
{
    const Dims &d = h->d;
    const DevState &s = h->host;
    if (d.ptype == kPredEmbedding) WR_TRY(launch_transpose(w->ffn_w, d.D, d.D, round_up(d.D, 32), d.Dp, s.pffn_wt, st));
    for (int l = 0; l < d.L && d.ptype == kPredLstm; ++l) {
        if (l > 0)
            WR_TRY(launch("lstm_weight_prep_kernel", lstm_weight_prep_kernel, dim3(256), dim3(256), 0, st, w->w_ih[l], d.H, d.Hp, d.H,
                          d.Hp, s.wt_ih[l]));
        else
            WR_TRY(launch("lstm_etab_kernel", lstm_etab_kernel, dim3(2048), dim3(256), 0, st, w->embed, w->w_ih[0], d.Ve, d.D, d.H,
                          d.Hp, s.etab));
        WR_TRY(launch("lstm_weight_prep_kernel", lstm_weight_prep_kernel, dim3(256), dim3(256), 0, st, w->w_hh[l], d.H, d.Hp, d.H,
                      d.Hp, s.wt_hh[l]));
        WR_TRY(launch("lstm_bias_prep_kernel", lstm_bias_prep_kernel, dim3((d.G4p + 255) / 256), dim3(256), 0, st, w->b_ih[l],
                      w->b_hh[l], d.H, d.Hp, s.bsum[l]));
    }
    if (d.ptype == kPredLstm) {
        WR_TRY(launch_transpose(w->proj_w, d.P, d.H, round_up(d.P, 32), d.Hp, s.proj_wt, st));
        const long n = (long)d.H * d.J + d.J;
        WR_TRY(launch("compose_proj_ffn_kernel", compose_proj_ffn_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                      w->pred_ffn_w, w->pred_ffn_b, w->proj_w, w->proj_b, d.J, d.P, d.H, round_up(d.J, 32), s.projffn_wt,
                      s.projffn_b));
    }
    WR_TRY(launch_transpose(w->pred_ffn_w, d.J, d.P, round_up(d.J, 32), d.Pp, s.predffn_wt, st));
    WR_TRY(launch_transpose(w->enc_ffn_w, d.J, d.E, d.J, d.E, s.encffn_wt, st));
    return launch_transpose(w->out_w, d.V, d.J, d.Vp, d.Jp, s.out_wt, st);
}

}  // namespace

extern "C" size_t wr_decoder_workspace_bytes(const wr_transducer_weights *w, int max_lanes, int max_utt, int Tmax,
                                             int max_hyp, int max_beam)
{
    if (!w || max_lanes <= 0 || max_utt <= 0 || Tmax <= 0) return 0;
    return carve(w, max_lanes, max_utt, Tmax, max_hyp, max_beam > 0 ? max_beam : 1, nullptr, nullptr, nullptr);
}

extern "C" int wr_decoder_create(const wr_transducer_weights *w, int max_lanes, int max_utt, int Tmax, int max_hyp,
                                 int max_beam, void *workspace_d, size_t workspace_bytes, void *stream, wr_decoder **out)
{
    if (int rc = check_weights(w)) return rc;
    WR_REQUIRE(out && workspace_d, WR_EINVAL, "decoder_create: null pointer argument");
    WR_REQUIRE(max_lanes > 0 && max_lanes <= kMaxLanes, WR_EUNSUPPORTED, "decoder_create: max_lanes=%d (1..%d)", max_lanes,
               kMaxLanes);
    WR_REQUIRE(max_utt > 0 && max_utt <= max_lanes && Tmax > 0 && max_hyp >= 0, WR_EINVAL, "decoder_create: bad sizes");
    if (max_beam <= 0) max_beam = 1;
    WR_REQUIRE(max_beam <= kMaxBeam, WR_EUNSUPPORTED, "decoder_create: beam %d exceeds %d", max_beam, kMaxBeam);
    const size_t need = carve(w, max_lanes, max_utt, Tmax, max_hyp, max_beam, nullptr, nullptr, nullptr);
    WR_REQUIRE(workspace_bytes >= need, WR_EWORKSPACE, "decoder_create: workspace %zu < required %zu", workspace_bytes, need);
    wr_decoder *h = new (std::nothrow) wr_decoder();
    WR_REQUIRE(h != nullptr, WR_EINVAL, "decoder_create: out of host memory");
    h->ws = static_cast<char *>(workspace_d);
    h->ws_bytes = workspace_bytes;
    carve(w, max_lanes, max_utt, Tmax, max_hyp, max_beam, h->ws, &h->host, &h->dev, h->zero_range);
    h->d = h->host.d;
    h->max_utt = max_utt; h->Tmax = Tmax; h->max_hyp = max_hyp; h->max_beam = max_beam;
    if (hipHostMalloc(reinterpret_cast<void **>(&h->h_active), 64, hipHostMallocDefault) != hipSuccess ||
        hipHostMalloc(reinterpret_cast<void **>(&h->h_stage), kStageSlots * sizeof(DevState), hipHostMallocDefault) != hipSuccess) {
        (void)wr_decoder_destroy(h);
        set_error("decoder_create: hipHostMalloc failed");
        return WR_ELAUNCH;
    }
    bool ev_ok = true;
    for (int i = 0; i < kStageSlots; ++i) ev_ok = ev_ok && hipEventCreateWithFlags(&h->stage_ev[i], hipEventDisableTiming) == hipSuccess;
    if (!ev_ok || hipStreamCreateWithFlags(&h->work, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming) != hipSuccess) {
        (void)wr_decoder_destroy(h);
        set_error("decoder_create: stream/event creation failed");
        return WR_ELAUNCH;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    DevState &s = h->host;
    s.embed = w->embed; s.proj_b = w->proj_b; s.predffn_b = w->pred_ffn_b; s.encffn_b = w->enc_ffn_b; s.out_b = w->out_b;
    (void)hipMemsetAsync(h->ws + h->zero_range[0], 0, h->zero_range[1] - h->zero_range[0], st);
    s.pos_w = w->pos_w; s.pffn_b = w->ffn_b; s.pnorm_w = w->norm_w; s.pnorm_b = w->norm_b; s.conv_w = w->conv_w;
    s.conv_b = w->conv_b;
    if (int rc = prepare_weights(h, w, st)) {
        (void)wr_decoder_destroy(h);
        return rc;
    }
    *out = h;
    return WR_OK;
}

// safe on a partly built handle (the failure paths of wr_decoder_create): whatever was not created is skipped
extern "C" int wr_decoder_destroy(wr_decoder *h)
{
    if (!h) return WR_OK;
    for_each_graph(h, [](GraphSlot &g) { if (g.exec) (void)hipGraphExecDestroy(g.exec); });
    if (h->work) (void)hipStreamSynchronize(h->work);
    if (h->h_active) (void)hipHostFree(h->h_active);
    if (h->h_stage) (void)hipHostFree(h->h_stage);
    if (h->bs.h_flags) (void)hipHostFree(h->bs.h_flags);
    for (hipEvent_t ev : h->stage_ev) if (ev) (void)hipEventDestroy(ev);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    if (h->work) (void)hipStreamDestroy(h->work);
    delete h;
    return WR_OK;
}

extern "C" int wr_decoder_set_graph(wr_decoder *h, int enable)
{
    WR_REQUIRE(h != nullptr, WR_EINVAL, "decoder_set_graph: null handle");
    h->use_graph = h->use_graph_beam = enable != 0;
    return WR_OK;
}

// decode_tdt.hpp: the counters behind wr_decoder_last_counters -- pinned host memory, complete since the last poll
void wr::decoder_counters(const wr_decoder *h, int32_t *out)
{
    for (int i = 0; i < 3; ++i) out[i] = h->h_active ? h->h_active[i] : 0;
}

extern "C" int wr_decoder_set_lookahead(wr_decoder *h, int frames)
{
    WR_REQUIRE(h != nullptr, WR_EINVAL, "decoder_set_lookahead: null handle");
    WR_REQUIRE(frames >= 0 && frames <= kMaxLook, WR_EINVAL, "decoder_set_lookahead: frames=%d (0..%d)", frames, kMaxLook);
    h->look = frames;
    return WR_OK;
}

namespace {

int upload_state(wr_decoder *h, hipStream_t st)
{
    // through a pinned slot: a copy from pageable memory would block the host until the work stream has drained
    const int slot = h->stage_next;
    h->stage_next = (slot + 1) % kStageSlots;
    (void)hipEventSynchronize(h->stage_ev[slot]);                  // the copy that last read this slot (long done, normally)
    h->h_stage[slot] = h->host;
    hipError_t e = hipMemcpyAsync(h->dev, &h->h_stage[slot], sizeof(DevState), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipEventRecord(h->stage_ev[slot], st);
    if (e != hipSuccess) { set_error("decoder: state upload failed: %s", hipGetErrorString(e)); return WR_ELAUNCH; }
    return WR_OK;
}

LaneArgs lane_args(const wr_decoder *h)
{
    const DevState &s = h->host;
    LaneArgs a;
    a.lane_active = s.lane_active; a.lane_t = s.lane_t; a.noblk = s.noblk; a.need_pred = s.need_pred;
    a.new_is_cache = s.new_is_cache; a.comm_slot = s.comm_slot; a.new_slot = s.new_slot;
    a.row_part = s.row_part; a.n_cb = s.n_cb; a.V = h->d.V;
    return a;
}

template <bool HW>
int launch_greedy_update(wr_decoder *h, int n_lanes, hipStream_t st)
{
    const LaneArgs a = lane_args(h);
    const int recs = (h->d.V + 31) / 32 <= 3 * 64 ? 3 : 8;   // records per lane of a wave: V <= 6144 -> 3, else 8 (V <= 16384)
    return with_int<3, 8>(recs, [&](auto r) {
        return launch("greedy_update_kernel", greedy_update_kernel<HW, decltype(r)::value>, dim3(n_lanes), dim3(256), 0, st, h->dev, a);
    });
}

int greedy_micro_step(wr_decoder *h, int n_lanes, hipStream_t st, int look)
{
    WR_TRY(launch_predictor_and_joint(h, n_lanes, st, look, look == 1));
    if (look == 1) return launch_greedy_update<false>(h, n_lanes, st);
    const int V = h->d.V;                           // <= 16384 (check_weights)
    const int per_thread = V <= 256 * 8 ? 8 : V <= 256 * 24 ? 24 : 64;
    WR_TRY(with_int<8, 24, 64>(per_thread, [&](auto n) {
        return launch("greedy_rows_kernel", greedy_rows_kernel<decltype(n)::value>, dim3(n_lanes, look), dim3(256), 0, st, h->dev);
    }));
    return launch("greedy_resolve_kernel", greedy_resolve_kernel, dim3(n_lanes), dim3(256), 0, st, h->dev, look);
}

// token-and-duration model: the two TDT kernels over row-major logits, for every `look` (1 included)
int tdt_micro_step(wr_decoder *h, int n_lanes, hipStream_t st, int look)
{
    WR_TRY(launch_predictor_and_joint(h, n_lanes, st, look, /*row_stats=*/false));
    const int V = h->d.V;                           // <= 16384 (check_weights)
    const int per_thread = V <= 256 * 8 ? 8 : V <= 256 * 24 ? 24 : 64;
    WR_TRY(with_int<8, 24, 64>(per_thread, [&](auto n) {
        return launch("tdt_rows_kernel", tdt_rows_kernel<decltype(n)::value>, dim3(n_lanes, look), dim3(256), 0, st, h->dev);
    }));
    return launch("tdt_resolve_kernel", tdt_resolve_kernel, dim3(n_lanes), dim3(256), 0, st, h->dev, look);
}

// `times`: the streaming forms of the update kernels (wr_prefix_beam_search_chunk); `ctx` (with `times`): their biased forms
int beam_frame(wr_decoder *h, int n_lanes, int n_utt, hipStream_t st, bool times = false, bool ctx = false)
{
    WR_TRY(launch_predictor_and_joint(h, n_lanes, st));
    const int V = h->d.V;                           // <= 16384 (check_weights)
    const int per_thread = V <= kTopkThreads * 4 ? 4 : V <= kTopkThreads * 10 ? 10 : 32;
    WR_TRY(with_int<4, 10, 32>(per_thread, [&](auto n) {
        return launch("beam_topk_kernel", beam_topk_kernel<decltype(n)::value>, dim3(n_lanes), dim3(kTopkThreads), 0, st, h->dev);
    }));
    if (ctx) return launch("beam_update_kernel", beam_update_kernel<true, true>, dim3(n_utt), dim3(kBeamUpdThreads), 0, st, h->dev);
    if (times) return launch("beam_update_kernel", beam_update_kernel<true>, dim3(n_utt), dim3(kBeamUpdThreads), 0, st, h->dev);
    return launch("beam_update_kernel", beam_update_kernel<false>, dim3(n_utt), dim3(kBeamUpdThreads), 0, st, h->dev);
}

// one step of the token-and-duration beam search: the lane GEMMs take each lane's frame from lane_t, as in the greedy search
int tdt_beam_step(wr_decoder *h, int n_lanes, int n_utt, hipStream_t st, bool times = false, bool ctx = false)
{
    WR_TRY(launch_predictor_and_joint(h, n_lanes, st));
    const int V = h->d.V;                           // <= 16384 (check_weights)
    const int per_thread = V <= kTopkThreads * 4 ? 4 : V <= kTopkThreads * 10 ? 10 : 32;
    WR_TRY(with_int<4, 10, 32>(per_thread, [&](auto n) {
        return launch("tdt_beam_topk_kernel", tdt_beam_topk_kernel<decltype(n)::value>, dim3(n_lanes), dim3(kTopkThreads), 0, st,
                      h->dev);
    }));
    if (ctx)
        return launch("tdt_beam_update_kernel", tdt_beam_update_kernel<true, true>, dim3(n_utt), dim3(kBeamUpdThreads), 0, st,
                      h->dev);
    if (times)
        return launch("tdt_beam_update_kernel", tdt_beam_update_kernel<true>, dim3(n_utt), dim3(kBeamUpdThreads), 0, st, h->dev);
    return launch("tdt_beam_update_kernel", tdt_beam_update_kernel<false>, dim3(n_utt), dim3(kBeamUpdThreads), 0, st, h->dev);
}

// Order the decoder's work stream after everything already enqueued on the caller's stream ...
hipStream_t enter(wr_decoder *h, hipStream_t caller)
{
    (void)hipEventRecord(h->ev_in, caller);
    (void)hipStreamWaitEvent(h->work, h->ev_in, 0);
    return h->work;
}
// ... and the caller's stream after the decoder's work.
void leave(wr_decoder *h, hipStream_t caller)
{
    (void)hipEventRecord(h->ev_out, h->work);
    (void)hipStreamWaitEvent(caller, h->ev_out, 0);
}

// Scope of one entry point on the work stream: leave() runs on EVERY exit path, so the caller's stream is always
// ordered after whatever was enqueued; unless ok() was called, the handle's streaming state and cached graphs are
// dropped as well (a failed call leaves the lanes in an undefined state).
struct WorkScope {
    wr_decoder *h;
    hipStream_t caller, st;
    bool good = false;
    WorkScope(wr_decoder *h_, hipStream_t caller_) : h(h_), caller(caller_), st(enter(h_, caller_)) {}
    void ok() { good = true; }
    ~WorkScope()
    {
        if (!good) {
            h->stream_lanes = -1;
            for_each_graph(h, [](GraphSlot &g) { g.key = -1; });
        }
        leave(h, caller);
    }
};

// Capture `reps` repetitions of `body` on `st` into an executable graph.  A failing body still ends the capture; its
// code is returned and no graph is kept.
template <typename F>
int capture(hipStream_t st, int reps, F body, hipGraphExec_t *out)
{
    hipGraph_t g = nullptr;
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
    if (e != hipSuccess) { set_error("decoder: hipStreamBeginCapture failed: %s", hipGetErrorString(e)); return WR_ELAUNCH; }
    int rc = WR_OK;
    for (int i = 0; i < reps && rc == WR_OK; ++i) rc = body();
    e = hipStreamEndCapture(st, &g);
    if (rc != WR_OK) {
        if (g) (void)hipGraphDestroy(g);
        return rc;
    }
    if (e != hipSuccess || !g) { set_error("decoder: hipStreamEndCapture failed: %s", hipGetErrorString(e)); return WR_ELAUNCH; }
    e = hipGraphInstantiate(out, g, nullptr, nullptr, 0);
    (void)hipGraphDestroy(g);
    if (e != hipSuccess) { set_error("decoder: hipGraphInstantiate failed: %s", hipGetErrorString(e)); return WR_ELAUNCH; }
    return WR_OK;
}

// make `slot` hold the graph of kStepsPerGraph repetitions of `body` for `key`
template <typename F>
int ensure_graph(GraphSlot &slot, int key, hipStream_t st, F body)
{
    if (slot.key == key) return WR_OK;
    if (slot.exec) { (void)hipGraphExecDestroy(slot.exec); slot.exec = nullptr; }
    WR_TRY(capture(st, kStepsPerGraph, body, &slot.exec));
    slot.key = key;
    return WR_OK;
}

// The polling loop of the two greedy searches (`what` names the entry point in the error texts): kStepsPerGraph steps
// at a time -- replayed from the graph `slot()` holds for `key` when the handle uses graphs -- then the three counters
// (lanes active, blank decisions, emissions) come back and `after_replay()` may look at them, until no lane is active.
// Running out of `max_micro` steps is an error, not truncated hypotheses returned as WR_OK; `budget_note` ends its text.
template <typename Slot, typename Step, typename After>
int run_until_idle(wr_decoder *h, hipStream_t st, const char *what, int key, long max_micro, const char *budget_note, Slot slot,
                   Step step, After after_replay)
{
    for (long done = 0; done < max_micro; done += kStepsPerGraph) {
        if (h->use_graph) {
            GraphSlot &g = slot();
            WR_TRY(ensure_graph(g, key, st, step));
            hipError_t e = hipGraphLaunch(g.exec, st);
            if (e != hipSuccess) { set_error("%s: hipGraphLaunch failed: %s", what, hipGetErrorString(e)); return WR_ELAUNCH; }
        } else {
            for (int i = 0; i < kStepsPerGraph; ++i) WR_TRY(step());
        }
        // the reference synchronises on every step (.item()); we do once per kStepsPerGraph micro-steps
        (void)hipMemcpyAsync(h->h_active, h->host.active_count, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        hipError_t e = hipStreamSynchronize(st);
        if (e != hipSuccess) { set_error("%s: stream error: %s", what, hipGetErrorString(e)); return WR_ELAUNCH; }
        if (h->h_active[0] <= 0) break;
        after_replay();
    }
    WR_REQUIRE(h->h_active[0] <= 0, WR_ELAUNCH, "%s: %d streams still active after %ld micro-steps%s", what, h->h_active[0],
               max_micro, budget_note);
    return WR_OK;
}

// DevState::tdt_durs of a checked duration set
unsigned long long pack_durations(const TdtDur &dur)
{
    unsigned long long durs = 0;
    for (int d = 0; d < kTdtMaxD; ++d)
        if (dur.slot[d] >= 0) durs |= (unsigned long long)d << (4 * dur.slot[d]);
    return durs;
}

// The steps of the plain prefix beam searches (`what` names the entry point in the error texts; `times`: the streaming
// form): the fixed count of T frames, kStepsPerGraph at a time, replayed from a graph if the handle says so.
int beam_plain_steps(wr_decoder *h, hipStream_t st, const char *what, int NLn, int B, int T, int beam, bool times, bool ctx = false)
{
    GraphSlot &slot = ctx ? h->beam_ctx_stream : times ? h->beam_stream : h->beam;
    const auto frame = [&] { return beam_frame(h, NLn, B, st, times, ctx); };
    if (h->use_graph_beam) WR_TRY(ensure_graph(slot, NLn * 1000 + beam, st, frame));
    for (int f = 0; f < T; f += kStepsPerGraph) {
        if (h->use_graph_beam) {
            hipError_t e = hipGraphLaunch(slot.exec, st);
            if (e != hipSuccess) { set_error("%s: hipGraphLaunch failed: %s", what, hipGetErrorString(e)); return WR_ELAUNCH; }
        } else {
            for (int i = 0; i < kStepsPerGraph; ++i) WR_TRY(frame());
        }
    }
    return WR_OK;
}

// The steps of the token-and-duration prefix beam searches: until no utterance has an entry below its frame count.  Every
// step moves the earliest frame of every running utterance on, so T steps always suffice.
int beam_tdt_steps(wr_decoder *h, hipStream_t st, const char *what, int NLn, int B, int T, int beam, bool times, bool ctx = false)
{
    return run_until_idle(
        h, st, what, NLn * 1000 + beam, (long)T + 1, "",
        [&]() -> GraphSlot & { return ctx ? h->beam_tdt_ctx_stream : times ? h->beam_tdt_stream : h->beam_tdt; },
        [&] { return tdt_beam_step(h, NLn, B, st, times, ctx); }, [] {});
}

// what a token-and-duration search adds to a greedy run
struct TdtRun {
    unsigned long long durs;      // DevState::tdt_durs
    int D;
    int32_t *hyp_frames;          // [N, max_hyp] or null
};

// mode 0: fresh utterances; 1: next chunk, keep the pending predictor state; 2: next chunk, reference quirk.
// `tdt` (mode 0 only): the token-and-duration search -- its own micro-step and graph slots, the rest is shared.
int greedy_run(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, int N, int T, int n_steps, int blank,
               int32_t *hyps_d, int32_t *hyp_lens_d, void *stream, int mode, const TdtRun *tdt = nullptr)
{
    const char *what = tdt ? "greedy_search_tdt" : "greedy_search";
    WR_REQUIRE(h && enc_out_d && enc_lens_d && hyps_d && hyp_lens_d, WR_EINVAL, "%s: null pointer argument", what);
    WR_REQUIRE(N > 0 && N <= h->d.NL && N <= h->max_utt, WR_EINVAL, "%s: N=%d exceeds the decoder's capacity", what, N);
    WR_REQUIRE(T > 0 && T <= h->Tmax, WR_EINVAL, "%s: T=%d exceeds the decoder's Tmax=%d", what, T, h->Tmax);
    if (tdt) {
        const int V = h->d.V - tdt->D;             // token columns of the joiner's row
        WR_REQUIRE(V >= 2, WR_EINVAL, "%s: the joiner has %d outputs, D=%d durations leave %d token columns (2 or more are needed)",
                   what, h->d.V, tdt->D, V);
        WR_REQUIRE(blank >= 0 && blank < V, WR_EINVAL, "%s: blank %d out of range [0,%d)", what, blank, V);
        WR_REQUIRE(h->d.Ve >= V, WR_EINVAL, "%s: the embedding table has %d rows, the token vocabulary %d", what, h->d.Ve, V);
    }
    WR_REQUIRE(n_steps >= 1 && blank >= 0 && blank < h->d.V, WR_EINVAL, "greedy_search: bad n_steps/blank");
    WR_REQUIRE(mode == 0 || h->stream_lanes == N, WR_EINVAL,
               "greedy_search_chunk: no stream state for %d lanes (call with reset first)", N);
    WorkScope scope(h, static_cast<hipStream_t>(stream));
    hipStream_t st = scope.st;
    DevState &s = h->host;
    s.enc = enc_out_d; s.enc_lens = enc_lens_d; s.ctc_logp = nullptr;
    s.n_utt = N; s.T = T; s.lanes_per_utt = 1; s.n_lanes = N;
    s.hyps = hyps_d; s.hyp_lens = hyp_lens_d; s.max_hyp = h->max_hyp; s.n_steps = n_steps; s.blank = blank; s.beam = 1;
    s.tdt_durs = tdt ? tdt->durs : 0; s.tdt_D = tdt ? tdt->D : 0; s.hyp_frames = tdt ? tdt->hyp_frames : nullptr;
    if (int rc = upload_state(h, st)) return rc;
    (void)hipMemsetAsync(s.active_count, 0, 3 * sizeof(int32_t), st);    // lanes active, blank decisions, emissions
    (void)hipMemsetAsync(s.lane_active, 0, sizeof(int32_t) * h->d.NLp, st);
    WR_TRY(launch_ep_all(h, st, (long)N * T, enc_out_d, s.ep_all));
    if (mode == 0) WR_TRY(launch("greedy_init_kernel", greedy_init_kernel, dim3(N), dim3(128), 0, st, h->dev));
    else WR_TRY(launch("greedy_chunk_init_kernel", greedy_chunk_init_kernel, dim3(N), dim3(128), 0, st, h->dev, mode == 2 ? 1 : 0));
    h->stream_lanes = tdt ? -1 : N;               // a TDT run leaves no state a chunk could continue from
    // look-ahead per replay: fixed, or (h->look == 0) chosen from the share of blank decisions in the previous
    // replay -- any value gives the same tokens, so switching between replays is safe.  TDT: 0 means 1 -- consecutive
    // frames waste the rows a duration jump skips, and the rule measured no faster than 1 at 64 streams and 18 % slower
    // at one (profiles/tdt_greedy_search.md)
    int look = h->look > 0 ? h->look : 1;
    int prev_blank = 0, prev_emit = 0;
    // every micro-step emits (at most n_steps per frame) or advances the frame, so the budget cannot run out
    const long max_micro = (long)T * ((long)n_steps + 1) + 1;
    WR_TRY(run_until_idle(
        h, st, tdt ? "greedy_search_tdt" : "greedy_search", N, max_micro, "",
        [&]() -> GraphSlot & { return tdt ? h->greedy_tdt[look] : h->greedy[look]; },
        [&] { return tdt ? tdt_micro_step(h, N, st, look) : greedy_micro_step(h, N, st, look); },
        [&] {
            if (h->look != 0 || tdt) return;
            const int nb = h->h_active[1] - prev_blank, ne = h->h_active[2] - prev_emit;
            prev_blank = h->h_active[1]; prev_emit = h->h_active[2];
            const float share = (nb + ne) > 0 ? (float)nb / (float)(nb + ne) : 0.f;
            look = share >= 0.75f ? 4 : share >= 0.62f ? 2 : 1;
            // beyond ~256 joiner rows a micro-step is matrix-core bound and extra frames are no longer free
            while (look > 1 && look * N > 256) look >>= 1;
        }));
    scope.ok();
    return WR_OK;
}
}  // namespace

// decode_tdt.hpp: the search behind wr_greedy_search_tdt (decode_tdt.cpp has checked durations, n_steps, pointers)
int wr::greedy_tdt_body(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, int N, int T, int n_steps, int blank,
                        const TdtDur &dur, int32_t *hyps_d, int32_t *hyp_lens_d, int32_t *hyp_frames_d, void *stream)
{
    TdtRun run{pack_durations(dur), dur.D, hyp_frames_d};
    return greedy_run(h, enc_out_d, enc_lens_d, N, T, n_steps, blank, hyps_d, hyp_lens_d, stream, 0, &run);
}

// decode_tdt.hpp: the search behind wr_prefix_beam_search_tdt (decode_tdt.cpp has checked durations, pointers, the handle)
int wr::beam_tdt_body(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, const float *ctc_logp_d, int B, int T,
                      int beam, float ctc_weight, float transducer_weight, int blank, const TdtDur &dur, int32_t *hyps_d,
                      int32_t *hyp_lens_d, double *scores_d, int32_t *n_hyps_d, void *stream)
{
    const char *what = "prefix_beam_search_tdt";
    WR_REQUIRE(beam >= 1 && beam <= h->max_beam, WR_EINVAL, "%s: beam=%d lies outside [1, %d], the decoder's max", what, beam,
               h->max_beam);
    WR_REQUIRE(B > 0 && B <= h->max_utt && (long)B * beam <= h->d.NL, WR_EINVAL, "%s: B*beam=%ld exceeds the decoder's capacity",
               what, (long)B * beam);
    WR_REQUIRE(T > 0 && T <= h->Tmax, WR_EINVAL, "%s: T=%d exceeds the decoder's Tmax=%d", what, T, h->Tmax);
    const int V = h->d.V - dur.D;                  // token columns of the joiner's row
    WR_REQUIRE(V >= 2, WR_EINVAL, "%s: the joiner has %d outputs, D=%d durations leave %d token columns (2 or more are needed)",
               what, h->d.V, dur.D, V);
    WR_REQUIRE(blank >= 0 && blank < V, WR_EINVAL, "%s: blank %d out of range [0,%d)", what, blank, V);
    WR_REQUIRE(h->d.Ve >= V, WR_EINVAL, "%s: the embedding table has %d rows, the token vocabulary %d", what, h->d.Ve, V);
    WR_REQUIRE(ctc_logp_d || (ctc_weight == 0.f && transducer_weight == 1.f), WR_EINVAL,
               "%s: no CTC posterior, so (ctc_weight, transducer_weight) must be (0, 1), got (%g, %g)", what, (double)ctc_weight,
               (double)transducer_weight);
    h->stream_lanes = -1;                         // the lanes' streaming state (caches, tokens) is overwritten
    WorkScope scope(h, static_cast<hipStream_t>(stream));
    hipStream_t st = scope.st;
    DevState &s = h->host;
    s.enc = enc_out_d; s.enc_lens = enc_lens_d; s.ctc_logp = ctc_logp_d;
    s.n_utt = B; s.T = T; s.lanes_per_utt = beam; s.n_lanes = B * beam;
    s.beam = beam; s.ctc_weight = ctc_weight; s.tr_weight = transducer_weight; s.blank = blank;
    s.Lmax = h->Tmax + 1;
    s.tdt_durs = pack_durations(dur); s.tdt_D = dur.D; s.hyp_frames = nullptr;
    if (int rc = upload_state(h, st)) return rc;
    (void)hipMemsetAsync(s.lane_active, 0, sizeof(int32_t) * h->d.NLp, st);
    const int NLn = B * beam;
    WR_TRY(launch_ep_all(h, st, (long)B * T, enc_out_d, s.ep_all));
    WR_TRY(launch("beam_init_kernel", beam_init_kernel, dim3(NLn), dim3(128), 0, st, h->dev));
    WR_TRY(launch("tdt_beam_begin_kernel", tdt_beam_begin_kernel, dim3(1), dim3(256), 0, st, h->dev));
    WR_TRY(beam_tdt_steps(h, st, what, NLn, B, T, beam, false));
    WR_TRY(launch("beam_export_kernel", beam_export_kernel, dim3(B), dim3(256), 0, st, h->dev, hyps_d, hyp_lens_d, scores_d, n_hyps_d));
    scope.ok();
    return WR_OK;
}

extern "C" int wr_greedy_search(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, int N, int T, int n_steps,
                                int blank, int32_t *hyps_d, int32_t *hyp_lens_d, void *stream)
{
    return greedy_run(h, enc_out_d, enc_lens_d, N, T, n_steps, blank, hyps_d, hyp_lens_d, stream, 0);
}

extern "C" int wr_greedy_search_chunk(wr_decoder *h, const float *enc_chunk_d, const int32_t *chunk_lens_d, int N, int T,
                                      int n_steps, int blank, int reset, int reference_new_cache, int32_t *hyps_d,
                                      int32_t *hyp_lens_d, void *stream)
{
    return greedy_run(h, enc_chunk_d, chunk_lens_d, N, T, n_steps, blank, hyps_d, hyp_lens_d, stream,
                      reset ? 0 : (reference_new_cache ? 2 : 1));
}

extern "C" int wr_prefix_beam_search(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d,
                                     const float *ctc_logp_d, int B, int T, int beam, float ctc_weight,
                                     float transducer_weight, int blank, int32_t *hyps_d, int32_t *hyp_lens_d,
                                     double *scores_d, int32_t *n_hyps_d, void *stream)
{
    WR_REQUIRE(h && enc_out_d && enc_lens_d && ctc_logp_d && hyps_d && hyp_lens_d && scores_d && n_hyps_d, WR_EINVAL,
               "prefix_beam_search: null pointer argument");
    WR_REQUIRE(beam >= 1 && beam <= h->max_beam, WR_EINVAL, "prefix_beam_search: beam=%d exceeds the decoder's max %d", beam,
               h->max_beam);
    WR_REQUIRE(B > 0 && B <= h->max_utt && B * beam <= h->d.NL, WR_EINVAL,
               "prefix_beam_search: B*beam=%d exceeds the decoder's capacity", B * beam);
    WR_REQUIRE(T > 0 && T <= h->Tmax, WR_EINVAL, "prefix_beam_search: T=%d exceeds the decoder's Tmax=%d", T, h->Tmax);
    WR_REQUIRE(blank >= 0 && blank < h->d.V, WR_EINVAL, "prefix_beam_search: bad blank");
    h->stream_lanes = -1;                         // the lanes' streaming state (caches, tokens) is overwritten
    WorkScope scope(h, static_cast<hipStream_t>(stream));
    hipStream_t st = scope.st;
    DevState &s = h->host;
    s.enc = enc_out_d; s.enc_lens = enc_lens_d; s.ctc_logp = ctc_logp_d;
    s.n_utt = B; s.T = T; s.lanes_per_utt = beam; s.n_lanes = B * beam;
    s.beam = beam; s.ctc_weight = ctc_weight; s.tr_weight = transducer_weight; s.blank = blank;
    s.Lmax = h->Tmax + 1;
    if (int rc = upload_state(h, st)) return rc;
    (void)hipMemsetAsync(s.lane_active, 0, sizeof(int32_t) * h->d.NLp, st);
    const int NLn = B * beam;
    WR_TRY(launch_ep_all(h, st, (long)B * T, enc_out_d, s.ep_all));
    WR_TRY(launch("beam_init_kernel", beam_init_kernel, dim3(NLn), dim3(128), 0, st, h->dev));
    WR_TRY(beam_plain_steps(h, st, "prefix_beam_search", NLn, B, T, beam, false));
    WR_TRY(launch("beam_export_kernel", beam_export_kernel, dim3(B), dim3(256), 0, st, h->dev, hyps_d, hyp_lens_d, scores_d, n_hyps_d));
    scope.ok();
    return WR_OK;
}

// ------------------------------------------------ streaming prefix beam search: host side --
namespace {

// where the caller's block puts things: one pass for the size (null base) and for the pointers
// (`ctx`: the biased form's block -- the plain block's contents, then the bonus, the graph state and the tags of every entry)
size_t beam_stream_carve(int n, int beam, int max_frames, char *base, BeamStreams *p, bool ctx = false)
{
    Carver c{base, 0};
    const size_t Lcap = (size_t)max_frames + 1, nb = (size_t)n * beam;
    p->bhyps = c.take<int32_t>(2 * nb * Lcap);
    p->btimes = c.take<int32_t>(2 * nb * Lcap);
    p->bhyp_lens = c.take<int32_t>(2 * nb);
    p->bscores = c.take<double>(nb);
    p->bvscores = c.take<double>(nb);
    p->base = c.take<int32_t>(n); p->F = c.take<int32_t>(n); p->state = c.take<int32_t>(n); p->flags = c.take<int32_t>(n);
    if (ctx) {
        p->ctx_score = c.take<double>(nb);
        p->ctx_state = c.take<int32_t>(nb);
        p->btags = c.take<int32_t>(2 * nb * Lcap);
    }
    return align_up(c.off, 256);
}

int beam_stream_check(const char *what, const wr_decoder *h, int max_streams, int beam, int max_frames)
{
    WR_REQUIRE(h != nullptr, WR_EINVAL, "%s: null handle", what);
    WR_REQUIRE(beam >= 1 && beam <= h->max_beam, WR_EINVAL, "%s: beam=%d lies outside [1, %d], the decoder's max", what, beam,
               h->max_beam);
    WR_REQUIRE(max_streams >= 1 && max_streams <= h->max_utt && (long)max_streams * beam <= h->d.NL, WR_EINVAL,
               "%s: max_streams=%d with beam %d exceeds the decoder's capacity", what, max_streams, beam);
    WR_REQUIRE(max_frames >= 1 && max_frames < (1 << 30), WR_EINVAL, "%s: max_frames=%d must be 1 or more", what, max_frames);
    return WR_OK;
}

// While a chunk call builds and uploads its state block the handle's hypothesis buffers are the attached ones; every other
// search finds the handle's own again.
struct BeamStreamState {
    DevState &s;
    DevState saved;
    BeamStreamState(wr_decoder *h) : s(h->host), saved(h->host)
    {
        const BeamStreams &bs = h->bs;
        s.bhyps = bs.bhyps; s.btimes = bs.btimes; s.bhyp_lens = bs.bhyp_lens; s.bscores = bs.bscores; s.bvscores = bs.bvscores;
        s.bs_base = bs.base; s.bs_F = bs.F; s.bs_state = bs.state; s.bs_flags = bs.flags;
        s.bctx_score = bs.ctx_score; s.bctx_state = bs.ctx_state; s.btags = bs.btags;      // null unless the block is a biased one
        s.Lmax = bs.max_frames + 1;
    }
    ~BeamStreamState()
    {
        s.bhyps = saved.bhyps; s.btimes = nullptr; s.bhyp_lens = saved.bhyp_lens; s.bscores = saved.bscores; s.bvscores = nullptr;
        s.bs_base = s.bs_F = s.bs_state = nullptr; s.bs_flags = nullptr;
        s.bctx_score = nullptr; s.bctx_state = nullptr; s.btags = nullptr;
        s.cg = ContextGraph{};
        s.Lmax = saved.Lmax;
    }
};

}  // namespace

// decode_stream.hpp: the size behind wr_decoder_beam_stream_workspace_bytes (0 for sizes no handle can have)
size_t wr::beam_stream_bytes(int max_streams, int beam, int max_frames, bool ctx)
{
    if (max_streams < 1 || beam < 1 || beam > kMaxBeam || max_frames < 1 || max_frames >= (1 << 30)) return 0;
    BeamStreams p;
    return beam_stream_carve(max_streams, beam, max_frames, nullptr, &p, ctx);
}

// decode_stream.hpp: wr_decoder_attach_beam_stream
int wr::beam_stream_attach(wr_decoder *h, int max_streams, int beam, int max_frames, void *workspace_d, size_t workspace_bytes,
                           bool ctx)
{
    const char *what = ctx ? "decoder_attach_beam_context_stream" : "decoder_attach_beam_stream";
    WR_TRY(beam_stream_check(what, h, max_streams, beam, max_frames));
    WR_REQUIRE(workspace_d != nullptr, WR_EINVAL, "%s: null workspace", what);
    BeamStreams p;                                // the handle is written only once everything here has succeeded
    const size_t need = beam_stream_carve(max_streams, beam, max_frames, static_cast<char *>(workspace_d), &p, ctx);
    WR_REQUIRE(workspace_bytes >= need, WR_EWORKSPACE, "%s: workspace %zu < required %zu", what, workspace_bytes, need);
    if (hipHostMalloc(reinterpret_cast<void **>(&p.h_flags), (size_t)kStageSlots * max_streams * sizeof(int32_t),
                      hipHostMallocDefault) != hipSuccess) {
        set_error("%s: hipHostMalloc failed", what);
        return WR_ELAUNCH;
    }
    if (h->work) (void)hipStreamSynchronize(h->work);       // no copy still reads the flags of the block being replaced
    if (h->bs.h_flags) (void)hipHostFree(h->bs.h_flags);
    p.attached = true;
    p.ctx = ctx;
    p.n = max_streams; p.beam = beam; p.max_frames = max_frames;
    p.phase.assign(max_streams, 0);
    p.frames.assign(max_streams, 0);
    h->bs = p;
    if (h->stream_lanes == kBeamStreamLanes || h->stream_lanes == kBeamCtxStreamLanes) h->stream_lanes = -1;
    return WR_OK;
}

// decode_stream.hpp: the search behind wr_prefix_beam_search_chunk (decode_stream.cpp has checked the durations -- `dur`
// holds them by jump, D = 0 for a plain model --, every pointer and the handle).  Checks what needs the handle and the
// host's record of the streams, all before the first HIP call, then runs the chunk.
int wr::beam_stream_chunk_body(wr_decoder *h, const float *enc_chunk_d, const int32_t *chunk_lens_d, const float *ctc_logp_chunk_d,
                               int B, int T, int beam, float ctc_weight, float transducer_weight, int blank, const TdtDur &dur,
                               const int32_t *flags, int32_t *hyps_d, int32_t *times_d, int32_t *hyp_lens_d, double *scores_d,
                               double *vscores_d, int32_t *n_hyps_d, void *stream, const BeamCtxArgs *cx)
{
    const char *what = cx ? "prefix_beam_search_context_chunk" : "prefix_beam_search_chunk";
    const bool tdt = dur.D > 0;
    const int my_lanes = cx ? kBeamCtxStreamLanes : kBeamStreamLanes;
    BeamStreams &bs = h->bs;
    WR_REQUIRE(bs.attached && bs.ctx == (cx != nullptr), WR_EINVAL, "%s: no stream state is attached (%s comes first)", what,
               cx ? "wr_decoder_attach_beam_context_stream" : "wr_decoder_attach_beam_stream");
    WR_REQUIRE(B == bs.n && beam == bs.beam, WR_EINVAL, "%s: B=%d, beam=%d differ from the attached %d streams of beam %d", what,
               B, beam, bs.n, bs.beam);
    WR_REQUIRE(T > 0 && T <= h->Tmax, WR_EINVAL, "%s: T=%d exceeds the decoder's Tmax=%d", what, T, h->Tmax);
    const int V = h->d.V - dur.D;                  // token columns of the joiner's row
    if (tdt) {
        WR_REQUIRE(V >= 2, WR_EINVAL, "%s: the joiner has %d outputs, D=%d durations leave %d token columns (2 or more are needed)",
                   what, h->d.V, dur.D, V);
        WR_REQUIRE(h->d.Ve >= V, WR_EINVAL, "%s: the embedding table has %d rows, the token vocabulary %d", what, h->d.Ve, V);
        WR_REQUIRE(ctc_logp_chunk_d || (ctc_weight == 0.f && transducer_weight == 1.f), WR_EINVAL,
                   "%s: no CTC posterior, so (ctc_weight, transducer_weight) must be (0, 1), got (%g, %g)", what, (double)ctc_weight,
                   (double)transducer_weight);
    } else {
        WR_REQUIRE(ctc_logp_chunk_d != nullptr, WR_EINVAL,
                   "%s: the plain search mixes the CTC posterior into every frame, as wr_prefix_beam_search does: it may not be null",
                   what);
    }
    WR_REQUIRE(blank >= 0 && blank < V, WR_EINVAL, "%s: blank %d out of range [0,%d)", what, blank, V);
    // the streams: another search on the handle has overwritten the lanes' predictor slots
    if (h->stream_lanes != my_lanes) {
        for (int &p : bs.phase) { bs.overwritten = bs.overwritten || p != 0; p = 0; }
    }
    const unsigned long long durs = tdt ? pack_durations(dur) : 0;
    bool continues = false;
    for (int b = 0; b < B; ++b) {
        const int f = flags ? flags[b] : 0;
        WR_REQUIRE((f & ~(cx ? 7 : 3)) == 0, WR_EINVAL, "%s: flags[%d]=%d has bits beyond reset (1)%s final (2)%s", what, b, f,
                   cx ? "," : " and", cx ? " and finalised export (4)" : "");
        if (f & 1) {
            WR_REQUIRE(T <= bs.max_frames, WR_EINVAL, "%s: stream %d: a chunk of %d frames exceeds max_frames=%d", what, b, T,
                       bs.max_frames);
            continue;
        }
        WR_REQUIRE(bs.phase[b] != 0 || !bs.overwritten, WR_EINVAL,
                   "%s: stream %d continues, but another search or wr_predictor_step on the handle has overwritten the streams "
                   "since (reset every stream)", what, b);
        WR_REQUIRE(bs.phase[b] != 0, WR_EINVAL, "%s: stream %d continues without ever having been reset", what, b);
        if (bs.phase[b] == 2) {
            WR_REQUIRE(!(f & 2), WR_EINVAL, "%s: stream %d is fed after its final call (reset it first)", what, b);
            continue;                              // finished: the device leaves it as it is
        }
        WR_REQUIRE(bs.frames[b] + T <= bs.max_frames, WR_EINVAL,
                   "%s: stream %d: %ld frames since its reset + a chunk of %d exceed max_frames=%d", what, b, bs.frames[b], T,
                   bs.max_frames);
        continues = true;
    }
    WR_REQUIRE(!continues || (bs.blank == blank && bs.D == dur.D && bs.durs == durs), WR_EINVAL,
               "%s: durations or blank changed in the middle of a stream (blank %d -> %d, D %d -> %d)", what, bs.blank, blank,
               bs.D, dur.D);
    if (cx) {
        const ContextGraph &g = cx->graph;
        WR_REQUIRE(g.S >= 1 && g.A >= 0, WR_EINVAL, "%s: a context graph of S=%d states and A=%d arcs (S >= 1, A >= 0)", what, g.S,
                   g.A);
        WR_REQUIRE(g.arc_begin && g.arc_token && g.arc_next && g.arc_score && g.escape && g.final_, WR_EINVAL,
                   "%s: null context-graph table pointer", what);
        WR_REQUIRE(g.S <= kContextMaxStates && g.A <= kContextMaxArcs, WR_EUNSUPPORTED,
                   "%s: a context graph of S=%d states and A=%d arcs exceeds %d states / %d arcs", what, g.S, g.A,
                   kContextMaxStates, kContextMaxArcs);
    }
    // ---- nothing is refused below this line; the host's record of the streams follows the call
    for (int b = 0; b < B; ++b) {
        const int f = flags ? flags[b] : 0;
        if (f & 1) { bs.phase[b] = 1; bs.frames[b] = 0; }
        if (bs.phase[b] == 1) { bs.frames[b] += T; if (f & 2) bs.phase[b] = 2; }
    }
    bs.overwritten = false;
    bs.blank = blank; bs.D = dur.D; bs.durs = durs;
    h->stream_lanes = -1;                         // until the call has succeeded
    WorkScope scope(h, static_cast<hipStream_t>(stream));
    hipStream_t st = scope.st;
    BeamStreamState swap(h);
    DevState &s = h->host;
    s.enc = enc_chunk_d; s.enc_lens = chunk_lens_d; s.ctc_logp = ctc_logp_chunk_d;
    s.n_utt = B; s.T = T; s.lanes_per_utt = beam; s.n_lanes = B * beam;
    s.beam = beam; s.ctc_weight = ctc_weight; s.tr_weight = transducer_weight; s.blank = blank;
    s.tdt_durs = durs; s.tdt_D = dur.D; s.hyp_frames = nullptr;
    if (cx) s.cg = cx->graph;                      // the table travels in the state block, never in a captured graph
    // the flags ride in the pinned slot of the state block's upload (upload_state waits for the slot's last copy, then
    // records the event behind both copies)
    const int slot = h->stage_next;
    (void)hipEventSynchronize(h->stage_ev[slot]);
    int32_t *hf = bs.h_flags + (size_t)slot * B;
    for (int b = 0; b < B; ++b) hf[b] = flags ? flags[b] : 0;
    if (hipMemcpyAsync(bs.flags, hf, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("%s: flags upload failed", what);
        return WR_ELAUNCH;
    }
    if (int rc = upload_state(h, st)) return rc;
    (void)hipMemsetAsync(s.active_count, 0, 3 * sizeof(int32_t), st);
    (void)hipMemsetAsync(s.lane_active, 0, sizeof(int32_t) * h->d.NLp, st);
    const int NLn = B * beam;
    WR_TRY(launch_ep_all(h, st, (long)B * T, enc_chunk_d, s.ep_all));
    WR_TRY(launch("beam_init_kernel", beam_init_kernel, dim3(NLn), dim3(128), 0, st, h->dev));
    if (cx) {
        if (tdt) {
            WR_TRY(launch("beam_chunk_begin_kernel", beam_chunk_begin_kernel<true, true>, dim3(B), dim3(kBeamUpdThreads), 0, st,
                          h->dev));
            WR_TRY(beam_tdt_steps(h, st, what, NLn, B, T, beam, true, true));
        } else {
            WR_TRY(launch("beam_chunk_begin_kernel", beam_chunk_begin_kernel<false, true>, dim3(B), dim3(kBeamUpdThreads), 0, st,
                          h->dev));
            WR_TRY(beam_plain_steps(h, st, what, NLn, B, T, beam, true, true));
        }
        WR_TRY(launch("beam_context_export_kernel", beam_context_export_kernel, dim3(B), dim3(256), 0, st, h->dev, hyps_d, times_d,
                      hyp_lens_d, scores_d, vscores_d, n_hyps_d, cx->trans_scores, cx->context_scores, cx->tags,
                      cx->context_states));
    } else {
        if (tdt) {
            WR_TRY(launch("beam_chunk_begin_kernel", beam_chunk_begin_kernel<true>, dim3(B), dim3(kBeamUpdThreads), 0, st, h->dev));
            WR_TRY(beam_tdt_steps(h, st, what, NLn, B, T, beam, true));
        } else {
            WR_TRY(launch("beam_chunk_begin_kernel", beam_chunk_begin_kernel<false>, dim3(B), dim3(kBeamUpdThreads), 0, st, h->dev));
            WR_TRY(beam_plain_steps(h, st, what, NLn, B, T, beam, true));
        }
        WR_TRY(launch("beam_stream_export_kernel", beam_stream_export_kernel, dim3(B), dim3(256), 0, st, h->dev, hyps_d, times_d,
                      hyp_lens_d, scores_d, vscores_d, n_hyps_d));
    }
    scope.ok();
    h->stream_lanes = my_lanes;
    return WR_OK;
}

namespace {
// row-major [L][N][H]  <->  k-major [L][Hp][NLp]
__global__ void cache_to_kmajor_kernel(const float *__restrict__ src, int N, int L, int H, int Hp, int NLp, float *__restrict__ dst)
{
    const long total = (long)L * N * H;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % H), n = (int)((i / H) % N), l = (int)(i / ((long)H * N));
        dst[((size_t)l * Hp + k) * NLp + n] = src[i];
    }
}
__global__ void cache_from_kmajor_kernel(const float *__restrict__ src, int N, int L, int H, int Hp, int NLp, float *__restrict__ dst)
{
    const long total = (long)L * N * H;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % H), n = (int)((i / H) % N), l = (int)(i / ((long)H * N));
        dst[i] = src[((size_t)l * Hp + k) * NLp + n];
    }
}

__global__ void step_setup_kernel(DevState *s, const int32_t *tokens, int N)
{
    const int n = blockIdx.x;                      // one workgroup per lane slot
    const int on = n < N;
    const int tok = on ? tokens[n] : 0;
    if (threadIdx.x == 0) {
        s->lane_active[n] = on;
        s->need_pred[n] = on;
        s->lane_t[n] = 0;
        s->token[n] = tok;
        s->comm_slot[n] = n;
        s->new_slot[n] = s->d.NLp + n;
    }
    if (s->d.ptype != kPredLstm) write_embedding_column(s, n, tok);
}

// LSTM step API: caller's cell state [L][N][H] -> the committed slots of the pool; the new slots' cell state -> caller
__global__ void pool_c_import_kernel(DevState *s, const float *__restrict__ src, int N)
{
    const Dims &d = s->d;
    const long total = (long)d.L * N * d.H;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % d.H), n = (int)((i / d.H) % N), l = (int)(i / ((long)d.H * N));
        s->pool_c[((size_t)l * 2 * d.NLp + n) * d.Hp + k] = src[i];
    }
}
__global__ void pool_c_export_kernel(DevState *s, float *__restrict__ dst, int N)
{
    const Dims &d = s->d;
    const long total = (long)d.L * N * d.H;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int k = (int)(i % d.H), n = (int)((i / d.H) % N), l = (int)(i / ((long)d.H * N));
        dst[i] = s->pool_c[((size_t)l * 2 * d.NLp + s->new_slot[n]) * d.Hp + k];
    }
}
}  // namespace

// Single predictor step for `N` lanes through the same kernels the decoders use (step API of
// predictor.py:160-200): tokens + cache in, projected output [N,P] and new cache [L,N,H] out.
extern "C" int wr_predictor_step(wr_decoder *h, const int32_t *tokens_d, const float *cache_h_d, const float *cache_c_d, int N,
                                 float *out_d, float *new_h_d, float *new_c_d, void *stream)
{
    WR_REQUIRE(h && tokens_d && cache_h_d && cache_c_d && out_d && new_h_d && new_c_d, WR_EINVAL,
               "predictor_step: null pointer argument");
    WR_REQUIRE(N > 0 && N <= h->d.NL, WR_EINVAL, "predictor_step: N=%d exceeds the decoder's capacity %d", N, h->d.NL);
    h->stream_lanes = -1;                         // the lanes' streaming state (caches, tokens) is overwritten
    WorkScope scope(h, static_cast<hipStream_t>(stream));
    hipStream_t st = scope.st;
    const Dims &d = h->d;
    DevState &s = h->host;
    s.n_utt = 1; s.T = 1; s.lanes_per_utt = d.NL; s.n_lanes = N; s.enc = nullptr; s.enc_lens = nullptr;
    if (int rc = upload_state(h, st)) return rc;
    // row-major [L][N][H] -> k-major and back, 64 workgroups
    const auto to_kmajor = [&](const float *src, float *dst) {
        return launch("cache_to_kmajor_kernel", cache_to_kmajor_kernel, dim3(64), dim3(256), 0, st, src, N, d.L, d.H, d.Hp, d.NLp, dst);
    };
    const auto from_kmajor = [&](const float *src, float *dst) {
        return launch("cache_from_kmajor_kernel", cache_from_kmajor_kernel, dim3(64), dim3(256), 0, st, src, N, d.L, d.H, d.Hp, d.NLp, dst);
    };
    WR_TRY(launch("step_setup_kernel", step_setup_kernel, dim3(d.NLp), dim3(64), 0, st, h->dev, tokens_d, N));
    if (d.ptype == kPredLstm) {
        // the caller's state becomes the lanes' committed slots: cell states as they are, hidden states through their
        // recurrent products (pool_g = W_hh . h + b, one GEMM per layer); then layer 0, layers >= 1, projection
        WR_TRY(to_kmajor(cache_h_d, s.new_hT));
        WR_TRY(launch("pool_c_import_kernel", pool_c_import_kernel, dim3(64), dim3(256), 0, st, h->dev, cache_c_d, N));
        for (int l = 0; l < d.L; ++l) WR_TRY(launch_gemm<kEpiSlotRow>(recurrent_job(h, l, N, s.comm_slot), d.G4p, N, st));
        WR_TRY(launch("lstm_layer0_kernel", lstm_layer0_kernel, dim3(N), dim3(256), 0, st, h->dev));
    } else {
        WR_TRY(to_kmajor(cache_h_d, s.cache_hT));
        WR_TRY(to_kmajor(cache_c_d, s.cache_cT));
    }
    WR_TRY(launch_predictor(h, N, st));
    // outT [Pp][NLp] -> out [N][P]: the same index map with L = 1
    WR_TRY(launch("cache_from_kmajor_kernel", cache_from_kmajor_kernel, dim3(32), dim3(256), 0, st, s.outT, N, 1, d.P, d.Pp, d.NLp, out_d));
    WR_TRY(from_kmajor(s.new_hT, new_h_d));
    if (d.ptype == kPredLstm) WR_TRY(launch("pool_c_export_kernel", pool_c_export_kernel, dim3(64), dim3(256), 0, st, h->dev, new_c_d, N));
    else WR_TRY(from_kmajor(s.new_cT, new_c_d));
    scope.ok();
    return WR_OK;
}

// ------------------------------------------------------------ hot-word greedy: host side --
namespace {

// where the hot-word workspace puts things: the device struct's own buffers, and what the handle keeps beside it
struct HwPlace {
    HwDev hw;
    float *q_wt, *o_wt, *c_wt;    // the k-major weights, writable (hw holds them const)
    float *ep2, *biasT;
    int32_t *state;
};

// one pass for the size (null base) and for the pointers; every take is 256-byte aligned
size_t hw_carve(const wr_decoder *h, int D, int max_ctx, char *base, HwPlace *p)
{
    Carver c{base, 0};
    const Dims &d = h->d;
    HwDev &v = p->hw;
    const size_t DD = (size_t)D * D, frames = (size_t)h->max_utt * h->Tmax;
    v.q_wt = p->q_wt = c.take<float>(DD);
    v.o_wt = p->o_wt = c.take<float>(DD);
    v.c_wt = p->c_wt = c.take<float>(2 * DD);
    for (int i = 0; i < 2; ++i) { v.kbuf[i] = c.take<float>((size_t)max_ctx * D); v.vbuf[i] = c.take<float>((size_t)max_ctx * D); }
    v.cold_c = c.take<float>(D);
    for (int i = 0; i < 2; ++i) {
        v.mqT[i] = c.take<float>(DD); v.mq_c[i] = c.take<float>(D);
        v.noT[i] = c.take<float>(DD);
        v.mqpT[i] = c.take<float>((size_t)d.Hp * D); v.mqp_c[i] = c.take<float>(D);
    }
    v.c1p_wt = c.take<float>((size_t)d.Hp * D); v.c1p_b = c.take<float>(D);
    v.cold_cp = c.take<float>(D);
    v.gate_tab = c.take<int32_t>(frames);
    p->ep2 = c.take<float>(2 * frames * d.J);
    v.cur_gate = p->state = c.take<int32_t>((size_t)4 * d.NLp);      // cur_gate is the first NLp words of the state
    p->biasT = c.take<float>((size_t)d.Pp * d.NLp);
    return align_up(c.off, 256);
}

int hw_check(const wr_decoder *h, const wr_hotword_weights *hw, int max_ctx)
{
    WR_REQUIRE(h && hw, WR_EINVAL, "hotword: null pointer argument");
    WR_REQUIRE(hw->dim > 0 && hw->heads > 0 && hw->hw_dim > 0 && hw->n_labels > 0 && max_ctx > 0, WR_EINVAL,
               "hotword: non-positive dimension");
    WR_REQUIRE(hw->dim == h->d.E && hw->dim == h->d.P, WR_EINVAL,
               "hotword: dim=%d must equal the encoder (%d) and predictor (%d) output sizes", hw->dim, h->d.E, h->d.P);
    WR_REQUIRE(hw->dim <= 512 && hw->hw_dim <= 256 && hw->n_labels <= 8 && hw->dim % hw->heads == 0 && hw->heads <= 16, WR_EUNSUPPORTED,
               "hotword: dim=%d (<= 512), hw_dim=%d (<= 256), n_labels=%d (<= 8), heads=%d (divides dim, <= 16)", hw->dim,
               hw->hw_dim, hw->n_labels, hw->heads);
    WR_REQUIRE(h->d.ptype != kPredLstm || h->d.Hp <= 4 * hw->dim, WR_EUNSUPPORTED,
               "hotword: LSTM hidden size %d exceeds 4 * dim (%d)", h->d.H, hw->dim);
    WR_REQUIRE((size_t)(21 * hw->dim + hw->heads * max_ctx) * sizeof(float) <= 60 * 1024, WR_EUNSUPPORTED,
               "hotword: max_ctx=%d does not fit the bias kernel's LDS", max_ctx);
    WR_REQUIRE(hw->q_w && hw->q_b && hw->k_w && hw->k_b && hw->v_w && hw->v_b && hw->o_w && hw->o_b && hw->bias_norm_w &&
                   hw->bias_norm_b && hw->combine_w && hw->combine_b && hw->out_norm_w && hw->out_norm_b && hw->hw_enc_w &&
                   hw->hw_enc_b && hw->hw_v_w && hw->hw_v_b && hw->hw_o_w && hw->hw_o_b && hw->hw_norm_w && hw->hw_norm_b &&
                   hw->hw_out_w && hw->hw_out_b, WR_EINVAL, "hotword: null weight pointer");
    return WR_OK;
}

int hw_micro_step(wr_decoder *h, int n_lanes, hipStream_t st)
{
    const Dims &d = h->d;
    // LSTM predictor: the projection runs inside hw_bias_kernel; stateless predictors write outT themselves
    bool recurrent_pending = false;
    WR_TRY(launch_predictor(h, n_lanes, st, d.ptype != kPredLstm, &recurrent_pending));
    const size_t lds = (size_t)(21 * h->hw.D + h->hw.heads * h->hw.max_ctx) * sizeof(float);   // <= 60 KiB (hw_check)
    WR_TRY(launch("hw_bias_kernel", hw_bias_kernel, dim3(n_lanes), dim3(kHwThreads), lds, st, h->dev, h->hw));
    // pred_ffn of the biased predictor output; the joiner activation takes the encoder stream the gate selected
    WR_TRY(launch_pred_ffn(h, pred_ffn_job(h, h->hw_biasT, false, n_lanes, 1, h->hw_ep2, h->hw_state), recurrent_pending, n_lanes, st));
    WR_TRY(launch_gemm<kEpiRowStats>(joint_out_job(h, n_lanes, true), d.Vp, n_lanes, st));
    return launch_greedy_update<true>(h, n_lanes, st);
}

}  // namespace

extern "C" size_t wr_hotword_workspace_bytes(const wr_decoder *h, const wr_hotword_weights *hw, int max_ctx)
{
    if (!h || !hw || hw->dim <= 0 || max_ctx <= 0) return 0;
    HwPlace p{};
    return hw_carve(h, hw->dim, max_ctx, nullptr, &p);
}

extern "C" int wr_decoder_attach_hotword(wr_decoder *h, const wr_hotword_weights *hw, int max_ctx, void *workspace_d,
                                         size_t workspace_bytes, void *stream)
{
    if (int rc = hw_check(h, hw, max_ctx)) return rc;
    WR_REQUIRE(workspace_d != nullptr, WR_EINVAL, "decoder_attach_hotword: null workspace");
    HwPlace p{};                                  // the handle is written only once everything here has succeeded
    const size_t need = hw_carve(h, hw->dim, max_ctx, static_cast<char *>(workspace_d), &p);
    WR_REQUIRE(workspace_bytes >= need, WR_EWORKSPACE, "decoder_attach_hotword: workspace %zu < required %zu", workspace_bytes,
               need);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int D = hw->dim;
    const Dims &d = h->d;
    HwDev &v = p.hw;
    v.D = D; v.heads = hw->heads; v.HW = hw->hw_dim; v.NLAB = hw->n_labels; v.max_ctx = max_ctx;
    WR_TRY(launch_transpose(hw->q_w, D, D, D, D, p.q_wt, st));                  // [out][in] -> [in][out]
    WR_TRY(launch_transpose(hw->o_w, D, D, D, D, p.o_wt, st));
    WR_TRY(launch_transpose(hw->combine_w, D, 2 * D, D, 2 * D, p.c_wt, st));    // [D][2D] -> [2D][D]
    v.q_b = hw->q_b; v.k_w = hw->k_w; v.k_b = hw->k_b; v.v_w = hw->v_w; v.v_b = hw->v_b;
    v.o_b = hw->o_b; v.bn_w = hw->bias_norm_w; v.bn_b = hw->bias_norm_b;
    v.c_b = hw->combine_b; v.on_w = hw->out_norm_w; v.on_b = hw->out_norm_b;
    v.he_w = hw->hw_enc_w; v.he_b = hw->hw_enc_b; v.hv_w = hw->hw_v_w; v.hv_b = hw->hw_v_b; v.ho_w = hw->hw_o_w;
    v.ho_b = hw->hw_o_b; v.hn_w = hw->hw_norm_w; v.hn_b = hw->hw_norm_b; v.hl_w = hw->hw_out_w; v.hl_b = hw->hw_out_b;
    v.lane_active = h->host.lane_active; v.need_pred = h->host.need_pred;
    v.proj_wt = d.ptype == kPredLstm ? h->host.proj_wt : nullptr; v.proj_b = h->host.proj_b;
    v.h_lastT = h->host.new_hT + (size_t)(d.L - 1) * d.Hp * d.NLp;
    v.Hp = d.Hp; v.P = d.P; v.proj_ld = round_up(d.P, 32); v.NLp = d.NLp;
    if (v.proj_wt != nullptr && d.Hp <= D) {
        const long nn = (long)d.Hp * D + D;
        WR_TRY(launch("hw_compose_kernel", hw_compose_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, st, hw->combine_w,
                      hw->combine_b, v.proj_wt, v.proj_b, D, d.P, d.H, d.Hp, v.proj_ld, v.c1p_wt, v.c1p_b));
    }
    (void)hipMemsetAsync(p.biasT, 0, (size_t)d.Pp * d.NLp * sizeof(float), st);   // padded rows / lanes stay zero
    h->hw = p.hw; h->hw_ep2 = p.ep2; h->hw_state = p.state; h->hw_biasT = p.biasT;
    h->hw_attached = true;
    h->hotword.key = -1;
    return WR_OK;
}

extern "C" int wr_greedy_search_hotword(wr_decoder *h, const float *enc_hot_d, const float *enc_cold_d, const float *enc_feat_d,
                                        const int32_t *enc_lens_d, const float *hidden_hot_d, int n_ctx_hot,
                                        const float *hidden_cold_d, int n_ctx_cold, int N, int T, int n_steps, int blank,
                                        int filter_on, int32_t *hyps_d, int32_t *hyp_lens_d, int32_t *trace_d, int trace_cap,
                                        int32_t *trace_lens_d, void *stream)
{
    WR_REQUIRE(h && enc_hot_d && enc_cold_d && enc_feat_d && enc_lens_d && hidden_hot_d && hidden_cold_d && hyps_d &&
                   hyp_lens_d && trace_d && trace_lens_d, WR_EINVAL, "greedy_search_hotword: null pointer argument");
    WR_REQUIRE(h->hw_attached, WR_EINVAL, "greedy_search_hotword: call wr_decoder_attach_hotword first");
    WR_REQUIRE(N > 0 && N <= h->d.NL && N <= h->max_utt, WR_EINVAL, "greedy_search_hotword: N=%d exceeds the decoder's capacity", N);
    WR_REQUIRE(T > 0 && T <= h->Tmax, WR_EINVAL, "greedy_search_hotword: T=%d exceeds the decoder's Tmax=%d", T, h->Tmax);
    WR_REQUIRE(n_steps >= 1 && blank >= 0 && blank < h->d.V && trace_cap >= 1, WR_EINVAL, "greedy_search_hotword: bad n_steps/blank/trace_cap");
    WR_REQUIRE(n_ctx_hot >= 1 && n_ctx_hot <= h->hw.max_ctx && n_ctx_cold >= 1 && n_ctx_cold <= h->hw.max_ctx, WR_EINVAL,
               "greedy_search_hotword: context lists of %d / %d entries (1..%d)", n_ctx_hot, n_ctx_cold, h->hw.max_ctx);
    h->stream_lanes = -1;                         // the lanes' streaming state is overwritten
    WorkScope scope(h, static_cast<hipStream_t>(stream));
    hipStream_t st = scope.st;
    const Dims &d = h->d;
    const HwDev &hw = h->hw;
    DevState &s = h->host;
    s.enc = enc_hot_d; s.enc_lens = enc_lens_d; s.ctc_logp = nullptr;
    s.n_utt = N; s.T = T; s.lanes_per_utt = 1; s.n_lanes = N;
    s.hyps = hyps_d; s.hyp_lens = hyp_lens_d; s.max_hyp = h->max_hyp; s.n_steps = n_steps; s.blank = blank; s.beam = 1;
    s.hw_on = 1; s.hw_filter = filter_on ? 1 : 0; s.hw_nctx[0] = n_ctx_cold; s.hw_nctx[1] = n_ctx_hot;
    s.gate_tab = hw.gate_tab;
    s.cur_gate = h->hw_state; s.gb_flag = h->hw_state + d.NLp; s.gb_end = h->hw_state + 2 * d.NLp; s.last_t = h->hw_state + 3 * d.NLp;
    s.trace = trace_d; s.trace_len = trace_lens_d; s.trace_cap = trace_cap;
    s.biasT = h->hw_biasT;
    const int rc_up = upload_state(h, st);
    s.hw_on = 0;                                  // the host copy goes back to plain greedy for the other entry points
    if (rc_up) return rc_up;
    (void)hipMemsetAsync(s.active_count, 0, 3 * sizeof(int32_t), st);
    (void)hipMemsetAsync(s.lane_active, 0, sizeof(int32_t) * d.NLp, st);
    // loop-invariant work: list projections, the gate of every frame, enc_ffn of both encoder streams
    WR_TRY(launch("hw_kv_kernel", hw_kv_kernel, dim3(n_ctx_cold, 2), dim3(256), 0, st, hw, hidden_cold_d, 0));
    WR_TRY(launch("hw_kv_kernel", hw_kv_kernel, dim3(n_ctx_hot, 2), dim3(256), 0, st, hw, hidden_hot_d, 1));
    {   // short lists: fold the query / output projections into K / V once per call
        const int nc[2] = {n_ctx_cold, n_ctx_hot};
        for (int i = 0; i < 2; ++i)
            if (nc[i] > 1 && hw.heads * nc[i] <= hw.D)
                WR_TRY(launch("hw_fold_kernel", hw_fold_kernel, dim3(hw.heads * nc[i]), dim3(256), 0, st, hw, i, nc[i]));
    }
    if (n_ctx_cold == 1)
        WR_TRY(launch("hw_cold_kernel", hw_cold_kernel, dim3(1), dim3(kHwThreads), (size_t)(3 + kHwThreads / 64) * hw.D * sizeof(float),
                      st, hw));
    WR_TRY(launch("hw_gate_table_kernel", hw_gate_table_kernel, dim3((unsigned)((long)N * T)), dim3(256),
                  (size_t)(hw.D + 2 * hw.HW) * sizeof(float), st, hw, enc_feat_d, (long)N * T));
    WR_TRY(launch_ep_all(h, st, (long)N * T, enc_cold_d, h->hw_ep2));
    WR_TRY(launch_ep_all(h, st, (long)N * T, enc_hot_d, h->hw_ep2 + (size_t)h->max_utt * h->Tmax * d.J));
    WR_TRY(launch("greedy_hw_init_kernel", greedy_hw_init_kernel, dim3(N), dim3(128), 0, st, h->dev));
    // every go-back re-decodes frames, at most once per 0 -> 1 flip of the gate: twice the plain loop's bound
    const long max_micro = 2 * ((long)T * ((long)n_steps + 2) + 1);
    WR_TRY(run_until_idle(
        h, st, "greedy_search_hotword", N, max_micro, " (go-backs exceeded the budget); hypotheses are incomplete",
        [&]() -> GraphSlot & { return h->hotword; }, [&] { return hw_micro_step(h, N, st); }, [] {}));
    scope.ok();
    return WR_OK;
}

#ifdef WR_STAMPS
// diagnostic build only: copy the stamp array to the host and clear it
extern "C" int wr_debug_read_stamps(unsigned long long *host, size_t n_words)
{
    const size_t total = (size_t)wr::kStampSlots * wr::kStampWgs * wr::kStampWaves * wr::kStampPts;
    if (!host || n_words < total) return (int)total;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(host, HIP_SYMBOL(wr::g_stamps), total * sizeof(unsigned long long)) != hipSuccess) return -1;
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(wr::g_stamps)) == hipSuccess) (void)hipMemset(p, 0, total * sizeof(unsigned long long));
    return 0;
}
#endif
