// Streaming CTC prefix beam search: what the entry points of ctc_stream.cpp share with the kernels of ctc_decode.hip
// (include/wr_api.h, "Streaming CTC prefix beam search").
#pragma once

#include "context_graph.hpp"

namespace wr {

constexpr int kCtcStreamMaxBeam = 16;          // = kMaxCtcBeam of ctc_decode.hip
constexpr int kCtcStreamLists = 3;             // tokens, times_b, times_nb

// One stream's part of the state block (byte offsets from the stream's start; `stride` bytes per stream).
//   head    int32[4]: a marker made of (beam, Lcap), a_next, the number of entries, the sequence buffer in use
//   pb, pnb, vb, vnb  double[beam];  hash  uint64[beam];  len, last  int32[beam]
//   seq     int32[3][2][beam][Lcap]: tokens / times_b / times_nb, each double-buffered
// The biased search's block (`ctx`) has its own layout: the plain one, then, behind the plain stride,
//   csc     double[beam]: the entries' bonuses;  cst  int32[beam]: their context-graph states
//   tag     int32[2][beam][Lcap]: a fourth list, the tags, double-buffered like the tokens it travels with
// so it is larger than the plain block for every (beam, Lcap).  csc_off / cst_off / tag_off are 0 in the plain layout,
// whose kernel instantiation never reads them.
struct CtcStreamState {
    size_t pb_off, pnb_off, vb_off, vnb_off, hash_off, len_off, last_off, seq_off, stride, csc_off, cst_off, tag_off;
};

constexpr int kCtcContextLists = 4;            // tokens, times_b, times_nb, tags

__host__ __device__ inline CtcStreamState ctc_stream_state_layout(int beam, int Lcap, bool ctx)
{
    CtcStreamState s;
    s.csc_off = 0; s.cst_off = 0; s.tag_off = 0;
    size_t off = 16;
    s.pb_off = off;   off += (size_t)beam * sizeof(double);
    s.pnb_off = off;  off += (size_t)beam * sizeof(double);
    s.vb_off = off;   off += (size_t)beam * sizeof(double);
    s.vnb_off = off;  off += (size_t)beam * sizeof(double);
    s.hash_off = off; off += (size_t)beam * sizeof(unsigned long long);
    s.len_off = off;  off += (size_t)beam * sizeof(int32_t);
    s.last_off = off; off += (size_t)beam * sizeof(int32_t);
    off = (off + 15) / 16 * 16;
    s.seq_off = off;  off += (size_t)kCtcStreamLists * 2 * beam * Lcap * sizeof(int32_t);
    off = (off + 255) / 256 * 256;
    if (ctx) {
        s.csc_off = off;  off += (size_t)beam * sizeof(double);
        s.cst_off = off;  off += (size_t)beam * sizeof(int32_t);
        off = (off + 15) / 16 * 16;
        s.tag_off = off;  off += (size_t)2 * beam * Lcap * sizeof(int32_t);
        off = (off + 255) / 256 * 256;
    }
    s.stride = off;
    return s;
}

// What the biased call adds to the plain one's arguments: the table, the flag and the four outputs.
struct CtcContextArgs {
    ContextGraph graph;
    int finalize;
    double *ctc_scores, *context_scores;
    int32_t *tags, *context_states;
};

struct CtcStreamWs {
    size_t tkv_off, tki_off, total;
};

inline CtcStreamWs ctc_stream_ws_layout(int B, int T, int beam)
{
    CtcStreamWs w;
    const size_t rows = (size_t)B * T;
    size_t off = 0;
    w.tkv_off = off; off = align_up(off + rows * beam * sizeof(float), 256);
    w.tki_off = off; off = align_up(off + rows * beam * sizeof(int32_t), 256);
    w.total = off;
    return w;
}

// ctc_decode.hip: the shape checks every CTC decode entry point starts with (B, T positive, V > 1, blank inside V, V <= 16320)
int ctc_decode_check_shape(int B, int T, int V, int blank);

// ctc_decode.hip: the launches behind wr_ctc_prefix_beam_search_chunk and wr_ctc_prefix_beam_search_context_chunk (`cx`),
// which have checked every argument: the fused log-softmax + top-`beam` of the chunk's B * T frames, then one workgroup per
// stream that loads its beam from the state block, consumes lens[b] frames, stores the beam back and exports.  With `cx`
// the kernel's biased instantiation runs, on the biased layout of the state block.
int ctc_prefix_beam_chunk_launch(const float *logits_d, const int32_t *lens_d, int B, int T, int V, int beam, int blank,
                                 int reset, int Lcap, void *state_d, int32_t *hyps_d, int32_t *hyp_lens_d, double *scores_d,
                                 double *viterbi_d, int32_t *times_d, int32_t *n_hyps_d, int32_t *n_frames_d,
                                 void *workspace_d, void *stream, const CtcContextArgs *cx);

}  // namespace wr
