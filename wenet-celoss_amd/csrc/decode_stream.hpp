// Streaming transducer prefix beam search: what the entry points of decode_stream.cpp share with the device decoder of
// decode.hip (include/wr_api.h, "Streaming transducer prefix beam search" and "Context-graph biasing in the streaming
// transducer prefix beam search").
#pragma once

#include "context_graph.hpp"
#include "rnnt_tdt.hpp"

namespace wr {

// What wr_prefix_beam_search_context_chunk adds to the plain chunk call: the context graph's table and the four further
// outputs.
struct BeamCtxArgs {
    ContextGraph graph;
    double *trans_scores, *context_scores;
    int32_t *tags, *context_states;
};

// decode.hip: bytes of the block wr_decoder_attach_beam_stream takes (`ctx`: wr_decoder_attach_beam_context_stream, whose
// block also holds every entry's bonus, graph state and tags); 0 for sizes no handle can have
size_t beam_stream_bytes(int max_streams, int beam, int max_frames, bool ctx = false);

// decode.hip: wr_decoder_attach_beam_stream / wr_decoder_attach_beam_context_stream (`ctx`) -- checks the sizes against the
// handle and the block against its size, then places the streams' buffers in it; every stream starts as never reset, and
// the block of the other form, if one was attached, is replaced
int beam_stream_attach(wr_decoder *h, int max_streams, int beam, int max_frames, void *workspace_d, size_t workspace_bytes,
                       bool ctx = false);

// decode.hip: the search behind wr_prefix_beam_search_chunk, which has checked the durations (`dur` holds them by jump; D = 0:
// a plain model), every pointer and the handle.  Checks what needs the handle (attached state, B, beam, T, the token
// vocabulary, the posterior, blank) and the host's record of every stream (flags, resets, final calls, max_frames, a change
// of durations or blank), all before the first HIP call, then runs the chunk.  `cx`: the biased call
// (wr_prefix_beam_search_context_chunk) -- the attached state must be the biased form's, flag bit 2 is legal, and the
// table's sizes and pointers are checked last.
int beam_stream_chunk_body(wr_decoder *h, const float *enc_chunk_d, const int32_t *chunk_lens_d, const float *ctc_logp_chunk_d,
                           int B, int T, int beam, float ctc_weight, float transducer_weight, int blank, const TdtDur &dur,
                           const int32_t *flags, int32_t *hyps_d, int32_t *times_d, int32_t *hyp_lens_d, double *scores_d,
                           double *vscores_d, int32_t *n_hyps_d, void *stream, const BeamCtxArgs *cx = nullptr);

}  // namespace wr
