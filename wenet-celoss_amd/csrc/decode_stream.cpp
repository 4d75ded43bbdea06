// Streaming transducer prefix beam search: the entry points (include/wr_api.h, "Streaming transducer prefix beam search").
// Host code only: what needs no handle internals is checked here, before the first HIP call; the kernels, their launches,
// the checks against the handle and the record of the streams are in decode.hip (decode_stream.hpp).
#include "decode_stream.hpp"

using namespace wr;

extern "C" size_t wr_decoder_beam_stream_workspace_bytes(const wr_decoder *h, int max_streams, int beam, int max_frames)
{
    return h ? beam_stream_bytes(max_streams, beam, max_frames) : 0;
}

extern "C" int wr_decoder_attach_beam_stream(wr_decoder *h, int max_streams, int beam, int max_frames, void *workspace_d,
                                             size_t workspace_bytes)
{
    return beam_stream_attach(h, max_streams, beam, max_frames, workspace_d, workspace_bytes);
}

extern "C" int wr_prefix_beam_search_chunk(wr_decoder *h, const float *enc_chunk_d, const int32_t *chunk_lens_d,
                                           const float *ctc_logp_chunk_d, int B, int T, int beam, float ctc_weight,
                                           float transducer_weight, int blank, const int32_t *durations, int D,
                                           const int32_t *flags, int32_t *hyps_d, int32_t *times_d, int32_t *hyp_lens_d,
                                           double *scores_d, double *vscores_d, int32_t *n_hyps_d, void *stream)
{
    const char *what = "prefix_beam_search_chunk";
    TdtDur dur{};                                 // D = 0: a plain model
    if (D != 0 || durations != nullptr) WR_TRY(tdt_durations(what, durations, D, &dur));
    WR_REQUIRE(enc_chunk_d && chunk_lens_d && hyps_d && times_d && hyp_lens_d && scores_d && vscores_d && n_hyps_d, WR_EINVAL,
               "%s: null pointer argument", what);
    WR_REQUIRE(h != nullptr, WR_EINVAL, "%s: null handle", what);
    return beam_stream_chunk_body(h, enc_chunk_d, chunk_lens_d, ctc_logp_chunk_d, B, T, beam, ctc_weight, transducer_weight,
                                  blank, dur, flags, hyps_d, times_d, hyp_lens_d, scores_d, vscores_d, n_hyps_d, stream);
}

// ---- the biased form (include/wr_api.h, "Context-graph biasing in the streaming transducer prefix beam search")
extern "C" size_t wr_decoder_beam_context_stream_workspace_bytes(const wr_decoder *h, int max_streams, int beam, int max_frames)
{
    return h ? beam_stream_bytes(max_streams, beam, max_frames, true) : 0;
}

extern "C" int wr_decoder_attach_beam_context_stream(wr_decoder *h, int max_streams, int beam, int max_frames, void *workspace_d,
                                                     size_t workspace_bytes)
{
    return beam_stream_attach(h, max_streams, beam, max_frames, workspace_d, workspace_bytes, true);
}

extern "C" int wr_prefix_beam_search_context_chunk(wr_decoder *h, const float *enc_chunk_d, const int32_t *chunk_lens_d,
                                                   const float *ctc_logp_chunk_d, int B, int T, int beam, float ctc_weight,
                                                   float transducer_weight, int blank, const int32_t *durations, int D,
                                                   const int32_t *flags, int32_t *hyps_d, int32_t *times_d, int32_t *hyp_lens_d,
                                                   double *scores_d, double *vscores_d, int32_t *n_hyps_d,
                                                   const int32_t *arc_begin_d, const int32_t *arc_token_d,
                                                   const int32_t *arc_next_d, const float *arc_score_d, const float *escape_d,
                                                   const int32_t *final_d, int S, int A, double *trans_scores_d,
                                                   double *context_scores_d, int32_t *tags_d, int32_t *context_states_d,
                                                   void *stream)
{
    const char *what = "prefix_beam_search_context_chunk";
    TdtDur dur{};                                 // D = 0: a plain model
    if (D != 0 || durations != nullptr) WR_TRY(tdt_durations(what, durations, D, &dur));
    WR_REQUIRE(enc_chunk_d && chunk_lens_d && hyps_d && times_d && hyp_lens_d && scores_d && vscores_d && n_hyps_d &&
                   trans_scores_d && context_scores_d && tags_d && context_states_d,
               WR_EINVAL, "%s: null pointer argument", what);
    WR_REQUIRE(h != nullptr, WR_EINVAL, "%s: null handle", what);
    const BeamCtxArgs cx{{arc_begin_d, arc_token_d, arc_next_d, arc_score_d, escape_d, final_d, S, A},
                         trans_scores_d, context_scores_d, tags_d, context_states_d};
    return beam_stream_chunk_body(h, enc_chunk_d, chunk_lens_d, ctc_logp_chunk_d, B, T, beam, ctc_weight, transducer_weight,
                                  blank, dur, flags, hyps_d, times_d, hyp_lens_d, scores_d, vscores_d, n_hyps_d, stream, &cx);
}
