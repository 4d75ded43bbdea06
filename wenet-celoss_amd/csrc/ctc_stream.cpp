// Streaming CTC prefix beam search: the entry points (include/wr_api.h, "Streaming CTC prefix beam search").  Host code
// only: every argument is checked here, in the order the header states, before the first HIP call; the kernels and their
// launches are in ctc_decode.hip (ctc_stream.hpp).
#include "ctc_stream.hpp"

using namespace wr;

extern "C" size_t wr_ctc_stream_state_bytes(int B, int beam, int Lcap)
{
    if (B <= 0 || beam <= 0 || beam > kCtcStreamMaxBeam || Lcap <= 0) return 0;
    return (size_t)B * ctc_stream_state_layout(beam, Lcap).stride;
}

extern "C" size_t wr_ctc_stream_workspace_bytes(int B, int T, int beam)
{
    if (B <= 0 || T <= 0 || beam <= 0) return 0;
    return ctc_stream_ws_layout(B, T, beam).total;
}

extern "C" int wr_ctc_prefix_beam_search_chunk(const float *logits_d, const int32_t *lens_d, int B, int T, int V, int beam,
                                               int blank, int reset, int frames_done, int Lcap, void *state_d,
                                               size_t state_bytes, int32_t *hyps_d, int32_t *hyp_lens_d, double *scores_d,
                                               double *viterbi_d, int32_t *times_d, int32_t *n_hyps_d, int32_t *n_frames_d,
                                               void *workspace_d, size_t workspace_bytes, void *stream)
{
    WR_TRY(ctc_decode_check_shape(B, T, V, blank));
    WR_REQUIRE(logits_d && lens_d && state_d && hyps_d && hyp_lens_d && scores_d && viterbi_d && times_d && n_hyps_d &&
                   n_frames_d && workspace_d,
               WR_EINVAL, "ctc_prefix_beam_search_chunk: null pointer argument");
    WR_REQUIRE(beam >= 1 && beam <= kCtcStreamMaxBeam && beam <= V, WR_EUNSUPPORTED,
               "ctc_prefix_beam_search_chunk: beam=%d (1..%d, at most V)", beam, kCtcStreamMaxBeam);
    WR_REQUIRE(Lcap >= 1, WR_EINVAL, "ctc_prefix_beam_search_chunk: Lcap=%d must be 1 or more", Lcap);
    WR_REQUIRE(frames_done >= 0, WR_EINVAL, "ctc_prefix_beam_search_chunk: frames_done=%d is negative", frames_done);
    WR_REQUIRE(!reset || frames_done == 0, WR_EINVAL,
               "ctc_prefix_beam_search_chunk: reset with frames_done=%d (a fresh stream has consumed nothing)", frames_done);
    WR_REQUIRE((long long)frames_done + T <= Lcap, WR_EUNSUPPORTED,
               "ctc_prefix_beam_search_chunk: frames_done=%d + T=%d exceeds Lcap=%d", frames_done, T, Lcap);
    WR_REQUIRE(state_bytes >= wr_ctc_stream_state_bytes(B, beam, Lcap), WR_EWORKSPACE,
               "ctc_prefix_beam_search_chunk: state block too small");
    WR_REQUIRE(workspace_bytes >= wr_ctc_stream_workspace_bytes(B, T, beam), WR_EWORKSPACE,
               "ctc_prefix_beam_search_chunk: workspace too small");
    return ctc_prefix_beam_chunk_launch(logits_d, lens_d, B, T, V, beam, blank, reset, Lcap, state_d, hyps_d, hyp_lens_d,
                                        scores_d, viterbi_d, times_d, n_hyps_d, n_frames_d, workspace_d, stream);
}

// ---- the biased twin (include/wr_api.h, "Context-graph biasing in the CTC prefix beam search") ----
extern "C" size_t wr_ctc_context_stream_state_bytes(int B, int beam, int Lcap)
{
    if (B <= 0 || beam <= 0 || beam > kCtcStreamMaxBeam || Lcap <= 0) return 0;
    return (size_t)B * ctc_context_state_layout(beam, Lcap).stride;
}

extern "C" int wr_ctc_prefix_beam_search_context_chunk(
    const float *logits_d, const int32_t *lens_d, int B, int T, int V, int beam, int blank, int reset, int frames_done, int Lcap,
    void *state_d, size_t state_bytes, const int32_t *arc_begin_d, const int32_t *arc_token_d, const int32_t *arc_next_d,
    const float *arc_score_d, const float *escape_d, const int32_t *final_d, int S, int A, int finalize, int32_t *hyps_d,
    int32_t *hyp_lens_d, double *scores_d, double *viterbi_d, int32_t *times_d, int32_t *n_hyps_d, int32_t *n_frames_d,
    double *ctc_scores_d, double *context_scores_d, int32_t *tags_d, int32_t *context_states_d, void *workspace_d,
    size_t workspace_bytes, void *stream)
{
    WR_TRY(ctc_decode_check_shape(B, T, V, blank));
    WR_REQUIRE(logits_d && lens_d && state_d && hyps_d && hyp_lens_d && scores_d && viterbi_d && times_d && n_hyps_d &&
                   n_frames_d && ctc_scores_d && context_scores_d && tags_d && context_states_d && workspace_d,
               WR_EINVAL, "ctc_prefix_beam_search_context_chunk: null pointer argument");
    WR_REQUIRE(beam >= 1 && beam <= kCtcStreamMaxBeam && beam <= V, WR_EUNSUPPORTED,
               "ctc_prefix_beam_search_context_chunk: beam=%d (1..%d, at most V)", beam, kCtcStreamMaxBeam);
    WR_REQUIRE(Lcap >= 1, WR_EINVAL, "ctc_prefix_beam_search_context_chunk: Lcap=%d must be 1 or more", Lcap);
    WR_REQUIRE(frames_done >= 0, WR_EINVAL, "ctc_prefix_beam_search_context_chunk: frames_done=%d is negative", frames_done);
    WR_REQUIRE(!reset || frames_done == 0, WR_EINVAL,
               "ctc_prefix_beam_search_context_chunk: reset with frames_done=%d (a fresh stream has consumed nothing)",
               frames_done);
    WR_REQUIRE((long long)frames_done + T <= Lcap, WR_EUNSUPPORTED,
               "ctc_prefix_beam_search_context_chunk: frames_done=%d + T=%d exceeds Lcap=%d", frames_done, T, Lcap);
    WR_REQUIRE(state_bytes >= wr_ctc_context_stream_state_bytes(B, beam, Lcap), WR_EWORKSPACE,
               "ctc_prefix_beam_search_context_chunk: state block too small");
    WR_REQUIRE(workspace_bytes >= wr_ctc_stream_workspace_bytes(B, T, beam), WR_EWORKSPACE,
               "ctc_prefix_beam_search_context_chunk: workspace too small");
    // the table: an empty graph (S = 1, A = 0) still has its six arrays, so every pointer must be there
    WR_REQUIRE(S >= 1 && A >= 0, WR_EINVAL, "ctc_prefix_beam_search_context_chunk: context graph with S=%d states, A=%d arcs", S, A);
    WR_REQUIRE(arc_begin_d && arc_token_d && arc_next_d && arc_score_d && escape_d && final_d, WR_EINVAL,
               "ctc_prefix_beam_search_context_chunk: null context graph pointer");
    WR_REQUIRE(S <= kCtcContextMaxStates && A <= kCtcContextMaxArcs, WR_EUNSUPPORTED,
               "ctc_prefix_beam_search_context_chunk: context graph with S=%d states, A=%d arcs exceeds %d, %d", S, A,
               kCtcContextMaxStates, kCtcContextMaxArcs);
    const CtcContextGraph graph{arc_begin_d, arc_token_d, arc_next_d, arc_score_d, escape_d, final_d, S, A};
    const CtcContextOut ctx{finalize != 0, ctc_scores_d, context_scores_d, tags_d, context_states_d};
    return ctc_prefix_beam_context_chunk_launch(logits_d, lens_d, B, T, V, beam, blank, reset, Lcap, state_d, graph, ctx, hyps_d,
                                                hyp_lens_d, scores_d, viterbi_d, times_d, n_hyps_d, n_frames_d, workspace_d,
                                                stream);
}
