// Streaming CTC prefix beam search, plain and context-biased: the entry points (include/wr_api.h, "Streaming CTC prefix beam
// search" and "Context-graph biasing in the CTC prefix beam search").  Host code only: every argument is checked here, in the
// order the header states, before the first HIP call; the kernels and their launches are in ctc_decode.hip (ctc_stream.hpp).
#include "ctc_stream.hpp"

using namespace wr;

static size_t state_bytes(int B, int beam, int Lcap, bool ctx)
{
    if (B <= 0 || beam <= 0 || beam > kCtcStreamMaxBeam || Lcap <= 0) return 0;
    return (size_t)B * ctc_stream_state_layout(beam, Lcap, ctx).stride;
}

extern "C" size_t wr_ctc_stream_state_bytes(int B, int beam, int Lcap) { return state_bytes(B, beam, Lcap, false); }

extern "C" size_t wr_ctc_context_stream_state_bytes(int B, int beam, int Lcap) { return state_bytes(B, beam, Lcap, true); }

extern "C" size_t wr_ctc_stream_workspace_bytes(int B, int T, int beam)
{
    if (B <= 0 || T <= 0 || beam <= 0) return 0;
    return ctc_stream_ws_layout(B, T, beam).total;
}

// Both chunk entry points: `what` names the one that was called, `cx` is the biased one's table, flag and outputs.
static int chunk_checked(const char *what, const float *logits_d, const int32_t *lens_d, int B, int T, int V, int beam,
                         int blank, int reset, int frames_done, int Lcap, void *state_d, size_t state_bytes_, int32_t *hyps_d,
                         int32_t *hyp_lens_d, double *scores_d, double *viterbi_d, int32_t *times_d, int32_t *n_hyps_d,
                         int32_t *n_frames_d, void *workspace_d, size_t workspace_bytes, void *stream, const CtcContextArgs *cx)
{
    WR_TRY(ctc_decode_check_shape(B, T, V, blank));
    WR_REQUIRE(logits_d && lens_d && state_d && hyps_d && hyp_lens_d && scores_d && viterbi_d && times_d && n_hyps_d &&
                   n_frames_d && workspace_d &&
                   (!cx || (cx->ctc_scores && cx->context_scores && cx->tags && cx->context_states)),
               WR_EINVAL, "%s: null pointer argument", what);
    WR_REQUIRE(beam >= 1 && beam <= kCtcStreamMaxBeam && beam <= V, WR_EUNSUPPORTED, "%s: beam=%d (1..%d, at most V)", what,
               beam, kCtcStreamMaxBeam);
    WR_REQUIRE(Lcap >= 1, WR_EINVAL, "%s: Lcap=%d must be 1 or more", what, Lcap);
    WR_REQUIRE(frames_done >= 0, WR_EINVAL, "%s: frames_done=%d is negative", what, frames_done);
    WR_REQUIRE(!reset || frames_done == 0, WR_EINVAL, "%s: reset with frames_done=%d (a fresh stream has consumed nothing)", what,
               frames_done);
    WR_REQUIRE((long long)frames_done + T <= Lcap, WR_EUNSUPPORTED, "%s: frames_done=%d + T=%d exceeds Lcap=%d", what,
               frames_done, T, Lcap);
    WR_REQUIRE(state_bytes_ >= state_bytes(B, beam, Lcap, cx != nullptr), WR_EWORKSPACE, "%s: state block too small", what);
    WR_REQUIRE(workspace_bytes >= wr_ctc_stream_workspace_bytes(B, T, beam), WR_EWORKSPACE, "%s: workspace too small", what);
    if (cx) {          // the table: an empty graph (S = 1, A = 0) still has its six arrays, so every pointer must be there
        const ContextGraph &g = cx->graph;
        WR_REQUIRE(g.S >= 1 && g.A >= 0, WR_EINVAL, "%s: context graph with S=%d states, A=%d arcs", what, g.S, g.A);
        WR_REQUIRE(g.arc_begin && g.arc_token && g.arc_next && g.arc_score && g.escape && g.final_, WR_EINVAL,
                   "%s: null context graph pointer", what);
        WR_REQUIRE(g.S <= kContextMaxStates && g.A <= kContextMaxArcs, WR_EUNSUPPORTED,
                   "%s: context graph with S=%d states, A=%d arcs exceeds %d, %d", what, g.S, g.A, kContextMaxStates,
                   kContextMaxArcs);
    }
    return ctc_prefix_beam_chunk_launch(logits_d, lens_d, B, T, V, beam, blank, reset, Lcap, state_d, hyps_d, hyp_lens_d,
                                        scores_d, viterbi_d, times_d, n_hyps_d, n_frames_d, workspace_d, stream, cx);
}

extern "C" int wr_ctc_prefix_beam_search_chunk(const float *logits_d, const int32_t *lens_d, int B, int T, int V, int beam,
                                               int blank, int reset, int frames_done, int Lcap, void *state_d,
                                               size_t state_bytes, int32_t *hyps_d, int32_t *hyp_lens_d, double *scores_d,
                                               double *viterbi_d, int32_t *times_d, int32_t *n_hyps_d, int32_t *n_frames_d,
                                               void *workspace_d, size_t workspace_bytes, void *stream)
{
    return chunk_checked("ctc_prefix_beam_search_chunk", logits_d, lens_d, B, T, V, beam, blank, reset, frames_done, Lcap,
                         state_d, state_bytes, hyps_d, hyp_lens_d, scores_d, viterbi_d, times_d, n_hyps_d, n_frames_d,
                         workspace_d, workspace_bytes, stream, nullptr);
}

extern "C" int wr_ctc_prefix_beam_search_context_chunk(
    const float *logits_d, const int32_t *lens_d, int B, int T, int V, int beam, int blank, int reset, int frames_done, int Lcap,
    void *state_d, size_t state_bytes, const int32_t *arc_begin_d, const int32_t *arc_token_d, const int32_t *arc_next_d,
    const float *arc_score_d, const float *escape_d, const int32_t *final_d, int S, int A, int finalize, int32_t *hyps_d,
    int32_t *hyp_lens_d, double *scores_d, double *viterbi_d, int32_t *times_d, int32_t *n_hyps_d, int32_t *n_frames_d,
    double *ctc_scores_d, double *context_scores_d, int32_t *tags_d, int32_t *context_states_d, void *workspace_d,
    size_t workspace_bytes, void *stream)
{
    const CtcContextArgs cx{{arc_begin_d, arc_token_d, arc_next_d, arc_score_d, escape_d, final_d, S, A}, finalize != 0,
                            ctc_scores_d, context_scores_d, tags_d, context_states_d};
    return chunk_checked("ctc_prefix_beam_search_context_chunk", logits_d, lens_d, B, T, V, beam, blank, reset, frames_done,
                         Lcap, state_d, state_bytes, hyps_d, hyp_lens_d, scores_d, viterbi_d, times_d, n_hyps_d, n_frames_d,
                         workspace_d, workspace_bytes, stream, &cx);
}
