// Token-and-duration (TDT) greedy and prefix beam search: the entry points (include/wr_api.h, "TDT greedy search" and "TDT
// prefix beam search").  Host code only: what
// needs no handle internals is checked here, before the first HIP call; the kernels, their launches and the checks
// against the handle are in decode.hip (decode_tdt.hpp).
#include "decode_tdt.hpp"

using namespace wr;

extern "C" int wr_greedy_search_tdt(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, int N, int T,
                                    int n_steps, int blank, const int32_t *durations, int D, int32_t *hyps_d,
                                    int32_t *hyp_lens_d, int32_t *hyp_frames_d, void *stream)
{
    TdtDur dur;
    WR_TRY(tdt_durations("greedy_search_tdt", durations, D, &dur));
    WR_REQUIRE(n_steps >= 1, WR_EINVAL, "greedy_search_tdt: n_steps=%d must be 1 or more", n_steps);
    WR_REQUIRE(enc_out_d && enc_lens_d && hyps_d && hyp_lens_d, WR_EINVAL, "greedy_search_tdt: null pointer argument");
    WR_REQUIRE(h != nullptr, WR_EINVAL, "greedy_search_tdt: null handle");
    return greedy_tdt_body(h, enc_out_d, enc_lens_d, N, T, n_steps, blank, dur, hyps_d, hyp_lens_d, hyp_frames_d, stream);
}

extern "C" int wr_prefix_beam_search_tdt(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d,
                                         const float *ctc_logp_d, int B, int T, int beam, float ctc_weight,
                                         float transducer_weight, int blank, const int32_t *durations, int D, int32_t *hyps_d,
                                         int32_t *hyp_lens_d, double *scores_d, int32_t *n_hyps_d, void *stream)
{
    TdtDur dur;
    WR_TRY(tdt_durations("prefix_beam_search_tdt", durations, D, &dur));
    WR_REQUIRE(enc_out_d && enc_lens_d && hyps_d && hyp_lens_d && scores_d && n_hyps_d, WR_EINVAL,
               "prefix_beam_search_tdt: null pointer argument");
    WR_REQUIRE(h != nullptr, WR_EINVAL, "prefix_beam_search_tdt: null handle");
    return beam_tdt_body(h, enc_out_d, enc_lens_d, ctc_logp_d, B, T, beam, ctc_weight, transducer_weight, blank, dur, hyps_d,
                         hyp_lens_d, scores_d, n_hyps_d, stream);
}

extern "C" int wr_decoder_last_counters(const wr_decoder *h, int32_t *out)
{
    WR_REQUIRE(h != nullptr && out != nullptr, WR_EINVAL, "decoder_last_counters: null pointer argument");
    decoder_counters(h, out);
    return WR_OK;
}
