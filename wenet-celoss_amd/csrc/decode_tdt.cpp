// Token-and-duration (TDT) greedy search: the entry point (include/wr_api.h, "TDT greedy search").  Host code only: what
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
