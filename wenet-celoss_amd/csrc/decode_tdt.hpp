// Token-and-duration (TDT) greedy search: what the entry point of decode_tdt.cpp shares with the device decoder of
// decode.hip (include/wr_api.h, "TDT greedy search").
#pragma once

#include "rnnt_tdt.hpp"

namespace wr {

// decode.hip: the search behind wr_greedy_search_tdt, which has checked the durations (`dur` holds them by jump), n_steps
// and every pointer.  Checks what needs the handle (N, T against its capacities, the token vocabulary V = joiner width - D,
// blank, the embedding rows), then runs the micro-steps.
int greedy_tdt_body(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, int N, int T, int n_steps, int blank,
                    const TdtDur &dur, int32_t *hyps_d, int32_t *hyp_lens_d, int32_t *hyp_frames_d, void *stream);

}  // namespace wr
