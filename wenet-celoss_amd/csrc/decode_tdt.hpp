// Token-and-duration (TDT) greedy and prefix beam search: what the entry points of decode_tdt.cpp share with the device
// decoder of decode.hip (include/wr_api.h, "TDT greedy search" and "TDT prefix beam search").
#pragma once

#include "rnnt_tdt.hpp"

namespace wr {

// decode.hip: the search behind wr_greedy_search_tdt, which has checked the durations (`dur` holds them by jump), n_steps
// and every pointer.  Checks what needs the handle (N, T against its capacities, the token vocabulary V = joiner width - D,
// blank, the embedding rows), then runs the micro-steps.
int greedy_tdt_body(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, int N, int T, int n_steps, int blank,
                    const TdtDur &dur, int32_t *hyps_d, int32_t *hyp_lens_d, int32_t *hyp_frames_d, void *stream);

// decode.hip: the search behind wr_prefix_beam_search_tdt (include/wr_api.h, "TDT prefix beam search"), which has checked
// the durations, every pointer and the handle.  Checks what needs the handle (beam, B * beam and T against its capacities,
// the token vocabulary, blank, the embedding rows) and that a missing CTC posterior comes with weights (0, 1), then runs
// the steps until no utterance has a frame left.
int beam_tdt_body(wr_decoder *h, const float *enc_out_d, const int32_t *enc_lens_d, const float *ctc_logp_d, int B, int T,
                  int beam, float ctc_weight, float transducer_weight, int blank, const TdtDur &dur, int32_t *hyps_d,
                  int32_t *hyp_lens_d, double *scores_d, int32_t *n_hyps_d, void *stream);

// decode.hip: the three counters the last polling search read back (wr_decoder_last_counters); `h` and `out` are not null
void decoder_counters(const wr_decoder *h, int32_t *out);

}  // namespace wr
