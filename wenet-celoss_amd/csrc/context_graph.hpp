// The context graph of the biased searches (include/wr_api.h, "Context-graph biasing in the CTC prefix beam search" and
// "... in the streaming transducer prefix beam search"): one deterministic table, state 0 the root, and the one walk over
// it.  The CTC chunk kernel takes the table as a kernel argument, the device decoder carries it by value in its state
// block (never in a captured graph).
#pragma once

#include "wr_common.hpp"

namespace wr {

constexpr int kContextMaxStates = 65536;
constexpr int kContextMaxArcs = 1048576;

// Device pointers: arc_begin[S + 1] CSR offsets, arc_token / arc_next / arc_score [A] (tokens strictly increasing within a
// state), escape / final_ [S].
struct ContextGraph {
    const int32_t *arc_begin, *arc_token, *arc_next;
    const float *arc_score, *escape;
    const int32_t *final_;
    int S, A;
};

struct ContextStep {
    int state;         // the state after the token
    float score;       // the arc's score, or the escape of the state left; the caller adds it: bonus + (double)score
    int tag;           // bit 0: the token starts a phrase, bit 1: it ends one
};

// next(state, token): runtime/core/decoder/context_graph.cc:86-108 on the table, the arc found by one binary search.  The
// incoming state is clamped into [0, S), every CSR bound into [0, A] and arc_next into [0, S) before it is used as an
// index.  A token without an arc goes back to the root and is not retried from there.
__host__ __device__ __forceinline__ ContextStep context_graph_next(const ContextGraph &g, int state, int tok)
{
    state = state < 0 ? 0 : (state < g.S ? state : g.S - 1);
    int lo = g.arc_begin[state], end = g.arc_begin[state + 1];
    lo = lo < 0 ? 0 : (lo < g.A ? lo : g.A);
    end = end < lo ? lo : (end < g.A ? end : g.A);
    int hi = end;
    while (lo < hi) {                                                  // first arc whose token is >= tok
        const int mid = lo + ((hi - lo) >> 1);
        if (g.arc_token[mid] < tok) lo = mid + 1;
        else hi = mid;
    }
    if (lo < end && g.arc_token[lo] == tok) {
        int nx = g.arc_next[lo];
        nx = nx < 0 ? 0 : (nx < g.S ? nx : g.S - 1);
        return {nx, g.arc_score[lo], (state == 0 ? 1 : 0) | (g.final_[nx] != 0 ? 2 : 0)};
    }
    return {0, g.escape[state], 0};
}

}  // namespace wr
