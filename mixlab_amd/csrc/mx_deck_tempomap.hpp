// mx_deck_tempomap.hpp -- the deck's tempo map (include/mixlab_gpu.h "TEMPO MAP"): the rules that the host function (mx_deck_tempomap.cpp) and
// the kernel (mx_k_deck_tempomap.hip) both evaluate, stated once (the onset and tie rules are FINE GRID's fg_*), the launch, and the deck's sixth analysis (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mx_common.hpp"
#include "mx_deck_analysis.hpp"
#include "mx_deck_finegrid.hpp"

namespace mx {

enum { TM_LANES = 256, TM_GROUP = MX_DECK_TEMPOMAP_GROUP, TM_MAX_WINDOW = MX_DECK_TEMPOMAP_MAX_WINDOW, TM_STAGED_MAX = MX_DECK_TEMPOMAP_STAGED_MAX };

// E_v - v T: the hops of window v (v < V, so v T < N)
__host__ __device__ inline uint32_t tm_window_len(uint32_t v, uint32_t W, uint32_t T, uint32_t N) {
    const uint64_t a = (uint64_t)v * T;
    return (uint32_t)((a + W < N ? a + W : (uint64_t)N) - a);
}
// V of N hops
inline uint64_t tm_windows(uint64_t N, uint32_t W, uint32_t T) { return N <= W ? 1u : (N - W + T - 1u) / T + 1u; }

// which form a launch takes: the host's rule (mx_k_deck_tempomap.hip states the measurement behind it), or a forced one (tools/deck_tempomap_forms.cpp)
enum { TM_FORM_RULE = 0, TM_FORM_STAGED = 1, TM_FORM_GLOBAL = 2 };

struct DkTempoArgs {
    const uint32_t* track; int64_t n_frames;
    uint32_t log_hop, N;          // N <= 2^26
    uint32_t n_periods, V;        // V * n_periods <= 2^20
    uint32_t W, T;
    uint64_t period0, dperiod;
    uint32_t trip;                // fg_trip(min(W, N), 0, period0, 0): at most 4096
    uint32_t form;                // TM_FORM_*
    uint32_t* w;                  // [N]
    mx_deck_comb* rec;            // [V * n_periods]
};
enum { DK_TEMPO_FORM_STAGED = 0, DK_TEMPO_FORM_GLOBAL = 1, DK_TEMPO_FORM_ONSET = 2, DK_TEMPO_FORM_TRIP = 3 };
void launch_deck_tempomap(const DkTempoArgs& a, uint32_t forms[4], hipStream_t s);
void launch_deck_tempomap_comb(const DkTempoArgs& a, uint32_t forms[4], hipStream_t s);   // the comb alone, over a w that is there (the cost tools time it by itself)

// ---- host ----
uint32_t deck_tempomap_check(const mx_deck_tempomap& s, uint64_t n_frames);   // V; throws Error(MX_ERR_INVALID) naming the rule
void deck_tempomap_span(uint64_t centre_q16, uint64_t halfwidth_q16, uint32_t window_beats, uint32_t stride_beats, uint64_t n_hops, uint32_t hop, mx_deck_tempomap& out,
                        uint32_t* clipped_or_null);
void deck_tempomap_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_tempomap& s, mx_deck_comb* recs, uint32_t* w_or_null);
void deck_tempomap_path(const mx_deck_comb* recs, uint32_t n_windows, uint32_t n_periods, uint64_t penalty, uint32_t* index);
void deck_tempomap_segments(const mx_deck_comb* recs, const mx_deck_tempomap& s, uint64_t n_frames, const uint32_t* index, mx_deck_tempo_segment* segs);
void deck_tempomap_at(const mx_deck_tempo_segment* segs, uint32_t n, int64_t pos, mx_deck_beats* grid, uint32_t* segment);
int64_t deck_tempomap_step(const mx_deck_beats& grid, int64_t out_period);

// one buffer -- the records (count_ = V * n_periods of them), then w (hops_ x 4 bytes) behind the room the records of THIS analysis take
class DeckTempoMap : public DeckTrackAnalysis {
public:
    explicit DeckTempoMap(const DeckTrack& deck);
    void analyse(const mx_deck_tempomap* s);                               // NULL: frees the results.  Asynchronous on the load stream.
    void read(uint64_t first, uint64_t n, mx_deck_comb* dst);              // waits for the analysis
    void read_onsets(uint64_t first, uint64_t n, uint32_t* w);             // waits for the analysis
    static void debug_last(uint32_t out[4]);
private:
    uint64_t hops_ = 0;
    size_t w_offset_ = 0;   // where w starts in the buffer: behind the records of the last analysis
};

}  // namespace mx
