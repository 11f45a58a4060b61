// mx_deck_bars.hpp -- the deck's bars and phrases (include/mixlab_gpu.h "BARS"): the rules that the host function (mx_deck_bars.cpp) and the
// kernels (mx_k_deck_bars.hip) both evaluate, stated once, the launch, and the deck's fifth analysis (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mx_common.hpp"
#include "mx_deck_analysis.hpp"
#include "mx_dev.hpp"
#include "mx_kernels.hpp"

namespace mx {

enum { BR_TILE = 1024, BR_LANES = 256, BR_BLOCK = MX_DECK_BARS_BLOCK, BR_MAX_W = 64, BR_MAX_BEATS = MX_DECK_BARS_MAX_BEATS, BR_MAX_FOLDS = MX_DECK_BARS_MAX_FOLDS };
static const size_t kBarsRecRoom = (size_t)BR_MAX_BEATS * sizeof(mx_deck_beat);

// f(n0 + k) from base = first_q32 + n0 * period_q32 (the host's, in 128 bits: lead 2^32 <= base < lead 2^32 + period).  k <= n_beats <= 16384 and the line lies at or
// before frame n_frames + lead, so the sum stays below 2^63.
__host__ __device__ inline int64_t br_line(uint64_t base, uint64_t period, uint32_t k, uint32_t lead) { return (int64_t)((base + (uint64_t)k * period) >> 32) - (int64_t)lead; }
// the split of a beat [a, c) into its halves [a, h) and [h, c): the first is the shorter one of an odd beat
__host__ __device__ inline int64_t br_half(int64_t a, int64_t c) { return a + ((c - a) >> 1); }
// d(i, j) of two beat vectors
__host__ __device__ inline uint32_t br_dist(const uint32_t* vi, const uint32_t* vj) {
    uint32_t d = 0;
    for (int c = 0; c < 6; ++c) d += vi[c] > vj[c] ? vi[c] - vj[c] : vj[c] - vi[c];
    return d;
}
// whether NOVELTY defines N_W[k]
__host__ __device__ inline bool br_defined(uint32_t k, uint32_t W, uint32_t n_beats) { return k >= W && k + W <= n_beats; }
// what one beat gives a fold: the clamp, per beat
__host__ __device__ inline uint64_t br_clamp(int64_t n) { return n > 0 ? (uint64_t)n : 0u; }

struct DkBarsArgs {
    const uint32_t* track; int64_t n_frames;
    uint64_t base, period;        // br_line's
    uint32_t lead, n_beats;       // n_beats 1 .. 16384
    uint32_t K, M, MQ, w_bar, w_phrase;
    mx_deck_beat* rec;            // [n_beats]
    uint64_t* folds;              // [M + MQ]
};
enum { DK_BARS_FORM_ONE_TILE = 0, DK_BARS_FORM_TILED = 1, DK_BARS_FORM_NOVELTY = 2, DK_BARS_FORM_DEFINED = 3 };
void launch_deck_bars(const DkBarsArgs& a, const DeckAnalyseTaps& taps, uint32_t forms[4], hipStream_t s);

// ---- host ----
struct BarsBeats { int64_t n0; uint64_t base; uint32_t n_beats; };                             // BEATS of checked settings
BarsBeats deck_bars_check(const mx_deck_bars& s, uint64_t n_frames, bool with_track);          // throws Error(MX_ERR_INVALID) naming the rule; without a track: n_beats 0
void deck_bars_tables(const mx_deck_analysis& a, mx_deck_bars& s);
void deck_bars_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_bars& s, mx_deck_beat* recs, uint64_t* H_or_null);
void deck_bars_pick(const uint64_t* H, const mx_deck_bars& s, mx_deck_bar_pick& out);
void deck_grid_next(const mx_deck_beats& grid, int64_t pos, int64_t* index, int64_t* line);

// one buffer, sized once -- room for MX_DECK_BARS_MAX_BEATS records (count_ of them written), then the folds (folds_ words)
class DeckBars : public DeckTrackAnalysis {
public:
    explicit DeckBars(const DeckTrack& deck);
    void analyse(const mx_deck_bars* s);                                   // NULL: frees the results.  Asynchronous on the load stream.
    void read(uint64_t first, uint64_t n, mx_deck_beat* dst);              // waits for the analysis
    void read_folds(uint64_t* H, uint32_t cap);                            // waits for the analysis
    static void debug_last(uint32_t out[4]);
private:
    uint32_t folds_ = 0;
};

}  // namespace mx
