// mx_deck_finegrid.hpp -- the deck's fine beat grid (include/mixlab_gpu.h "FINE GRID"): the rules that the host function
// (mx_deck_finegrid.cpp) and the kernels (mx_k_deck_finegrid.hip) both evaluate, stated once, the launch, and the deck's fourth analysis (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mx_common.hpp"
#include "mx_deck_analysis.hpp"
#include "mx_dev.hpp"

namespace mx {

enum { FG_LANES = MX_DECK_FINEGRID_LANES, FG_TILE = 256, FG_HALO_BEFORE = 2, FG_HALO_AFTER = 1 };
static const uint64_t FG_PERIOD_MIN = (uint64_t)4 << 16, FG_PERIOD_MAX = (uint64_t)32768 << 16;

// s^2 of one track frame as the deck stores it (L in the low half); at most 2^32
__host__ __device__ inline uint64_t fg_square(uint32_t frame) {
    const int32_t s = (int32_t)(int16_t)(frame & 0xffffu) + (int32_t)(int16_t)(frame >> 16);
    const uint32_t m = (uint32_t)(s < 0 ? -s : s);
    return (uint64_t)m * m;
}
// o[i] from A[i] and A[i - 1]: subtract, clamp, then shift
__host__ __device__ inline uint32_t fg_onset(uint32_t a, uint32_t before) { return (a > before ? a - before : 0u) >> 4; }
// the tooth weight from three onsets
__host__ __device__ inline uint32_t fg_tooth(uint32_t o_before, uint32_t o, uint32_t o_after) { return o_before + 2u * o + o_after; }
// ceil(P): the phases of a candidate
__host__ __device__ inline uint32_t fg_phases(uint64_t P) { return (uint32_t)((P + 65535u) >> 16); }
// one (candidate, phase) against another under the tie rule: the larger score, then the smaller phase
__host__ __device__ inline bool fg_better(uint64_t s, uint32_t phi, uint64_t s0, uint32_t phi0) { return s > s0 || (s == s0 && phi < phi0); }
// the teeth of phase 0 that fit N hops from first_hop on at period P, cut at max_beats: the trip count of the loop over k (first_hop < N)
inline uint64_t fg_trip(uint64_t N, uint32_t first_hop, uint64_t P, uint32_t max_beats) {
    const uint64_t fit = (((N - first_hop) << 16) + P - 1u) / P;   // the k with (k P) >> 16 < N - first_hop, i.e. k P < (N - first_hop) 2^16
    return max_beats && max_beats < fit ? max_beats : fit;
}

struct DkFineArgs {
    const uint32_t* track; int64_t n_frames;
    uint32_t log_hop, N;          // N <= 2^26
    uint32_t n_periods, first_hop;
    uint64_t period0, dperiod;
    uint32_t trip;                // fg_trip at period0, the smallest period (at most 2^24)
    uint32_t* w;                  // [N]
    mx_deck_comb* rec;            // [n_periods]
};
enum { DK_FINE_FORM_ONE_PASS = 0, DK_FINE_FORM_STRIDED = 1, DK_FINE_FORM_ONSET = 2, DK_FINE_FORM_TRIP = 3 };
void launch_deck_finegrid(const DkFineArgs& a, uint32_t forms[4], hipStream_t s);
// w[0 .. N) alone (the tempo map's onsets are these); the onset workgroups it launched
uint32_t launch_deck_fine_onsets(const uint32_t* track, int64_t n_frames, uint32_t log_hop, uint32_t N, uint32_t* w, hipStream_t s);

// ---- host ----
void deck_finegrid_check(const mx_deck_finegrid& s, uint64_t n_frames, bool with_track);   // throws Error(MX_ERR_INVALID) naming the rule; without a track: every rule but first_hop < N
uint64_t deck_finegrid_count(uint64_t n_frames, uint32_t hop);
void deck_finegrid_span(uint64_t centre_q16, uint64_t halfwidth_q16, uint32_t beat_limit, uint64_t n_hops, uint32_t hop, mx_deck_finegrid& out, uint32_t* clipped_or_null);
uint64_t deck_finegrid_period(double period_columns, uint32_t column, uint32_t hop);
void deck_finegrid_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_finegrid& s, mx_deck_comb* recs, uint32_t* w_or_null);
void deck_finegrid_pick(const mx_deck_comb* recs, const mx_deck_finegrid& s, double rate, mx_deck_fine_pick& out);
void deck_sync(const mx_deck_beats& leader, int64_t leader_pos, int64_t leader_step, const mx_deck_beats& follower, int64_t follower_pos, mx_deck_sync_result& out);

// one buffer -- room for MX_DECK_FINEGRID_MAX_PERIODS comb records (count_ of them written), then w (hops_ x 4 bytes)
class DeckFineGrid : public DeckTrackAnalysis {
public:
    explicit DeckFineGrid(const DeckTrack& deck);
    void analyse(const mx_deck_finegrid* s);                               // NULL: frees the results.  Asynchronous on the load stream.
    void read(uint64_t first, uint64_t n, mx_deck_comb* dst);              // waits for the analysis
    void read_onsets(uint64_t first, uint64_t n, uint32_t* w);             // waits for the analysis
    static void debug_last(uint32_t out[4]);
private:
    uint64_t hops_ = 0;
};

}  // namespace mx
