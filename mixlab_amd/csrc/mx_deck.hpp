// mx_deck.hpp -- the deck (include/mixlab_gpu.h "the deck"): host state machine, the descriptors its feed kernel reads, and the launch plan both sides share (internal).
#pragma once
#include <cstdint>
#include <vector>

#include "mx_common.hpp"

namespace mx {

class Graph;

enum { DECK_Q = 32, DECK_WINDOW = 4 * MX_DECK_CHUNK + MX_DECK_TAPS, DECK_BANK_FLOATS = (MX_DECK_PHASES + 1) * MX_DECK_TAPS };

// what the kernel knows of one deck of a feed
struct DeckDev { const uint32_t* track; float* out; int64_t n_frames; };
// ... and of one tick of it: mx_deck_tick without what the kernel does not read, plus the form the host chose for the tick
enum { DECK_FORM_ZERO = 0, DECK_FORM_PLAY = 1 };
struct DeckTickDev { int64_t pos, step, dstep; uint32_t loop_in, loop_len; uint32_t form, bank; };

// u(n) of a tick (the header's POSITION)
__host__ __device__ inline int64_t deck_u(int64_t pos, int64_t step, int64_t dstep, int64_t n) { return pos + n * step + dstep * (n * (n - 1) / 2); }
// floor division / floormod by a positive divisor
__host__ __device__ inline int64_t deck_floordiv(int64_t a, int64_t b) { int64_t q = a / b; if ((a % b) != 0 && a < 0) --q; return q; }
__host__ __device__ inline int64_t deck_fold(int64_t u, int64_t in_q, int64_t len_q) { int64_t r = (u - in_q) % len_q; if (r < 0) r += len_q; return in_q + r; }

// the lanes of a tick differ in phase unless it moves by whole frames at a constant step (then two coefficient rows serve the whole tick)
__host__ __device__ inline bool deck_phase_varies(const DeckTickDev& t) { return t.dstep != 0 || (t.step & 0xFFFFFFFFll) != 0; }

// The launch plan of one chunk (frames [n0, n0 + cnt) of a playing tick), the same on the host (mx_deck_debug_last_feed) and in the kernel: the chunk STREAMS when its
// positions move in one direction and, in a looping tick, lie within one wrap of the loop -- then its taps read the frames [lo, lo + len) and `shift` (a multiple of the
// loop length, Q32) is what folding subtracts from every u of the chunk.  Anything else GATHERS.
struct DeckChunkPlan { bool stream; int64_t lo; uint32_t len; int64_t shift; };
__host__ __device__ inline DeckChunkPlan deck_chunk_plan(const DeckTickDev& t, uint32_t n0, uint32_t cnt) {
    DeckChunkPlan p{false, 0, 0, 0};
    const int64_t s0 = t.step + (int64_t)n0 * t.dstep, s1 = t.step + (int64_t)(n0 + cnt - 1) * t.dstep;   // the increments inside the chunk lie between these
    if ((s0 < 0 && s1 > 0) || (s0 > 0 && s1 < 0)) return p;
    int64_t ua = deck_u(t.pos, t.step, t.dstep, n0), ub = deck_u(t.pos, t.step, t.dstep, (int64_t)n0 + cnt - 1);
    if (ua > ub) { const int64_t x = ua; ua = ub; ub = x; }
    if (t.loop_len) {
        const int64_t in_q = (int64_t)t.loop_in << DECK_Q, len_q = (int64_t)t.loop_len << DECK_Q;
        const int64_t wa = deck_floordiv(ua - in_q, len_q);
        if (wa != deck_floordiv(ub - in_q, len_q)) return p;
        p.shift = wa * len_q;
    }
    const int64_t lo = ((ua - p.shift) >> DECK_Q) - 15, hi = ((ub - p.shift) >> DECK_Q) + 16;
    if (hi - lo + 1 > (int64_t)DECK_WINDOW) return p;   // (cannot happen while |step| <= 4 * 2^32: 4 (cnt - 1) + 32 frames at the most)
    p.stream = true; p.lo = lo; p.len = (uint32_t)(hi - lo + 1);
    return p;
}

// ---- key-lock (the header's KEY-LOCK; mx_k_deck_keylock.hip) ----
// what the two kernels know of one key-locked deck of a feed.  rec[0], rec[1]: the two grains before the feed's first (from `state`, which the search kernel reads at its
// start and writes at its end); rec[2 + k]: grain k of grains[0 .. n_grains).
struct KlGrainIn { int64_t a; uint32_t first, _pad; };
struct KlRec { int64_t g; int32_t delta; uint32_t dist; };
struct KlDeckDev { const uint32_t* track; float* out; int64_t n_frames, pitch; KlRec* rec; int64_t* state; const KlGrainIn* grains; uint32_t n_grains, log_hop, overlap, radius, bank, _pad; };
// ... and of one tick of it: frame n has clock tt = m0 + n, lies in grain rec[gi0 + (tt >> log_hop)] at m = tt & (hop - 1); first0: grain rec[gi0] has no previous grain
struct KlTickDev { uint32_t m0, gi0, first0, play; };

// ---- host ----
void deck_keylock_check(const mx_deck_keylock& k);                                   // throws Error(MX_ERR_INVALID) naming the rule
void deck_keylock_search(const int16_t* interleaved, uint64_t n_frames, int64_t C, int64_t A, uint32_t overlap, uint32_t radius, int32_t& delta, uint32_t& dist);
// analysis (the header's ANALYSIS; mx_k_deck_analyse.hip)
void deck_analysis_check(const mx_deck_analysis& a);                                 // throws Error(MX_ERR_INVALID) naming the rule
void deck_analysis_bands(double rate, double f_lo, double f_hi, uint32_t taps, mx_deck_analysis& a);
uint64_t deck_column_count(uint64_t n_frames, uint32_t column);
void deck_columns_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_analysis& a, uint64_t first, uint64_t n, mx_deck_column* cols, uint64_t* R_or_null);
void deck_beatgrid(const mx_deck_column* cols, uint64_t n_cols, const uint64_t* R, uint32_t max_lag, uint32_t column, double rate, double bpm_lo, double bpm_hi, mx_deck_grid& out);
// whole-track tonality and loudness (the header's KEY AND LOUDNESS; mx_k_deck_tonality.hip, mx_k_deck_loudness.hip)
void deck_tonality_check(const mx_deck_tonality& t);                                 // throws Error(MX_ERR_INVALID) naming the rule
uint64_t deck_tonality_count(uint64_t n_frames, const mx_deck_tonality& t);
void deck_tonality_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_tonality& t, uint64_t first, uint64_t n, void* dst);
void deck_loudness_check(const mx_deck_loudness& l);                                 // throws Error(MX_ERR_INVALID) naming the rule
uint64_t deck_loudness_count(uint64_t n_frames, uint32_t block_frames);
void deck_loudness_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_loudness& l, mx_loudness_tick* dst, uint64_t cap);
// the fine beat grid and sync (the header's FINE GRID; mx_deck_finegrid.cpp, mx_k_deck_finegrid.hip)
void deck_finegrid_check(const mx_deck_finegrid& s, uint64_t n_frames, bool with_track);   // throws Error(MX_ERR_INVALID) naming the rule; without a track: every rule but first_hop < N
uint64_t deck_finegrid_count(uint64_t n_frames, uint32_t hop);
void deck_finegrid_span(uint64_t centre_q16, uint64_t halfwidth_q16, uint32_t beat_limit, uint64_t n_hops, uint32_t hop, mx_deck_finegrid& out, uint32_t* clipped_or_null);
uint64_t deck_finegrid_period(double period_columns, uint32_t column, uint32_t hop);
void deck_finegrid_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_finegrid& s, mx_deck_comb* recs, uint32_t* w_or_null);
void deck_finegrid_pick(const mx_deck_comb* recs, const mx_deck_finegrid& s, double rate, mx_deck_fine_pick& out);
void deck_sync(const mx_deck_beats& leader, int64_t leader_pos, int64_t leader_step, const mx_deck_beats& follower, int64_t follower_pos, mx_deck_sync_result& out);
void deck_check(const mx_deck_params& p, uint64_t n_frames);                         // throws Error(MX_ERR_INVALID) naming the rule
void deck_plan(const mx_deck_head& in, const mx_deck_params* params, const int64_t* seek, uint32_t spt, uint64_t n_frames, mx_deck_tick& tick, mx_deck_head& out);
int64_t deck_step(uint32_t track_rate, uint32_t graph_rate, double speed);
const float* deck_tables_host();                                                       // MX_DECK_BANKS x DECK_BANK_FLOATS, computed once
void deck_stream_retired(hipStream_t s);                                               // the stream is going away: the feed's staging slots last used on it let go of it

class Deck {
public:
    Deck(uint64_t n_frames, int device);
    ~Deck();
    Deck(const Deck&) = delete; Deck& operator=(const Deck&) = delete;
    void load_i16(uint64_t first, const int16_t* interleaved, uint64_t n);
    void schedule(uint32_t tick, const mx_deck_params* params, const int64_t* seek);
    void read_ticks(uint32_t first, uint32_t n, mx_deck_tick* dst) const;
    const mx_deck_head& head() const { return head_; }
    uint64_t n_frames() const { return n_frames_; }
    int device() const { return device_; }
    static void feed(Deck* const* decks, const uint32_t* nodes, size_t n, Graph& g, uint32_t n_ticks);
    static void debug_last_feed(uint32_t out[6]);
    void set_keylock(const mx_deck_keylock* k);                            // NULL: off.  Restarts the grain clock.
    uint32_t grain_count() const { return (uint32_t)grains_.size(); }
    void read_grains(uint32_t first, uint32_t n, mx_deck_grain* dst);      // waits for the device
    static void debug_last_keylock(uint32_t out[4]);
    void analyse(const mx_deck_analysis* a);                               // NULL: frees the results.  Asynchronous on the load stream.
    void read_columns(uint64_t first, uint64_t n, mx_deck_column* dst);    // waits for the analysis
    void read_autocorr(uint64_t* R, uint32_t cap);                         // waits for the analysis
    static void debug_last_analysis(uint32_t out[4]);
    void analyse_tonality(const mx_deck_tonality* t);                      // NULL: frees the results.  Asynchronous on the load stream.
    void read_tonality(uint64_t first, uint64_t n, void* dst, size_t cap_bytes);   // waits for the analysis
    static void debug_last_tonality(uint32_t out[4]);
    void analyse_loudness(const mx_deck_loudness* l);                      // NULL: frees the results.  Asynchronous on the load stream.
    void read_loudness(uint64_t first, uint64_t n, mx_loudness_tick* dst);  // waits for the analysis
    static void debug_last_loudness(uint32_t out[4]);
    void analyse_finegrid(const mx_deck_finegrid* s);                      // NULL: frees the results.  Asynchronous on the load stream.
    void read_finegrid(uint64_t first, uint64_t n, mx_deck_comb* dst);     // waits for the analysis
    void read_fine_onsets(uint64_t first, uint64_t n, uint32_t* w);        // waits for the analysis
    static void debug_last_finegrid(uint32_t out[4]);

private:
    void fetch_grains();
    struct Event { uint32_t tick; bool has_params, has_seek; mx_deck_params params; int64_t seek; };
    uint64_t n_frames_; int device_;
    DevBuf track_;
    hipStream_t load_stream_ = nullptr; hipEvent_t loaded_ = nullptr; bool load_pending_ = false;
    mx_deck_head head_{};
    std::vector<Event> sched_;          // at most one per tick, in no order
    std::vector<mx_deck_tick> ticks_;   // the last feed's records
    // key-lock: the setting, the grain clock t (playing output frames since the last restart), and the graph of the last feed (another one restarts the clock)
    bool kl_on_ = false; mx_deck_keylock kl_{}; uint32_t kl_bank_ = 0, kl_log_hop_ = 0;
    uint64_t kl_t_ = 0;
    const Graph* last_graph_ = nullptr;
    uint64_t last_lineage_ = 0;               // Graph::lineage() of that feed: a graph that adopted the last one's state is the same graph to the grain clock
    DevBuf kl_state_;                   // g of the last two grains, 2 x int64: written and read by the search kernel only
    DevBuf kl_rec_;                     // KlRec x (2 + the grains of the last feed)
    std::vector<mx_deck_grain> grains_; // the last feed's grain records; g / delta / dist are fetched from kl_rec_ by read_grains
    bool grains_fetched_ = true;
    // analysis: one buffer -- columns (an_cols_ x 56 bytes), R (an_lag_ x 8), onsets (an_cols_ x 4) -- written on load_stream_ only; an_cols_ = 0: none
    DevBuf an_;
    uint64_t an_cols_ = 0; uint32_t an_lag_ = 0;
    // whole-track tonality: one buffer -- ton_segs_ records of ton_rec_bytes_, then the decimated frames -- and the table set of ton_tab_for_ with its decimator taps ton_fir_ (kept while the settings
    // that shape them stay); loudness: one buffer -- loud_blocks_ records, then the walk states.  All written on load_stream_ only; a count of 0: none
    DevBuf ton_, ton_tab_;
    uint64_t ton_segs_ = 0; size_t ton_rec_bytes_ = 0; mx_deck_tonality ton_tab_for_{}; int16_t ton_fir_[64] = {};
    DevBuf loud_;
    uint64_t loud_blocks_ = 0;
    // fine grid: one buffer -- room for 8192 comb records, then w (fg_hops_ x 4 bytes) -- written on load_stream_ only; fg_periods_ = 0: none
    DevBuf fg_;
    uint32_t fg_periods_ = 0; uint64_t fg_hops_ = 0;
};

}  // namespace mx
