// mx_deck.hpp -- the deck (include/mixlab_gpu.h "the deck"): host state machine, the descriptors its feed kernel reads, and the launch plan both sides share (internal).
#pragma once
#include <cstdint>
#include <vector>

#include "mx_common.hpp"
#include "mx_deck_bars.hpp"
#include "mx_deck_columns.hpp"
#include "mx_deck_echo.hpp"
#include "mx_deck_filter.hpp"
#include "mx_deck_finegrid.hpp"
#include "mx_deck_loudkey.hpp"
#include "mx_deck_reverb.hpp"
#include "mx_deck_tempomap.hpp"

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
void deck_check(const mx_deck_params& p, uint64_t n_frames);                         // throws Error(MX_ERR_INVALID) naming the rule
void deck_plan(const mx_deck_head& in, const mx_deck_params* params, const int64_t* seek, uint32_t spt, uint64_t n_frames, mx_deck_tick& tick, mx_deck_head& out);
int64_t deck_step(uint32_t track_rate, uint32_t graph_rate, double speed);
const float* deck_tables_host();                                                       // MX_DECK_BANKS x DECK_BANK_FLOATS, computed once
void deck_stream_retired(hipStream_t s);                                               // the stream is going away: the feed's staging slots last used on it let go of it

// key-lock of one deck: the setting, the grain clock t (playing output frames since the last restart), and the graph of the last feed (another one restarts the clock)
struct DeckKeylock {
    bool on = false; mx_deck_keylock k{}; uint32_t bank = 0, log_hop = 0;
    uint64_t t = 0;
    const Graph* last_graph = nullptr;
    uint64_t last_lineage = 0;          // Graph::lineage() of that feed: a graph that adopted the last one's state is the same graph to the grain clock
    DevBuf state;                       // g of the last two grains, 2 x int64: written and read by the search kernel only
    DevBuf rec;                         // KlRec x (2 + the grains of the last feed)
    std::vector<mx_deck_grain> grains;  // the last feed's grain records; g / delta / dist are fetched from rec by read_grains
    bool grains_fetched = true;
};
// the key-locked ticks and grain counts of the last feed as mx_deck_debug_last_keylock reads them: a copy, taken under the feed's lock (mx_deck.cpp)
struct DeckKlTick { KlTickDev t; uint32_t log_hop, overlap; };
struct DeckLastKeylock { std::vector<DeckKlTick> ticks; uint32_t spt = 0, searched = 0, unsearched = 0; };
DeckLastKeylock deck_last_keylock();

// The track, the transport state machine and the feed (mx_deck.cpp), key-lock (mx_deck_keylock.cpp), the sweep filter, the echo and the reverb
// (mx_deck_filter.hpp, mx_deck_echo.hpp, mx_deck_reverb.hpp: members with their own setting, schedule and device memory -- four state values, a delay line, twelve rings), and the six whole-track analyses, each a member that holds its own results and sees of the deck a DeckTrack and nothing else (mx_deck_analysis.hpp).
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
    uint32_t grain_count() const { return (uint32_t)keylock_.grains.size(); }
    void read_grains(uint32_t first, uint32_t n, mx_deck_grain* dst);      // waits for the device
    static void debug_last_keylock(uint32_t out[4]);

private:
    void fetch_grains();
    struct Event { uint32_t tick; bool has_params, has_seek; mx_deck_params params; int64_t seek; };
    uint64_t n_frames_; int device_;
    DevBuf track_;
    hipStream_t load_stream_ = nullptr; hipEvent_t loaded_ = nullptr; bool load_pending_ = false;
    DeckTrack for_analyses_;            // the four fields above that an analysis reads, as the constructor left them
    mx_deck_head head_{};
    std::vector<Event> sched_;          // at most one per tick, in no order
    std::vector<mx_deck_tick> ticks_;   // the last feed's records
    DeckKeylock keylock_;

public:
    // the whole-track analyses (mx_abi_deck.cpp calls them directly)
    DeckColumns columns{for_analyses_};
    DeckTonality tonality{for_analyses_};
    DeckLoudness loudness{for_analyses_};
    DeckFineGrid finegrid{for_analyses_};
    DeckBars bars{for_analyses_};
    DeckTempoMap tempomap{for_analyses_};
    // the beat echo behind the feed and key-lock (mx_abi_deck.cpp calls it directly; the feed plans, launches and commits it)
    DeckEcho echo{device_};
    // the sweep filter between them and the echo (the same protocol: plan, launch, commit)
    DeckFilter filter{device_};
    // the reverb behind the echo, last of the passes (the same protocol)
    DeckReverb reverb{device_};
};

}  // namespace mx
