// mx_deck_echo.hpp -- the deck's beat echo (include/mixlab_gpu.h "ECHO"): the setting rules, the per-tick state machine of one deck's echo
// (clock, ramps, schedule), the descriptors its kernel reads, and the block cutting both sides share (internal).
#pragma once
#include <cstdint>
#include <vector>

#include "mx_common.hpp"

namespace mx {

enum { ECHO_LOG_RING = 19, ECHO_RING = 1 << ECHO_LOG_RING, ECHO_LANES = 1024, ECHO_TICK_ON = 1u, ECHO_TICK_PINGPONG = 2u, ECHO_TICK_RAMP = 4u };

// what the kernel knows of one deck of a feed that has an echo in any of its ticks: its port (n_ticks x spt frames, L R adjacent) and its delay line (ECHO_RING frames)
struct EchoDeckDev { float2* port; float2* line; };
// ... and of one tick of it: the clock t of the tick's first frame, the delay, a and b of PER FRAME, and the three ramped gains as (old, new) -- a tick without
// ECHO_TICK_RAMP uses `new` as it stands.  A tick without ECHO_TICK_ON has no echo: the kernel leaves its frames alone.
struct EchoTickDev { uint64_t t0; double a, b; uint32_t delay, flags; float send0, send1, fb0, fb1, wet0, wet1; };
static_assert(sizeof(EchoTickDev) == 56, "EchoTickDev is 56 bytes");

__host__ __device__ inline uint32_t echo_delay_of(uint32_t d) { return d; }
__host__ __device__ inline uint32_t echo_delay_of(const EchoTickDev& t) { return (t.flags & ECHO_TICK_ON) ? t.delay : 0u; }

// The block rule (the header's BLOCKS), the same on the host (mx_deck_echo_plan, mx_deck_debug_last_echo, the choice of form) and in the kernel: the end of the
// maximal block that starts at frame f0 of the feed, in tick k = f0 / spt, a tick with an echo.  Frames are counted from the feed's first; `ticks` holds one entry per
// tick, delay 0 for a tick without an echo.  Frame f of tick kk belongs while the tick has an echo and f - D(kk) + 1 < f0: what it reads was written before the block.
template <class T>
__host__ __device__ inline uint64_t echo_block_end(uint64_t f0, uint32_t k, uint32_t n_ticks, uint32_t spt, const T* ticks) {
    for (uint32_t kk = k; kk < n_ticks; ++kk) {
        const uint64_t a = (uint64_t)kk * spt, b = a + spt;
        const uint32_t D = echo_delay_of(ticks[kk]);
        if (!D) return a;
        const uint64_t limit = f0 + D - 1;
        if (limit < b) return limit > a ? limit : a;
    }
    return (uint64_t)n_ticks * spt;
}

void deck_echo_check(const mx_deck_echo& e);                                        // throws Error(MX_ERR_INVALID) naming the rule
uint32_t deck_echo_delay(const mx_deck_beats& grid, int64_t step_q32, uint32_t num, uint32_t den);
// (first frame, frames) of every block of a feed of n_ticks ticks of spt frames with these delays (0: a tick without an echo)
struct EchoBlock { uint64_t first, frames; };
void deck_echo_cut(uint32_t spt, const uint32_t* delay, uint32_t n_ticks, std::vector<EchoBlock>& out);
// true when the echo frames of the feed are one block: the form without a barrier renders them
bool deck_echo_one_block(uint32_t spt, const uint32_t* delay, uint32_t n_ticks);

// The echo of one deck: the setting in force, the clock, the schedule for the next feed, and the delay line.  The feed (mx_deck.cpp) asks it for the coming ticks'
// descriptors (plan), launches, and hands the state after them back (commit); a feed that fails commits nothing.
class DeckEcho {
public:
    struct State { bool on = false; mx_deck_echo set{}; uint64_t t = 0; };
    explicit DeckEcho(const int& device) : device_(device) {}   // (the deck's device, resolved by the deck's constructor)
    void schedule(uint32_t tick, const mx_deck_echo* e);        // NULL: off from that tick.  Checks the setting; allocates the line at the first setting.
    void drop_schedule() { sched_.clear(); }
    bool scheduled_beyond(uint32_t n_ticks, uint32_t& tick) const;
    // the coming n_ticks ticks: ticks[n_ticks] (empty for a deck with no echo and no schedule), the state after them; true when any tick has an echo
    bool plan(uint32_t n_ticks, uint32_t spt, std::vector<EchoTickDev>& ticks, State& after) const;
    void commit(const State& after) { st_ = after; sched_.clear(); }
    const State& state() const { return st_; }
    float2* line() const { return (float2*)line_.p; }
    const void* last_graph = nullptr;   // the graph of the last feed that rendered an echo: a deck that changes graphs waits for the device once

private:
    struct Event { uint32_t tick; bool on; mx_deck_echo set; };
    const int& device_;
    State st_;
    std::vector<Event> sched_;          // at most one per tick, in no order
    DevBuf line_;
};

// the echo decks of the last feed as mx_deck_debug_last_echo reads them: per deck the delays of its ticks (0: no echo), a copy taken under the feed's lock (mx_deck.cpp)
struct DeckLastEcho { std::vector<std::vector<uint32_t>> delays; uint32_t spt = 0; };
DeckLastEcho deck_last_echo();
void deck_debug_last_echo(uint32_t out[4]);

}  // namespace mx
