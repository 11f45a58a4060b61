// mx_deck_filter.hpp -- the deck's resonant sweep filter (include/mixlab_gpu.h "FILTER"): the setting rules, the per-tick state machine of one
// deck's filter (ramps, schedule, off -> on), the descriptors its kernel reads, and the frame arithmetic both sides share (internal).
#pragma once
#include <cstdint>
#include <vector>

#include "mx_common.hpp"

namespace mx {

enum { FILTER_BLOCK = 64, FILTER_TICK_ON = 1u, FILTER_TICK_RAMP = 2u, FILTER_TICK_CLEAR = 4u };

// what the kernel knows of one deck of a feed that has a filter in any of its ticks: its port (n_ticks x spt frames, L R adjacent) and its four state values
// (s1 s2 of L, s1 s2 of R)
struct FilterDeckDev { float2* port; double* state; };
// ... and of one tick of it: g, k and wet as (old, new) -- a tick without FILTER_TICK_RAMP uses `new` as it stands.  FILTER_TICK_CLEAR: the state is zero at the
// tick's first frame (off -> on).  A tick without FILTER_TICK_ON has no filter: the kernel leaves its frames alone.
struct FilterTickDev { uint32_t flags, kind; double g0, g1, k0, k1, w0, w1; };
static_assert(sizeof(FilterTickDev) == 56, "FilterTickDev is 56 bytes");

// ---- PER FRAME, the same code on the host (mx_deck_filter_host) and in the kernel.  Every operation is a statement of its own; the build never fuses. ----
struct FilterCoef { double kn, wn, a1, a2, a3; };
__host__ __device__ inline FilterCoef filter_coef(const FilterTickDev& t, uint32_t n, uint32_t spt) {
    double gn = t.g1, kn = t.k1, wn = t.w1;
    if (t.flags & FILTER_TICK_RAMP) {
        const double w = (double)n / (double)spt;
        const double dg = t.g1 - t.g0, dk = t.k1 - t.k0, dw = t.w1 - t.w0;
        const double pg = dg * w, pk = dk * w, pw = dw * w;
        gn = t.g0 + pg; kn = t.k0 + pk; wn = t.w0 + pw;
    }
    const double gk = gn + kn;
    const double gg = gn * gk;
    const double d = 1.0 + gg;
    const double a1 = 1.0 / d;
    const double a2 = gn * a1;
    const double a3 = gn * a2;
    return FilterCoef{kn, wn, a1, a2, a3};
}
// the recurrence of one channel: v1 and v2 of this frame, s1 and s2 moved on
__host__ __device__ inline void filter_step(double x, double a1, double a2, double a3, double& s1, double& s2, double& v1, double& v2) {
    const double v3 = x - s2;
    const double p1 = a1 * s1, p2 = a2 * v3;
    v1 = p1 + p2;
    const double q1 = a2 * s1, q2 = a3 * v3;
    const double q = q1 + q2;
    v2 = s2 + q;
    const double d1 = v1 + v1, d2 = v2 + v2;
    s1 = d1 - s1;
    s2 = d2 - s2;
}
// the response picked from v1 and v2, and the wet mix
__host__ __device__ inline float filter_out(uint32_t kind, double x, double kn, double wn, double v1, double v2) {
    double f;
    if (kind == MX_DECK_FILTER_LP) f = v2;
    else if (kind == MX_DECK_FILTER_BP) f = v1;
    else {
        const double kv = kn * v1;
        const double nf = x - kv;
        f = kind == MX_DECK_FILTER_HP ? nf - v2 : nf;
    }
    const double diff = f - x;
    const double m = wn * diff;
    return (float)(x + m);
}

void deck_filter_check(const mx_deck_filter& f);                                     // throws Error(MX_ERR_INVALID) naming the rule
void deck_filter_design(uint32_t kind, double cutoff_hz, double q, double rate, double wet, mx_deck_filter& out);
void deck_filter_knob(double knob, double rate, double q, mx_deck_filter& out, uint32_t& on);

// RAMPS and the off -> on rule for one tick: `on` / `set` are the filter as the tick before left it; ev: the tick has an event, ev_set its setting (NULL: off).
// Returns the tick's descriptor (flags 0: no filter in this tick) and moves on / set on.
struct FilterState { bool on = false; mx_deck_filter set{}; };
FilterTickDev deck_filter_plan_tick(FilterState& s, bool ev, const mx_deck_filter* ev_set);
void deck_filter_host(float* frames, uint32_t spt, uint32_t n_ticks, const mx_deck_filter* const* settings, mx_deck_filter_carry& carry);

// The filter of one deck: the setting in force, the schedule for the next feed, and the four state values in device memory.  The feed (mx_deck.cpp) asks it for the
// coming ticks' descriptors (plan), launches, and hands the state after them back (commit); a feed that fails commits nothing.
class DeckFilter {
public:
    typedef FilterState State;
    explicit DeckFilter(const int& device) : device_(device) {}   // (the deck's device, resolved by the deck's constructor)
    void schedule(uint32_t tick, const mx_deck_filter* f);        // NULL: off from that tick.  Checks the setting; allocates the state at the first setting.
    void drop_schedule() { sched_.clear(); }
    bool scheduled_beyond(uint32_t n_ticks, uint32_t& tick) const;
    // the coming n_ticks ticks: ticks[n_ticks] (empty for a deck with no filter and no schedule), the state after them; true when any tick has a filter
    bool plan(uint32_t n_ticks, std::vector<FilterTickDev>& ticks, State& after) const;
    void commit(const State& after) { st_ = after; sched_.clear(); }
    const State& state() const { return st_; }
    double* dev_state() const { return (double*)state_.p; }
    void read_state(double s[4]) const;                             // waits for the device; zeros when off or never on
    const void* last_graph = nullptr;   // the graph of the last feed that rendered a filter: a deck that changes graphs waits for the device once

private:
    struct Event { uint32_t tick; bool on; mx_deck_filter set; };
    const int& device_;
    State st_;
    std::vector<Event> sched_;          // at most one per tick, in no order
    DevBuf state_;
};

// the filter decks of the last feed as mx_deck_debug_last_filter reads them: out[0 .. 4), a copy taken under the feed's lock (mx_deck.cpp)
struct DeckLastFilter { uint32_t out[4] = {0, 0, 0, 0}; };
DeckLastFilter deck_last_filter();

}  // namespace mx
