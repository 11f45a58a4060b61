// mx_deck_reverb.hpp -- the deck's reverb (include/mixlab_gpu.h "REVERB"): the setting rules, the per-tick state machine of one deck's
// reverb (clock, ramps, schedule), the descriptors its kernel reads, and the frame arithmetic and block cutting both sides share (internal).
#pragma once
#include <cstdint>
#include <vector>

#include "mx_common.hpp"

namespace mx {

enum { REVERB_LANES = 256, REVERB_TANK = 8, REVERB_DIFF = 4, REVERB_TICK_ON = 1u, REVERB_TICK_RAMP = 2u,
       REVERB_TANK_RING = MX_DECK_REVERB_TANK_RING, REVERB_DIFF_RING = MX_DECK_REVERB_DIFF_RING, REVERB_DIFF_AT = REVERB_TANK * REVERB_TANK_RING };
// MEMORY: the longest block (its frames are at most the reach, at most the longest diffuser) plus the longest delay plus one stays under the ring, so no lane of a
// block overwrites a slot another lane of that block still reads
static_assert(MX_DECK_REVERB_MAX_DIFF + MX_DECK_REVERB_MAX_DELAY + 1 < MX_DECK_REVERB_TANK_RING, "a block's tank writes stay clear of its tank reads");
static_assert(MX_DECK_REVERB_MAX_DIFF + MX_DECK_REVERB_MAX_DIFF < MX_DECK_REVERB_DIFF_RING, "a block's diffuser writes stay clear of its diffuser reads");
static_assert(MX_DECK_REVERB_MIN_DIFF <= MX_DECK_REVERB_MIN_DELAY - 1 && MX_DECK_REVERB_MAX_DIFF <= MX_DECK_REVERB_MAX_DELAY - 1, "the reach lies within MIN_DIFF .. MAX_DIFF");
static_assert(REVERB_DIFF_AT + REVERB_DIFF * REVERB_DIFF_RING == MX_DECK_REVERB_LINE_FLOATS, "MX_DECK_REVERB_LINE_FLOATS is the twelve rings");
static_assert(sizeof(mx_deck_reverb) == 104 && sizeof(mx_deck_reverb_carry) == 120, "the header's sizes");

// what the kernel knows of one deck of a feed that has a reverb in any of its ticks: its port (n_ticks x spt frames, L R adjacent) and its twelve rings (MEMORY)
struct ReverbDeckDev { float2* port; float* lines; };
// ... and of one tick of it: the clock t of the tick's first frame, a, b and gd of PER FRAME, the delays, the reach of BLOCKS, and the eleven ramped values as
// (old, new) -- a tick without REVERB_TICK_RAMP uses `new` as it stands.  A tick without REVERB_TICK_ON has no reverb: the kernel leaves its frames alone.
struct ReverbTickDev {
    uint64_t t0; double a, b, gd; uint32_t delay[REVERB_TANK], diff[REVERB_DIFF]; uint32_t flags, reach;
    float send0, send1, dry0, dry1, wet0, wet1, gain0[REVERB_TANK], gain1[REVERB_TANK];
};
static_assert(sizeof(ReverbTickDev) == 176, "ReverbTickDev is 176 bytes");

__host__ __device__ inline uint32_t reverb_reach_of(uint32_t r) { return r; }
__host__ __device__ inline uint32_t reverb_reach_of(const ReverbTickDev& t) { return (t.flags & REVERB_TICK_ON) ? t.reach : 0u; }
inline uint32_t reverb_reach(const mx_deck_reverb& r) {
    uint32_t reach = r.diff[0];
    for (int j = 1; j < REVERB_DIFF; ++j) reach = r.diff[j] < reach ? r.diff[j] : reach;
    for (int i = 0; i < REVERB_TANK; ++i) reach = r.delay[i] - 1 < reach ? r.delay[i] - 1 : reach;
    return reach;
}

// The block rule (the header's BLOCKS), the same on the host (mx_deck_reverb_plan, mx_deck_debug_last_reverb) and in the kernel: the end of the maximal block that
// starts at frame f0 of the feed, in tick k = f0 / spt, a tick with a reverb.  Frames are counted from the feed's first; `ticks` holds one entry per tick, reach 0 for
// a tick without a reverb.  Frame f of tick kk belongs while the tick has a reverb and f - R(kk) < f0: what it reads was written before the block.
template <class T>
__host__ __device__ inline uint64_t reverb_block_end(uint64_t f0, uint32_t k, uint32_t n_ticks, uint32_t spt, const T* ticks) {
    for (uint32_t kk = k; kk < n_ticks; ++kk) {
        const uint64_t a = (uint64_t)kk * spt, b = a + spt;
        const uint32_t R = reverb_reach_of(ticks[kk]);
        if (!R) return a;
        const uint64_t limit = f0 + R;
        if (limit < b) return limit > a ? limit : a;
    }
    return (uint64_t)n_ticks * spt;
}

// ---- PER FRAME, the same code on the host (mx_deck_reverb_host) and in the kernel.  Every operation is a statement of its own; the build never fuses. ----
// the value of clock s in a ring of `ring` floats: zero below clock 0, whatever the slot holds (the slot index is in range for every s, so the load is unconditional)
__host__ __device__ inline double reverb_at(const float* ring_base, int64_t s, uint32_t ring) {
    const float v = ring_base[(uint64_t)s & (uint64_t)(ring - 1)];
    return s < 0 ? 0.0 : (double)v;
}
__host__ __device__ inline float reverb_gain(float g0, float g1, bool ramp, double w) {
    if (!ramp) return g1;
    const double d = (double)g1 - (double)g0;
    const double p = d * w;
    return (float)((double)g0 + p);
}
// frame n of tick k: port[0], port[1] are the frame's L and R
__host__ __device__ inline void reverb_frame(float* lines, const ReverbTickDev& k, uint32_t n, uint32_t spt, float* port) {
    const uint64_t t = k.t0 + n;
    const bool ramp = (k.flags & REVERB_TICK_RAMP) != 0;
    const double w = (double)n / (double)spt;
    const double send = (double)reverb_gain(k.send0, k.send1, ramp, w), dry = (double)reverb_gain(k.dry0, k.dry1, ramp, w), wet = (double)reverb_gain(k.wet0, k.wet1, ramp, w);
    const double x[2] = {(double)port[0], (double)port[1]};
    double e[2];
#pragma unroll
    for (int c = 0; c < 2; ++c) {                                    // 2., 3.
        double u = send * x[c];
#pragma unroll
        for (int j = 2 * c; j < 2 * c + 2; ++j) {
            float* const q = lines + REVERB_DIFF_AT + j * REVERB_DIFF_RING;
            const double p = reverb_at(q, (int64_t)t - (int64_t)k.diff[j], REVERB_DIFF_RING);
            const double gp = k.gd * p;
            const double v = u - gp;
            const float vf = (float)v;
            q[t & (uint64_t)(REVERB_DIFF_RING - 1)] = vf;
            const double wv = (double)vf;
            const double gw = k.gd * wv;
            u = p + gw;
        }
        e[c] = u;
    }
    double f[REVERB_TANK], h[REVERB_TANK];
#pragma unroll
    for (int i = 0; i < REVERB_TANK; ++i) {                          // 4.
        const float* const r = lines + i * REVERB_TANK_RING;
        const int64_t s = (int64_t)t - (int64_t)k.delay[i];
        const double r0 = reverb_at(r, s, REVERB_TANK_RING), rm = reverb_at(r, s - 1, REVERB_TANK_RING), rp = reverb_at(r, s + 1, REVERB_TANK_RING);
        const double p0 = k.b * r0, pm = k.a * rm, pp = k.a * rp;
        const double s0 = p0 + pm;
        f[i] = s0 + pp;
        const double gn = (double)reverb_gain(k.gain0[i], k.gain1[i], ramp, w);
        h[i] = gn * f[i];
    }
#pragma unroll
    for (int d = 1; d < REVERB_TANK; d <<= 1) {                      // 5.
#pragma unroll
        for (int i = 0; i < REVERB_TANK; ++i) {
            if (i & d) continue;
            const double lo = h[i] + h[i + d], hi = h[i] - h[i + d];
            h[i] = lo; h[i + d] = hi;
        }
    }
    const double C = 0x1.6a09e667f3bcdp-2;
#pragma unroll
    for (int i = 0; i < REVERB_TANK; ++i) {                          // 6.
        const double m = h[i] * C;
        lines[i * REVERB_TANK_RING + (t & (uint64_t)(REVERB_TANK_RING - 1))] = (float)(m + e[i & 1]);
    }
#pragma unroll
    for (int c = 0; c < 2; ++c) {                                    // 7.
        const double d0 = f[c] - f[c + 2], d1 = f[c + 4] - f[c + 6];
        const double sum = d0 + d1;
        const double o = sum * 0.5;
        const double px = dry * x[c], po = wet * o;
        port[c] = (float)(px + po);
    }
}

void deck_reverb_check(const mx_deck_reverb& r);                                     // throws Error(MX_ERR_INVALID) naming the rule
void deck_reverb_design(double rate, double size, double t60, double damp, double diffusion, double send, double dry, double wet, mx_deck_reverb& out);
// (first frame, frames) of every block of a feed of n_ticks ticks of spt frames with these reaches (0: a tick without a reverb)
struct ReverbBlock { uint64_t first, frames; };
void deck_reverb_cut(uint32_t spt, const uint32_t* reach, uint32_t n_ticks, std::vector<ReverbBlock>& out);

// CLOCK, RAMPS and the off -> on rule for one tick of spt frames: s is the reverb as the tick before left it; ev: the tick has an event, ev_set its setting (NULL:
// off).  Returns the tick's descriptor (flags 0: no reverb in this tick) and moves s on.
struct ReverbState { bool on = false; mx_deck_reverb set{}; uint64_t t = 0; };
ReverbTickDev deck_reverb_plan_tick(ReverbState& s, bool ev, const mx_deck_reverb* ev_set, uint32_t spt);
void deck_reverb_host(float* frames, uint32_t spt, uint32_t n_ticks, const mx_deck_reverb* const* settings, float* lines, mx_deck_reverb_carry& carry);

// The reverb of one deck: the setting in force, the clock, the schedule for the next feed, and the twelve rings.  The feed (mx_deck.cpp) asks it for the coming
// ticks' descriptors (plan), launches, and hands the state after them back (commit); a feed that fails commits nothing.
class DeckReverb {
public:
    typedef ReverbState State;
    explicit DeckReverb(const int& device) : device_(device) {}   // (the deck's device, resolved by the deck's constructor)
    void schedule(uint32_t tick, const mx_deck_reverb* r);         // NULL: off from that tick.  Checks the setting; allocates the lines at the first setting.
    void drop_schedule() { sched_.clear(); }
    bool scheduled_beyond(uint32_t n_ticks, uint32_t& tick) const;
    // the coming n_ticks ticks: ticks[n_ticks] (empty for a deck with no reverb and no schedule), the state after them; true when any tick has a reverb
    bool plan(uint32_t n_ticks, uint32_t spt, std::vector<ReverbTickDev>& ticks, State& after) const;
    void commit(const State& after) { st_ = after; sched_.clear(); }
    const State& state() const { return st_; }
    float* lines() const { return (float*)lines_.p; }
    void read_lines(float* dst) const;                              // waits for the device; zeros for a deck that never had a setting
    const void* last_graph = nullptr;   // the graph of the last feed that rendered a reverb: a deck that changes graphs waits for the device once

private:
    struct Event { uint32_t tick; bool on; mx_deck_reverb set; };
    const int& device_;
    State st_;
    std::vector<Event> sched_;          // at most one per tick, in no order
    DevBuf lines_;
};

// the reverb decks of the last feed as mx_deck_debug_last_reverb reads them: per deck the reaches of its ticks (0: no reverb), a copy taken under the feed's lock
struct DeckLastReverb { std::vector<std::vector<uint32_t>> reaches; uint32_t spt = 0; };
DeckLastReverb deck_last_reverb();
void deck_debug_last_reverb(uint32_t out[4]);

}  // namespace mx
