// mx_deck_echo.cpp -- the deck's beat echo, host side (include/mixlab_gpu.h "ECHO"): the setting rules, the delay of a beat fraction in exact
// integers, the per-tick state machine (clock, ramps, schedule), the delay line, and the block cutting restated for the host (mx_deck_echo_plan,
// mx_deck_debug_last_echo).  The descriptors travel with the feed's (mx_deck.cpp); the kernel is mx_k_deck_echo.hip.
#include "mx_deck_echo.hpp"

#include <algorithm>
#include <cmath>

namespace mx {

void deck_echo_check(const mx_deck_echo& e) {
    if (e.delay < MX_DECK_ECHO_MIN_DELAY || e.delay > MX_DECK_ECHO_MAX_DELAY) throw Error(MX_ERR_INVALID, "deck echo: delay outside MX_DECK_ECHO_MIN_DELAY .. MX_DECK_ECHO_MAX_DELAY");
    if (!std::isfinite(e.send) || !std::isfinite(e.feedback) || !std::isfinite(e.wet) || !std::isfinite(e.damp)) throw Error(MX_ERR_INVALID, "deck echo: send, feedback, wet or damp is not finite");
    if (std::fabs(e.send) > 1.0f) throw Error(MX_ERR_INVALID, "deck echo: |send| above 1");
    if (std::fabs(e.feedback) > 1.0f) throw Error(MX_ERR_INVALID, "deck echo: |feedback| above 1");
    if (std::fabs(e.wet) > 4.0f) throw Error(MX_ERR_INVALID, "deck echo: |wet| above 4");
    if (!(e.damp >= 0.0f && e.damp <= 1.0f)) throw Error(MX_ERR_INVALID, "deck echo: damp outside 0 .. 1");
    if (e.flags & ~MX_DECK_ECHO_PINGPONG) throw Error(MX_ERR_INVALID, "deck echo: a flag bit other than MX_DECK_ECHO_PINGPONG");
}

uint32_t deck_echo_delay(const mx_deck_beats& grid, int64_t step_q32, uint32_t num, uint32_t den) {
    if (!step_q32 || !num || !den) throw Error(MX_ERR_INVALID, "deck echo delay: step, num or den is 0");
    if (grid.period_q32 <= 0) throw Error(MX_ERR_INVALID, "deck echo delay: the grid has no period");
    const unsigned __int128 n = (unsigned __int128)(uint64_t)grid.period_q32 * num;
    const unsigned __int128 d = (unsigned __int128)(step_q32 < 0 ? (uint64_t)0 - (uint64_t)step_q32 : (uint64_t)step_q32) * den;   // (|INT64_MIN| too)
    unsigned __int128 q = n / d; const unsigned __int128 r = n % d;
    if (2 * r > d || (2 * r == d && (q & 1))) ++q;
    if (q < MX_DECK_ECHO_MIN_DELAY || q > MX_DECK_ECHO_MAX_DELAY) throw Error(MX_ERR_INVALID, "deck echo delay: the result lies outside MX_DECK_ECHO_MIN_DELAY .. MX_DECK_ECHO_MAX_DELAY");
    return (uint32_t)q;
}

void deck_echo_cut(uint32_t spt, const uint32_t* delay, uint32_t n_ticks, std::vector<EchoBlock>& out) {
    const uint64_t total = (uint64_t)n_ticks * spt;
    for (uint64_t f = 0; f < total;) {
        const uint32_t k = (uint32_t)(f / spt);
        if (!delay[k]) { f = (uint64_t)(k + 1) * spt; continue; }
        const uint64_t e = echo_block_end(f, k, n_ticks, spt, delay);
        out.push_back(EchoBlock{f, e - f});
        f = e;
    }
}

bool deck_echo_one_block(uint32_t spt, const uint32_t* delay, uint32_t n_ticks) {
    uint32_t k = 0;
    while (k < n_ticks && !delay[k]) ++k;
    if (k == n_ticks) return true;
    const uint64_t e = echo_block_end((uint64_t)k * spt, k, n_ticks, spt, delay);
    for (uint32_t kk = (uint32_t)(e / spt); kk < n_ticks; ++kk) if (delay[kk]) return false;   // (e in the middle of a tick: that tick has an echo)
    return true;
}

void DeckEcho::schedule(uint32_t tick, const mx_deck_echo* e) {
    if (e) {
        deck_echo_check(*e);
        if (!line_.p) {
            hip_check(hipSetDevice(device_), "hipSetDevice");
            line_.alloc((size_t)ECHO_RING * sizeof(float2));
            hip_check(hipMemset(line_.p, 0, (size_t)ECHO_RING * sizeof(float2)), "hipMemset(deck echo line)");
        }
    }
    auto it = std::find_if(sched_.begin(), sched_.end(), [&](const Event& ev) { return ev.tick == tick; });
    if (it == sched_.end()) { sched_.push_back(Event{tick, false, mx_deck_echo{}}); it = sched_.end() - 1; }
    it->on = e != nullptr;
    if (e) it->set = *e;
}

bool DeckEcho::scheduled_beyond(uint32_t n_ticks, uint32_t& tick) const {
    for (const Event& e : sched_) if (e.tick >= n_ticks) { tick = e.tick; return true; }
    return false;
}

bool DeckEcho::plan(uint32_t n_ticks, uint32_t spt, std::vector<EchoTickDev>& ticks, State& after) const {
    State s = st_;
    ticks.clear();
    if (!s.on && sched_.empty()) { after = s; return false; }
    ticks.assign(n_ticks, EchoTickDev{});
    std::vector<const Event*> at(sched_.empty() ? 0 : n_ticks, nullptr);
    for (const Event& e : sched_) at[e.tick] = &e;
    bool any = false;
    for (uint32_t k = 0; k < n_ticks; ++k) {
        const Event* e = at.empty() ? nullptr : at[k];
        bool ramp = false;
        float old[3] = {s.set.send, s.set.feedback, s.set.wet};
        if (e && !e->on) s.on = false;
        else if (e) {
            if (!s.on) { s.t = 0; old[0] = old[1] = old[2] = 0.0f; }   // off -> on starts clean: the kernel reads every line frame before t = 0 as zero
            s.on = true; s.set = e->set; ramp = true;
        }
        if (!s.on) continue;
        const double a = (double)s.set.damp * 0.25, b = 1.0 - (a + a);
        ticks[k] = EchoTickDev{s.t, a, b, s.set.delay,
                               (uint32_t)ECHO_TICK_ON | ((s.set.flags & MX_DECK_ECHO_PINGPONG) ? (uint32_t)ECHO_TICK_PINGPONG : 0u) | (ramp ? (uint32_t)ECHO_TICK_RAMP : 0u),
                               old[0], s.set.send, old[1], s.set.feedback, old[2], s.set.wet};
        s.t += spt;
        any = true;
    }
    after = s;
    return any;
}

void deck_debug_last_echo(uint32_t out[4]) {
    const DeckLastEcho last = deck_last_echo();
    out[0] = out[1] = out[2] = out[3] = 0;
    for (const std::vector<uint32_t>& d : last.delays) {
        if (deck_echo_one_block(last.spt, d.data(), (uint32_t)d.size())) { ++out[0]; continue; }
        ++out[1];
        std::vector<EchoBlock> blocks;
        deck_echo_cut(last.spt, d.data(), (uint32_t)d.size(), blocks);
        out[2] += (uint32_t)blocks.size();
        for (const EchoBlock& b : blocks) if (b.first / last.spt != (b.first + b.frames - 1) / last.spt) ++out[3];
    }
}

}  // namespace mx
