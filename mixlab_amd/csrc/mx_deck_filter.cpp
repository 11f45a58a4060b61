// mx_deck_filter.cpp -- the deck's resonant sweep filter, host side (include/mixlab_gpu.h "FILTER"): the setting rules, the design helpers
// (cutoff and Q to g and k, the DJ knob), the per-tick state machine (ramps, schedule, off -> on), the four state values in device memory, and PER FRAME restated
// for the host (mx_deck_filter_host).  The descriptors travel with the feed's (mx_deck.cpp); the kernel is mx_k_deck_filter.hip.
#include "mx_deck_filter.hpp"

#include <algorithm>
#include <cmath>

namespace mx {

void deck_filter_check(const mx_deck_filter& f) {
    if (f.kind > MX_DECK_FILTER_NOTCH) throw Error(MX_ERR_INVALID, "deck filter: kind outside MX_DECK_FILTER_LP .. MX_DECK_FILTER_NOTCH");
    if (f.flags) throw Error(MX_ERR_INVALID, "deck filter: flags must be 0");
    if (f._pad) throw Error(MX_ERR_INVALID, "deck filter: _pad must be 0");
    if (!std::isfinite(f.g) || !std::isfinite(f.k) || !std::isfinite(f.wet)) throw Error(MX_ERR_INVALID, "deck filter: g, k or wet is not finite");
    if (!(f.g >= MX_DECK_FILTER_MIN_G && f.g <= MX_DECK_FILTER_MAX_G)) throw Error(MX_ERR_INVALID, "deck filter: g outside MX_DECK_FILTER_MIN_G .. MX_DECK_FILTER_MAX_G");
    if (!(f.k >= MX_DECK_FILTER_MIN_K && f.k <= MX_DECK_FILTER_MAX_K)) throw Error(MX_ERR_INVALID, "deck filter: k outside MX_DECK_FILTER_MIN_K .. MX_DECK_FILTER_MAX_K");
    if (!(f.wet >= 0.0f && f.wet <= 1.0f)) throw Error(MX_ERR_INVALID, "deck filter: wet outside 0 .. 1");
}

void deck_filter_design(uint32_t kind, double cutoff_hz, double q, double rate, double wet, mx_deck_filter& out) {
    if (!std::isfinite(cutoff_hz) || !std::isfinite(q) || !std::isfinite(rate) || !std::isfinite(wet)) throw Error(MX_ERR_INVALID, "deck filter design: an argument is not finite");
    if (!(rate > 0.0) || !(q > 0.0)) throw Error(MX_ERR_INVALID, "deck filter design: rate and q must be positive");
    if (!(cutoff_hz > 0.0 && cutoff_hz < 0.5 * rate)) throw Error(MX_ERR_INVALID, "deck filter design: the cutoff lies outside 0 .. rate / 2");
    const double pi = 3.14159265358979323846;
    const mx_deck_filter f{kind, 0u, (float)std::tan(pi * cutoff_hz / rate), (float)(1.0 / q), (float)wet, 0u};
    deck_filter_check(f);
    out = f;
}

void deck_filter_knob(double knob, double rate, double q, mx_deck_filter& out, uint32_t& on) {
    if (!std::isfinite(knob) || std::fabs(knob) > 1.0) throw Error(MX_ERR_INVALID, "deck filter knob: the knob lies outside -1 .. 1");
    if (!std::isfinite(rate) || !(rate > 0.0)) throw Error(MX_ERR_INVALID, "deck filter knob: rate must be positive");
    if (std::fabs(knob) < 1.0 / 64.0) {
        if (!std::isfinite(q) || !(q > 0.0)) throw Error(MX_ERR_INVALID, "deck filter knob: q must be positive");
        on = 0;
        return;
    }
    const double a = std::fabs(knob);
    const double hz = knob < 0.0 ? 20000.0 * std::pow(80.0 / 20000.0, a) : 20.0 * std::pow(8000.0 / 20.0, a);
    mx_deck_filter f{};
    deck_filter_design(knob < 0.0 ? MX_DECK_FILTER_LP : MX_DECK_FILTER_HP, std::min(hz, 0.45 * rate), q, rate, 1.0, f);
    out = f; on = 1;
}

FilterTickDev deck_filter_plan_tick(FilterState& s, bool ev, const mx_deck_filter* ev_set) {
    uint32_t flags = 0;
    double old[3] = {(double)s.set.g, (double)s.set.k, (double)s.set.wet};
    if (ev && !ev_set) s.on = false;
    else if (ev) {
        if (!s.on) { old[0] = (double)ev_set->g; old[1] = (double)ev_set->k; old[2] = 0.0; flags |= FILTER_TICK_CLEAR; }   // off -> on: a fade-in at the target cutoff, from a clean state
        s.on = true; s.set = *ev_set; flags |= FILTER_TICK_RAMP;
    }
    if (!s.on) return FilterTickDev{};
    return FilterTickDev{flags | FILTER_TICK_ON, s.set.kind, old[0], (double)s.set.g, old[1], (double)s.set.k, old[2], (double)s.set.wet};
}

void deck_filter_host(float* frames, uint32_t spt, uint32_t n_ticks, const mx_deck_filter* const* settings, mx_deck_filter_carry& carry) {
    if (spt < 1 || spt > MX_DECK_MAX_SPT) throw Error(MX_ERR_INVALID, "deck filter: frames per tick outside 1 .. MX_DECK_MAX_SPT");
    if (carry.on > 1 || carry._pad) throw Error(MX_ERR_INVALID, "deck filter: the carried block's on is neither 0 nor 1, or its _pad is not 0");
    if (carry.on) deck_filter_check(carry.last);
    for (uint32_t k = 0; k < n_ticks; ++k) if (settings[k]) deck_filter_check(*settings[k]);
    FilterState st{carry.on != 0, carry.last};
    double s[4] = {carry.s[0], carry.s[1], carry.s[2], carry.s[3]};
    for (uint32_t k = 0; k < n_ticks; ++k) {
        const FilterTickDev t = deck_filter_plan_tick(st, true, settings[k]);
        if (!(t.flags & FILTER_TICK_ON)) continue;
        if (t.flags & FILTER_TICK_CLEAR) s[0] = s[1] = s[2] = s[3] = 0.0;
        float* const p = frames + (size_t)k * spt * 2;
        for (uint32_t n = 0; n < spt; ++n) {
            const FilterCoef c = filter_coef(t, n, spt);
            for (int ch = 0; ch < 2; ++ch) {
                const double x = (double)p[2 * (size_t)n + ch];
                double v1, v2;
                filter_step(x, c.a1, c.a2, c.a3, s[2 * ch], s[2 * ch + 1], v1, v2);
                p[2 * (size_t)n + ch] = filter_out(t.kind, x, c.kn, c.wn, v1, v2);
            }
        }
    }
    carry.on = st.on ? 1u : 0u; carry.last = st.set; carry._pad = 0;
    const bool keep = st.on;   // (a filter that is off has no state: the next on starts from zero)
    for (int i = 0; i < 4; ++i) carry.s[i] = keep ? s[i] : 0.0;
}

void DeckFilter::schedule(uint32_t tick, const mx_deck_filter* f) {
    if (f) {
        deck_filter_check(*f);
        if (!state_.p) {
            hip_check(hipSetDevice(device_), "hipSetDevice");
            state_.alloc(4 * sizeof(double));
            hip_check(hipMemset(state_.p, 0, 4 * sizeof(double)), "hipMemset(deck filter state)");
        }
    }
    auto it = std::find_if(sched_.begin(), sched_.end(), [&](const Event& ev) { return ev.tick == tick; });
    if (it == sched_.end()) { sched_.push_back(Event{tick, false, mx_deck_filter{}}); it = sched_.end() - 1; }
    it->on = f != nullptr;
    if (f) it->set = *f;
}

bool DeckFilter::scheduled_beyond(uint32_t n_ticks, uint32_t& tick) const {
    for (const Event& e : sched_) if (e.tick >= n_ticks) { tick = e.tick; return true; }
    return false;
}

bool DeckFilter::plan(uint32_t n_ticks, std::vector<FilterTickDev>& ticks, State& after) const {
    State s = st_;
    ticks.clear();
    if (!s.on && sched_.empty()) { after = s; return false; }
    ticks.assign(n_ticks, FilterTickDev{});
    std::vector<const Event*> at(sched_.empty() ? 0 : n_ticks, nullptr);
    for (const Event& e : sched_) at[e.tick] = &e;
    bool any = false;
    for (uint32_t k = 0; k < n_ticks; ++k) {
        const Event* e = at.empty() ? nullptr : at[k];
        ticks[k] = deck_filter_plan_tick(s, e != nullptr, e && e->on ? &e->set : nullptr);
        any = any || (ticks[k].flags & FILTER_TICK_ON);
    }
    after = s;
    return any;
}

void DeckFilter::read_state(double s[4]) const {
    s[0] = s[1] = s[2] = s[3] = 0.0;
    if (!st_.on || !state_.p) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    hip_check(hipMemcpy(s, state_.p, 4 * sizeof(double), hipMemcpyDeviceToHost), "hipMemcpy(deck filter state)");
}

}  // namespace mx
