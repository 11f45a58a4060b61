// mx_deck_reverb.cpp -- the deck's reverb, host side (include/mixlab_gpu.h "REVERB"): the setting rules, the design helper (size and decay
// time to prime delays and gains), the per-tick state machine (clock, ramps, schedule, off -> on), the twelve rings in device memory, the block cutting restated for
// the host (mx_deck_reverb_plan, mx_deck_debug_last_reverb) and PER FRAME restated for the host (mx_deck_reverb_host).  The descriptors travel with the feed's
// (mx_deck.cpp); the kernel is mx_k_deck_reverb.hip.
#include "mx_deck_reverb.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace mx {

void deck_reverb_check(const mx_deck_reverb& r) {
    for (int i = 0; i < REVERB_TANK; ++i)
        if (r.delay[i] < MX_DECK_REVERB_MIN_DELAY || r.delay[i] > MX_DECK_REVERB_MAX_DELAY) throw Error(MX_ERR_INVALID, "deck reverb: a delay outside MX_DECK_REVERB_MIN_DELAY .. MX_DECK_REVERB_MAX_DELAY");
    for (int j = 0; j < REVERB_DIFF; ++j)
        if (r.diff[j] < MX_DECK_REVERB_MIN_DIFF || r.diff[j] > MX_DECK_REVERB_MAX_DIFF) throw Error(MX_ERR_INVALID, "deck reverb: a diffuser delay outside MX_DECK_REVERB_MIN_DIFF .. MX_DECK_REVERB_MAX_DIFF");
    bool finite = std::isfinite(r.send) && std::isfinite(r.dry) && std::isfinite(r.wet) && std::isfinite(r.damp) && std::isfinite(r.diffusion);
    for (int i = 0; i < REVERB_TANK; ++i) finite = finite && std::isfinite(r.gain[i]);
    if (!finite) throw Error(MX_ERR_INVALID, "deck reverb: a gain, send, dry, wet, damp or diffusion is not finite");
    for (int i = 0; i < REVERB_TANK; ++i) if (std::fabs(r.gain[i]) > 1.0f) throw Error(MX_ERR_INVALID, "deck reverb: |gain| above 1");
    if (std::fabs(r.send) > 1.0f) throw Error(MX_ERR_INVALID, "deck reverb: |send| above 1");
    if (std::fabs(r.dry) > 1.0f) throw Error(MX_ERR_INVALID, "deck reverb: |dry| above 1");
    if (std::fabs(r.wet) > 4.0f) throw Error(MX_ERR_INVALID, "deck reverb: |wet| above 4");
    if (!(r.damp >= 0.0f && r.damp <= 1.0f)) throw Error(MX_ERR_INVALID, "deck reverb: damp outside 0 .. 1");
    if (!(r.diffusion >= 0.0f && r.diffusion <= 0.75f)) throw Error(MX_ERR_INVALID, "deck reverb: diffusion outside 0 .. 0.75");
    if (r.flags) throw Error(MX_ERR_INVALID, "deck reverb: flags must be 0");
}

// the smallest prime >= x (x below 2^31 here: trial division)
static uint64_t prime_from(uint64_t x) {
    for (uint64_t p = x < 2 ? 2 : x;; ++p) {
        bool prime = true;
        for (uint64_t d = 2; d * d <= p; ++d) if (p % d == 0) { prime = false; break; }
        if (prime) return p;
    }
}

void deck_reverb_design(double rate, double size, double t60, double damp, double diffusion, double send, double dry, double wet, mx_deck_reverb& out) {
    if (!std::isfinite(rate) || !std::isfinite(size) || !std::isfinite(t60) || !std::isfinite(damp) || !std::isfinite(diffusion) || !std::isfinite(send) || !std::isfinite(dry) ||
        !std::isfinite(wet))
        throw Error(MX_ERR_INVALID, "deck reverb design: an argument is not finite");
    if (!(rate > 0.0) || !(t60 > 0.0)) throw Error(MX_ERR_INVALID, "deck reverb design: rate and t60_seconds must be positive");
    if (!(size >= 0.25 && size <= 4.0)) throw Error(MX_ERR_INVALID, "deck reverb design: size outside 0.25 .. 4");
    static const double base[REVERB_TANK] = {1087, 1283, 1447, 1663, 1871, 2053, 2281, 2477}, dbase[REVERB_DIFF] = {229, 613, 241, 587};
    mx_deck_reverb r{};
    for (int i = 0; i < REVERB_TANK; ++i) {
        const double want = std::floor(base[i] * size * rate / 48000.0 + 0.5);
        if (!(want <= (double)MX_DECK_REVERB_MAX_DELAY)) throw Error(MX_ERR_INVALID, "deck reverb design: a delay lies outside MX_DECK_REVERB_MIN_DELAY .. MX_DECK_REVERB_MAX_DELAY");
        uint64_t p = prime_from((uint64_t)want);
        for (bool again = true; again;) {
            again = false;
            for (int l = 0; l < i; ++l) if (r.delay[l] == p) { p = prime_from(p + 1); again = true; }
        }
        if (p < MX_DECK_REVERB_MIN_DELAY || p > MX_DECK_REVERB_MAX_DELAY) throw Error(MX_ERR_INVALID, "deck reverb design: a delay lies outside MX_DECK_REVERB_MIN_DELAY .. MX_DECK_REVERB_MAX_DELAY");
        r.delay[i] = (uint32_t)p;
        r.gain[i] = (float)std::pow(10.0, -3.0 * (double)r.delay[i] / (rate * t60));
    }
    for (int j = 0; j < REVERB_DIFF; ++j) {
        const double want = std::floor(dbase[j] * rate / 48000.0 + 0.5);
        if (!(want <= (double)MX_DECK_REVERB_MAX_DIFF)) throw Error(MX_ERR_INVALID, "deck reverb design: a diffuser delay lies outside MX_DECK_REVERB_MIN_DIFF .. MX_DECK_REVERB_MAX_DIFF");
        const uint64_t p = prime_from((uint64_t)want);
        if (p < MX_DECK_REVERB_MIN_DIFF || p > MX_DECK_REVERB_MAX_DIFF) throw Error(MX_ERR_INVALID, "deck reverb design: a diffuser delay lies outside MX_DECK_REVERB_MIN_DIFF .. MX_DECK_REVERB_MAX_DIFF");
        r.diff[j] = (uint32_t)p;
    }
    r.send = (float)send; r.dry = (float)dry; r.wet = (float)wet; r.damp = (float)damp; r.diffusion = (float)diffusion; r.flags = 0;
    deck_reverb_check(r);
    out = r;
}

void deck_reverb_cut(uint32_t spt, const uint32_t* reach, uint32_t n_ticks, std::vector<ReverbBlock>& out) {
    const uint64_t total = (uint64_t)n_ticks * spt;
    for (uint64_t f = 0; f < total;) {
        const uint32_t k = (uint32_t)(f / spt);
        if (!reach[k]) { f = (uint64_t)(k + 1) * spt; continue; }
        const uint64_t e = reverb_block_end(f, k, n_ticks, spt, reach);
        out.push_back(ReverbBlock{f, e - f});
        f = e;
    }
}

ReverbTickDev deck_reverb_plan_tick(ReverbState& s, bool ev, const mx_deck_reverb* ev_set, uint32_t spt) {
    bool ramp = false;
    mx_deck_reverb old = s.set;
    if (ev && !ev_set) s.on = false;
    else if (ev) {
        if (!s.on) {   // off -> on starts clean: the clock at 0 (every line reads zero below it), all eleven ramped values from 0
            s.t = 0; old.send = old.dry = old.wet = 0.0f;
            for (int i = 0; i < REVERB_TANK; ++i) old.gain[i] = 0.0f;
        }
        s.on = true; s.set = *ev_set; ramp = true;
    }
    ReverbTickDev t{};
    if (!s.on) return t;
    t.t0 = s.t;
    t.a = (double)s.set.damp * 0.25;
    const double a2 = t.a + t.a;
    t.b = 1.0 - a2;
    t.gd = (double)s.set.diffusion;
    for (int i = 0; i < REVERB_TANK; ++i) { t.delay[i] = s.set.delay[i]; t.gain0[i] = old.gain[i]; t.gain1[i] = s.set.gain[i]; }
    for (int j = 0; j < REVERB_DIFF; ++j) t.diff[j] = s.set.diff[j];
    t.flags = (uint32_t)REVERB_TICK_ON | (ramp ? (uint32_t)REVERB_TICK_RAMP : 0u);
    t.reach = reverb_reach(s.set);
    t.send0 = old.send; t.send1 = s.set.send; t.dry0 = old.dry; t.dry1 = s.set.dry; t.wet0 = old.wet; t.wet1 = s.set.wet;
    s.t += spt;
    return t;
}

void deck_reverb_host(float* frames, uint32_t spt, uint32_t n_ticks, const mx_deck_reverb* const* settings, float* lines, mx_deck_reverb_carry& carry) {
    if (spt < 1 || spt > MX_DECK_MAX_SPT) throw Error(MX_ERR_INVALID, "deck reverb: frames per tick outside 1 .. MX_DECK_MAX_SPT");
    if (carry.on > 1 || carry._pad) throw Error(MX_ERR_INVALID, "deck reverb: the carried block's on is neither 0 nor 1, or its _pad is not 0");
    if (carry.on) deck_reverb_check(carry.last);
    for (uint32_t k = 0; k < n_ticks; ++k) if (settings[k]) deck_reverb_check(*settings[k]);
    ReverbState st{carry.on != 0, carry.last, carry.t};
    for (uint32_t k = 0; k < n_ticks; ++k) {
        const ReverbTickDev t = deck_reverb_plan_tick(st, true, settings[k], spt);
        if (!(t.flags & REVERB_TICK_ON)) continue;
        float* const p = frames + (size_t)k * spt * 2;
        for (uint32_t n = 0; n < spt; ++n) reverb_frame(lines, t, n, spt, p + 2 * (size_t)n);   // (frame by frame in clock order: every block cut gives these values)
    }
    carry.t = st.t; carry.last = st.set; carry.on = st.on ? 1u : 0u; carry._pad = 0;
}

void DeckReverb::schedule(uint32_t tick, const mx_deck_reverb* r) {
    if (r) {
        deck_reverb_check(*r);
        if (!lines_.p) {
            hip_check(hipSetDevice(device_), "hipSetDevice");
            lines_.alloc((size_t)MX_DECK_REVERB_LINE_FLOATS * sizeof(float));
            hip_check(hipMemset(lines_.p, 0, (size_t)MX_DECK_REVERB_LINE_FLOATS * sizeof(float)), "hipMemset(deck reverb lines)");
        }
    }
    auto it = std::find_if(sched_.begin(), sched_.end(), [&](const Event& ev) { return ev.tick == tick; });
    if (it == sched_.end()) { sched_.push_back(Event{tick, false, mx_deck_reverb{}}); it = sched_.end() - 1; }
    it->on = r != nullptr;
    if (r) it->set = *r;
}

bool DeckReverb::scheduled_beyond(uint32_t n_ticks, uint32_t& tick) const {
    for (const Event& e : sched_) if (e.tick >= n_ticks) { tick = e.tick; return true; }
    return false;
}

bool DeckReverb::plan(uint32_t n_ticks, uint32_t spt, std::vector<ReverbTickDev>& ticks, State& after) const {
    State s = st_;
    ticks.clear();
    if (!s.on && sched_.empty()) { after = s; return false; }
    ticks.assign(n_ticks, ReverbTickDev{});
    std::vector<const Event*> at(sched_.empty() ? 0 : n_ticks, nullptr);
    for (const Event& e : sched_) at[e.tick] = &e;
    bool any = false;
    for (uint32_t k = 0; k < n_ticks; ++k) {
        const Event* e = at.empty() ? nullptr : at[k];
        ticks[k] = deck_reverb_plan_tick(s, e != nullptr, e && e->on ? &e->set : nullptr, spt);
        any = any || (ticks[k].flags & REVERB_TICK_ON);
    }
    after = s;
    return any;
}

void DeckReverb::read_lines(float* dst) const {
    std::memset(dst, 0, (size_t)MX_DECK_REVERB_LINE_FLOATS * sizeof(float));
    if (!lines_.p) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    hip_check(hipMemcpy(dst, lines_.p, (size_t)MX_DECK_REVERB_LINE_FLOATS * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy(deck reverb lines)");
}

void deck_debug_last_reverb(uint32_t out[4]) {
    const DeckLastReverb last = deck_last_reverb();
    out[0] = out[1] = out[2] = out[3] = 0;
    for (const std::vector<uint32_t>& r : last.reaches) {
        ++out[0];
        std::vector<ReverbBlock> blocks;
        deck_reverb_cut(last.spt, r.data(), (uint32_t)r.size(), blocks);
        out[1] += (uint32_t)blocks.size();
        for (const ReverbBlock& b : blocks) {
            if (b.first / last.spt != (b.first + b.frames - 1) / last.spt) ++out[2];
            out[3] = std::max(out[3], (uint32_t)b.frames);
        }
    }
}

}  // namespace mx
