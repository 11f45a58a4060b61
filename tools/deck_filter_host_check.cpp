// deck_filter_host_check.cpp -- the pure host functions of the deck's sweep filter (mixlab_amd/csrc/mx_deck_filter.cpp) under the host's address and
// undefined-behaviour sanitizers: a stand-alone program, no device, nothing loaded into Python.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I mixlab_amd/csrc tools/deck_filter_host_check.cpp mixlab_amd/csrc/mx_deck_filter.cpp -fsanitize=address,undefined -o deck_filter_host_check
//   ./deck_filter_host_check [rounds]
//
// It draws random settings (valid, at the range ends, and broken in every field), random schedules (off, on, repeats, kind changes) and random frames, and runs
// mx::deck_filter_check, _design, _knob, the per-tick plan and mx::deck_filter_host over exactly sized heap buffers, whole and split through the carried block: the
// two groupings must agree to the bit, and the sanitizers must stay silent.  The two device helpers the file links against are stubs that abort: nothing here may
// reach them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "mx_deck_filter.hpp"

namespace mx {
void hip_check(hipError_t, const char* what) { std::fprintf(stderr, "a pure host function reached the device (%s)\n", what); std::abort(); }
void DevBuf::alloc(size_t) { std::fprintf(stderr, "a pure host function allocated device memory\n"); std::abort(); }
void DevBuf::free_() {}
}  // namespace mx

static std::mt19937_64 rng(20250923);
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static uint32_t pick(uint32_t n) { return (uint32_t)(rng() % n); }

static mx_deck_filter draw(bool valid) {
    static const float gs[] = {MX_DECK_FILTER_MIN_G, MX_DECK_FILTER_MAX_G, 0.05f, 0.3f, 1.0f}, ks[] = {MX_DECK_FILTER_MIN_K, MX_DECK_FILTER_MAX_K, 0.1f, 0.7f};
    mx_deck_filter f{pick(4), 0u, pick(2) ? gs[pick(5)] : (float)std::exp(uni(std::log(2.5e-4), std::log(16.0))), pick(2) ? ks[pick(4)] : (float)uni(0.05001, 2.0), (float)uni(0.0, 1.0), 0u};
    if (pick(4) == 0) f.wet = pick(2) ? 0.0f : 1.0f;
    if (valid) return f;
    switch (pick(8)) {
        case 0: f.kind = 4 + pick(1000); break;
        case 1: f.flags = 1 + pick(7); break;
        case 2: f._pad = 1; break;
        case 3: f.g = pick(2) ? NAN : INFINITY; break;
        case 4: f.k = pick(2) ? -1.0f : 2.5f; break;
        case 5: f.wet = pick(2) ? -0.5f : NAN; break;
        case 6: f.g = pick(2) ? 0.0f : 17.0f; break;
        default: f.k = NAN; break;
    }
    return f;
}

template <class F> static bool refuses(F&& call) {
    try { call(); } catch (const mx::Error& e) { if (e.code != MX_ERR_INVALID) std::abort(); return true; }
    return false;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 400;
    size_t checks = 0, designs = 0, knobs = 0, ticks_run = 0, frames_run = 0, refused = 0;
    for (int r = 0; r < rounds; ++r) {
        // the rules
        for (int i = 0; i < 16; ++i) {
            const bool valid = pick(2);
            const mx_deck_filter f = draw(valid);
            if (refuses([&] { mx::deck_filter_check(f); }) == valid) { std::fprintf(stderr, "deck_filter_check: a %s setting was %s\n", valid ? "valid" : "broken", valid ? "refused" : "passed"); return 1; }
            ++checks;
        }
        // design and knob, in and out of range
        for (int i = 0; i < 8; ++i) {
            mx_deck_filter out{}; uint32_t on = 7;
            const double rate = pick(2) ? 48000.0 : uni(-1000.0, 200000.0), hz = std::exp(uni(std::log(0.1), std::log(1.0e5))), q = pick(8) ? uni(0.3, 25.0) : (pick(2) ? 0.0 : NAN);
            if (!refuses([&] { mx::deck_filter_design(pick(5), hz, q, rate, uni(-0.2, 1.2), out); })) mx::deck_filter_check(out);
            ++designs;
            if (!refuses([&] { mx::deck_filter_knob(uni(-1.1, 1.1), rate, q, out, on); }) && on) mx::deck_filter_check(out);
            ++knobs;
        }
        // a random schedule over random frames: the plan tick by tick, then the host function whole and in two parts through the carried block
        const uint32_t spt = pick(4) ? 1 + pick(130) : 1 + pick(900), n_ticks = 1 + pick(14), cut = pick(n_ticks + 1);
        std::vector<mx_deck_filter> pool(4);
        for (mx_deck_filter& f : pool) f = draw(true);
        std::vector<const mx_deck_filter*> settings(n_ticks, nullptr);
        const mx_deck_filter* cur = nullptr;
        for (uint32_t k = 0; k < n_ticks; ++k) {
            const uint32_t what = pick(6);
            if (what == 0) cur = nullptr; else if (what < 3) cur = &pool[pick(4)];
            settings[k] = cur;
        }
        mx::FilterState st;
        for (uint32_t k = 0; k < n_ticks; ++k) {
            const bool ev = pick(2) || (settings[k] == nullptr) != !st.on;
            const mx::FilterTickDev t = mx::deck_filter_plan_tick(st, ev, settings[k]);
            if (((t.flags & mx::FILTER_TICK_ON) != 0) != (settings[k] != nullptr)) { std::fprintf(stderr, "plan: tick %u on / off disagrees with its setting\n", k); return 1; }
            if ((t.flags & mx::FILTER_TICK_CLEAR) && !(t.flags & mx::FILTER_TICK_RAMP)) { std::fprintf(stderr, "plan: a cleared tick without a ramp\n"); return 1; }
        }
        std::vector<float> whole((size_t)n_ticks * spt * 2);
        for (float& v : whole) v = pick(16) ? (float)uni(-1.0, 1.0) : (pick(2) ? 0.0f : -0.0f);
        std::vector<float> parts = whole;
        mx_deck_filter_carry a{}, b{};
        mx::deck_filter_host(whole.data(), spt, n_ticks, settings.data(), a);
        {   // each part in a buffer of its own size, so that a frame read or written past a part's end is seen
            std::vector<float> p0(parts.begin(), parts.begin() + (size_t)cut * spt * 2), p1(parts.begin() + (size_t)cut * spt * 2, parts.end());
            std::vector<const mx_deck_filter*> s0(settings.begin(), settings.begin() + cut), s1(settings.begin() + cut, settings.end());
            mx::deck_filter_host(p0.data(), spt, cut, s0.data(), b);
            mx::deck_filter_host(p1.data(), spt, n_ticks - cut, s1.data(), b);
            std::copy(p0.begin(), p0.end(), parts.begin());
            std::copy(p1.begin(), p1.end(), parts.begin() + p0.size());
        }
        if (std::memcmp(whole.data(), parts.data(), whole.size() * sizeof(float)) || std::memcmp(&a, &b, sizeof a)) { std::fprintf(stderr, "host: whole and split disagree (round %d)\n", r); return 1; }
        ticks_run += n_ticks; frames_run += (size_t)n_ticks * spt;
        // refusals write nothing
        {
            const mx_deck_filter bad = draw(false);
            std::vector<const mx_deck_filter*> s = settings;
            s[pick(n_ticks)] = &bad;
            std::vector<float> before = whole;
            mx_deck_filter_carry c = a;
            if (!refuses([&] { mx::deck_filter_host(whole.data(), spt, n_ticks, s.data(), c); }) || std::memcmp(before.data(), whole.data(), whole.size() * sizeof(float)) || std::memcmp(&a, &c, sizeof a)) {
                std::fprintf(stderr, "host: a broken setting was not refused cleanly\n"); return 1;
            }
            ++refused;
        }
    }
    std::printf("deck_filter_host_check: %d rounds, %zu checks, %zu designs, %zu knobs, %zu ticks and %zu frames through mx_deck_filter_host, %zu refusals: clean\n", rounds, checks, designs, knobs,
                ticks_run, frames_run, refused);
    return 0;
}
