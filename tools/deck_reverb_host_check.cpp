// deck_reverb_host_check.cpp -- the pure host functions of the deck's reverb (mixlab_amd/csrc/mx_deck_reverb.cpp) under the host's address and undefined-behaviour
// sanitizers: a stand-alone program, no device, nothing loaded into Python.
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -O1 -g -ffp-contract=off -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         -I include -I mixlab_amd/csrc tools/deck_reverb_host_check.cpp mixlab_amd/csrc/mx_deck_reverb.cpp -fsanitize=address,undefined -o deck_reverb_host_check
//   ./deck_reverb_host_check [rounds]
//
// It draws random settings (valid, at the range ends, and broken in every field), designs in and out of range, random schedules (off, on, repeats, changes of the
// reach) and random frames, and runs mx::deck_reverb_check, _design, the block cut, the per-tick plan and mx::deck_reverb_host over exactly sized heap buffers -- the
// lines too: one float more or less than MX_DECK_REVERB_LINE_FLOATS would be seen --, whole and split through the carried block: the two groupings must agree to the
// bit, and the sanitizers must stay silent.  The device helpers the file links against are stubs that abort: nothing here may reach them.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "mx_deck_reverb.hpp"

namespace mx {
void hip_check(hipError_t, const char* what) { std::fprintf(stderr, "a pure host function reached the device (%s)\n", what); std::abort(); }
void DevBuf::alloc(size_t) { std::fprintf(stderr, "a pure host function allocated device memory\n"); std::abort(); }
void DevBuf::free_() {}
DeckLastReverb deck_last_reverb() { return DeckLastReverb{}; }
}  // namespace mx

static std::mt19937_64 rng(20251021);
static double uni(double a, double b) { return std::uniform_real_distribution<double>(a, b)(rng); }
static uint32_t pick(uint32_t n) { return (uint32_t)(rng() % n); }

static mx_deck_reverb draw(bool valid) {
    mx_deck_reverb r{};
    const uint32_t form = pick(4);   // 0: every delay at the floor, 1: at the ceiling, else anywhere
    for (int i = 0; i < 8; ++i) {
        r.delay[i] = form == 0 ? MX_DECK_REVERB_MIN_DELAY : form == 1 ? MX_DECK_REVERB_MAX_DELAY : MX_DECK_REVERB_MIN_DELAY + pick(MX_DECK_REVERB_MAX_DELAY - MX_DECK_REVERB_MIN_DELAY + 1);
        r.gain[i] = pick(8) ? (float)uni(-1.0, 1.0) : (pick(2) ? 1.0f : -1.0f);
    }
    for (int j = 0; j < 4; ++j) r.diff[j] = form == 0 ? MX_DECK_REVERB_MIN_DIFF : form == 1 ? MX_DECK_REVERB_MAX_DIFF : MX_DECK_REVERB_MIN_DIFF + pick(MX_DECK_REVERB_MAX_DIFF - MX_DECK_REVERB_MIN_DIFF + 1);
    r.send = (float)uni(-1.0, 1.0); r.dry = (float)uni(-1.0, 1.0); r.wet = (float)uni(-4.0, 4.0); r.damp = (float)uni(0.0, 1.0); r.diffusion = pick(4) ? (float)uni(0.0, 0.75) : 0.75f;
    if (valid) return r;
    switch (pick(10)) {
        case 0: r.delay[pick(8)] = pick(2) ? MX_DECK_REVERB_MIN_DELAY - 1 - pick(128) : MX_DECK_REVERB_MAX_DELAY + 1 + pick(100000); break;
        case 1: r.diff[pick(4)] = pick(2) ? pick(MX_DECK_REVERB_MIN_DIFF) : MX_DECK_REVERB_MAX_DIFF + 1 + pick(100000); break;
        case 2: r.gain[pick(8)] = pick(2) ? NAN : 1.5f; break;
        case 3: r.send = pick(2) ? INFINITY : -1.25f; break;
        case 4: r.dry = pick(2) ? NAN : 1.0001f; break;
        case 5: r.wet = pick(2) ? -INFINITY : 4.5f; break;
        case 6: r.damp = pick(2) ? -0.5f : NAN; break;
        case 7: r.diffusion = pick(2) ? 0.76f : -0.01f; break;
        case 8: r.diffusion = NAN; break;
        default: r.flags = 1 + pick(7); break;
    }
    return r;
}

template <class F> static bool refuses(F&& call) {
    try { call(); } catch (const mx::Error& e) { if (e.code != MX_ERR_INVALID) std::abort(); return true; }
    return false;
}

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 200;
    size_t checks = 0, designs = 0, designed = 0, cuts = 0, blocks_cut = 0, ticks_run = 0, frames_run = 0, refused = 0;
    for (int r = 0; r < rounds; ++r) {
        // the rules
        for (int i = 0; i < 16; ++i) {
            const bool valid = pick(2);
            const mx_deck_reverb s = draw(valid);
            if (refuses([&] { mx::deck_reverb_check(s); }) == valid) { std::fprintf(stderr, "deck_reverb_check: a %s setting was %s\n", valid ? "valid" : "broken", valid ? "refused" : "passed"); return 1; }
            ++checks;
        }
        // designs, in and out of range
        for (int i = 0; i < 8; ++i) {
            mx_deck_reverb out{};
            const double rate = pick(4) ? (pick(2) ? 48000.0 : 44100.0) : uni(-1000.0, 400000.0), size = pick(8) ? uni(0.2, 4.2) : (pick(2) ? 0.0 : NAN), t60 = pick(8) ? uni(0.01, 30.0) : (pick(2) ? 0.0 : -1.0);
            if (!refuses([&] { mx::deck_reverb_design(rate, size, t60, uni(-0.1, 1.1), uni(-0.05, 0.8), uni(-1.1, 1.1), uni(-1.1, 1.1), uni(-4.2, 4.2), out); })) { mx::deck_reverb_check(out); ++designed; }
            ++designs;
        }
        // a random schedule over random frames: the cut, the plan tick by tick, then the host function whole and in two parts through the carried block
        const uint32_t spt = pick(4) ? 1 + pick(130) : 1 + pick(2500), n_ticks = 1 + pick(14), cutp = pick(n_ticks + 1);
        std::vector<mx_deck_reverb> pool(4);
        for (mx_deck_reverb& s : pool) s = draw(true);
        std::vector<const mx_deck_reverb*> settings(n_ticks, nullptr);
        const mx_deck_reverb* cur = nullptr;
        for (uint32_t k = 0; k < n_ticks; ++k) {
            const uint32_t what = pick(6);
            if (what == 0) cur = nullptr; else if (what < 3) cur = &pool[pick(4)];
            settings[k] = cur;
        }
        {
            std::vector<uint32_t> reach(n_ticks);
            for (uint32_t k = 0; k < n_ticks; ++k) reach[k] = settings[k] ? mx::reverb_reach(*settings[k]) : 0u;
            std::vector<mx::ReverbBlock> blocks;
            mx::deck_reverb_cut(spt, reach.data(), n_ticks, blocks);
            uint64_t covered = 0, want = 0;
            for (uint32_t k = 0; k < n_ticks; ++k) if (reach[k]) want += spt;
            for (const mx::ReverbBlock& b : blocks) {
                covered += b.frames;
                if (!b.frames || b.frames > MX_DECK_REVERB_MAX_DIFF) { std::fprintf(stderr, "cut: a block of %llu frames\n", (unsigned long long)b.frames); return 1; }
                for (uint64_t f = b.first; f < b.first + b.frames; ++f)
                    if (!reach[f / spt] || f - b.first >= reach[f / spt]) { std::fprintf(stderr, "cut: frame %llu reads inside its own block\n", (unsigned long long)f); return 1; }
            }
            if (covered != want) { std::fprintf(stderr, "cut: the blocks do not cover the reverb's frames\n"); return 1; }
            ++cuts; blocks_cut += blocks.size();
        }
        mx::ReverbState st;
        for (uint32_t k = 0; k < n_ticks; ++k) {
            const bool ev = pick(2) || (settings[k] == nullptr) != !st.on;
            const uint64_t t_before = st.t; const bool was_on = st.on;
            const mx::ReverbTickDev t = mx::deck_reverb_plan_tick(st, ev, settings[k], spt);
            if (((t.flags & mx::REVERB_TICK_ON) != 0) != (settings[k] != nullptr)) { std::fprintf(stderr, "plan: tick %u on / off disagrees with its setting\n", k); return 1; }
            if (settings[k] && t.t0 != (was_on ? t_before : 0)) { std::fprintf(stderr, "plan: tick %u has the wrong clock\n", k); return 1; }
            if (settings[k] && (t.reach < MX_DECK_REVERB_MIN_DIFF || t.reach > MX_DECK_REVERB_MAX_DIFF)) { std::fprintf(stderr, "plan: a reach out of range\n"); return 1; }
        }
        std::vector<float> whole((size_t)n_ticks * spt * 2);
        for (float& v : whole) v = pick(16) ? (float)uni(-1.0, 1.0) : (pick(2) ? 0.0f : -0.0f);
        std::vector<float> parts = whole;
        std::vector<float> lines_a(MX_DECK_REVERB_LINE_FLOATS), lines_b;
        for (float& v : lines_a) v = (float)uni(-1.0, 1.0);   // (any content at first: a read below clock 0 is zero whatever the slot holds)
        lines_b = lines_a;
        mx_deck_reverb_carry a{}, b{};
        mx::deck_reverb_host(whole.data(), spt, n_ticks, settings.data(), lines_a.data(), a);
        {   // each part in a buffer of its own size, so that a frame read or written past a part's end is seen
            std::vector<float> p0(parts.begin(), parts.begin() + (size_t)cutp * spt * 2), p1(parts.begin() + (size_t)cutp * spt * 2, parts.end());
            std::vector<const mx_deck_reverb*> s0(settings.begin(), settings.begin() + cutp), s1(settings.begin() + cutp, settings.end());
            mx::deck_reverb_host(p0.data(), spt, cutp, s0.data(), lines_b.data(), b);
            mx::deck_reverb_host(p1.data(), spt, n_ticks - cutp, s1.data(), lines_b.data(), b);
            std::copy(p0.begin(), p0.end(), parts.begin());
            std::copy(p1.begin(), p1.end(), parts.begin() + p0.size());
        }
        if (std::memcmp(whole.data(), parts.data(), whole.size() * sizeof(float)) || std::memcmp(&a, &b, sizeof a) ||
            std::memcmp(lines_a.data(), lines_b.data(), lines_a.size() * sizeof(float))) { std::fprintf(stderr, "host: whole and split disagree (round %d)\n", r); return 1; }
        ticks_run += n_ticks; frames_run += (size_t)n_ticks * spt;
        // refusals write nothing
        {
            const mx_deck_reverb bad = draw(false);
            std::vector<const mx_deck_reverb*> s = settings;
            s[pick(n_ticks)] = &bad;
            std::vector<float> before = whole, lines_before = lines_a;
            mx_deck_reverb_carry c = a;
            if (!refuses([&] { mx::deck_reverb_host(whole.data(), spt, n_ticks, s.data(), lines_a.data(), c); }) || std::memcmp(before.data(), whole.data(), whole.size() * sizeof(float)) ||
                std::memcmp(&a, &c, sizeof a) || std::memcmp(lines_before.data(), lines_a.data(), lines_a.size() * sizeof(float))) {
                std::fprintf(stderr, "host: a broken setting was not refused cleanly\n"); return 1;
            }
            ++refused;
        }
    }
    std::printf("deck_reverb_host_check: %d rounds, %zu checks, %zu designs (%zu given), %zu cuts of %zu blocks, %zu ticks and %zu frames through mx_deck_reverb_host, %zu refusals: clean\n",
                rounds, checks, designs, designed, cuts, blocks_cut, ticks_run, frames_run, refused);
    return 0;
}
