// deck_bars_check.cpp -- the pure host functions of the deck's bars and phrases (mixlab_amd/csrc/mx_deck_bars.cpp) under the host's address and undefined-behaviour
// sanitizers: a plain executable, no device, no Python in the checked process.  tools/deck_bars_check.py builds it -- this file and mx_deck_bars.cpp instrumented,
// everything else from libmixlab_gpu.so -- and runs it.  It walks the corners where an index or a shift could go wrong (a filter halo before frame 0 and past the last
// frame, a last beat that ends on the last frame, W = 64 at both ends of the records, grids far from the track, every refusal) and checks what must hold of any result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../mixlab_amd/csrc/mx_deck_bars.hpp"

using namespace mx;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static bool refused(const std::function<void()>& f) {
    try { f(); } catch (const Error& e) { return e.code == MX_ERR_INVALID; }
    return false;
}

static mx_deck_bars settings(int64_t first, int64_t period, uint32_t K, uint32_t lead, uint32_t M, uint32_t Q, uint32_t wb, uint32_t wp, uint32_t max_beats) {
    mx_deck_bars s{};
    s.grid = mx_deck_beats{first, period};
    s.lead = lead; s.taps = K; s.beats_per_bar = M; s.bars_per_phrase = Q; s.w_bar = wb; s.w_phrase = wp; s.max_beats = max_beats;
    // a crude low-pass pair within the tap rule: equal taps that sum to 16384 (lo), and a single centre tap (hi)
    for (uint32_t k = 0; k < K; ++k) s.lo[k] = (int16_t)(16384 / K);
    s.lo[(K - 1) / 2] = (int16_t)(s.lo[(K - 1) / 2] + 16384 - (16384 / K) * K);
    s.hi[(K - 1) / 2] = 16384;
    return s;
}

static void run(const char* what, uint64_t n_frames, const mx_deck_bars& s, uint32_t want_beats) {
    std::vector<int16_t> x(2 * n_frames);
    uint32_t r = 12345u + (uint32_t)n_frames;
    for (uint64_t f = 0; f < n_frames; ++f) {
        r = r * 1664525u + 1013904223u;
        const int level = 1 + (int)((f / 3000) % 7) * 4000;
        x[2 * f] = (int16_t)((int)(r >> 16) % level);
        x[2 * f + 1] = f % 5 ? x[2 * f] : (int16_t)-32768;
    }
    const BarsBeats b = deck_bars_check(s, n_frames, true);
    EXPECT(b.n_beats == want_beats);
    const uint32_t M = s.beats_per_bar, MQ = M * s.bars_per_phrase;
    std::vector<mx_deck_beat> recs(b.n_beats);      // exactly n_beats and M + M Q: a write past either is the sanitizer's to find
    std::vector<uint64_t> H(M + MQ);
    deck_bars_host(x.data(), n_frames, s, recs.data(), H.data());
    deck_bars_host(x.data(), n_frames, s, recs.data(), nullptr);
    uint64_t sum_bar = 0, sum_phrase = 0, fold_bar = 0, fold_phrase = 0;
    for (uint32_t k = 0; k < b.n_beats; ++k) {
        EXPECT(recs[k].n_bar >= 0 && recs[k].n_phrase >= 0);
        EXPECT(k + 1 == b.n_beats || recs[k].first_frame + recs[k].frames == recs[k + 1].first_frame);
        EXPECT((uint64_t)recs[k].first_frame + recs[k].frames <= n_frames);
        sum_bar += (uint64_t)recs[k].n_bar; sum_phrase += (uint64_t)recs[k].n_phrase;
    }
    for (uint32_t m = 0; m < M; ++m) fold_bar += H[m];
    for (uint32_t m = 0; m < MQ; ++m) fold_phrase += H[M + m];
    EXPECT(fold_bar == sum_bar && fold_phrase == sum_phrase);
    mx_deck_bar_pick p{};
    deck_bars_pick(H.data(), s, p);
    EXPECT(p.bar_sum == sum_bar && p.bar_best <= p.bar_sum && p.phrase_best <= p.phrase_sum && p.phrase_sum <= sum_phrase);
    if (p.bar_sum) {
        EXPECT(p.bar_phase < M && p.phrase_phase < MQ && p.phrase_phase % M == p.bar_phase && p.bars.period_q32 == (int64_t)M * s.grid.period_q32);
        int64_t n = 0, line = 0;
        deck_grid_next(p.bars, (int64_t)recs[0].first_frame << 32, &n, &line);
        EXPECT(line >= ((int64_t)recs[0].first_frame << 32) && line - p.bars.period_q32 < ((int64_t)recs[0].first_frame << 32));
    }
    std::printf("%-46s %6u beats, bar %u of %u, phrase %u of %u\n", what, b.n_beats, p.bar_phase, M, p.phrase_phase, MQ);
}

int main() {
    const int64_t ONE = (int64_t)1 << 32;
    const int64_t P = 2100 * ONE + (ONE * 6) / 10;
    const uint64_t exact = (uint64_t)((13 * P) >> 32);
    run("K = 127, lead 0, the last beat ends at n_frames", exact, settings(0, P, 127, 0, 4, 4, 2, 3, 0), 13);
    run("one frame short", exact - 1, settings(0, P, 127, 0, 4, 4, 2, 3, 0), 12);
    run("K = 1, period 2048", 2048 * 20 + 300, settings(300 * ONE, 2048 * ONE, 1, 128, 2, 1, 1, 1, 0), 20);
    run("W = 64 at both ends of 128 beats", 2048 * 128 + 128, settings(128 * ONE, 2048 * ONE, 9, 128, 8, 16, 64, 64, 0), 128);
    run("W = 64 and 127 beats: nothing defined", 2048 * 127 + 128, settings(128 * ONE, 2048 * ONE, 9, 128, 8, 16, 64, 64, 0), 127);
    run("first_q32 = -2^62", 260000, settings(-((int64_t)1 << 62), 131072 * ONE, 63, 4096, 3, 5, 1, 2, 0), 1);
    run("first_q32 = 2^62, the shortest period", 50000, settings((int64_t)1 << 62, 2048 * ONE, 63, 0, 4, 4, 4, 8, 0), 24);
    run("max_beats 5 of many", 300000, settings(777 * ONE + 99, 5000 * ONE + 12345, 31, 64, 4, 2, 2, 2, 5), 5);
    run("one beat", 2049 + 128, settings(128 * ONE, 2049 * ONE, 3, 128, 2, 1, 1, 1, 0), 1);

    // every refusal, and that nothing is written on the way to it
    const mx_deck_bars ok = settings(300 * ONE, 2400 * ONE, 63, 128, 4, 4, 4, 8, 0);
    auto bad = [&](const std::function<void(mx_deck_bars&)>& change, uint64_t n_frames = 100000) {
        mx_deck_bars s = ok;
        change(s);
        return refused([&] { (void)deck_bars_check(s, n_frames, true); });
    };
    EXPECT(!bad([](mx_deck_bars&) {}));
    EXPECT(bad([&](mx_deck_bars& s) { s.grid.period_q32 = 2048 * ONE - 1; }) && bad([&](mx_deck_bars& s) { s.grid.period_q32 = 131072 * ONE + 1; }));
    EXPECT(bad([](mx_deck_bars& s) { s.grid.first_q32 = ((int64_t)1 << 62) + 1; }) && bad([](mx_deck_bars& s) { s.grid.first_q32 = INT64_MIN; }));
    EXPECT(bad([](mx_deck_bars& s) { s.lead = 4097; }) && bad([](mx_deck_bars& s) { s.taps = 62; }) && bad([](mx_deck_bars& s) { s.taps = 129; }));
    EXPECT(bad([](mx_deck_bars& s) { s.beats_per_bar = 1; }) && bad([](mx_deck_bars& s) { s.beats_per_bar = 9; }));
    EXPECT(bad([](mx_deck_bars& s) { s.bars_per_phrase = 0; }) && bad([](mx_deck_bars& s) { s.bars_per_phrase = 17; }));
    EXPECT(bad([](mx_deck_bars& s) { s.w_bar = 0; }) && bad([](mx_deck_bars& s) { s.w_phrase = 65; }));
    EXPECT(bad([](mx_deck_bars& s) { s.lo[126] = 1; }) && bad([](mx_deck_bars& s) { s.hi[0] = -16384; }));
    EXPECT(bad([](mx_deck_bars&) {}, 0) && bad([](mx_deck_bars&) {}, ((uint64_t)1 << 30) + 1) && bad([](mx_deck_bars&) {}, 2500));
    EXPECT(bad([](mx_deck_bars&) {}, (uint64_t)2400 * 16385 + 300) && !bad([](mx_deck_bars& s) { s.max_beats = 16384; }, (uint64_t)2400 * 16385 + 300));
    std::vector<int16_t> x(2 * 100000);
    mx_deck_beat one{};
    EXPECT(refused([&] { deck_bars_host(nullptr, 100000, ok, &one, nullptr); }) && refused([&] { deck_bars_host(x.data(), 100000, ok, nullptr, nullptr); }));
    mx_deck_bar_pick p{};
    EXPECT(refused([&] { deck_bars_pick(nullptr, ok, p); }));
    mx_deck_analysis a{};
    a.column = 512; a.taps = 3; a.max_lag = 16; a.lo[1] = a.hi[1] = 16384;
    mx_deck_bars t = ok;
    deck_bars_tables(a, t);
    EXPECT(t.taps == 3 && t.lo[1] == 16384 && t.lo[0] == 0 && t.beats_per_bar == 4);
    a.taps = 4;
    EXPECT(refused([&] { deck_bars_tables(a, t); }) && t.taps == 3);
    // the next line at the edges of its range
    int64_t n = 0, line = 0;
    const int64_t FAR = (int64_t)1 << 62;
    deck_grid_next(mx_deck_beats{-FAR, 2}, FAR, &n, &line);
    EXPECT(n == FAR && line == FAR);
    deck_grid_next(mx_deck_beats{FAR, (int64_t)1 << 56}, -FAR, &n, &line);
    EXPECT(n == -128 && line == -FAR);
    deck_grid_next(mx_deck_beats{5, 10}, -6, nullptr, &line);
    EXPECT(line == -5);
    EXPECT(refused([&] { deck_grid_next(mx_deck_beats{-FAR, 1}, FAR, &n, &line); }) && refused([&] { deck_grid_next(mx_deck_beats{0, 0}, 0, &n, &line); }));
    EXPECT(refused([&] { deck_grid_next(mx_deck_beats{0, ((int64_t)1 << 56) + 1}, 0, &n, &line); }) && refused([&] { deck_grid_next(mx_deck_beats{0, 1}, FAR + 1, &n, &line); }));
    if (failures) { std::fprintf(stderr, "%d failures\n", failures); return 1; }
    std::puts("deck_bars_check: ok");
    return 0;
}
