// deck_tempomap_check.cpp -- the pure host functions of the deck's tempo map (mixlab_amd/csrc/mx_deck_tempomap.cpp) under the host's address and undefined-behaviour
// sanitizers: a plain executable, no device, no Python in the checked process.  tools/deck_tempomap_check.py builds it -- this file and mx_deck_tempomap.cpp
// instrumented, everything else from libmixlab_gpu.so -- and runs it.  It walks the corners where an index or a shift could go wrong (a last window one hop long and
// one shorter than a period, a window at the cap, 2^20 records, the largest scores and penalty of the path, grids and positions at 2^62, every refusal) with buffers of
// exactly the size the header states, and checks what must hold of any result.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <vector>

#include "../mixlab_amd/csrc/mx_deck_bars.hpp"
#include "../mixlab_amd/csrc/mx_deck_tempomap.hpp"

using namespace mx;

static int failures = 0;
#define EXPECT(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static bool refused(const std::function<void()>& f) {
    try { f(); } catch (const Error& e) { return e.code == MX_ERR_INVALID; }
    return false;
}

static mx_deck_tempomap settings(uint32_t hop, uint32_t n, uint64_t p0, uint32_t d, uint32_t W, uint32_t T) {
    mx_deck_tempomap s{};
    s.hop = hop; s.n_periods = n; s.period0_q16 = p0; s.dperiod_q16 = d; s.window_hops = W; s.stride_hops = T;
    return s;
}

static std::vector<int16_t> track(uint64_t n_frames, uint32_t every) {
    std::vector<int16_t> x(2 * n_frames);
    uint32_t r = 12345u + (uint32_t)n_frames;
    for (uint64_t f = 0; f < n_frames; ++f) {
        r = r * 1664525u + 1013904223u;
        const int level = f % every < 12 ? 20000 : 40;
        x[2 * f] = (int16_t)((int)(r >> 16) % level);
        x[2 * f + 1] = f % 7 ? x[2 * f] : (int16_t)-32768;
    }
    return x;
}

static void run(const char* what, uint64_t n_frames, const mx_deck_tempomap& s, uint32_t want_windows, uint64_t penalty) {
    const std::vector<int16_t> x = track(n_frames, 333);
    const uint32_t V = deck_tempomap_check(s, n_frames);
    EXPECT(V == want_windows);
    const uint64_t N = (n_frames + s.hop - 1) / s.hop;
    std::vector<mx_deck_comb> recs((size_t)V * s.n_periods);   // exactly V * n_periods, N, V and V: a write past any is the sanitizer's to find
    std::vector<uint32_t> w((size_t)N), idx(V);
    std::vector<mx_deck_tempo_segment> segs(V);
    deck_tempomap_host(x.data(), n_frames, s, recs.data(), w.data());
    deck_tempomap_host(x.data(), n_frames, s, recs.data(), nullptr);
    for (uint32_t v = 0; v < V; ++v)
        for (uint32_t j = 0; j < s.n_periods; ++j) {
            const mx_deck_comb& r = recs[(size_t)v * s.n_periods + j];
            EXPECT(r.phase < fg_phases(s.period0_q16 + (uint64_t)j * s.dperiod_q16) && r.score < ((uint64_t)1 << 30) && r.beats <= s.window_hops / 4 + 1);
            EXPECT((uint64_t)v * s.stride_hops + r.phase < N || r.beats == 0);
        }
    deck_tempomap_path(recs.data(), V, s.n_periods, penalty, idx.data());
    for (uint32_t v = 0; v < V; ++v) EXPECT(idx[v] < s.n_periods);
    deck_tempomap_segments(recs.data(), s, n_frames, idx.data(), segs.data());
    EXPECT(segs[0].start_q32 == -((int64_t)1 << 62));
    uint32_t empty = 0;
    for (uint32_t v = 0; v < V; ++v) {
        EXPECT(segs[v].window == v && ((segs[v].flags & MX_DECK_TEMPO_EMPTY) != 0) == (segs[v].score == 0));
        empty += segs[v].flags & MX_DECK_TEMPO_EMPTY;
        if (v && segs[v].grid.period_q32) {
            int64_t n = 0, line = 0;
            deck_grid_next(segs[v].grid, segs[v].start_q32, &n, &line);
            EXPECT(line == segs[v].start_q32);                  // a start is a line of its grid
        }
        mx_deck_beats g{}; uint32_t at = 0;
        deck_tempomap_at(segs.data(), V, segs[v].start_q32, &g, &at);
        EXPECT(at >= v && segs[at].start_q32 <= segs[v].start_q32);
        if (g.period_q32) EXPECT(deck_tempomap_step(g, g.period_q32) == ((int64_t)1 << 32));
    }
    mx_deck_beats g{}; uint32_t at = 0;
    deck_tempomap_at(segs.data(), V, (int64_t)1 << 62, &g, &at);
    deck_tempomap_at(segs.data(), V, -((int64_t)1 << 62), &g, &at);
    EXPECT(at == 0 || segs[at].start_q32 == -((int64_t)1 << 62));
    std::printf("%-52s %7u windows x %4u periods, %u empty\n", what, V, s.n_periods, empty);
}

int main() {
    const uint64_t Q = 65536;
    run("a 1-frame track", 1, settings(16, 3, 4 * Q, 7, 10, 3), 1, 0);
    run("T = W, a last window one hop long", 97 * 16, settings(16, 9, 7 * Q + 0x3001, 0x3001, 32, 32), 4, 100);
    run("a last window shorter than a period", 129 * 32 - 7, settings(32, 5, 20 * Q + Q / 2, 1234, 64, 60), 3, 1);
    run("T = 1, W = 8, one period", 40 * 16, settings(16, 1, 4 * Q, 0, 8, 1), 33, (uint64_t)1 << 40);
    run("W at the cap, h = 16, periods round 8000 hops", 300000, settings(16, 5, 8000 * Q, 3000, 16384, 1000), 4, 50);
    run("h = 256, the last hop short", 6 * 256 + 100, settings(256, 2, 4 * Q, 3 * Q / 2, 12, 3), 1, 7);
    run("2^20 records", 16393 * 16, settings(16, 64, 4 * Q, 1, 10, 1), 16384, 3);
    run("1024 periods, 12 windows, the largest penalty", 20000, settings(16, 1024, 30 * Q, 64, 200, 100), 12, (uint64_t)1 << 40);

    // the path at the edges of its range: every score 2^40, the penalty 2^40, the largest table
    {
        const uint32_t V = 16, J = 1024;
        std::vector<mx_deck_comb> recs((size_t)V * J, mx_deck_comb{(uint64_t)1 << 40, 0, 0});
        std::vector<uint32_t> idx(V, 99);
        deck_tempomap_path(recs.data(), V, J, (uint64_t)1 << 40, idx.data());
        for (uint32_t v = 0; v < V; ++v) EXPECT(idx[v] == 0);
        recs[5 * J + 1000].score = ((uint64_t)1 << 40) - 1;
        deck_tempomap_path(recs.data(), V, J, 0, idx.data());
        EXPECT(idx[5] == 0 && idx[4] == 0);
        EXPECT(refused([&] { deck_tempomap_path(recs.data(), V, J, ((uint64_t)1 << 40) + 1, idx.data()); }));
        EXPECT(refused([&] { deck_tempomap_path(recs.data(), 1025, J, 0, idx.data()); }) && refused([&] { deck_tempomap_path(recs.data(), 0, J, 0, idx.data()); }));
        recs[7].score = ((uint64_t)1 << 40) + 1;
        EXPECT(refused([&] { deck_tempomap_path(recs.data(), V, J, 0, idx.data()); }));
        EXPECT(refused([&] { deck_tempomap_path(nullptr, V, J, 0, idx.data()); }) && refused([&] { deck_tempomap_path(recs.data(), V, J, 0, nullptr); }));
    }

    // every refusal of the check
    const mx_deck_tempomap ok = settings(16, 2, 10 * Q, 5, 40, 20);
    auto bad = [&](const std::function<void(mx_deck_tempomap&)>& change, uint64_t n_frames = 1000) {
        mx_deck_tempomap s = ok;
        change(s);
        return refused([&] { (void)deck_tempomap_check(s, n_frames); });
    };
    EXPECT(!bad([](mx_deck_tempomap&) {}));
    EXPECT(bad([](mx_deck_tempomap& s) { s.hop = 8; }) && bad([](mx_deck_tempomap& s) { s.hop = 48; }) && bad([](mx_deck_tempomap& s) { s.hop = 512; }));
    EXPECT(bad([](mx_deck_tempomap& s) { s.n_periods = 0; }) && bad([](mx_deck_tempomap& s) { s.n_periods = 1025; }) && bad([](mx_deck_tempomap& s) { s.dperiod_q16 = 0; }));
    EXPECT(bad([&](mx_deck_tempomap& s) { s.period0_q16 = 4 * Q - 1; }) && bad([&](mx_deck_tempomap& s) { s.period0_q16 = 32768 * Q; }));
    EXPECT(bad([](mx_deck_tempomap& s) { s.period0_q16 = ~(uint64_t)0; }) && bad([](mx_deck_tempomap& s) { s.dperiod_q16 = 0xffffffffu; s.n_periods = 1024; }));
    EXPECT(bad([](mx_deck_tempomap& s) { s.window_hops = 21; }) && !bad([](mx_deck_tempomap& s) { s.window_hops = 22; }) && bad([](mx_deck_tempomap& s) { s.window_hops = 16385; }));
    EXPECT(bad([](mx_deck_tempomap& s) { s.stride_hops = 0; }) && bad([](mx_deck_tempomap& s) { s.stride_hops = 41; }) && bad([](mx_deck_tempomap& s) { s._pad = 1; }));
    EXPECT(bad([](mx_deck_tempomap&) {}, 0) && bad([](mx_deck_tempomap&) {}, ((uint64_t)1 << 30) + 1) && bad([](mx_deck_tempomap& s) { s.stride_hops = 1; }, (uint64_t)1 << 30));
    EXPECT(bad([&](mx_deck_tempomap& s) { s = settings(16, 1024, 4 * Q, 1, 10, 1); }, 1034 * 16) && !bad([&](mx_deck_tempomap& s) { s = settings(16, 1024, 4 * Q, 1, 10, 1); }, 1033 * 16));

    // span at the edges of its range
    mx_deck_tempomap s{}; uint32_t clipped = 9;
    deck_tempomap_span(8192 * Q, (uint64_t)1 << 62, 4096, 4096, 1 << 20, 256, s, &clipped);
    EXPECT(clipped == 1 && s.window_hops == 16384 && s.stride_hops == 16384 && s.period0_q16 + (uint64_t)(s.n_periods - 1) * s.dperiod_q16 == 8192 * Q);
    deck_tempomap_span(4 * Q, 0, 1, 1, 1, 16, s, nullptr);
    EXPECT(s.n_periods == 1 && s.window_hops == 8 && s.stride_hops == 4);
    const mx_deck_tempomap before = s;
    EXPECT(refused([&] { deck_tempomap_span(4 * Q - 1, 0, 1, 1, 1, 16, s, nullptr); }) && refused([&] { deck_tempomap_span(8192 * Q + 1, 0, 1, 1, 1, 16, s, nullptr); }));
    EXPECT(refused([&] { deck_tempomap_span(4 * Q, 0, 0, 1, 1, 16, s, nullptr); }) && refused([&] { deck_tempomap_span(4 * Q, 0, 1, 4097, 1, 16, s, nullptr); }));
    EXPECT(refused([&] { deck_tempomap_span(4 * Q, 0, 1, 1, 0, 16, s, nullptr); }) && refused([&] { deck_tempomap_span(4 * Q, 0, 1, 1, 1, 17, s, nullptr); }));
    EXPECT(refused([&] { deck_tempomap_span(4 * Q, (uint64_t)1 << 30, 1, 1, 1 << 26, 16, s, nullptr); }) && !std::memcmp(&s, &before, sizeof s));

    // look-up and warp at the edges of theirs
    const int64_t FAR = (int64_t)1 << 62;
    mx_deck_tempo_segment two[2] = {{-FAR, {5, 10}, 1, 0, 0}, {FAR, {FAR, (int64_t)1 << 56}, 1, 1, 0}};
    mx_deck_beats g{}; uint32_t at = 7;
    deck_tempomap_at(two, 2, FAR, &g, &at);
    EXPECT(at == 1 && g.first_q32 == FAR);
    deck_tempomap_at(two, 2, FAR - 1, nullptr, &at);
    EXPECT(at == 0);
    deck_tempomap_at(two, 2, -FAR, &g, nullptr);
    EXPECT(g.period_q32 == 10);
    EXPECT(refused([&] { deck_tempomap_at(two, 2, FAR + 1, &g, &at); }) && refused([&] { deck_tempomap_at(two, 2, INT64_MIN, &g, &at); }));
    EXPECT(refused([&] { deck_tempomap_at(two + 1, 1, 0, &g, &at); }) && refused([&] { deck_tempomap_at(two, 0, 0, &g, &at); }) && refused([&] { deck_tempomap_at(nullptr, 2, 0, &g, &at); }));
    EXPECT(deck_tempomap_step(mx_deck_beats{0, (int64_t)1 << 56}, (int64_t)1 << 54) == ((int64_t)4 << 32) && deck_tempomap_step(mx_deck_beats{0, 1}, (int64_t)1 << 56) == 0);
    EXPECT(deck_tempomap_step(mx_deck_beats{0, 3}, (int64_t)2 << 32) == 2 && deck_tempomap_step(mx_deck_beats{0, 1}, (int64_t)2 << 32) == 0);   // 1.5 -> 2, 0.5 -> 0
    EXPECT(refused([&] { (void)deck_tempomap_step(mx_deck_beats{0, (int64_t)1 << 56}, ((int64_t)1 << 54) - ((int64_t)1 << 20)); }) && refused([&] { (void)deck_tempomap_step(mx_deck_beats{0, 0}, 1); }));
    EXPECT(refused([&] { (void)deck_tempomap_step(mx_deck_beats{0, 1}, 0); }) && refused([&] { (void)deck_tempomap_step(mx_deck_beats{0, ((int64_t)1 << 56) + 1}, 1); }));
    EXPECT(refused([&] { (void)deck_tempomap_step(mx_deck_beats{0, 1}, INT64_MIN); }) && refused([&] { (void)deck_tempomap_step(mx_deck_beats{0, INT64_MIN}, 1); }));

    // segments: a path index at n_periods, NULL
    {
        const std::vector<int16_t> x = track(1000, 100);
        std::vector<mx_deck_comb> recs(3 * 2);
        std::vector<uint32_t> idx(3, 0);
        std::vector<mx_deck_tempo_segment> segs(3);
        deck_tempomap_host(x.data(), 1000, ok, recs.data(), nullptr);
        idx[2] = 2;
        EXPECT(refused([&] { deck_tempomap_segments(recs.data(), ok, 1000, idx.data(), segs.data()); }));
        idx[2] = 1;
        deck_tempomap_segments(recs.data(), ok, 1000, idx.data(), segs.data());
        EXPECT(refused([&] { deck_tempomap_segments(nullptr, ok, 1000, idx.data(), segs.data()); }) && refused([&] { deck_tempomap_segments(recs.data(), ok, 1000, nullptr, segs.data()); }));
        EXPECT(refused([&] { deck_tempomap_host(nullptr, 1000, ok, recs.data(), nullptr); }) && refused([&] { deck_tempomap_host(x.data(), 1000, ok, nullptr, nullptr); }));
    }
    if (failures) { std::fprintf(stderr, "%d failures\n", failures); return 1; }
    std::puts("deck_tempomap_check: ok");
    return 0;
}
