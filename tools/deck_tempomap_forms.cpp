// deck_tempomap_forms.cpp -- the two forms of the tempo map's comb kernel (mixlab_amd/csrc/mx_k_deck_tempomap.hip) timed alternately in one
// process on one device, beside the two yardsticks of the section: mx_deck_tempomap_host on one thread, and what a host did before there was a tempo map -- one
// whole-track fine grid launch per window, cut to the window by first_hop / max_beats.  tools/deck_tempomap_cost.py builds it against libmixlab_gpu.so and runs it.
// A ten-minute 48 kHz click track whose period ramps, h = 64; several searches over it.  Before anything is timed the records of both forms are compared with the host
// function's, byte for byte.  Times are hipEvent times round the comb launch alone (the onsets are launched once, before), the median of `reps` after 3 warm-ups.
//
//     deck_tempomap_forms [seconds = 600] [reps = 20]
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../mixlab_amd/csrc/mx_deck_tempomap.hpp"

using namespace mx;

#define HIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static double median(std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; }

int main(int argc, char** argv) {
    const uint64_t seconds = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 600, n = seconds * 48000;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 20, warm = 3;
    const uint32_t hop = 64, log_hop = 6;
    if (n < 48000 || n > kDeckMaxFrames || reps < 1) { std::fprintf(stderr, "seconds outside 1 .. 22369, or reps below 1\n"); return 2; }
    // a burst of 200 frames on a +-300 floor; the period ramps from 22 000 to 23 700 frames (131 to 121.5 BPM) over the track
    std::vector<int16_t> x(2 * n);
    uint32_t r = 17;
    auto rnd = [&](int amp) { r = r * 1664525u + 1013904223u; return (int16_t)((int)((r >> 8) % (2u * amp + 1u)) - amp); };
    for (uint64_t f = 0; f < 2 * n; ++f) x[f] = rnd(300);
    uint64_t bursts = 0;
    for (double at = 5000.4; at + 200 < (double)n; at += 22000.0 + 1700.0 * at / (double)n, ++bursts)
        for (uint64_t f = (uint64_t)at; f < (uint64_t)at + 200; ++f) { x[2 * f] = rnd(20000); x[2 * f + 1] = rnd(20000); }
    const uint64_t N = (n + hop - 1) / hop;
    std::printf("track: %llu frames, %llu bursts, %llu hops of %u\n", (unsigned long long)n, (unsigned long long)bursts, (unsigned long long)N, hop);

    uint32_t* track = nullptr; uint32_t* w = nullptr; mx_deck_comb* rec = nullptr;
    HIP(hipMalloc((void**)&track, n * 4)); HIP(hipMalloc((void**)&w, N * 4)); HIP(hipMalloc((void**)&rec, (size_t)MX_DECK_TEMPOMAP_MAX_RECORDS * sizeof(mx_deck_comb)));
    HIP(hipMemcpy(track, x.data(), n * 4, hipMemcpyHostToDevice));   // int16 L, R interleaved is the deck's own layout: L in the low half of a word
    hipStream_t s; HIP(hipStreamCreate(&s));
    hipEvent_t e0, e1; HIP(hipEventCreate(&e0)); HIP(hipEventCreate(&e1));
    launch_deck_fine_onsets(track, (int64_t)n, log_hop, (uint32_t)N, w, s);
    HIP(hipStreamSynchronize(s));

    struct Search { const char* what; double width; uint32_t window_beats, stride_beats; };
    const Search searches[] = {{"16 beats every 8, +-6 %", 0.06, 16, 8}, {"8 beats every 4, +-10 %", 0.10, 8, 4}, {"16 beats every 8, +-0.3 %", 0.003, 16, 8},
                               {"32 beats every 16, +-2 %", 0.02, 32, 16}, {"64 beats every 32, +-1 % (W at the cap)", 0.01, 64, 32},
                               {"24 beats every 12, +-3 %", 0.03, 24, 12}, {"16 beats every 8, the centre alone", 0.0, 16, 8}};
    const uint64_t centre = (uint64_t)(22850.0 / hop * 65536.0);
    for (const Search& q : searches) {
        mx_deck_tempomap t{}; uint32_t clipped = 0;
        deck_tempomap_span(centre, (uint64_t)((double)centre * q.width), q.window_beats, q.stride_beats, N, hop, t, &clipped);
        const uint32_t V = deck_tempomap_check(t, n);
        const size_t n_rec = (size_t)V * t.n_periods;
        std::vector<mx_deck_comb> want(n_rec), got(n_rec);
        const auto h0 = std::chrono::steady_clock::now();
        deck_tempomap_host(x.data(), n, t, want.data(), nullptr);
        const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - h0).count();
        DkTempoArgs a{track, (int64_t)n, log_hop, (uint32_t)N, t.n_periods, V, t.window_hops, t.stride_hops, t.period0_q16, t.dperiod_q16,
                      (uint32_t)fg_trip(std::min<uint64_t>(t.window_hops, N), 0, t.period0_q16, 0), TM_FORM_RULE, w, rec};
        uint32_t forms[4] = {0, 0, 0, 0};
        std::vector<float> ms[2];
        for (uint32_t form : {(uint32_t)TM_FORM_STAGED, (uint32_t)TM_FORM_GLOBAL}) {
            a.form = form;
            HIP(hipMemsetAsync(rec, 0xff, n_rec * sizeof(mx_deck_comb), s));
            launch_deck_tempomap_comb(a, forms, s);
            HIP(hipGetLastError());
            HIP(hipStreamSynchronize(s));
            HIP(hipMemcpy(got.data(), rec, n_rec * sizeof(mx_deck_comb), hipMemcpyDeviceToHost));
            if (std::memcmp(got.data(), want.data(), n_rec * sizeof(mx_deck_comb))) { std::fprintf(stderr, "%s: form %u differs from mx_deck_tempomap_host\n", q.what, form); return 1; }
        }
        for (int k = 0; k < warm + reps; ++k)
            for (int f = 0; f < 2; ++f) {   // alternately
                a.form = f ? TM_FORM_GLOBAL : TM_FORM_STAGED;
                HIP(hipEventRecord(e0, s));
                launch_deck_tempomap_comb(a, forms, s);
                HIP(hipEventRecord(e1, s));
                HIP(hipEventSynchronize(e1));
                float t_ms = 0; HIP(hipEventElapsedTime(&t_ms, e0, e1));
                if (k >= warm) ms[f].push_back(t_ms);
            }
        a.form = TM_FORM_RULE;
        launch_deck_tempomap_comb(a, forms, s);
        HIP(hipStreamSynchronize(s));
        // what a host did before: per window one fine grid analysis of the whole track from first_hop = v T on, cut at the teeth a window holds (the tooth weights
        // computed afresh each time, as mx_deck_analyse_finegrid does).  Its records are not the map's (max_beats cuts by teeth, not at E_v); only its time is of interest.
        std::vector<float> before;
        if (t.n_periods <= MX_DECK_FINEGRID_MAX_PERIODS)
            for (int k = 0; k < 1 + 3; ++k) {
                HIP(hipEventRecord(e0, s));
                for (uint32_t v = 0; v < V; ++v) {
                    const uint32_t first = v * t.stride_hops, beats = std::max<uint32_t>(2, (uint32_t)(((uint64_t)t.window_hops << 16) / t.period0_q16));
                    DkFineArgs fa{track, (int64_t)n, log_hop, (uint32_t)N, t.n_periods, first, t.period0_q16, t.dperiod_q16, (uint32_t)fg_trip(N, first, t.period0_q16, beats), w, rec};
                    uint32_t ff[4];
                    launch_deck_finegrid(fa, ff, s);
                }
                HIP(hipEventRecord(e1, s));
                HIP(hipEventSynchronize(e1));
                float t_ms = 0; HIP(hipEventElapsedTime(&t_ms, e0, e1));
                if (k >= 1) before.push_back(t_ms);
            }
        launch_deck_fine_onsets(track, (int64_t)n, log_hop, (uint32_t)N, w, s);   // (the fine grid launches wrote the same w; once more for good measure)
        HIP(hipStreamSynchronize(s));
        std::printf("%-40s periods=%u dperiod=%u W=%u T=%u windows=%u records=%zu trip=%u clipped=%u | staged ms median=%.4f min=%.4f | global ms median=%.4f min=%.4f | "
                    "rule: staged=%u global=%u | host one thread ms=%.1f | a fine grid launch per window ms median=%.2f\n",
                    q.what, t.n_periods, t.dperiod_q16, t.window_hops, t.stride_hops, V, n_rec, a.trip, clipped, median(ms[0]), *std::min_element(ms[0].begin(), ms[0].end()),
                    median(ms[1]), *std::min_element(ms[1].begin(), ms[1].end()), forms[DK_TEMPO_FORM_STAGED], forms[DK_TEMPO_FORM_GLOBAL], host_ms,
                    before.empty() ? 0.0 : median(before));
        std::fflush(stdout);
    }
    HIP(hipFree(track)); HIP(hipFree(w)); HIP(hipFree(rec));
    std::puts("deck_tempomap_forms done");
    return 0;
}
