// mx_deck_tempomap.cpp -- the deck's tempo map, host side (include/mixlab_gpu.h "TEMPO MAP"): the setting rules, the rules themselves in plain
// C++ (mx_deck_tempomap_host: the CPU test path and the single-thread baseline), span, path, segments, look-up and warp (pure integer arithmetic), and the deck's
// sixth analysis.
#include <algorithm>
#include <cstring>
#include <vector>

#include "mx_deck_tempomap.hpp"

namespace mx {

typedef __int128 i128;

static const int64_t kMaxStep = (int64_t)4 << 32, kMaxPeriod = (int64_t)1 << 56, kFar = (int64_t)1 << 62;
static const uint64_t kMaxPenalty = (uint64_t)1 << 40, kMaxScore = (uint64_t)1 << 40;
static const uint64_t kSpanPeriodMax = (uint64_t)(TM_MAX_WINDOW / 2) << 16;   // 2 ceil(P) <= the cap

static void hop_check(uint32_t hop) {
    if (hop < 16 || hop > 256 || (hop & (hop - 1))) throw Error(MX_ERR_INVALID, "deck tempo map: hop must be a power of two, 16 .. 256");
}

// every rule that needs no track; P_max
static uint64_t settings_check(const mx_deck_tempomap& s) {
    hop_check(s.hop);
    if (s.n_periods < 1 || s.n_periods > MX_DECK_TEMPOMAP_MAX_PERIODS) throw Error(MX_ERR_INVALID, "deck tempo map: n_periods outside 1 .. 1024");
    if (s.n_periods > 1 && s.dperiod_q16 < 1) throw Error(MX_ERR_INVALID, "deck tempo map: dperiod_q16 must be at least 1 with more than one period");
    const uint64_t Pmax = s.period0_q16 + (uint64_t)(s.n_periods - 1) * s.dperiod_q16;   // (period0 <= 2^31 is held first: no overflow)
    if (s.period0_q16 < FG_PERIOD_MIN || s.period0_q16 > FG_PERIOD_MAX || Pmax > FG_PERIOD_MAX) throw Error(MX_ERR_INVALID, "deck tempo map: a period outside 4 .. 32768 hops");
    if (s.window_hops > TM_MAX_WINDOW || s.window_hops < 2u * (uint64_t)fg_phases(Pmax))
        throw Error(MX_ERR_INVALID, "deck tempo map: window_hops outside 2 ceil(P_max) .. 16384");
    if (s.stride_hops < 1 || s.stride_hops > s.window_hops) throw Error(MX_ERR_INVALID, "deck tempo map: stride_hops outside 1 .. window_hops");
    if (s._pad) throw Error(MX_ERR_INVALID, "deck tempo map: _pad must be 0");
    return Pmax;
}

static uint32_t windows_check(const mx_deck_tempomap& s, uint64_t N) {
    const uint64_t V = tm_windows(N, s.window_hops, s.stride_hops);
    if (V * s.n_periods > MX_DECK_TEMPOMAP_MAX_RECORDS) throw Error(MX_ERR_INVALID, "deck tempo map: windows x n_periods above 2^20");
    return (uint32_t)V;
}

uint32_t deck_tempomap_check(const mx_deck_tempomap& s, uint64_t n_frames) {
    settings_check(s);
    if (n_frames < 1 || n_frames > kDeckMaxFrames) throw Error(MX_ERR_INVALID, "deck tempo map: n_frames outside 1 .. 2^30");
    return windows_check(s, (n_frames + s.hop - 1) / s.hop);
}

void deck_tempomap_span(uint64_t centre, uint64_t halfwidth, uint32_t K, uint32_t stride_beats, uint64_t N, uint32_t hop, mx_deck_tempomap& out, uint32_t* clipped) {
    hop_check(hop);
    if (centre < FG_PERIOD_MIN || centre > kSpanPeriodMax) throw Error(MX_ERR_INVALID, "deck tempo map: the centre period lies outside 4 .. 8192 hops");
    if (N < 1 || N > ((uint64_t)1 << 26)) throw Error(MX_ERR_INVALID, "deck tempo map: n_hops outside 1 .. 2^26");
    if (K < 1 || K > 4096) throw Error(MX_ERR_INVALID, "deck tempo map: window_beats outside 1 .. 4096");
    if (stride_beats < 1 || stride_beats > 4096) throw Error(MX_ERR_INVALID, "deck tempo map: stride_beats outside 1 .. 4096");
    if (halfwidth > FG_PERIOD_MAX) halfwidth = FG_PERIOD_MAX;
    const uint64_t d = std::max<uint64_t>(1, 32768 / K);
    const uint64_t want = (halfwidth + d - 1) / d;
    const uint64_t m = std::min<uint64_t>(want, 511);
    const uint64_t below = std::min(m, (centre - FG_PERIOD_MIN) / d), above = std::min(m, (kSpanPeriodMax - centre) / d);
    const uint64_t Pmax = centre + above * d;
    const uint64_t W0 = std::max<uint64_t>(((uint64_t)K * Pmax + 65535u) >> 16, 2u * (uint64_t)fg_phases(Pmax)), W = std::min<uint64_t>(W0, TM_MAX_WINDOW);
    const uint64_t T0 = std::max<uint64_t>(1, ((uint64_t)stride_beats * centre) >> 16), T = std::min(T0, W);
    mx_deck_tempomap s{};
    s.hop = hop; s.n_periods = (uint32_t)(below + above + 1); s.period0_q16 = centre - below * d; s.dperiod_q16 = (uint32_t)d;
    s.window_hops = (uint32_t)W; s.stride_hops = (uint32_t)T; s._pad = 0;
    settings_check(s);
    windows_check(s, N);
    out = s;
    if (clipped) *clipped = (below < want || above < want || W < W0 || T < T0) ? 1u : 0u;
}

void deck_tempomap_host(const int16_t* x, uint64_t n_frames, const mx_deck_tempomap& s, mx_deck_comb* recs, uint32_t* w_or_null) {
    if (!x || !recs) throw Error(MX_ERR_INVALID, "deck tempo map: NULL argument");
    const uint32_t V = deck_tempomap_check(s, n_frames);
    const uint64_t N = (n_frames + s.hop - 1) / s.hop;
    std::vector<uint32_t> o((size_t)N), w((size_t)N);
    uint32_t before = 0;
    for (uint64_t i = 0; i < N; ++i) {
        uint64_t e = 0;
        for (uint64_t f = i * s.hop; f < std::min<uint64_t>((i + 1) * s.hop, n_frames); ++f)
            e += fg_square((uint32_t)(uint16_t)x[2 * f] | ((uint32_t)(uint16_t)x[2 * f + 1] << 16));
        const uint32_t a = tempo_root(e);
        o[(size_t)i] = fg_onset(a, before);
        before = a;
    }
    for (uint64_t i = 0; i < N; ++i) w[(size_t)i] = fg_tooth(i ? o[(size_t)i - 1] : 0u, o[(size_t)i], i + 1 < N ? o[(size_t)i + 1] : 0u);
    if (w_or_null) std::memcpy(w_or_null, w.data(), (size_t)N * sizeof(uint32_t));
    for (uint32_t v = 0; v < V; ++v) {
        const uint64_t a = (uint64_t)v * s.stride_hops, E = a + tm_window_len(v, s.window_hops, s.stride_hops, (uint32_t)N);
        for (uint32_t j = 0; j < s.n_periods; ++j) {
            const uint64_t P = s.period0_q16 + (uint64_t)j * s.dperiod_q16;
            mx_deck_comb best{0, 0, 0};
            for (uint32_t phi = 0; phi < fg_phases(P); ++phi) {
                uint64_t S = 0; uint32_t n = 0;
                for (uint64_t k = 0;; ++k) {
                    const uint64_t i = a + phi + ((k * P) >> 16);
                    if (i >= E) break;
                    S += w[(size_t)i]; ++n;
                }
                if (phi == 0 || S > best.score) { best.score = S; best.phase = phi; best.beats = n; }
            }
            recs[(size_t)v * s.n_periods + j] = best;
        }
    }
}

void deck_tempomap_path(const mx_deck_comb* recs, uint32_t V, uint32_t J, uint64_t penalty, uint32_t* index) {
    if (!recs || !index) throw Error(MX_ERR_INVALID, "deck tempo map: NULL argument");
    if (V < 1 || J < 1 || (uint64_t)V * J > MX_DECK_TEMPOMAP_MAX_RECORDS) throw Error(MX_ERR_INVALID, "deck tempo map: windows x n_periods outside 1 .. 2^20");
    if (penalty > kMaxPenalty) throw Error(MX_ERR_INVALID, "deck tempo map: penalty above 2^40");
    for (size_t k = 0; k < (size_t)V * J; ++k)
        if (recs[k].score > kMaxScore) throw Error(MX_ERR_INVALID, "deck tempo map: a score above 2^40");
    // |D| <= V 2^40 + 2^40 2^20 <= 2^61
    std::vector<int64_t> D(J), next(J);
    std::vector<uint32_t> from((size_t)V * J, 0u);
    for (uint32_t j = 0; j < J; ++j) D[j] = (int64_t)recs[j].score;
    const int64_t pen = (int64_t)penalty;
    for (uint32_t v = 1; v < V; ++v) {
        for (uint32_t j = 0; j < J; ++j) {
            int64_t best = 0; uint32_t bi = 0;
            for (uint32_t i = 0; i < J; ++i) {
                const int64_t c = D[i] - pen * (int64_t)(i > j ? i - j : j - i);
                if (i == 0 || c > best) { best = c; bi = i; }
            }
            next[j] = (int64_t)recs[(size_t)v * J + j].score + best;
            from[(size_t)v * J + j] = bi;
        }
        D.swap(next);
    }
    uint32_t j = 0;
    for (uint32_t i = 1; i < J; ++i)
        if (D[i] > D[j]) j = i;
    for (uint32_t v = V; v-- > 0;) { index[v] = j; j = from[(size_t)v * J + j]; }
}

static i128 floor_div(i128 a, i128 b) { i128 q = a / b; if (a % b != 0 && (a < 0) != (b < 0)) --q; return q; }   // b > 0

void deck_tempomap_segments(const mx_deck_comb* recs, const mx_deck_tempomap& s, uint64_t n_frames, const uint32_t* index, mx_deck_tempo_segment* segs) {
    if (!recs || !index || !segs) throw Error(MX_ERR_INVALID, "deck tempo map: NULL argument");
    const uint32_t V = deck_tempomap_check(s, n_frames);
    for (uint32_t v = 0; v < V; ++v)
        if (index[v] >= s.n_periods) throw Error(MX_ERR_INVALID, "deck tempo map: a path index at or above n_periods");
    const mx_deck_beats none{0, 0};
    mx_deck_beats last = none;   // the grid an empty window inherits: the nearest earlier one, or (before any) the first there is
    for (uint32_t v = 0; v < V && !last.period_q32; ++v) {
        const mx_deck_comb& r = recs[(size_t)v * s.n_periods + index[v]];
        if (r.score) {
            const uint64_t P = s.period0_q16 + (uint64_t)index[v] * s.dperiod_q16;
            last = mx_deck_beats{(int64_t)((((uint64_t)v * s.stride_hops + r.phase) * s.hop + s.hop / 2) << 32), (int64_t)((P * s.hop) << 16)};
        }
    }
    for (uint32_t v = 0; v < V; ++v) {
        const mx_deck_comb& r = recs[(size_t)v * s.n_periods + index[v]];
        mx_deck_tempo_segment g{};
        g.score = r.score; g.window = v;
        if (r.score) {
            const uint64_t P = s.period0_q16 + (uint64_t)index[v] * s.dperiod_q16;
            // (v T + phase) h + h / 2 < 2^31 frames (v T < N, phase < 2^15 hops); P h <= 2^39
            last = mx_deck_beats{(int64_t)((((uint64_t)v * s.stride_hops + r.phase) * s.hop + s.hop / 2) << 32), (int64_t)((P * s.hop) << 16)};
        } else {
            g.flags = MX_DECK_TEMPO_EMPTY;
        }
        g.grid = last;
        if (v == 0) {
            g.start_q32 = -kFar;
        } else {
            const int64_t m = (int64_t)((((uint64_t)v * s.stride_hops + (s.window_hops - s.stride_hops) / 2u) * s.hop) << 32);   // below 2^31 frames
            g.start_q32 = m;
            if (last.period_q32) g.start_q32 = (int64_t)((i128)last.first_q32 - floor_div((i128)last.first_q32 - m, last.period_q32) * last.period_q32);   // mx_deck_grid_next
        }
        segs[v] = g;
    }
}

void deck_tempomap_at(const mx_deck_tempo_segment* segs, uint32_t n, int64_t pos, mx_deck_beats* grid, uint32_t* segment) {
    if (!segs || !n) throw Error(MX_ERR_INVALID, "deck tempo map: no segments");
    if (pos > kFar || pos < -kFar) throw Error(MX_ERR_INVALID, "deck tempo map: a position beyond 2^62 in magnitude");
    for (uint32_t v = n; v-- > 0;)
        if (segs[v].start_q32 <= pos) {
            if (grid) *grid = segs[v].grid;
            if (segment) *segment = v;
            return;
        }
    throw Error(MX_ERR_INVALID, "deck tempo map: the position lies before the first segment's start");
}

int64_t deck_tempomap_step(const mx_deck_beats& grid, int64_t out_period) {
    if (grid.period_q32 < 1 || grid.period_q32 > kMaxPeriod) throw Error(MX_ERR_INVALID, "deck tempo map: a grid period outside 1 .. 2^56");
    if (out_period < 1 || out_period > kMaxPeriod) throw Error(MX_ERR_INVALID, "deck tempo map: out_period_q32 outside 1 .. 2^56");
    const i128 n = (i128)grid.period_q32 << 32, d = out_period;
    i128 q = n / d; const i128 r = n % d;
    if (2 * r > d || (2 * r == d && (q & 1))) ++q;
    if (q > (i128)kMaxStep) throw Error(MX_ERR_INVALID, "deck tempo map: the step is above 4 * 2^32");
    return (int64_t)q;
}

// ---- the deck's sixth analysis ----
static DeckLastForms last_tempomap;   // mx_deck_debug_last_tempomap

DeckTempoMap::DeckTempoMap(const DeckTrack& deck) : DeckTrackAnalysis(deck, last_tempomap) {}

void DeckTempoMap::analyse(const mx_deck_tempomap* s) {
    const uint32_t V = s ? deck_tempomap_check(*s, deck_.n_frames) : 0;
    const uint64_t N = s ? (deck_.n_frames + s->hop - 1) / s->hop : 0;
    const size_t rec_room = (size_t)V * (s ? s->n_periods : 0) * sizeof(mx_deck_comb);
    // w lies behind THIS analysis' records: in a buffer that stays its place may move under an analysis in flight, which the stream's own order makes safe
    if (!prepare(rec_room + (size_t)N * sizeof(uint32_t), !s)) return;
    uint32_t log_hop = 0;
    while ((1u << log_hop) < s->hop) ++log_hop;
    DkTempoArgs a{deck_.track, (int64_t)deck_.n_frames, log_hop, (uint32_t)N, s->n_periods, V, s->window_hops, s->stride_hops, s->period0_q16, s->dperiod_q16,
                  (uint32_t)fg_trip(std::min<uint64_t>(s->window_hops, N), 0, s->period0_q16, 0), TM_FORM_RULE, (uint32_t*)((char*)buf_.p + rec_room), (mx_deck_comb*)buf_.p};
    uint32_t forms[4];
    launch_deck_tempomap(a, forms, deck_.load_stream);
    hops_ = N; w_offset_ = rec_room;
    launched("deck tempo map launch", (uint64_t)V * s->n_periods, forms);
}

void DeckTempoMap::read(uint64_t first, uint64_t n, mx_deck_comb* dst) {
    read_window(first, n, dst, sizeof(mx_deck_comb), 0, count_, {"deck: no tempo map", "deck: a window beyond the tempo map's records", "deck: dst is NULL", "hipMemcpy(deck tempo map)"});
}

void DeckTempoMap::read_onsets(uint64_t first, uint64_t n, uint32_t* w) {
    read_window(first, n, w, sizeof(uint32_t), w_offset_, hops_, {"deck: no tempo map", "deck: a window beyond the tempo map's hops", "deck: w is NULL", "hipMemcpy(deck tempo onsets)"});
}

void DeckTempoMap::debug_last(uint32_t out[4]) { last_tempomap.get(out); }

}  // namespace mx
