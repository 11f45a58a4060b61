// mx_deck_bars.cpp -- the deck's bars and phrases, host side (include/mixlab_gpu.h "BARS"): the setting rules and BEATS, the rules themselves in
// plain C++ (mx_deck_bars_host: the CPU test path and the single-thread baseline), pick and next line (pure integer arithmetic), and the deck's fifth analysis.
#include "mx_deck_bars.hpp"
#include "mx_deck_columns.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace mx {

typedef __int128 i128;

static const int64_t kPeriodMin = (int64_t)2048 << 32, kPeriodMax = (int64_t)1 << 49, kFar = (int64_t)1 << 62, kSyncPeriodMax = (int64_t)1 << 56;

static i128 floor_div(i128 a, i128 b) { i128 q = a / b; if (a % b != 0 && (a < 0) != (b < 0)) --q; return q; }   // b > 0 everywhere below

BarsBeats deck_bars_check(const mx_deck_bars& s, uint64_t n_frames, bool with_track) {
    if (s.grid.period_q32 < kPeriodMin || s.grid.period_q32 > kPeriodMax) throw Error(MX_ERR_INVALID, "deck bars: grid.period_q32 outside 2048 .. 131072 frames");
    if (s.grid.first_q32 > kFar || s.grid.first_q32 < -kFar) throw Error(MX_ERR_INVALID, "deck bars: grid.first_q32 beyond 2^62 in magnitude");
    if (s.lead > 4096) throw Error(MX_ERR_INVALID, "deck bars: lead above 4096");
    if (!(s.taps & 1u) || s.taps > 127) throw Error(MX_ERR_INVALID, "deck bars: taps is not odd in 1 .. 127");
    if (s.beats_per_bar < 2 || s.beats_per_bar > 8) throw Error(MX_ERR_INVALID, "deck bars: beats_per_bar outside 2 .. 8");
    if (s.bars_per_phrase < 1 || s.bars_per_phrase > 16) throw Error(MX_ERR_INVALID, "deck bars: bars_per_phrase outside 1 .. 16");
    if (s.w_bar < 1 || s.w_bar > BR_MAX_W) throw Error(MX_ERR_INVALID, "deck bars: w_bar outside 1 .. 64");
    if (s.w_phrase < 1 || s.w_phrase > BR_MAX_W) throw Error(MX_ERR_INVALID, "deck bars: w_phrase outside 1 .. 64");
    for (const int16_t* t : {s.lo, s.hi}) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < 127; ++k) {
            if (k >= s.taps && t[k]) throw Error(MX_ERR_INVALID, std::string("deck bars: ") + (t == s.lo ? "lo" : "hi") + " has a non-zero entry at index taps or above");
            sum += (uint32_t)(t[k] < 0 ? -(int32_t)t[k] : (int32_t)t[k]);
        }
        if (sum > 32767) throw Error(MX_ERR_INVALID, std::string("deck bars: the sum of |") + (t == s.lo ? "lo" : "hi") + "[k]| is above 32767");
    }
    BarsBeats b{0, 0, 0};
    const i128 P = s.grid.period_q32, lead = (i128)s.lead << 32;
    b.n0 = (int64_t)-floor_div((i128)s.grid.first_q32 - lead, P);          // ceil((lead - first) / P): |n0| <= 2^19 + 1
    b.base = (uint64_t)((i128)s.grid.first_q32 + (i128)b.n0 * P);          // in [lead, lead + P)
    if (!with_track) return b;
    if (n_frames < 1 || n_frames > kDeckMaxFrames) throw Error(MX_ERR_INVALID, "deck bars: n_frames outside 1 .. 2^30");
    // line k lies at or before n_frames  <=>  base + k P < (n_frames + lead + 1) 2^32
    const i128 fit = floor_div((((i128)n_frames + 1) << 32) + lead - 1 - (i128)b.base, P);   // the largest such k, or negative
    uint64_t n = fit > 0 ? (uint64_t)fit : 0u;
    if (!n) throw Error(MX_ERR_INVALID, "deck bars: the grid places no whole beat in the track");
    if (s.max_beats && s.max_beats < n) n = s.max_beats;
    if (n > BR_MAX_BEATS) throw Error(MX_ERR_INVALID, "deck bars: more than 16384 beats (set max_beats)");
    b.n_beats = (uint32_t)n;
    return b;
}

void deck_bars_tables(const mx_deck_analysis& a, mx_deck_bars& s) {
    deck_analysis_check(a);
    s.taps = a.taps;
    std::memcpy(s.lo, a.lo, sizeof s.lo);
    std::memcpy(s.hi, a.hi, sizeof s.hi);
}

void deck_bars_host(const int16_t* x, uint64_t n_frames, const mx_deck_bars& s, mx_deck_beat* recs, uint64_t* H) {
    if (!x || !recs) throw Error(MX_ERR_INVALID, "deck bars: NULL argument");
    const BarsBeats b = deck_bars_check(s, n_frames, true);
    const uint32_t K = s.taps, D = (K - 1) / 2, n = b.n_beats;
    const uint64_t P = (uint64_t)s.grid.period_q32;
    // sv[f + D] = s[f] for the frames the last beat's filter reaches: zero outside the track
    const int64_t end = br_line(b.base, P, n, s.lead);
    std::vector<int32_t> sv((size_t)end + 2 * D, 0);
    for (int64_t f = 0; f < std::min<int64_t>((int64_t)n_frames, end + D); ++f) sv[(size_t)f + D] = (int32_t)x[2 * f] + (int32_t)x[2 * f + 1];
    for (uint32_t k = 0; k < n; ++k) {
        const int64_t a = br_line(b.base, P, k, s.lead), c = br_line(b.base, P, k + 1, s.lead), h = br_half(a, c);
        mx_deck_beat r{};
        r.first_frame = (uint32_t)a; r.frames = (uint32_t)(c - a);
        for (int half = 0; half < 2; ++half) {
            uint64_t e[3] = {0u, 0u, 0u};
            for (int64_t f = half ? h : a; f < (half ? c : h); ++f) {
                const int32_t* w = sv.data() + f;
                int32_t a1 = 0, a2 = 0;   // exact: |a| <= 65536 * 32767
                for (uint32_t i = 0; i < K; ++i) { a1 += (int32_t)s.lo[i] * w[i]; a2 += (int32_t)s.hi[i] * w[i]; }
                const int32_t low = a1 >> 14, bb = a2 >> 14, band[3] = {low, bb - low, w[D] - bb};
                for (int j = 0; j < 3; ++j) e[j] += (uint64_t)((int64_t)band[j] * band[j]);
            }
            for (int j = 0; j < 3; ++j) r.v[3 * half + j] = tempo_root(e[j]);
        }
        recs[k] = r;
    }
    for (int which = 0; which < 2; ++which) {
        const uint32_t W = which ? s.w_phrase : s.w_bar;
        for (uint32_t k = 0; k < n; ++k) {
            int64_t N = 0;
            if (br_defined(k, W, n)) {
                int64_t cross = 0, past = 0, future = 0;
                for (uint32_t i = k - W; i < k; ++i)
                    for (uint32_t j = k; j < k + W; ++j) cross += br_dist(recs[i].v, recs[j].v);
                for (uint32_t i = k - W; i < k; ++i)
                    for (uint32_t j = k - W; j < k; ++j) past += br_dist(recs[i].v, recs[j].v);
                for (uint32_t i = k; i < k + W; ++i)
                    for (uint32_t j = k; j < k + W; ++j) future += br_dist(recs[i].v, recs[j].v);
                N = 2 * cross - past - future;
            }
            (which ? recs[k].n_phrase : recs[k].n_bar) = N;
        }
    }
    if (H) {
        const uint32_t M = s.beats_per_bar, MQ = M * s.bars_per_phrase;
        std::fill(H, H + M + MQ, (uint64_t)0);
        for (uint32_t k = 0; k < n; ++k) { H[k % M] += br_clamp(recs[k].n_bar); H[M + k % MQ] += br_clamp(recs[k].n_phrase); }
    }
}

void deck_bars_pick(const uint64_t* H, const mx_deck_bars& s, mx_deck_bar_pick& out) {
    if (!H) throw Error(MX_ERR_INVALID, "deck bars: H is NULL");
    const BarsBeats b = deck_bars_check(s, 0, false);
    const uint32_t M = s.beats_per_bar, MQ = M * s.bars_per_phrase;
    mx_deck_bar_pick p{};
    uint32_t mb = 0;
    for (uint32_t m = 0; m < M; ++m) {
        p.bar_sum += H[m];                       // n_beats * 2^44 at the most: no overflow
        if (H[m] > H[mb]) mb = m;
    }
    if (p.bar_sum) {
        uint32_t mp = mb;
        for (uint32_t m = mb; m < MQ; m += M) {
            p.phrase_sum += H[M + m];
            if (H[M + m] > H[M + mp]) mp = m;
        }
        p.bar_phase = mb; p.phrase_phase = mp; p.bar_best = H[mb]; p.phrase_best = H[M + mp];
        const i128 P = s.grid.period_q32;
        p.bars = mx_deck_beats{(int64_t)((i128)b.base + mb * P), (int64_t)(M * P)};       // base < 2^45: far inside int64
        p.phrases = mx_deck_beats{(int64_t)((i128)b.base + mp * P), (int64_t)(MQ * P)};
    }
    out = p;
}

void deck_grid_next(const mx_deck_beats& g, int64_t pos, int64_t* index, int64_t* line) {
    if (g.period_q32 < 1 || g.period_q32 > kSyncPeriodMax) throw Error(MX_ERR_INVALID, "deck grid next: a period outside 1 .. 2^56");
    if (pos > kFar || pos < -kFar || g.first_q32 > kFar || g.first_q32 < -kFar) throw Error(MX_ERR_INVALID, "deck grid next: a position or first beat beyond 2^62 in magnitude");
    const i128 n = -floor_div((i128)g.first_q32 - pos, g.period_q32);
    if (n > (i128)INT64_MAX) throw Error(MX_ERR_INVALID, "deck grid next: the index is beyond int64");
    if (index) *index = (int64_t)n;
    if (line) *line = (int64_t)((i128)g.first_q32 + n * g.period_q32);   // in [pos, pos + period): at most 2^62 + 2^56
}

// ---- the deck's fifth analysis ----
static DeckLastForms last_bars;   // mx_deck_debug_last_bars

DeckBars::DeckBars(const DeckTrack& deck) : DeckTrackAnalysis(deck, last_bars) {}

void DeckBars::analyse(const mx_deck_bars* s) {
    BarsBeats b{0, 0, 0};
    if (s) b = deck_bars_check(*s, deck_.n_frames, true);
    // need does not depend on the settings: there is room for any, so no later call grows the buffer (nor waits for the one before)
    if (!prepare(kBarsRecRoom + (size_t)BR_MAX_FOLDS * sizeof(uint64_t), !s)) return;
    DeckAnalyseTaps taps{};
    for (uint32_t k = 0; k < s->taps; ++k) { taps.lo[k] = s->lo[k]; taps.hi[k] = s->hi[k]; }
    const uint32_t M = s->beats_per_bar, MQ = M * s->bars_per_phrase;
    DkBarsArgs a{deck_.track, (int64_t)deck_.n_frames, b.base, (uint64_t)s->grid.period_q32, s->lead, b.n_beats, s->taps, M, MQ, s->w_bar, s->w_phrase,
                 (mx_deck_beat*)buf_.p, (uint64_t*)((char*)buf_.p + kBarsRecRoom)};
    uint32_t forms[4];
    launch_deck_bars(a, taps, forms, deck_.load_stream);
    folds_ = M + MQ;
    launched("deck bars launch", b.n_beats, forms);
}

void DeckBars::read(uint64_t first, uint64_t n, mx_deck_beat* dst) {
    read_window(first, n, dst, sizeof(mx_deck_beat), 0, count_, {"deck: no bars analysis", "deck: a window beyond the bars analysis' beats", "deck: dst is NULL", "hipMemcpy(deck bars)"});
}

// (all of the folds or nothing: no window, and no early return)
void DeckBars::read_folds(uint64_t* H, uint32_t cap) {
    if (!count_) throw Error(MX_ERR_INVALID, "deck: no bars analysis");
    if (cap < folds_) throw Error(MX_ERR_INVALID, "deck: cap is below the bars analysis' M + M Q");
    if (!H) throw Error(MX_ERR_INVALID, "deck: H is NULL");
    wait_and_copy(H, kBarsRecRoom, (size_t)folds_ * sizeof(uint64_t), "hipMemcpy(deck bar folds)");
}

void DeckBars::debug_last(uint32_t out[4]) { last_bars.get(out); }

}  // namespace mx
