// mx_deck_finegrid.cpp -- the deck's fine beat grid, host side (include/mixlab_gpu.h "FINE GRID"): the setting rules, the rules themselves in
// plain C++ (mx_deck_finegrid_host: the CPU test path and the single-thread baseline), span, pick and sync (pure integer arithmetic), and the deck's fourth analysis.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mx_deck_finegrid.hpp"

namespace mx {

typedef __int128 i128;

static const int64_t kMaxStep = (int64_t)4 << 32, kMaxPeriod = (int64_t)1 << 56, kMaxPos = (int64_t)1 << 62;

static void hop_check(uint32_t hop) {
    if (hop < 16 || hop > 256 || (hop & (hop - 1))) throw Error(MX_ERR_INVALID, "deck fine grid: hop must be a power of two, 16 .. 256");
}

uint64_t deck_finegrid_count(uint64_t n_frames, uint32_t hop) {
    if (n_frames < 1 || n_frames > kDeckMaxFrames) throw Error(MX_ERR_INVALID, "deck fine grid: n_frames outside 1 .. 2^30");
    hop_check(hop);
    return (n_frames + hop - 1) / hop;
}

// without a track: every rule but first_hop < N (mx_deck_finegrid_pick has none)
void deck_finegrid_check(const mx_deck_finegrid& s, uint64_t n_frames, bool with_track) {
    hop_check(s.hop);
    if (s.n_periods < 1 || s.n_periods > MX_DECK_FINEGRID_MAX_PERIODS) throw Error(MX_ERR_INVALID, "deck fine grid: n_periods outside 1 .. 8192");
    if (s.n_periods > 1 && s.dperiod_q16 < 1) throw Error(MX_ERR_INVALID, "deck fine grid: dperiod_q16 must be at least 1 with more than one period");
    if (s.period0_q16 < FG_PERIOD_MIN || s.period0_q16 > FG_PERIOD_MAX || s.period0_q16 + (uint64_t)(s.n_periods - 1) * s.dperiod_q16 > FG_PERIOD_MAX)
        throw Error(MX_ERR_INVALID, "deck fine grid: a period outside 4 .. 32768 hops");
    if (s.max_beats == 1) throw Error(MX_ERR_INVALID, "deck fine grid: max_beats must be 0 or at least 2");
    if (s._pad) throw Error(MX_ERR_INVALID, "deck fine grid: _pad must be 0");
    if (with_track && s.first_hop >= deck_finegrid_count(n_frames, s.hop)) throw Error(MX_ERR_INVALID, "deck fine grid: first_hop is not below the track's hops");
}

void deck_finegrid_span(uint64_t centre, uint64_t halfwidth, uint32_t B, uint64_t N, uint32_t hop, mx_deck_finegrid& out, uint32_t* clipped) {
    hop_check(hop);
    if (centre < FG_PERIOD_MIN || centre > FG_PERIOD_MAX) throw Error(MX_ERR_INVALID, "deck fine grid: the centre period lies outside 4 .. 32768 hops");
    if (N < 1 || N > ((uint64_t)1 << 26)) throw Error(MX_ERR_INVALID, "deck fine grid: n_hops outside 1 .. 2^26");
    if (B == 1) throw Error(MX_ERR_INVALID, "deck fine grid: the beat limit must be 0 or at least 2");
    if (halfwidth > FG_PERIOD_MAX) halfwidth = FG_PERIOD_MAX;   // (no wider than the whole range: nothing is lost, and the sums below stay small)
    uint64_t K = ((N << 16) + centre - 1) / centre;             // >= 1
    if (B && B < K) K = B;
    const uint64_t d = std::max<uint64_t>(1, 32768 / K);
    const uint64_t want = (halfwidth + d - 1) / d;
    const uint64_t m = std::min<uint64_t>(want, 4095);
    const uint64_t below = std::min(m, (centre - FG_PERIOD_MIN) / d), above = std::min(m, (FG_PERIOD_MAX - centre) / d);
    mx_deck_finegrid s{};
    s.hop = hop; s.n_periods = (uint32_t)(below + above + 1); s.period0_q16 = centre - below * d; s.dperiod_q16 = (uint32_t)d; s.first_hop = 0; s.max_beats = B; s._pad = 0;
    out = s;
    if (clipped) *clipped = (below < want || above < want) ? 1u : 0u;
}

uint64_t deck_finegrid_period(double period_columns, uint32_t column, uint32_t hop) {
    hop_check(hop);
    if (column < 64 || column > 4096 || (column & (column - 1))) throw Error(MX_ERR_INVALID, "deck fine grid: column must be a power of two, 64 .. 4096");
    if (!std::isfinite(period_columns)) throw Error(MX_ERR_INVALID, "deck fine grid: period_columns is not finite");
    const double x = period_columns * ((double)column / (double)hop * 65536.0);   // (the factor is a power of two: the product is exact short of overflow)
    if (!(x >= (double)FG_PERIOD_MIN - 1.0 && x <= (double)FG_PERIOD_MAX + 1.0)) throw Error(MX_ERR_INVALID, "deck fine grid: the period lies outside 4 .. 32768 hops");
    const uint64_t p = (uint64_t)std::nearbyint(x);   // the default rounding mode: to nearest, ties to even
    if (p < FG_PERIOD_MIN || p > FG_PERIOD_MAX) throw Error(MX_ERR_INVALID, "deck fine grid: the period lies outside 4 .. 32768 hops");
    return p;
}

void deck_finegrid_host(const int16_t* x, uint64_t n_frames, const mx_deck_finegrid& s, mx_deck_comb* recs, uint32_t* w_or_null) {
    if (!x || !recs) throw Error(MX_ERR_INVALID, "deck fine grid: NULL argument");
    deck_finegrid_check(s, n_frames, true);
    const uint64_t N = deck_finegrid_count(n_frames, s.hop);
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
    for (uint32_t j = 0; j < s.n_periods; ++j) {
        const uint64_t P = s.period0_q16 + (uint64_t)j * s.dperiod_q16;
        mx_deck_comb best{0, 0, 0};
        for (uint32_t phi = 0; phi < fg_phases(P); ++phi) {
            uint64_t S = 0; uint32_t n = 0;
            for (uint64_t k = 0; !s.max_beats || k < s.max_beats; ++k) {
                const uint64_t i = (uint64_t)s.first_hop + phi + ((k * P) >> 16);
                if (i >= N) break;
                S += w[(size_t)i]; ++n;
            }
            if (phi == 0 || S > best.score) { best.score = S; best.phase = phi; best.beats = n; }
        }
        recs[j] = best;
    }
}

void deck_finegrid_pick(const mx_deck_comb* recs, const mx_deck_finegrid& s, double rate, mx_deck_fine_pick& out) {
    if (!recs) throw Error(MX_ERR_INVALID, "deck fine grid: recs is NULL");
    deck_finegrid_check(s, 0, false);
    if (!std::isfinite(rate) || !(rate > 0.0)) throw Error(MX_ERR_INVALID, "deck fine grid: rate must be finite and positive");
    uint32_t best = 0;
    for (uint32_t j = 1; j < s.n_periods; ++j)
        if (recs[j].score > recs[best].score) best = j;
    mx_deck_fine_pick p{};
    if (recs[best].score) {
        const uint64_t P = s.period0_q16 + (uint64_t)best * s.dperiod_q16;
        p.grid.period_q32 = (int64_t)((P * s.hop) << 16);                                                              // P h <= 2^39
        p.grid.first_q32 = (int64_t)((((uint64_t)s.first_hop + recs[best].phase) * s.hop + s.hop / 2) << 32);       // below 2^31 frames
        p.score = recs[best].score; p.index = best; p.n_beats = recs[best].beats;
        p.bpm = (60.0 * rate * 65536.0) / ((double)P * (double)s.hop);
    }
    out = p;
}

// round(n / d) to nearest, ties to even; n >= 0, d > 0
static i128 div_half_even(i128 n, i128 d) {
    i128 q = n / d; const i128 r = n % d;
    if (2 * r > d || (2 * r == d && (q & 1))) ++q;
    return q;
}
static i128 floor_mod(i128 a, i128 m) { i128 r = a % m; if (r < 0) r += m; return r; }

void deck_sync(const mx_deck_beats& l, int64_t lpos, int64_t lstep, const mx_deck_beats& f, int64_t fpos, mx_deck_sync_result& out) {
    if (l.period_q32 < 1 || l.period_q32 > kMaxPeriod || f.period_q32 < 1 || f.period_q32 > kMaxPeriod) throw Error(MX_ERR_INVALID, "deck sync: a period outside 1 .. 2^56");
    auto far = [](int64_t v) { return v > kMaxPos || v < -kMaxPos; };
    if (far(lpos) || far(fpos) || far(l.first_q32) || far(f.first_q32)) throw Error(MX_ERR_INVALID, "deck sync: a position or first beat beyond 2^62 in magnitude");
    const i128 Pl = l.period_q32, Pf = f.period_q32;
    const i128 mag = div_half_even((lstep < 0 ? -(i128)lstep : (i128)lstep) * Pf, Pl);
    if (mag > (i128)kMaxStep) throw Error(MX_ERR_INVALID, "deck sync: the follower's step is above 4 * 2^32 in magnitude");
    const i128 a = floor_mod((i128)lpos - l.first_q32, Pl), b = div_half_even(a * Pf, Pl), c = floor_mod((i128)fpos - f.first_q32, Pf);
    i128 delta = b - c;                    // in (-Pf, Pf]
    while (2 * delta > Pf) delta -= Pf;
    while (2 * delta <= -Pf) delta += Pf;
    out.step_q32 = lstep < 0 ? -(int64_t)mag : (int64_t)mag;
    out.seek_q32 = (int64_t)((i128)fpos + delta);   // |fpos| <= 2^62, |delta| <= 2^55
    out.delta_q32 = (int64_t)delta;
}

// ---- the deck's fourth analysis ----
static DeckLastForms last_finegrid;   // mx_deck_debug_last_finegrid
static const size_t kRecRoom = (size_t)MX_DECK_FINEGRID_MAX_PERIODS * sizeof(mx_deck_comb);

DeckFineGrid::DeckFineGrid(const DeckTrack& deck) : DeckTrackAnalysis(deck, last_finegrid) {}

void DeckFineGrid::analyse(const mx_deck_finegrid* s) {
    if (s) deck_finegrid_check(*s, deck_.n_frames, true);
    const uint64_t N = s ? deck_finegrid_count(deck_.n_frames, s->hop) : 0;
    // need does not depend on n_periods: there is room for any, so a second stage never grows the buffer (nor waits for the first)
    if (!prepare(kRecRoom + (size_t)N * sizeof(uint32_t), !s)) return;
    uint32_t log_hop = 0;
    while ((1u << log_hop) < s->hop) ++log_hop;
    DkFineArgs a{deck_.track, (int64_t)deck_.n_frames, log_hop, (uint32_t)N, s->n_periods, s->first_hop, s->period0_q16, s->dperiod_q16,
                 (uint32_t)fg_trip(N, s->first_hop, s->period0_q16, s->max_beats), (uint32_t*)((char*)buf_.p + kRecRoom), (mx_deck_comb*)buf_.p};
    uint32_t forms[4];
    launch_deck_finegrid(a, forms, deck_.load_stream);
    hops_ = N;
    launched("deck fine grid launch", s->n_periods, forms);
}

void DeckFineGrid::read(uint64_t first, uint64_t n, mx_deck_comb* dst) {
    read_window(first, n, dst, sizeof(mx_deck_comb), 0, count_, {"deck: no fine grid", "deck: a window beyond the fine grid's periods", "deck: dst is NULL", "hipMemcpy(deck fine grid)"});
}

void DeckFineGrid::read_onsets(uint64_t first, uint64_t n, uint32_t* w) {
    read_window(first, n, w, sizeof(uint32_t), kRecRoom, hops_, {"deck: no fine grid", "deck: a window beyond the fine grid's hops", "deck: w is NULL", "hipMemcpy(deck fine onsets)"});
}

void DeckFineGrid::debug_last(uint32_t out[4]) { last_finegrid.get(out); }

}  // namespace mx
