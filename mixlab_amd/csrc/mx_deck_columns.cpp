// mx_deck_columns.cpp -- the deck's band columns and beat grid, host side (include/mixlab_gpu.h "ANALYSIS"): the setting rules, the band
// tables, the rules themselves in plain C++ (mx_deck_columns_host: the CPU test path), the beat grid, and the deck's first analysis.
#include "mx_deck_columns.hpp"

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "mx_dev.hpp"
#include "mx_kernels.hpp"

namespace mx {

void deck_analysis_check(const mx_deck_analysis& a) {
    if (a.column < 64 || a.column > 4096 || (a.column & (a.column - 1))) throw Error(MX_ERR_INVALID, "deck analysis: column is not a power of two in 64 .. 4096");
    if (!(a.taps & 1u) || a.taps > 127) throw Error(MX_ERR_INVALID, "deck analysis: taps is not odd in 1 .. 127");
    if (a.max_lag < 16 || a.max_lag > 1024) throw Error(MX_ERR_INVALID, "deck analysis: max_lag outside 16 .. 1024");
    if (a._pad) throw Error(MX_ERR_INVALID, "deck analysis: _pad must be 0");
    for (const int16_t* t : {a.lo, a.hi}) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < 127; ++k) {
            if (k >= a.taps && t[k]) throw Error(MX_ERR_INVALID, std::string("deck analysis: ") + (t == a.lo ? "lo" : "hi") + " has a non-zero entry at index taps or above");
            sum += (uint32_t)(t[k] < 0 ? -(int32_t)t[k] : (int32_t)t[k]);
        }
        if (sum > 32767) throw Error(MX_ERR_INVALID, std::string("deck analysis: the sum of |") + (t == a.lo ? "lo" : "hi") + "[k]| is above 32767");
    }
}

uint64_t deck_column_count(uint64_t n_frames, uint32_t column) {
    if (n_frames < 1 || n_frames > kDeckMaxFrames) throw Error(MX_ERR_INVALID, "deck analysis: n_frames outside 1 .. 2^30");
    if (column < 64 || column > 4096 || (column & (column - 1))) throw Error(MX_ERR_INVALID, "deck analysis: column is not a power of two in 64 .. 4096");
    return (n_frames + column - 1) / column;
}

void deck_analysis_bands(double rate, double f_lo, double f_hi, uint32_t taps, mx_deck_analysis& a) {
    if (!(std::isfinite(rate) && rate > 0.0)) throw Error(MX_ERR_INVALID, "deck analysis bands: rate is not finite and positive");
    if (!(f_lo > 0.0 && f_lo < f_hi && f_hi < rate / 2.0)) throw Error(MX_ERR_INVALID, "deck analysis bands: the cutoffs are not 0 < f_lo < f_hi < rate / 2");
    if (!(taps & 1u) || taps > 127) throw Error(MX_ERR_INVALID, "deck analysis bands: taps is not odd in 1 .. 127");
    const double pi = 3.14159265358979323846;
    const int K = (int)taps, D = (K - 1) / 2;
    mx_deck_analysis out = a;
    out.taps = taps;
    const double cut[2] = {f_lo, f_hi};
    int16_t* const tab[2] = {out.lo, out.hi};
    for (int b = 0; b < 2; ++b) {
        const double fc = 2.0 * cut[b] / rate;
        double g[127], sum = 0.0;
        for (int k = 0; k <= D; ++k) {   // the first half and the centre; the rest mirrors them
            const double x = fc * (double)(k - D), w = 0.5 - 0.5 * std::cos(2.0 * pi * (double)(k + 1) / (double)(K + 1));
            g[k] = g[K - 1 - k] = fc * (x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x)) * w;
        }
        for (int k = 0; k < K; ++k) sum += g[k];
        long total = 0, c[127];
        for (int k = 0; k < K; ++k) { c[k] = std::lround(16384.0 * g[k] / sum); total += c[k]; }
        c[D] += 16384 - total;
        long mag = 0;
        for (int k = 0; k < K; ++k) mag += c[k] < 0 ? -c[k] : c[k];
        if (mag > 32767) throw Error(MX_ERR_INVALID, "deck analysis bands: the sum of |c| is above 32767 at these cutoffs");
        for (int k = 0; k < 127; ++k) tab[b][k] = k < K ? (int16_t)c[k] : (int16_t)0;
    }
    a = out;
}

void deck_columns_host(const int16_t* x, uint64_t n_frames, const mx_deck_analysis& a, uint64_t first, uint64_t n, mx_deck_column* cols, uint64_t* R) {
    if (!x) throw Error(MX_ERR_INVALID, "deck columns: interleaved is NULL");
    deck_analysis_check(a);
    const uint64_t N = deck_column_count(n_frames, a.column);
    if (first > N || n > N - first) throw Error(MX_ERR_INVALID, "deck columns: a window beyond the track's columns");
    if (n && !cols) throw Error(MX_ERR_INVALID, "deck columns: cols is NULL");
    if (R && (first != 0 || n != N)) throw Error(MX_ERR_INVALID, "deck columns: the autocorrelation needs all the columns, first = 0 and n = N");
    const uint32_t C = a.column, K = a.taps, D = (K - 1) / 2;
    auto s = [&](int64_t f) -> int32_t { return f < 0 || f >= (int64_t)n_frames ? 0 : (int32_t)x[2 * f] + (int32_t)x[2 * f + 1]; };
    std::vector<int32_t> w((size_t)C + K - 1);
    uint32_t before = 0;   // A[first - 1]
    if (first) {
        uint64_t e = 0;
        for (uint64_t f = (first - 1) * C; f < first * C; ++f) { const int64_t v = s((int64_t)f); e += (uint64_t)(v * v); }
        before = tempo_root(e);
    }
    for (uint64_t c = first; c < first + n; ++c) {
        const uint64_t f0 = c * C;
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(C, n_frames - f0);
        for (uint32_t i = 0; i < cnt + K - 1; ++i) w[i] = s((int64_t)f0 - (int64_t)D + (int64_t)i);
        mx_deck_column r{INT32_MAX, INT32_MIN, {0u, 0u, 0u}, 0u, {0u, 0u, 0u}, 0u};
        for (uint32_t i = 0; i < cnt; ++i) {
            int32_t a1 = 0, a2 = 0;   // exact: |a| <= 65536 * 32767
            for (uint32_t k = 0; k < K; ++k) { a1 += (int32_t)a.lo[k] * w[i + k]; a2 += (int32_t)a.hi[k] * w[i + k]; }
            const int32_t sv = w[i + D], low = a1 >> 14, b = a2 >> 14, band[3] = {low, b - low, sv - b};
            r.smin = std::min(r.smin, sv); r.smax = std::max(r.smax, sv);
            for (int j = 0; j < 3; ++j) {
                const uint64_t m = (uint64_t)(band[j] < 0 ? -(int64_t)band[j] : (int64_t)band[j]);
                r.peak[j] = std::max(r.peak[j], (uint32_t)m);
                r.energy[j] += m * m;
            }
            r.e += (uint64_t)((int64_t)sv * sv);
        }
        const uint32_t A = tempo_root(r.e);
        r.onset = (A > before ? A - before : 0u) >> 6;
        before = A;
        cols[c - first] = r;
    }
    if (R)
        for (uint64_t l = 0; l < a.max_lag; ++l) {
            uint64_t acc = 0;
            for (uint64_t c = 0; c + l < N; ++c) acc += (uint64_t)cols[c].onset * cols[c + l].onset;
            R[l] = acc;
        }
}

// (the library is built with -ffp-contract=off: the multiply and the add of i_k are two roundings, as the header says)
void deck_beatgrid(const mx_deck_column* cols, uint64_t n_cols, const uint64_t* R, uint32_t max_lag, uint32_t column, double rate, double bpm_lo, double bpm_hi, mx_deck_grid& out) {
    if (!R || (n_cols && !cols)) throw Error(MX_ERR_INVALID, "deck beat grid: NULL argument");
    if (column < 64 || column > 4096 || (column & (column - 1)) || max_lag < 16 || max_lag > 1024)
        throw Error(MX_ERR_INVALID, "deck beat grid: column is not a power of two in 64 .. 4096, or max_lag is outside 16 .. 1024");
    if (!(std::isfinite(rate) && rate > 0.0 && std::isfinite(bpm_lo) && bpm_lo > 0.0 && std::isfinite(bpm_hi) && bpm_hi >= bpm_lo))
        throw Error(MX_ERR_INVALID, "deck beat grid: rate, bpm_lo and bpm_hi must be finite and positive, bpm_lo <= bpm_hi");
    out = mx_deck_grid{0.0, 0.0, 0.0, 0u, 0u, 0u};
    uint32_t best = 0; double d = 0.0;
    if (!tempo_lag([&](uint32_t l) { return (double)R[l]; }, max_lag, column, rate, bpm_lo, bpm_hi, best, d)) return;
    const double P = (double)best + d;
    if (!(P >= 1.0 && P <= (double)max_lag)) return;
    const uint32_t phases = (uint32_t)std::ceil(P);
    uint64_t best_sum = 0; uint32_t phi_best = 0;
    for (uint32_t phi = 0; phi < phases; ++phi) {
        uint64_t sum = 0;
        for (uint64_t k = 0;; ++k) {
            const double step = (double)k * P;
            const double at = (double)phi + step;
            const int64_t i = (int64_t)std::floor(at);
            if (i >= (int64_t)n_cols) break;
            sum += cols[i].onset;
        }
        if (phi == 0 || sum > best_sum) { best_sum = sum; phi_best = phi; }
    }
    out.bpm = 60.0 * rate / ((double)column * P); out.period_columns = P; out.confidence = (double)R[best] / (double)R[0];
    out.first_beat_frame = (uint64_t)phi_best * column; out.lag = best; out.phase_column = phi_best;
}

// ---- the deck's first analysis ----
static DeckLastForms last_columns;   // mx_deck_debug_last_analysis

DeckColumns::DeckColumns(const DeckTrack& deck) : DeckTrackAnalysis(deck, last_columns) {}

DeckColumns::~DeckColumns() {   // (the deck has waited for the device by now)
    if (analysed_) (void)hipEventDestroy(analysed_);
    if (rendered_) (void)hipEventDestroy(rendered_);
}

void DeckColumns::analyse(const mx_deck_analysis* a) {
    if (a) deck_analysis_check(*a);
    const uint64_t N = a ? deck_column_count(deck_.n_frames, a->column) : 0;
    const size_t need = a ? (size_t)N * sizeof(mx_deck_column) + (size_t)a->max_lag * sizeof(uint64_t) + (size_t)N * sizeof(uint32_t) : 0;
    hip_check(hipSetDevice(deck_.device), "hipSetDevice");
    if (a && !analysed_) hip_check(hipEventCreateWithFlags(&analysed_, hipEventDisableTiming), "hipEventCreate");
    // a render in flight on another stream still reads the records: the load stream waits for it on the device, so the rewrite in place is ordered behind it, and so
    // is prepare()'s host wait for the load stream where the buffer goes
    if (rendered_) hip_check(hipStreamWaitEvent(deck_.load_stream, rendered_, 0), "hipStreamWaitEvent(deck waveform)");
    if (!prepare(need, !a)) return;
    DeckAnalyseTaps taps{};
    for (uint32_t k = 0; k < a->taps; ++k) { taps.lo[k] = a->lo[k]; taps.hi[k] = a->hi[k]; }
    uint64_t* const R = (uint64_t*)((char*)buf_.p + (size_t)N * sizeof(mx_deck_column));
    uint32_t forms[4];
    launch_deck_analyse(deck_.track, deck_.n_frames, a->column, a->taps, a->max_lag, taps, buf_.p, (uint32_t*)(R + a->max_lag), R, N, forms, deck_.load_stream);
    lag_ = a->max_lag;
    column_ = a->column;
    launched("deck analyse launch", N, forms);
    hip_check(hipEventRecord(analysed_, deck_.load_stream), "hipEventRecord");   // what a render waits for, on the device
}

void DeckColumns::read_columns(uint64_t first, uint64_t n, mx_deck_column* dst) {
    read_window(first, n, dst, sizeof(mx_deck_column), 0, count_, {"deck: no analysis", "deck: a window beyond the analysis' columns", "deck: dst is NULL", "hipMemcpy(deck columns)"});
}

// (all of R or nothing: no window, and no early return)
void DeckColumns::read_autocorr(uint64_t* R, uint32_t cap) {
    if (!count_) throw Error(MX_ERR_INVALID, "deck: no analysis");
    if (cap < lag_) throw Error(MX_ERR_INVALID, "deck: cap is below the analysis' max_lag");
    if (!R) throw Error(MX_ERR_INVALID, "deck: R is NULL");
    wait_and_copy(R, (size_t)count_ * sizeof(mx_deck_column), (size_t)lag_ * sizeof(uint64_t), "hipMemcpy(deck autocorrelation)");
}

void DeckColumns::debug_last(uint32_t out[4]) { last_columns.get(out); }

}  // namespace mx
