// mx_deck_waveform.cpp -- the deck's waveform picture, host side (include/mixlab_gpu.h "WAVEFORM"): the setting rules, the view arithmetic, the
// picture in plain C++ (mx_deck_waveform_host: the CPU test path), what the launch takes, and the render of a deck's column analysis.
#include "mx_deck_waveform.hpp"

#include <algorithm>
#include <string>
#include <vector>

#include "mx_deck_columns.hpp"
#include "mx_dev.hpp"
#include "mx_kernels.hpp"
#include "mx_video.hpp"

namespace mx {

static const int64_t kOne = 1;

void deck_waveform_check(const mx_deck_waveform& p) {
    if ((p.w & 1u) || p.w < 2 || p.w > 8192) throw Error(MX_ERR_INVALID, "deck waveform: w is not even in 2 .. 8192");
    if ((p.h & 1u) || p.h < 4 || p.h > 4320) throw Error(MX_ERR_INVALID, "deck waveform: h is not even in 4 .. 4320");
    if (p.first_frame < -(kOne << 30) || p.first_frame > (kOne << 30)) throw Error(MX_ERR_INVALID, "deck waveform: first_frame beyond +-2^30");
    if (p.frames_per_px < 1 || p.frames_per_px > (1u << 20)) throw Error(MX_ERR_INVALID, "deck waveform: frames_per_px outside 1 .. 2^20");
    if ((uint64_t)p.w * p.frames_per_px > ((uint64_t)1 << 30)) throw Error(MX_ERR_INVALID, "deck waveform: w * frames_per_px is above 2^30");
    if (p.style > MX_WAVE_ENVELOPE) throw Error(MX_ERR_INVALID, "deck waveform: style is neither MX_WAVE_BANDS nor MX_WAVE_ENVELOPE");
    for (int b = 0; b < 3; ++b)
        if (p.gain_q16[b] > (1u << 20)) throw Error(MX_ERR_INVALID, "deck waveform: gain_q16[" + std::to_string(b) + "] is above 2^20");
    if (p.n_grids > MX_WAVE_MAX_GRIDS) throw Error(MX_ERR_INVALID, "deck waveform: n_grids is above 16");
    if (p.n_markers > MX_WAVE_MAX_MARKERS) throw Error(MX_ERR_INVALID, "deck waveform: n_markers is above 32");
    if (p.n_ranges > MX_WAVE_MAX_RANGES) throw Error(MX_ERR_INVALID, "deck waveform: n_ranges is above 8");
    if (p._pad) throw Error(MX_ERR_INVALID, "deck waveform: _pad must be 0");
    if (p.bg._pad || p.line._pad || p.band[0]._pad || p.band[1]._pad || p.band[2]._pad) throw Error(MX_ERR_INVALID, "deck waveform: a colour's _pad must be 0");
    for (uint32_t k = 0; k < p.n_grids; ++k) {
        const mx_wave_grid& g = p.grid[k];
        const std::string who = "deck waveform: grid " + std::to_string(k);
        if (g.grid.period_q32 < (kOne << 32) || g.grid.period_q32 > (kOne << 56)) throw Error(MX_ERR_INVALID, who + ": period_q32 outside 2^32 .. 2^56");
        if (g.grid.first_q32 < -(kOne << 61) || g.grid.first_q32 > (kOne << 61)) throw Error(MX_ERR_INVALID, who + ": first_q32 beyond +-2^61");
        if (g.from_q32 > g.to_q32) throw Error(MX_ERR_INVALID, who + ": from_q32 is above to_q32");
        if (g.inset > p.h / 2) throw Error(MX_ERR_INVALID, who + ": inset is above h / 2");
        if (g.colour._pad) throw Error(MX_ERR_INVALID, who + ": the colour's _pad must be 0");
    }
    for (uint32_t k = 0; k < p.n_markers; ++k) {
        const mx_wave_marker& m = p.marker[k];
        const std::string who = "deck waveform: marker " + std::to_string(k);
        if (m.width < 1 || m.width > 16) throw Error(MX_ERR_INVALID, who + ": width outside 1 .. 16");
        if (m.colour._pad) throw Error(MX_ERR_INVALID, who + ": the colour's _pad must be 0");
    }
    for (uint32_t k = 0; k < p.n_ranges; ++k) {
        const mx_wave_range& r = p.range[k];
        const std::string who = "deck waveform: range " + std::to_string(k);
        if (r.from_frame > r.to_frame) throw Error(MX_ERR_INVALID, who + ": from_frame is above to_frame");
        if (r.colour._pad || r._pad) throw Error(MX_ERR_INVALID, who + ": _pad must be 0");
    }
}

int64_t deck_waveform_view(int64_t pos_q32, uint32_t fpp, uint32_t playhead_x) {
    if (fpp < 1 || fpp > (1u << 20)) throw Error(MX_ERR_INVALID, "deck waveform view: frames_per_px outside 1 .. 2^20");
    if (playhead_x > 8191) throw Error(MX_ERR_INVALID, "deck waveform view: playhead_x is above 8191");
    const int64_t first = (pos_q32 >> 32) - (int64_t)playhead_x * fpp;   // (|pos >> 32| <= 2^31, the product below 2^33)
    if (first < -(kOne << 30) || first > (kOne << 30)) throw Error(MX_ERR_INVALID, "deck waveform view: the result lies beyond +-2^30");
    return first;
}

static uint32_t wave_log_c(uint32_t column) {
    if (column < 64 || column > 4096 || (column & (column - 1))) throw Error(MX_ERR_INVALID, "deck waveform: column is not a power of two in 64 .. 4096");
    uint32_t l = 0;
    while ((1u << l) < column) ++l;
    return l;
}
static uint32_t pack(const mx_wave_colour& c) { return (uint32_t)c.y | (uint32_t)c.u << 8 | (uint32_t)c.v << 16; }

void deck_waveform_args(const mx_deck_waveform& p, uint64_t n_cols, uint32_t log_c, uint64_t n_frames, WaveArgs& a) {
    a.n_cols = (int64_t)n_cols; a.n_frames = (int64_t)n_frames; a.log_c = log_c;
    a.w = p.w; a.h = p.h; a.fpp = p.frames_per_px; a.style = p.style; a.first_frame = p.first_frame;
    for (int b = 0; b < 3; ++b) { a.gain[b] = p.gain_q16[b]; a.band[b] = pack(p.band[b]); }
    a.bg = pack(p.bg); a.line = pack(p.line);
    a.n_grids = p.n_grids; a.n_markers = p.n_markers; a.n_ranges = p.n_ranges; a._pad = 0;
    for (uint32_t k = 0; k < MX_WAVE_MAX_GRIDS; ++k) {
        const mx_wave_grid& g = p.grid[k];
        a.grid[k] = k < p.n_grids ? WaveGridDev{g.grid.first_q32, g.grid.period_q32, g.from_q32, g.to_q32, pack(g.colour), g.inset} : WaveGridDev{0, 1, 0, 0, 0u, 0u};
    }
    const int64_t fpp = p.frames_per_px, reach = kOne << 31;   // a marker further than this from first_frame is not in the picture: w fpp <= 2^30, width / 2 * fpp <= 2^23
    for (uint32_t k = 0; k < MX_WAVE_MAX_MARKERS; ++k) {
        a.marker[k] = WaveMarkDev{0, 0, 0u, 0u};
        if (k >= p.n_markers) continue;
        const mx_wave_marker& m = p.marker[k];
        a.marker[k].colour = pack(m.colour);
        if (m.frame < p.first_frame - reach || m.frame > p.first_frame + reach) continue;   // (so that the difference below cannot leave int64)
        const int64_t n = m.frame - p.first_frame;
        const int64_t xm = n >= 0 ? n / fpp : -((-n + fpp - 1) / fpp);                      // floor
        const int64_t lo = xm - (int64_t)(m.width / 2u), hi = lo + m.width;
        a.marker[k].x0 = (int32_t)std::clamp<int64_t>(lo, 0, p.w);
        a.marker[k].x1 = (int32_t)std::clamp<int64_t>(hi, 0, p.w);
    }
    for (uint32_t k = 0; k < MX_WAVE_MAX_RANGES; ++k) {
        const mx_wave_range& r = p.range[k];
        a.range[k] = k < p.n_ranges ? WaveRangeDev{r.from_frame, r.to_frame, pack(r.colour), 0u} : WaveRangeDev{0, 0, 0u, 0u};
    }
}

// one pixel column's analysis columns: false when it lies outside the track
static bool wave_span(const WaveArgs& a, uint32_t x, int64_t& c0, int64_t& c1) {
    const int64_t F0 = a.first_frame + (int64_t)x * a.fpp, F1 = F0 + a.fpp;
    c0 = std::max<int64_t>(0, F0 >> a.log_c);
    c1 = std::min<int64_t>(a.n_cols - 1, (F1 - 1) >> a.log_c);
    return c0 <= c1;
}

void deck_waveform_forms(const WaveArgs& a, uint32_t forms[4]) {
    forms[0] = forms[1] = forms[2] = forms[3] = 0u;
    for (uint32_t x0 = 0; x0 < a.w; x0 += MX_WAVE_STRIP) {
        const uint32_t x1 = std::min(x0 + MX_WAVE_STRIP, a.w);
        bool any = false, several = false;
        int64_t lo = 0, hi = -1, c0, c1;
        for (uint32_t x = x0; x < x1; ++x)
            if (wave_span(a, x, c0, c1)) {
                if (!any) lo = c0;
                any = true; hi = c1;
                several = several || c1 > c0;
            }
        ++forms[!any ? 2 : several ? 1 : 0];
        if (any) forms[3] = std::max(forms[3], (uint32_t)(hi - lo + 1));
    }
}

// the lines of grid g in the frames [F0, F1) of a track of n_frames (GRID LINE)
static bool wave_grid_hit(const WaveGridDev& g, int64_t F0, int64_t F1, int64_t n_frames) {
    const int64_t A = std::max(std::clamp<int64_t>(F0, 0, n_frames) << 32, g.from), B = std::min(std::clamp<int64_t>(F1, 0, n_frames) << 32, g.to);
    if (A >= B) return false;
    const int64_t r = (A - g.first) % g.period;              // C's remainder: the sign of the dividend
    return A - r + (r > 0 ? g.period : 0) < B;               // the first line at or after A
}

void deck_waveform_host(const mx_deck_column* cols, uint64_t n_cols, uint32_t column, uint64_t n_frames, const mx_deck_waveform& p, uint8_t* y, int32_t y_stride,
                        uint8_t* u, uint8_t* v, int32_t c_stride) {
    if (!cols || !y || !u || !v) throw Error(MX_ERR_INVALID, "deck waveform: NULL argument");
    deck_waveform_check(p);
    const uint32_t log_c = wave_log_c(column);
    if (n_cols != deck_column_count(n_frames, column)) throw Error(MX_ERR_INVALID, "deck waveform: n_cols is not ceil(n_frames / column)");
    if (y_stride < (int32_t)p.w || c_stride < (int32_t)(p.w / 2)) throw Error(MX_ERR_INVALID, "deck waveform: a stride below the visible width");
    WaveArgs a{};
    deck_waveform_args(p, n_cols, log_c, n_frames, a);
    const uint32_t w = p.w, h = p.h, half = h / 2;
    std::vector<uint32_t> px((size_t)w * h);   // packed colours
    for (uint32_t x = 0; x < w; ++x) {
        const int64_t F0 = a.first_frame + (int64_t)x * a.fpp, F1 = F0 + a.fpp;
        uint32_t bg = a.bg;
        for (uint32_t k = 0; k < a.n_ranges; ++k)
            if (std::max(a.range[k].from, F0) < std::min(a.range[k].to, F1)) bg = a.range[k].colour;
        int64_t c0, c1;
        const bool in = wave_span(a, x, c0, c1);
        uint32_t up[3] = {0, 0, 0}, dn[3] = {0, 0, 0};
        if (in) {
            uint32_t P[3] = {0, 0, 0};
            int32_t smax = INT32_MIN, smin = INT32_MAX;
            for (int64_t c = c0; c <= c1; ++c) {
                for (int b = 0; b < 3; ++b) P[b] = std::max(P[b], cols[c].peak[b]);
                smax = std::max(smax, cols[c].smax); smin = std::min(smin, cols[c].smin);
            }
            auto height = [&](uint64_t v, uint32_t gain) { return (uint32_t)std::min<uint64_t>(half, (v * gain * half) >> 32); };
            if (a.style == MX_WAVE_BANDS) for (int b = 0; b < 3; ++b) up[b] = dn[b] = height(P[b], a.gain[b]);
            else { up[0] = height((uint64_t)std::max<int64_t>(smax, 0), a.gain[0]); dn[0] = height((uint64_t)std::max<int64_t>(-(int64_t)smin, 0), a.gain[0]); }
        }
        uint32_t lines = 0;
        for (uint32_t k = 0; k < a.n_grids; ++k) if (wave_grid_hit(a.grid[k], F0, F1, a.n_frames)) lines |= 1u << k;
        for (uint32_t r = 0; r < h; ++r) {
            const bool top = r < half;
            const uint32_t d = top ? half - 1 - r : r - half;
            const uint32_t* H = top ? up : dn;
            uint32_t c = bg;
            if (in) {
                if (d == 0) c = a.line;
                for (int b = 0; b < 3; ++b) if (d < H[b]) c = a.band[b];
            }
            for (uint32_t k = 0; k < a.n_grids; ++k)
                if ((lines >> k & 1u) && r >= a.grid[k].inset && r < h - a.grid[k].inset) c = a.grid[k].colour;
            for (uint32_t k = 0; k < a.n_markers; ++k)
                if ((int32_t)x >= a.marker[k].x0 && (int32_t)x < a.marker[k].x1) c = a.marker[k].colour;
            px[(size_t)r * w + x] = c;
        }
    }
    for (uint32_t r = 0; r < h; ++r)
        for (uint32_t x = 0; x < w; ++x) y[(size_t)r * y_stride + x] = (uint8_t)(px[(size_t)r * w + x] & 0xffu);
    for (uint32_t cy = 0; cy < half; ++cy)
        for (uint32_t cx = 0; cx < w / 2; ++cx) {
            uint32_t su = 2, sv = 2;
            for (uint32_t j = 0; j < 4; ++j) {
                const uint32_t c = px[(size_t)(2 * cy + (j >> 1)) * w + 2 * cx + (j & 1u)];
                su += c >> 8 & 0xffu; sv += c >> 16 & 0xffu;
            }
            u[(size_t)cy * c_stride + cx] = (uint8_t)(su >> 2); v[(size_t)cy * c_stride + cx] = (uint8_t)(sv >> 2);
        }
}

// ---- the render of a deck's column analysis ----
static DeckLastForms last_waveform;   // mx_deck_debug_last_waveform

void deck_debug_last_waveform(uint32_t out[4]) { last_waveform.get(out); }

DFrame* DeckColumns::render_waveform(const mx_deck_waveform& p, hipStream_t s) {
    if (!count_) throw Error(MX_ERR_INVALID, "deck: no analysis");
    deck_waveform_check(p);
    hip_check(hipSetDevice(deck_.device), "hipSetDevice");
    if (!rendered_) hip_check(hipEventCreateWithFlags(&rendered_, hipEventDisableTiming), "hipEventCreate");
    FrameRef o(DFrame::create_unfilled(p.w, p.h, MX_PIXFMT_YUV420P, false), false);   // (MX_ERR_NOMEM leaves everything as it was)
    WaveArgs a{};
    deck_waveform_args(p, count_, wave_log_c(column_), deck_.n_frames, a);
    a.cols = (const uint32_t*)buf_.p;
    for (int k = 0; k < 3; ++k) a.plane[k] = o->data[k];
    a.stride_y = o->stride[0]; a.stride_c = o->stride[1];
    uint32_t forms[4];
    deck_waveform_forms(a, forms);
    hip_check(hipStreamWaitEvent(s, analysed_, 0), "hipStreamWaitEvent(deck analysis)");   // the records are written on the load stream: no host wait
    launch_deck_waveform(a, s);
    hip_check(hipGetLastError(), "deck waveform launch");
    hip_check(hipEventRecord(rendered_, s), "hipEventRecord");   // what a later analyse orders itself behind
    last_waveform.set(forms);
    o->retain();
    return o.f;
}

}  // namespace mx
