// mx_deck_waveform.hpp -- the deck's waveform picture (include/mixlab_gpu.h "WAVEFORM"; mx_k_deck_waveform.hip): the host-only rule functions,
// and what the launch takes.  The render itself is DeckColumns::render_waveform (mx_deck_columns.hpp): it needs the records' buffer, count and C and nothing else
// of the deck (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mx_common.hpp"

namespace mx {

void deck_waveform_check(const mx_deck_waveform& p);                                  // throws Error(MX_ERR_INVALID) naming the rule
int64_t deck_waveform_view(int64_t pos_q32, uint32_t frames_per_px, uint32_t playhead_x);
void deck_waveform_host(const mx_deck_column* cols, uint64_t n_cols, uint32_t column, uint64_t n_frames, const mx_deck_waveform& p, uint8_t* y, int32_t y_stride,
                        uint8_t* u, uint8_t* v, int32_t c_stride);

// ---- the kernel's argument block (passed by value: uniform indices into it are scalar loads) ----
// colours travel packed, y | u << 8 | v << 16
struct WaveGridDev { int64_t first, period, from, to; uint32_t colour, inset; };      // 40 bytes
struct WaveMarkDev { int32_t x0, x1; uint32_t colour, _pad; };                        // the marker's pixel columns [x0, x1) cut to [0, w): one division a marker, on the host
struct WaveRangeDev { int64_t from, to; uint32_t colour, _pad; };
struct WaveArgs {
    const uint32_t* cols; int64_t n_cols; int64_t n_frames; uint32_t log_c;          // the records (14 words each), N, the track's length, log2 C
    uint32_t w, h, fpp, style;
    int64_t first_frame;
    uint32_t gain[3];
    uint32_t bg, line, band[3];
    uint8_t* plane[3]; uint32_t stride_y, stride_c;                                   // the new frame: strides multiples of 64, stride_y = 64 * strips
    uint32_t n_grids, n_markers, n_ranges, _pad;
    WaveGridDev grid[MX_WAVE_MAX_GRIDS]; WaveMarkDev marker[MX_WAVE_MAX_MARKERS]; WaveRangeDev range[MX_WAVE_MAX_RANGES];
};
// p (checked) over an analysis of n_cols columns of 2^log_c frames: everything of `a` but the pointers and strides
void deck_waveform_args(const mx_deck_waveform& p, uint64_t n_cols, uint32_t log_c, uint64_t n_frames, WaveArgs& a);
// the strips of that launch by form (mx_deck_debug_last_waveform)
void deck_waveform_forms(const WaveArgs& a, uint32_t forms[4]);
void deck_debug_last_waveform(uint32_t out[4]);

}  // namespace mx
