// mx_k_deck_waveform.hip -- the deck's waveform picture (include/mixlab_gpu.h "the deck", WAVEFORM): one launch from the column records to a frame.
//
// k_deck_waveform       a workgroup of 256 owns a STRIP of 64 pixel columns over the full height of the three planes, so the strip's records are reduced exactly once and
//                       nothing passes through device memory between the reduction and the fill (the alternative, a reduction kernel ahead of workgroups that each
//                       take a band of rows, needs a buffer per render whose lifetime somebody has to manage; DESIGN.md has the measurement that goes with the choice).
//                       1. REDUCE: the strip's records are one contiguous run of 14-word records, of which the first five words -- smin, smax, the peaks -- are
//                          wanted.  Consecutive lanes take consecutive wanted words (runs of five dwords, nine skipped: every cache line of the run is touched
//                          once, and no load is issued for the 9 words of 14 nobody reads), eight words a lane in flight before the first is used, and fold
//                          them into the pixel columns the record meets by integer LDS atomics (min / max: no order matters).  A record's pixel columns come
//                          from two 32-bit divisions: relative to the strip's first frame everything is below 2^27.
//                       2. OVERLAYS, once per pixel column and never per pixel: a (grid, pixel column) pair per lane evaluates GRID LINE -- one int64 remainder --
//                          and sets the grid's bit in the column's line mask; the grid is uniform over a wave, so its entry comes by scalar loads from the kernel
//                          arguments.  Lanes 0 .. 63 then take a pixel column each: the ranges (compares only), the heights (uint64 products), the topmost marker
//                          (the host has turned every marker into a span of pixel columns: one division a marker, not one a column), and pack the column's eight
//                          words into LDS.
//                       3. FILL: a lane takes two rows x 32 pixel columns: it evaluates LAYERS per pixel from the packed columns (LDS reads that a wave's lanes share
//                          are broadcasts), and stores four aligned 16-byte pieces of luma, one of U and one of V -- chroma from the same pixels it has just computed.
//                          Pixel columns at or beyond w (the last strip) are stride padding: Y 0, chroma 0x80, written by the same stores.  Where the chroma stride
//                          reaches beyond the last strip's 32 bytes (ceil(w / 64) odd), the last workgroup fills that too.
// Integers throughout.  Every store lies inside its plane by construction: rows below h (h / 2), bytes below 64 * strips = stride_y (32 * strips <= stride_c); the
// launcher refuses strides that do not fit.  Every load of a record lies in [0, N).
#include "mx_deck_waveform.hpp"
#include "mx_dev.hpp"
#include "mx_kernels.hpp"

namespace mx {

enum { WV_LANES = 256, WV_STRIP = 64, WV_REC_WORDS = 14, WV_USED_WORDS = 5, WV_BATCH = 8 };   // smin, smax and the three peaks lead a record
static_assert(sizeof(mx_deck_column) == 4 * WV_REC_WORDS, "mx_deck_column is 14 words");
static_assert(WV_STRIP == MX_WAVE_STRIP, "the strip the header names");

// one pixel of a packed column: ca = {background, in-track | (marker + 1) << 8, line mask, up0 | up1 << 16}, cb = {up2 | dn0 << 16, dn1 | dn2 << 16, -, -}
__device__ __forceinline__ uint32_t wv_pixel(const uint4 ca, const uint4 cb, uint32_t y, uint32_t half, uint32_t h, uint32_t line, uint32_t band0, uint32_t band1,
                                             uint32_t band2, const uint32_t* s_gcol, const uint32_t* s_ginset, const uint32_t* s_mcol) {
    const bool top = y < half;
    const uint32_t d = top ? half - 1u - y : y - half;
    uint32_t c = ca.x;
    if (ca.y & 1u) {
        const uint32_t h0 = top ? (ca.w & 0xffffu) : (cb.x >> 16), h1 = top ? (ca.w >> 16) : (cb.y & 0xffffu), h2 = top ? (cb.x & 0xffffu) : (cb.y >> 16);
        if (d == 0u) c = line;
        if (d < h0) c = band0;
        if (d < h1) c = band1;
        if (d < h2) c = band2;
    }
    uint32_t lines = ca.z;
    while (lines) {   // the topmost grid whose rows hold y (rare: only in the pixel columns that hold a line)
        const uint32_t k = 31u - (uint32_t)__clz((int)lines);
        if (y >= s_ginset[k] && y < h - s_ginset[k]) { c = s_gcol[k]; break; }
        lines &= ~(1u << k);
    }
    const uint32_t mk = ca.y >> 8;
    if (mk) c = s_mcol[mk - 1u];
    return c;
}

__global__ __launch_bounds__(WV_LANES) void k_deck_waveform(const WaveArgs a) {
    __shared__ int32_t s_min[WV_STRIP], s_max[WV_STRIP];
    __shared__ uint32_t s_pk[3][WV_STRIP], s_lines[WV_STRIP];
    __shared__ uint4 s_col[WV_STRIP][2];
    __shared__ uint32_t s_gcol[MX_WAVE_MAX_GRIDS], s_ginset[MX_WAVE_MAX_GRIDS], s_mcol[MX_WAVE_MAX_MARKERS];
    const uint32_t tid = threadIdx.x;
    const uint32_t x0 = blockIdx.x * WV_STRIP, nx = min((uint32_t)WV_STRIP, a.w - x0);
    const int64_t Fs = a.first_frame + (int64_t)x0 * a.fpp, Fe = Fs + (int64_t)nx * a.fpp;
    if (tid < WV_STRIP) { s_min[tid] = INT32_MAX; s_max[tid] = INT32_MIN; s_pk[0][tid] = s_pk[1][tid] = s_pk[2][tid] = 0u; s_lines[tid] = 0u; }
    if (tid < MX_WAVE_MAX_GRIDS) { s_gcol[tid] = a.grid[tid].colour; s_ginset[tid] = a.grid[tid].inset; }
    if (tid < MX_WAVE_MAX_MARKERS) s_mcol[tid] = a.marker[tid].colour;
    __syncthreads();

    // 1. the strip's records, as dwords
    const int64_t ca = max((int64_t)0, Fs >> a.log_c), cb = min(a.n_cols - 1, (Fe - 1) >> a.log_c);
    if (ca <= cb) {
        const uint32_t n_w = (uint32_t)(cb - ca + 1) * WV_USED_WORDS;   // (at most 2^20 + 2 records)
        const uint32_t* __restrict__ src = a.cols + ca * WV_REC_WORDS;
        const int32_t rel0 = (int32_t)((ca << a.log_c) - Fs);           // in (-C, 64 fpp)
        const uint32_t C = 1u << a.log_c;
        for (uint32_t base = 0; base < n_w; base += WV_LANES * WV_BATCH) {
            uint32_t v[WV_BATCH];
#pragma unroll
            for (int u = 0; u < WV_BATCH; ++u) {   // the batch's loads leave together: one memory latency a batch, not one a word
                const uint32_t j = base + (uint32_t)u * WV_LANES + tid, rec = j / WV_USED_WORDS;
                v[u] = j < n_w ? src[rec * WV_REC_WORDS + (j - rec * WV_USED_WORDS)] : 0u;
            }
#pragma unroll
            for (int u = 0; u < WV_BATCH; ++u) {
                const uint32_t j = base + (uint32_t)u * WV_LANES + tid, rec = j / WV_USED_WORDS, f = j - rec * WV_USED_WORDS;
                if (j >= n_w) continue;
                const int32_t rel = rel0 + (int32_t)(rec << a.log_c);       // the record's first frame, from the strip's: pixel column x meets it when
                const uint32_t xa = rel > 0 ? (uint32_t)rel / a.fpp : 0u;   //   (x + 1) fpp > rel  and  x fpp < rel + C
                const uint32_t xb = min((uint32_t)(rel + (int32_t)C - 1) / a.fpp, nx - 1u);
                for (uint32_t x = xa; x <= xb; ++x) {
                    if (f == 0u) atomicMin(&s_min[x], (int32_t)v[u]);
                    else if (f == 1u) atomicMax(&s_max[x], (int32_t)v[u]);
                    else atomicMax(&s_pk[f - 2u][x], v[u]);
                }
            }
        }
    }

    // 2. the grids' lines: a (grid, pixel column) pair per lane, the grid uniform over a wave
    for (uint32_t t = tid; t < WV_STRIP * a.n_grids; t += WV_LANES) {
        const uint32_t x = t & (WV_STRIP - 1u), k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(t >> 6));
        if (x >= nx) continue;
        const int64_t F0 = Fs + (int64_t)x * a.fpp, F1 = F0 + a.fpp;
        const int64_t first = a.grid[k].first, period = a.grid[k].period;
        const int64_t A = max(min(max(F0, (int64_t)0), a.n_frames) << 32, a.grid[k].from), B = min(min(max(F1, (int64_t)0), a.n_frames) << 32, a.grid[k].to);
        if (A >= B) continue;
        const int64_t r = (A - first) % period;   // (the sign of the dividend)
        if (A - r + (r > 0 ? period : 0) < B) atomicOr(&s_lines[x], 1u << k);
    }
    __syncthreads();

    const uint32_t half = a.h >> 1;
    if (tid < WV_STRIP) {
        const uint32_t x = tid;
        uint4 qa = make_uint4(0u, 0u, 0u, 0u), qb = make_uint4(0u, 0u, 0u, 0u);
        if (x < nx) {
            const int64_t F0 = Fs + (int64_t)x * a.fpp, F1 = F0 + a.fpp;
            uint32_t bg = a.bg;
            for (uint32_t k = 0; k < a.n_ranges; ++k)
                if (max(a.range[k].from, F0) < min(a.range[k].to, F1)) bg = a.range[k].colour;
            const bool in = F1 > 0 && F0 < (a.n_cols << a.log_c);
            uint32_t up[3] = {0u, 0u, 0u}, dn[3] = {0u, 0u, 0u};
            if (in) {
                auto height = [&](unsigned long long v, uint32_t gain) { return (uint32_t)min((unsigned long long)half, (v * gain * half) >> 32); };
                if (a.style == MX_WAVE_BANDS) {
#pragma unroll
                    for (int b = 0; b < 3; ++b) up[b] = dn[b] = height(s_pk[b][x], a.gain[b]);
                } else {
                    up[0] = height((unsigned long long)max(s_max[x], 0), a.gain[0]);
                    dn[0] = height((unsigned long long)max(-(int64_t)s_min[x], (int64_t)0), a.gain[0]);
                }
            }
            uint32_t mk = 0u;
            const int32_t xg = (int32_t)(x0 + x);
            for (uint32_t k = 0; k < a.n_markers; ++k)
                if (xg >= a.marker[k].x0 && xg < a.marker[k].x1) mk = k + 1u;
            qa = make_uint4(bg, (in ? 1u : 0u) | mk << 8, s_lines[x], up[0] | up[1] << 16);
            qb = make_uint4(up[2] | dn[0] << 16, dn[1] | dn[2] << 16, 0u, 0u);
        }
        s_col[x][0] = qa; s_col[x][1] = qb;
    }
    __syncthreads();

    // 3. two rows x 32 pixel columns a lane
    const uint32_t line = a.line, band0 = a.band[0], band1 = a.band[1], band2 = a.band[2];
    for (uint32_t task = tid; task < 2u * half; task += WV_LANES) {
        const uint32_t hs = task & 1u, rp = task >> 1, y0 = 2u * rp;
        uint32_t Y0[8], Y1[8], U[4], V[4];
#pragma unroll
        for (int j = 0; j < 8; ++j) { Y0[j] = 0u; Y1[j] = 0u; }
#pragma unroll
        for (int j = 0; j < 4; ++j) { U[j] = 0u; V[j] = 0u; }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const uint32_t xl = hs * 32u + 2u * (uint32_t)j;
            uint32_t yy0 = 0u, yy1 = 0u, cu = 0x80u, cv = 0x80u;   // the stride padding
            if (xl < nx) {
                const uint4 ca0 = s_col[xl][0], cb0 = s_col[xl][1], ca1 = s_col[xl + 1u][0], cb1 = s_col[xl + 1u][1];
                const uint32_t p00 = wv_pixel(ca0, cb0, y0, half, a.h, line, band0, band1, band2, s_gcol, s_ginset, s_mcol);
                const uint32_t p01 = wv_pixel(ca1, cb1, y0, half, a.h, line, band0, band1, band2, s_gcol, s_ginset, s_mcol);
                const uint32_t p10 = wv_pixel(ca0, cb0, y0 + 1u, half, a.h, line, band0, band1, band2, s_gcol, s_ginset, s_mcol);
                const uint32_t p11 = wv_pixel(ca1, cb1, y0 + 1u, half, a.h, line, band0, band1, band2, s_gcol, s_ginset, s_mcol);
                yy0 = (p00 & 0xffu) | (p01 & 0xffu) << 8; yy1 = (p10 & 0xffu) | (p11 & 0xffu) << 8;
                cu = ((p00 >> 8 & 0xffu) + (p01 >> 8 & 0xffu) + (p10 >> 8 & 0xffu) + (p11 >> 8 & 0xffu) + 2u) >> 2;
                cv = ((p00 >> 16 & 0xffu) + (p01 >> 16 & 0xffu) + (p10 >> 16 & 0xffu) + (p11 >> 16 & 0xffu) + 2u) >> 2;
            }
            Y0[j >> 1] |= yy0 << (16 * (j & 1)); Y1[j >> 1] |= yy1 << (16 * (j & 1));
            U[j >> 2] |= cu << (8 * (j & 3)); V[j >> 2] |= cv << (8 * (j & 3));
        }
        uint8_t* const l0 = a.plane[0] + (size_t)y0 * a.stride_y + x0 + hs * 32u;
        uint8_t* const l1 = l0 + a.stride_y;
        const size_t co = (size_t)rp * a.stride_c + (x0 >> 1) + hs * 16u;
        *reinterpret_cast<uint4*>(l0) = make_uint4(Y0[0], Y0[1], Y0[2], Y0[3]); *reinterpret_cast<uint4*>(l0 + 16) = make_uint4(Y0[4], Y0[5], Y0[6], Y0[7]);
        *reinterpret_cast<uint4*>(l1) = make_uint4(Y1[0], Y1[1], Y1[2], Y1[3]); *reinterpret_cast<uint4*>(l1 + 16) = make_uint4(Y1[4], Y1[5], Y1[6], Y1[7]);
        *reinterpret_cast<uint4*>(a.plane[1] + co) = make_uint4(U[0], U[1], U[2], U[3]);
        *reinterpret_cast<uint4*>(a.plane[2] + co) = make_uint4(V[0], V[1], V[2], V[3]);
    }

    // the chroma stride beyond the last strip
    const uint32_t done_c = gridDim.x * (WV_STRIP / 2u);
    if (blockIdx.x == gridDim.x - 1u && a.stride_c > done_c) {
        const uint32_t pieces = (a.stride_c - done_c) >> 4;   // 16-byte pieces a row (the launcher has checked the stride)
        const uint4 blank = make_uint4(0x80808080u, 0x80808080u, 0x80808080u, 0x80808080u);
        for (uint32_t t = tid; t < half * pieces; t += WV_LANES) {
            const uint32_t row = t / pieces, q = t - row * pieces;
            const size_t o = (size_t)row * a.stride_c + done_c + q * 16u;
            *reinterpret_cast<uint4*>(a.plane[1] + o) = blank; *reinterpret_cast<uint4*>(a.plane[2] + o) = blank;
        }
    }
}

void launch_deck_waveform(const WaveArgs& a, hipStream_t s) {
    const uint32_t strips = (a.w + WV_STRIP - 1u) / WV_STRIP;
    if (a.stride_y != strips * WV_STRIP || a.stride_c < strips * (WV_STRIP / 2u) || (a.stride_c & 15u) || a.log_c < 6 || a.log_c > 12 || a.n_cols < 1 || (a.h & 1u) || (a.w & 1u))
        throw Error(MX_ERR_INTERNAL, "deck waveform: a frame or an analysis the kernel is not laid out for");
    hipLaunchKernelGGL(k_deck_waveform, dim3(strips), dim3(WV_LANES), 0, s, a);
}

}  // namespace mx
