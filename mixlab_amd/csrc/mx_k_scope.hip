// mx_k_scope.hip -- video scope taps (mixlab_gpu.h mx_graph_set_video_scopes): the luma / U / V histograms, the waveform
// monitor's column histograms and the vectorscope of ONE yuv420p frame in ONE launch.
//
// Every count is a u32 sum of ones, so any order of accumulation gives the same record.  The shape:
//   * a workgroup counts into LDS with non-returning LDS atomics (ds_add_u32) and adds its non-zero counters to the record once, at its end,
//     with vector global atomics (global_atomic_add_u32, no return) -- thread v of a wave adds counter v of a row, so a wave-instruction covers
//     256 contiguous bytes.  The record's counters are zero when the launch starts (the host clears them on the same stream); a two-stage
//     reduce would need a second launch per frame or a last-arriver protocol for no gain: the flush is a few thousand adds per workgroup.
//   * luma workgroups own a run of up to 32 waveform column buckets over a band of rows: LDS rows = buckets, 257 counters apart (a flat
//     picture sends neighbouring lanes to the SAME value of neighbouring buckets: with a stride of 256 that is one bank).  hist[0] is not
//     counted per sample: it is the column sum of the workgroup's bucket rows, taken at the flush.  Without a waveform the 32 rows are
//     replicas chosen by the lane's chunk index, so a flat picture spreads over 32 counters instead of one.
//   * chroma workgroups take a band of rows of both chroma planes: hist[1] / hist[2] in 8 replicas each and the 128 x 128 vectorscope as
//     u16 halves of 8192 words (32 KiB; a workgroup sees fewer than 65 536 sample pairs, so a half never carries into its neighbour).
//   * pre-aggregation: a lane run-length codes its 16 bytes (one add per run of equal counters, not per sample), and when every active lane
//     of the wave is about to add the same count to the same counter -- the blank frame, any flat area -- one lane adds the total.
// Loads are 16 bytes per lane from 16-byte aligned addresses; bytes outside the workgroup's columns (and the stride padding) are skipped.
#include <algorithm>

#include "mx_common.hpp"
#include "mx_dev.hpp"

namespace mx {

static constexpr uint32_t SCOPE_THREADS = 256;
static constexpr uint32_t SCOPE_ROWS = 32;               // LDS rows of a luma workgroup: column buckets, or replicas
static constexpr uint32_t SCOPE_PITCH = 257;             // counters per LDS row (256 + 1: rows start on consecutive banks)
static constexpr uint32_t SCOPE_CREP = 8;                // replicas of the chroma histograms
static constexpr uint32_t SCOPE_VEC_WORDS = 128 * 128 / 2;
static constexpr uint32_t SCOPE_LDS_WORDS = SCOPE_VEC_WORDS + 2 * SCOPE_CREP * SCOPE_PITCH;   // 12 304 words (the chroma role; luma needs 8 224)
static constexpr uint32_t SCOPE_NONE = 0xffffffffu;
static_assert(SCOPE_ROWS * SCOPE_PITCH <= SCOPE_LDS_WORDS, "the luma rows fit the chroma role's LDS");

struct ScopeGeom {   // launcher-filled
    uint32_t tiles_x, luma_rows, luma_bands;     // luma workgroups: tiles_x column tiles x luma_bands bands of luma_rows rows
    uint32_t chroma_rows, chroma_bands;          // chroma workgroups: bands of chroma_rows rows over the whole width
    uint32_t q, rs;                              // wave_cols / width and wave_cols % width: a step of one column moves x * C by (q, rs)
};

__device__ __forceinline__ void lds_add(uint32_t* s, uint32_t idx, uint32_t n) {
    const uint32_t i0 = __builtin_amdgcn_readfirstlane(idx), n0 = __builtin_amdgcn_readfirstlane(n);
    const uint64_t act = __ballot(1), same = __ballot(idx == i0 && n == n0);
    if (same == act) {   // every active lane: same counter, same count
        if (__lane_id() == (uint32_t)__ffsll((unsigned long long)act) - 1u)
            (void)__hip_atomic_fetch_add(&s[i0], n0 * (uint32_t)__popcll(act), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
        (void)__hip_atomic_fetch_add(&s[idx], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
}
__device__ __forceinline__ void global_add(uint32_t* p, uint32_t n) {
    if (n) (void)__hip_atomic_fetch_add(p, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t byte_of(const uint4& w, uint32_t i) {
    const uint32_t d = i < 4 ? w.x : (i < 8 ? w.y : (i < 12 ? w.z : w.w));
    return (d >> (8u * (i & 3u))) & 255u;
}

// the luma role: columns [xa, xb) = buckets [c0, c0 + nb) (or everything, rows = replicas) of rows [y0, y1)
__device__ __forceinline__ void scope_luma(const ScopeArgs& a, const ScopeGeom& g, uint32_t* s, uint32_t tile, uint32_t band) {
    const uint32_t tid = threadIdx.x, W = a.width, C = a.wave_cols;
    uint32_t c0 = 0, nb = SCOPE_ROWS, xa = 0, xb = W;
    if (C) {
        c0 = tile * SCOPE_ROWS; nb = min(SCOPE_ROWS, C - c0);
        xa = (uint32_t)(((uint64_t)c0 * W + C - 1) / C);              // the first column of bucket c0: ceil(c0 W / C)
        xb = (uint32_t)(((uint64_t)(c0 + nb) * W + C - 1) / C);       // ... of bucket c0 + nb (W for the last tile)
    }
    for (uint32_t i = tid; i < SCOPE_ROWS * SCOPE_PITCH; i += SCOPE_THREADS) s[i] = 0u;
    __syncthreads();
    const uint32_t y0 = band * g.luma_rows, y1 = min(a.height, y0 + g.luma_rows);
    if (xb > xa) {
        const uint32_t xs = xa & ~15u, cpr = (xb - xs + 15u) >> 4;       // 16-byte chunks per row of the tile
        uint32_t P = 1; while (P < cpr && P < SCOPE_THREADS) P <<= 1;     // lanes per row: the workgroup takes SCOPE_THREADS / P rows at a time
        const uint32_t tx = tid & (P - 1u), ty = tid / P, rows_at_once = SCOPE_THREADS / P;
        for (uint32_t cx = tx; cx < cpr; cx += P) {
            const uint32_t x0 = xs + 16u * cx;
            uint32_t row0, rem0;
            if (C) { const uint32_t t = x0 * C; const uint32_t c = t / W; rem0 = t - c * W; row0 = c - c0; }   // x C < 2^32: width <= 16 384, C <= 256
            else { row0 = cx & (SCOPE_ROWS - 1u); rem0 = 0u; }
            for (uint32_t y = y0 + ty; y < y1; y += rows_at_once) {
                const uint4 w = *reinterpret_cast<const uint4*>(a.y + (size_t)y * a.y_stride + x0);
                uint32_t row = row0, rem = rem0, cur = SCOPE_NONE, cnt = 0u;
#pragma unroll
                for (uint32_t i = 0; i < 16; ++i) {
                    const uint32_t x = x0 + i;
                    const uint32_t key = (x >= xa && x < xb) ? row * SCOPE_PITCH + byte_of(w, i) : SCOPE_NONE;
                    if (key != cur) { if (cur != SCOPE_NONE) lds_add(s, cur, cnt); cur = key; cnt = 0u; }
                    ++cnt;
                    row += g.q; rem += g.rs;
                    if (rem >= W) { rem -= W; ++row; }
                }
                if (cur != SCOPE_NONE) lds_add(s, cur, cnt);
            }
        }
    }
    __syncthreads();
    // flush: thread v owns value v -- a wave adds 64 consecutive counters of one record row
    uint32_t* hist0 = a.rec + 8;
    uint32_t* wave = a.rec + 8 + 768;
    uint32_t sum = 0u;
    for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t n = s[b * SCOPE_PITCH + tid];
        sum += n;
        if (C) global_add(&wave[(size_t)(c0 + b) * 256u + tid], n);
    }
    global_add(&hist0[tid], sum);
}

// the chroma role: rows [y0, y1) of both chroma planes, whole width
__device__ __forceinline__ void scope_chroma(const ScopeArgs& a, const ScopeGeom& g, uint32_t* s, uint32_t band) {
    const uint32_t tid = threadIdx.x, pw = a.width >> 1, ph = a.height >> 1;
    const bool vec_on = a.vectorscope != 0u;
    uint32_t* vecw = s;
    uint32_t* hu = s + SCOPE_VEC_WORDS;
    uint32_t* hv = hu + SCOPE_CREP * SCOPE_PITCH;
    for (uint32_t i = tid + (vec_on ? 0u : SCOPE_VEC_WORDS); i < SCOPE_LDS_WORDS; i += SCOPE_THREADS) s[i] = 0u;
    __syncthreads();
    const uint32_t y0 = band * g.chroma_rows, y1 = min(ph, y0 + g.chroma_rows);
    const uint32_t cpr = (pw + 15u) >> 4;
    uint32_t P = 1; while (P < cpr && P < SCOPE_THREADS) P <<= 1;
    const uint32_t tx = tid & (P - 1u), ty = tid / P, rows_at_once = SCOPE_THREADS / P;
    for (uint32_t cx = tx; cx < cpr; cx += P) {
        const uint32_t x0 = 16u * cx, rep = (cx & (SCOPE_CREP - 1u)) * SCOPE_PITCH;
        for (uint32_t y = y0 + ty; y < y1; y += rows_at_once) {
            const uint4 wu = *reinterpret_cast<const uint4*>(a.u + (size_t)y * a.u_stride + x0);
            const uint4 wv = *reinterpret_cast<const uint4*>(a.v + (size_t)y * a.v_stride + x0);
            uint32_t cur = SCOPE_NONE, cnt = 0u;   // cur: u | v << 8 of the running pair
            auto put = [&](uint32_t uv, uint32_t n) {
                const uint32_t u = uv & 255u, v = uv >> 8;
                lds_add(hu, rep + u, n);
                lds_add(hv, rep + v, n);
                if (vec_on) { const uint32_t idx = (v >> 1) * 128u + (u >> 1); lds_add(vecw, idx >> 1, n << (16u * (idx & 1u))); }
            };
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t key = (x0 + i < pw) ? (byte_of(wu, i) | byte_of(wv, i) << 8) : SCOPE_NONE;
                if (key != cur) { if (cur != SCOPE_NONE) put(cur, cnt); cur = key; cnt = 0u; }
                ++cnt;
            }
            if (cur != SCOPE_NONE) put(cur, cnt);
        }
    }
    __syncthreads();
    uint32_t* hist1 = a.rec + 8 + 256;
    uint32_t* hist2 = a.rec + 8 + 512;
    uint32_t su = 0u, sv = 0u;
    for (uint32_t r = 0; r < SCOPE_CREP; ++r) { su += hu[r * SCOPE_PITCH + tid]; sv += hv[r * SCOPE_PITCH + tid]; }
    global_add(&hist1[tid], su);
    global_add(&hist2[tid], sv);
    if (vec_on) {
        uint32_t* vec = a.rec + 8 + 768 + (size_t)256 * a.wave_cols;
        for (uint32_t i = tid; i < SCOPE_VEC_WORDS; i += SCOPE_THREADS) {
            const uint32_t w = vecw[i];
            global_add(&vec[2u * i], w & 0xffffu);
            global_add(&vec[2u * i + 1u], w >> 16);
        }
    }
}

__global__ __launch_bounds__(SCOPE_THREADS) void k_video_scope(const ScopeArgs a, const ScopeGeom g) {
    __shared__ uint32_t s[SCOPE_LDS_WORDS];
    if (blockIdx.x == 0 && threadIdx.x < 8) {   // the 32-byte header
        const uint32_t t = threadIdx.x;
        a.rec[t] = t == 0 ? a.present : t == 1 ? a.counted : t == 2 ? a.pixfmt : t == 3 ? a.width : t == 4 ? a.height : t == 5 ? a.tick_in_run : 0u;
    }
    if (!a.counted) return;
    const uint32_t n_luma = g.tiles_x * g.luma_bands;
    if (blockIdx.x < n_luma) scope_luma(a, g, s, blockIdx.x % g.tiles_x, blockIdx.x / g.tiles_x);
    else scope_chroma(a, g, s, blockIdx.x - n_luma);
}

// 16-byte chunks one workgroup takes: enough that its flush (up to 8 448 / 16 896 adds) does not outweigh its counting, few enough that a
// 1080p frame still spreads over every CU
static constexpr uint32_t SCOPE_LUMA_CHUNKS = 1024, SCOPE_CHROMA_CHUNKS = 512;

void launch_video_scope(const ScopeArgs& a, hipStream_t s) {
    ScopeGeom g{};
    if (!a.counted) {
        g.tiles_x = g.luma_bands = 1; g.luma_rows = 1; g.chroma_rows = 1;
        hipLaunchKernelGGL(k_video_scope, dim3(1), dim3(SCOPE_THREADS), 0, s, a, g);
        return;
    }
    const uint32_t W = a.width, H = a.height, C = a.wave_cols, pw = W >> 1, ph = H >> 1;
    if (((uintptr_t)a.y | (uintptr_t)a.u | (uintptr_t)a.v | a.y_stride | a.u_stride | a.v_stride) & 15u) throw Error(MX_ERR_INTERNAL, "scope: frame planes are not 16-byte aligned");
    if (a.y_stride < ((W + 15u) & ~15u) || a.u_stride < ((pw + 15u) & ~15u) || a.v_stride < ((pw + 15u) & ~15u)) throw Error(MX_ERR_INTERNAL, "scope: a row's last 16-byte chunk lies beyond the stride");
    if (W > 16384u || H > 16384u || !W || !H) throw Error(MX_ERR_INVALID, "scope: frame size out of range");
    g.tiles_x = C ? (C + SCOPE_ROWS - 1) / SCOPE_ROWS : 1u;
    g.q = C / W; g.rs = C % W;
    const uint32_t tile_w = (W + g.tiles_x - 1) / g.tiles_x, cpr = (tile_w + 15u) / 16u + 1u;
    g.luma_rows = std::max(1u, SCOPE_LUMA_CHUNKS / cpr);
    g.luma_bands = (H + g.luma_rows - 1) / g.luma_rows;
    const uint32_t cpr_c = (pw + 15u) / 16u;
    g.chroma_rows = std::max(1u, std::min(SCOPE_CHROMA_CHUNKS / cpr_c, 65535u / pw));   // fewer than 65 536 pairs per workgroup: the u16 halves cannot carry
    g.chroma_bands = (ph + g.chroma_rows - 1) / g.chroma_rows;
    hipLaunchKernelGGL(k_video_scope, dim3(g.tiles_x * g.luma_bands + g.chroma_bands), dim3(SCOPE_THREADS), 0, s, a, g);
}

}  // namespace mx
