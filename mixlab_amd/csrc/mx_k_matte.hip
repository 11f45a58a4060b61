// mx_k_matte.hip -- the matte refiner (mixlab_gpu.h mx_video_matte): clean, choke, soften and garbage mask of the coverage plane of ONE
// yuv420p / yuva420p frame in ONE launch, written as a new yuva420p frame: Y, U and V copied in whole words, the coverage plane computed.  Integer arithmetic,
// bit-exact against tests/video_matte_model.py.
//
// Two shapes, the stages compiled in or out as k_video_grade's are:
//   * k_video_matte_stream<CLEAN, MASK> -- settings without CHOKE and SOFTEN (and every setting on a frame without coverage, whose choked and softened plane is the
//     constant clean(255)).  The keyer's shape (mx_k_key.hip): a thread owns 8 chroma samples of a chroma row and the 2 x 16 luma samples under them, ONE 8-byte or
//     16-byte access per plane, lane and row; no LDS, no barrier, no cross-lane traffic.  MASK is a template parameter: the rectangle's path is four 32-bit
//     subtractions and a minimum and holds none of the circle's 64-bit squares and root.  A wipe launches this form every tick;
//   * k_video_matte_tile<HALO, MASK> -- CHOKE and / or SOFTEN on a frame with coverage.  A workgroup of 256 owns a tile of 64 x 32 luma samples (and the 32 x 16
//     chroma samples under it: 128 + 64 + 64 = 256 words of Y, U and V, one per thread).  It stages the tile's coverage with a halo of HALO = |choke| + soften rounded
//     up to 4, 8 or 12 samples per side in LDS as bytes, cleaned on the way in (aligned dword reads; a dword that begins beyond the row is not read at all), runs the
//     minimum / maximum as a horizontal and a vertical pass from one byte tile into the other and back, the binomial as a horizontal pass into 32-bit sums (20 bits
//     are needed) and a vertical pass out of them in which a thread owns 8 consecutive samples of a row, rounds ONCE, multiplies the mask and stores 8 bytes.
//     The header's clamp cl() is applied to the INDEX of every tap (each stage clamps to the plane on its own, as the specification nests them), so neither stride
//     padding nor a sample beyond the plane is ever read as picture, and a minimum or maximum never sees a filler value.
//     Up to 2048 workgroups there is one tile per workgroup; beyond that (above 1080p: 1020 tiles) a workgroup walks tiles 2048 apart.
//   * the ramps' divisions by a frame-constant span are the keyer's multiply by ceil(2^40 / span) and a shift (exact: numerator < 2^24, span < 2^16);
//   * the circle's root is v_sqrt_f32 of the 43-bit argument corrected by integer steps until r^2 <= x < (r + 1)^2 holds in 64 bits.
#include "mx_common.hpp"
#include "mx_dev.hpp"
#include "mx_video.hpp"

#include <algorithm>

namespace mx {

static constexpr uint32_t MATTE_THREADS = 256, MATTE_TW = 64, MATTE_TH = 32, MATTE_MAX_WGS = 2048;
enum { MATTE_MASK_NONE = 0, MATTE_MASK_RECT = 1, MATTE_MASK_CIRCLE = 2 };

__device__ __forceinline__ uint32_t m_byte(uint32_t w, uint32_t i) { return (w >> (8u * i)) & 255u; }
__device__ __forceinline__ uint32_t m_word(const uint4& w, uint32_t i) { return i == 0 ? w.x : (i == 1 ? w.y : (i == 2 ? w.z : w.w)); }

// CLEAN: 0 at or below black, 255 at or above white, ((a - black) * 255) / (white - black) between them, the tests in this order
template <bool CLEAN> __device__ __forceinline__ uint32_t matte_clean(const MatteArgs& a, uint32_t v) {
    if constexpr (!CLEAN) return v;
    if (v <= a.clean_black) return 0u;
    if (v >= a.clean_white) return 255u;
    return (uint32_t)(((uint64_t)((v - a.clean_black) * 255u) * a.m_clean) >> 40);
}

// floor(sqrt(x)), x < 2^43: the float root is within a few units; the steps make it exact
__device__ __forceinline__ int32_t matte_isqrt(uint64_t x) {
    uint64_t r = (uint64_t)__builtin_amdgcn_sqrtf((float)x);
    while (r * r > x) --r;
    while ((r + 1u) * (r + 1u) <= x) ++r;
    return (int32_t)r;
}

// the part of the mask's distance that a row shares: RECT min(py - y0, y1 - py); CIRCLE (py - y0)^2
template <int MASK> struct MatteRow { int32_t dy; uint64_t dy2; };
template <int MASK> __device__ __forceinline__ MatteRow<MASK> matte_row(const MatteArgs& a, uint32_t y) {
    MatteRow<MASK> r{0, 0ull};
    const int32_t py = 16 * (int32_t)y + 8;
    if constexpr (MASK == MATTE_MASK_RECT) r.dy = min(py - a.mask_y0, a.mask_y1 - py);
    if constexpr (MASK == MATTE_MASK_CIRCLE) { const int64_t d = (int64_t)py - a.mask_y0; r.dy2 = (uint64_t)(d * d); }
    return r;
}
// (a3 * m) / 255 of the sample at column x of a row
template <int MASK> __device__ __forceinline__ uint32_t matte_mask(const MatteArgs& a, const MatteRow<MASK>& row, uint32_t x, uint32_t a3) {
    if constexpr (MASK == MATTE_MASK_NONE) return a3;
    const int32_t px = 16 * (int32_t)x + 8;
    int32_t d;
    if constexpr (MASK == MATTE_MASK_RECT) d = min(min(px - a.mask_x0, a.mask_x1 - px), row.dy);
    else { const int64_t dx = (int64_t)px - a.mask_x0; d = a.mask_x1 - matte_isqrt((uint64_t)(dx * dx) + row.dy2); }
    uint32_t m;
    if (d <= 0) m = 0u;
    else if ((uint32_t)d >= a.mask_feather) m = 255u;
    else m = (uint32_t)(((uint64_t)((uint32_t)d * 255u) * a.m_feather) >> 40);
    if (a.mask_invert) m = 255u - m;
    return (a3 * m) / 255u;
}

// ---- the streaming form ----
template <bool CLEAN, int MASK>
__global__ __launch_bounds__(MATTE_THREADS) void k_video_matte_stream(const MatteArgs a) {
    const uint32_t Wc = a.width >> 1;
    for (uint32_t id = blockIdx.x * MATTE_THREADS + threadIdx.x; id < a.n_threads; id += gridDim.x * MATTE_THREADS) {
        const uint32_t r = id / a.chunks_x, c0 = 8u * (id - r * a.chunks_x), x0 = 2u * c0;
        // chroma: byte for byte, and the blank frame's chroma beyond the row
        const uint2 wu = *reinterpret_cast<const uint2*>(a.u + (size_t)r * a.u_stride + c0);
        const uint2 wv = *reinterpret_cast<const uint2*>(a.v + (size_t)r * a.v_stride + c0);
        uint2 pu = make_uint2(0u, 0u), pv = make_uint2(0u, 0u);
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const bool vis = c0 + j < Wc;
            const uint32_t bu = (vis ? m_byte(j < 4 ? wu.x : wu.y, j & 3u) : 0x80u) << (8u * (j & 3u)), bv = (vis ? m_byte(j < 4 ? wv.x : wv.y, j & 3u) : 0x80u) << (8u * (j & 3u));
            if (j < 4) { pu.x |= bu; pv.x |= bv; } else { pu.y |= bu; pv.y |= bv; }
        }
        *reinterpret_cast<uint2*>(a.ou + (size_t)r * a.ou_stride + c0) = pu;
        *reinterpret_cast<uint2*>(a.ov + (size_t)r * a.ov_stride + c0) = pv;
#pragma unroll
        for (uint32_t ry = 0; ry < 2; ++ry) {
            const uint32_t y = 2u * r + ry;
            const uint4 wy = *reinterpret_cast<const uint4*>(a.y + (size_t)y * a.y_stride + x0);
            uint4 wa = make_uint4(~0u, ~0u, ~0u, ~0u);   // no coverage plane: opaque
            if (a.a_in) wa = *reinterpret_cast<const uint4*>(a.a_in + (size_t)y * a.a_stride + x0);
            const MatteRow<MASK> row = matte_row<MASK>(a, y);
            uint32_t py[4] = {0u, 0u, 0u, 0u}, pa[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const bool vis = x0 + i < a.width;
                const uint32_t k = matte_mask<MASK>(a, row, x0 + i, matte_clean<CLEAN>(a, m_byte(m_word(wa, i >> 2), i & 3u)));
                py[i >> 2] |= (vis ? m_byte(m_word(wy, i >> 2), i & 3u) : 0u) << (8u * (i & 3u));   // beyond the row: the blank frame's luma and an opaque coverage
                pa[i >> 2] |= (vis ? k : 255u) << (8u * (i & 3u));
            }
            *reinterpret_cast<uint4*>(a.oy + (size_t)y * a.oy_stride + x0) = make_uint4(py[0], py[1], py[2], py[3]);
            *reinterpret_cast<uint4*>(a.oa + (size_t)y * a.oa_stride + x0) = make_uint4(pa[0], pa[1], pa[2], pa[3]);
        }
    }
}

// ---- the neighbourhood form ----
// The tile's region is RW x RH samples: the tile and HALO samples on every side.  LDS: two byte tiles of the region and the horizontal sums of the binomial,
// 64 columns x RH rows of uint32.  HALO 4: 2 x 2 880 + 10 240 = 16 000 bytes; HALO 8: 2 x 3 840 + 12 288 = 19 968; HALO 12: 2 x 4 928 + 14 336 = 24 192.
template <int HALO, int MASK>
__global__ __launch_bounds__(MATTE_THREADS) void k_video_matte_tile(const MatteArgs a) {
    constexpr uint32_t RW = MATTE_TW + 2u * HALO, RH = MATTE_TH + 2u * HALO, RD = RW / 4u;
    __shared__ __attribute__((aligned(16))) uint32_t b0w[RD * RH], b1w[RD * RH], hs[MATTE_TW * RH];   // every size is a multiple of 16 bytes
    uint8_t* const b0 = reinterpret_cast<uint8_t*>(b0w);
    uint8_t* const b1 = reinterpret_cast<uint8_t*>(b1w);
    const uint32_t W = a.width, H = a.height, Wc = W >> 1, Hc = H >> 1, t = threadIdx.x;
    const int32_t r = (int32_t)a.choke_r, sft = (int32_t)a.soften;
    for (uint32_t tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const uint32_t ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
        const int32_t X0 = (int32_t)(tx * MATTE_TW), Y0 = (int32_t)(ty * MATTE_TH), RX = X0 - HALO, RY = Y0 - HALO;
        // the plane's part of the region, in region coordinates: every tap's index is clamped into it (cl() of the header; the region holds HALO >= |choke| + soften
        // samples beyond the tile, so a clamp against the region's own edge only ever moves a tap that no visible sample depends on)
        const int32_t lx_lo = max(0, -RX), lx_hi = min((int32_t)RW - 1, (int32_t)W - 1 - RX), ly_lo = max(0, -RY), ly_hi = min((int32_t)RH - 1, (int32_t)H - 1 - RY);

        // Y, U, V: one word per thread -- 32 rows x 4 words of 16 luma bytes, 16 rows x 4 words of 8 chroma bytes per chroma plane
        if (t < 128u) {
            const uint32_t y = (uint32_t)Y0 + (t >> 2), x = (uint32_t)X0 + 16u * (t & 3u);
            if (y < H && x < a.lw16) {
                const uint4 w = *reinterpret_cast<const uint4*>(a.y + (size_t)y * a.y_stride + x);
                uint32_t p[4];
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    uint32_t o = 0u;
#pragma unroll
                    for (uint32_t i = 0; i < 4; ++i) o |= ((x + 4u * q + i < W) ? m_byte(m_word(w, q), i) : 0u) << (8u * i);   // beyond the row: the blank frame's luma
                    p[q] = o;
                }
                *reinterpret_cast<uint4*>(a.oy + (size_t)y * a.oy_stride + x) = make_uint4(p[0], p[1], p[2], p[3]);
            }
        } else {
            const uint32_t k = t - 128u, pl = k >> 6, cy = ((uint32_t)Y0 >> 1) + ((k & 63u) >> 2), cx = ((uint32_t)X0 >> 1) + 8u * (k & 3u);
            if (cy < Hc && cx < a.cw8) {
                const uint8_t* src = pl ? a.v + (size_t)cy * a.v_stride : a.u + (size_t)cy * a.u_stride;
                uint8_t* dst = pl ? a.ov + (size_t)cy * a.ov_stride : a.ou + (size_t)cy * a.ou_stride;
                const uint2 w = *reinterpret_cast<const uint2*>(src + cx);
                uint2 p = make_uint2(0u, 0u);
#pragma unroll
                for (uint32_t i = 0; i < 8; ++i) {
                    const uint32_t b = ((cx + i < Wc) ? m_byte(i < 4 ? w.x : w.y, i & 3u) : 0x80u) << (8u * (i & 3u));   // ... and its chroma
                    if (i < 4) p.x |= b; else p.y |= b;
                }
                *reinterpret_cast<uint2*>(dst + cx) = p;
            }
        }

        // a1 = clean(A_in) into b0, four samples per aligned dword; a dword that begins outside the plane is never read (its bytes are never indexed either)
        for (uint32_t i = t; i < RD * RH; i += MATTE_THREADS) {
            const uint32_t ly = i / RD, ld = i - ly * RD;
            const int32_t gy = RY + (int32_t)ly, gx = RX + 4 * (int32_t)ld;
            uint32_t o = 0u;
            if (gy >= 0 && gy < (int32_t)H && gx >= 0 && gx < (int32_t)W) {
                const uint32_t w = *reinterpret_cast<const uint32_t*>(a.a_in + (size_t)gy * a.a_stride + (uint32_t)gx);
                if (a.flags & MX_MATTE_CLEAN) {
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) o |= matte_clean<true>(a, m_byte(w, q)) << (8u * q);
                } else o = w;
            }
            b0w[i] = o;
        }
        __syncthreads();

        if (r > 0) {   // CHOKE: b0 -> (rows) b1 -> (columns) b0
            const bool grow = a.choke_grow != 0u;
            for (uint32_t i = t; i < RW * RH; i += MATTE_THREADS) {
                const uint32_t ly = i / RW;
                const int32_t lx = (int32_t)(i - ly * RW);
                const uint8_t* row = b0 + ly * RW;
                uint32_t m = row[min(max(lx - r, lx_lo), lx_hi)];
                for (int32_t k = -r + 1; k <= r; ++k) { const uint32_t v = row[min(max(lx + k, lx_lo), lx_hi)]; m = grow ? max(m, v) : min(m, v); }
                b1[i] = (uint8_t)m;
            }
            __syncthreads();
            for (uint32_t i = t; i < RW * RH; i += MATTE_THREADS) {
                const uint32_t ly = i / RW, lx = i - ly * RW;
                uint32_t m = b1[(uint32_t)min(max((int32_t)ly - r, ly_lo), ly_hi) * RW + lx];
                for (int32_t k = -r + 1; k <= r; ++k) { const uint32_t v = b1[(uint32_t)min(max((int32_t)ly + k, ly_lo), ly_hi) * RW + lx]; m = grow ? max(m, v) : min(m, v); }
                b0[i] = (uint8_t)m;
            }
            __syncthreads();
        }

        if (sft > 0) {   // SOFTEN, rows: hs[ly][x] = sum_i b[i] a2(cl(x + i), ly), at most 255 * 2^12
            for (uint32_t i = t; i < MATTE_TW * RH; i += MATTE_THREADS) {
                const uint32_t ly = i / MATTE_TW;
                const int32_t lx = (int32_t)(i - ly * MATTE_TW) + HALO;
                const uint8_t* row = b0 + ly * RW;
                uint32_t acc = 0u;
                for (int32_t k = -sft; k <= sft; ++k) acc += a.binom[k + sft] * (uint32_t)row[min(max(lx + k, lx_lo), lx_hi)];
                hs[i] = acc;
            }
            __syncthreads();
        }

        // out: a thread owns 8 consecutive samples of one of the tile's 32 rows
        {
            const uint32_t oy = t >> 3, ox = 8u * (t & 7u), y = (uint32_t)Y0 + oy, x = (uint32_t)X0 + ox;
            if (y < H && x < a.lw16) {
                uint32_t v[8];
                if (sft > 0) {
#pragma unroll
                    for (uint32_t q = 0; q < 8; ++q) v[q] = 0u;
                    for (int32_t k = -sft; k <= sft; ++k) {
                        const uint32_t ly = (uint32_t)min(max((int32_t)oy + HALO + k, ly_lo), ly_hi), w = a.binom[k + sft];
                        const uint4 h0 = *reinterpret_cast<const uint4*>(&hs[ly * MATTE_TW + ox]), h1 = *reinterpret_cast<const uint4*>(&hs[ly * MATTE_TW + ox + 4u]);
#pragma unroll
                        for (uint32_t q = 0; q < 4; ++q) { v[q] += w * m_word(h0, q); v[q + 4u] += w * m_word(h1, q); }
                    }
                    const uint32_t sh = 4u * (uint32_t)sft;
#pragma unroll
                    for (uint32_t q = 0; q < 8; ++q) v[q] = (v[q] + (1u << (sh - 1u))) >> sh;   // the ONE rounding: at most 255 * 2^24 + 2^23 < 2^32
                } else {
                    const uint32_t d = ((oy + HALO) * RW + HALO + ox) / 4u, w0 = b0w[d], w1 = b0w[d + 1u];   // HALO = 4, 12: dword-aligned only
#pragma unroll
                    for (uint32_t q = 0; q < 8; ++q) v[q] = m_byte(q < 4 ? w0 : w1, q & 3u);
                }
                const MatteRow<MASK> row = matte_row<MASK>(a, y);
                uint2 p = make_uint2(0u, 0u);
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q) {
                    const uint32_t b = ((x + q < W) ? matte_mask<MASK>(a, row, x + q, v[q]) : 255u) << (8u * (q & 3u));   // beyond the row: an opaque coverage
                    if (q < 4) p.x |= b; else p.y |= b;
                }
                *reinterpret_cast<uint2*>(a.oa + (size_t)y * a.oa_stride + x) = p;
            }
        }
        __syncthreads();   // the next tile's staging overwrites b0 and hs
    }
}

static uint64_t matte_magic(uint32_t span) { return span ? ((1ull << 40) + span - 1u) / span : 0ull; }

template <int MASK> static void launch_matte_stream(const MatteArgs& a, uint32_t wgs, hipStream_t s) {
    if (a.flags & MX_MATTE_CLEAN) hipLaunchKernelGGL((k_video_matte_stream<true, MASK>), dim3(wgs), dim3(MATTE_THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_video_matte_stream<false, MASK>), dim3(wgs), dim3(MATTE_THREADS), 0, s, a);
}
template <int MASK> static void launch_matte_tile(const MatteArgs& a, uint32_t halo, uint32_t wgs, hipStream_t s) {
    if (halo <= 4u) hipLaunchKernelGGL((k_video_matte_tile<4, MASK>), dim3(wgs), dim3(MATTE_THREADS), 0, s, a);
    else if (halo <= 8u) hipLaunchKernelGGL((k_video_matte_tile<8, MASK>), dim3(wgs), dim3(MATTE_THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_video_matte_tile<12, MASK>), dim3(wgs), dim3(MATTE_THREADS), 0, s, a);
}

void launch_video_matte(MatteArgs a, hipStream_t s) {
    const uint32_t W = a.width, H = a.height, Wc = W >> 1, Hc = H >> 1;
    if (!W || !H || (W & 1u) || (H & 1u) || W > 16384u || H > 16384u) throw Error(MX_ERR_INVALID, "matte: frame size must be even, non-zero and at most 16384");
    // the keyer's checks: every access is one aligned word (8 bytes of chroma, 16 of luma and coverage, or a part of one), and a row's last word stays inside the stride
    const uint32_t cw8 = (Wc + 7u) & ~7u, lw16 = 2u * cw8;
    if (((uintptr_t)a.u | (uintptr_t)a.v | (uintptr_t)a.ou | (uintptr_t)a.ov | a.u_stride | a.v_stride | a.ou_stride | a.ov_stride) & 7u) throw Error(MX_ERR_INTERNAL, "matte: chroma planes are not 8-byte aligned");
    if (((uintptr_t)a.y | (uintptr_t)a.oy | (uintptr_t)a.oa | (uintptr_t)a.a_in | a.y_stride | a.oy_stride | a.oa_stride | (a.a_in ? a.a_stride : 0u)) & 15u) throw Error(MX_ERR_INTERNAL, "matte: luma / coverage planes are not 16-byte aligned");
    if (a.u_stride < cw8 || a.v_stride < cw8 || a.ou_stride < cw8 || a.ov_stride < cw8 || a.y_stride < lw16 || a.oy_stride < lw16 || a.oa_stride < lw16 || (a.a_in && a.a_stride < lw16))
        throw Error(MX_ERR_INTERNAL, "matte: a row's last chunk lies beyond the stride");
    if (!a.oa) throw Error(MX_ERR_INTERNAL, "matte: the output frame has no coverage plane");
    if (a.choke_r > 6u || a.soften > 6u) throw Error(MX_ERR_INTERNAL, "matte: a radius above 6");
    a.cw8 = cw8; a.lw16 = lw16;
    a.m_clean = matte_magic((uint32_t)a.clean_white - (uint32_t)a.clean_black);
    a.m_feather = matte_magic(a.mask_feather);
    for (uint32_t k = 0; k < 13u; ++k) a.binom[k] = 0u;
    if (a.soften) {   // C(2s, k), k = 0 .. 2s
        uint64_t c = 1;
        for (uint32_t k = 0; k <= 2u * a.soften; ++k) { a.binom[k] = (uint32_t)c; c = c * (2u * a.soften - k) / (k + 1u); }
    }
    const int mask = !(a.flags & MX_MATTE_MASK) ? MATTE_MASK_NONE : (a.mask_shape == MX_MATTE_MASK_CIRCLE ? MATTE_MASK_CIRCLE : MATTE_MASK_RECT);
    const uint32_t halo = a.a_in ? a.choke_r + a.soften : 0u;   // without coverage the choked and softened plane is the constant clean(255)
    if (halo == 0u) {
        a.chunks_x = cw8 / 8u;
        a.n_threads = a.chunks_x * Hc;   // <= 1024 x 8192
        const uint32_t wgs = std::min((a.n_threads + MATTE_THREADS - 1u) / MATTE_THREADS, MATTE_MAX_WGS);
        if (mask == MATTE_MASK_NONE) launch_matte_stream<MATTE_MASK_NONE>(a, wgs, s);
        else if (mask == MATTE_MASK_RECT) launch_matte_stream<MATTE_MASK_RECT>(a, wgs, s);
        else launch_matte_stream<MATTE_MASK_CIRCLE>(a, wgs, s);
        return;
    }
    a.tiles_x = (W + MATTE_TW - 1u) / MATTE_TW;
    a.n_tiles = a.tiles_x * ((H + MATTE_TH - 1u) / MATTE_TH);   // <= 256 x 512
    const uint32_t wgs = std::min(a.n_tiles, MATTE_MAX_WGS);
    if (mask == MATTE_MASK_NONE) launch_matte_tile<MATTE_MASK_NONE>(a, halo, wgs, s);
    else if (mask == MATTE_MASK_RECT) launch_matte_tile<MATTE_MASK_RECT>(a, halo, wgs, s);
    else launch_matte_tile<MATTE_MASK_CIRCLE>(a, halo, wgs, s);
}

}  // namespace mx
