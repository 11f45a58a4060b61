// mx_k_key.hip -- the keyer (mixlab_gpu.h mx_video_key): a chroma or luma key of ONE yuv420p / yuva420p frame in ONE launch,
// written as a new yuva420p frame: Y copied, U / V copied or spill-suppressed, the coverage plane computed.  Integer arithmetic, bit-exact against
// tests/video_key_model.py.
//
// The shape:
//   * a thread owns 8 consecutive chroma samples of a chroma row -- 8 bytes of U and of V, and under them 16 luma samples of two luma rows: every plane
//     is read and written with ONE 8-byte (chroma) or 16-byte (luma, coverage) access per lane and row, at the frame's own alignment (rows are 64-byte
//     aligned, so a row's last chunk may reach into the stride padding: what is read there never reaches a visible sample, and what is written there is
//     the value DFrame::create left);
//   * the coverage of a luma sample is the 2x bilinear upsample of the per-chroma-sample key ac: it needs ac one column to the right and one row
//     below.  Both come from RECOMPUTATION, not from LDS: the thread keys a ninth sample (one extra byte of U and V per row) and the row below its own
//     (served by L2: the neighbouring thread reads the same bytes); a thread that walks several chroma rows (rows_per_thread, large frames only) carries
//     the row below over as its next row.  No barrier, no LDS, no cross-lane traffic: the kernel is a single streaming pass;
//   * d = floor(sqrt(d2 << 8)) is v_sqrt_f32 of the (rounded) argument followed by an integer correction of one step either way -- the argument goes up
//     to 33 292 800 > 2^24, so the float root alone is not the specification -- and the ramps' divisions by a frame-constant span are a multiply by
//     ceil(2^40 / span) and a shift (exact: numerator < 2^24, span < 2^16, so numerator x (span x magic - 2^40) < 2^40).
#include "mx_common.hpp"
#include "mx_dev.hpp"
#include "mx_video.hpp"

namespace mx {

static constexpr uint32_t KEY_THREADS = 256;

__device__ __forceinline__ uint32_t key_ramp(uint32_t d, uint32_t lo, uint32_t hi, uint64_t magic) {
    if (d <= lo) return 0u;
    if (d >= hi) return 255u;
    return (uint32_t)(((uint64_t)((d - lo) * 255u) * magic) >> 40);
}
// floor(sqrt(d2 << 8)), d2 <= 130 050
__device__ __forceinline__ uint32_t key_dist_q4(uint32_t d2) {
    const uint32_t x = d2 << 8;
    uint32_t r = (uint32_t)__builtin_amdgcn_sqrtf((float)x);   // within one of the integer root: 1 ulp of a value below 5 771, and x rounded to 24 bits moves the root by < 2^-11
    if (r * r > x) --r;
    else if ((r + 1u) * (r + 1u) <= x) ++r;
    return r;
}
__device__ __forceinline__ uint32_t byte8(const uint2& w, uint32_t i) { return ((i < 4 ? w.x : w.y) >> (8u * (i & 3u))) & 255u; }
__device__ __forceinline__ uint32_t byte16(const uint4& w, uint32_t i) {
    const uint32_t d = i < 4 ? w.x : (i < 8 ? w.y : (i < 12 ? w.z : w.w));
    return (d >> (8u * (i & 3u))) & 255u;
}
__device__ __forceinline__ uint32_t spill_sample(uint32_t c, uint32_t w) {   // 128 + tdiv((c - 128) * (255 - w), 255)
    return (uint32_t)(128 + ((int32_t)c - 128) * (int32_t)(255u - w) / 255);
}

// chroma row r of the thread's chunk: ac[0..8] (chroma mode; [8] = the sample right of the chunk, clamped to the row), and -- when `write` -- the row's U' / V'
__device__ __forceinline__ void key_chroma_row(const KeyArgs& a, uint32_t c0, uint32_t r, bool write, uint32_t (&ac)[9]) {
    const uint32_t Wc = a.width >> 1;
    const uint2 wu = *reinterpret_cast<const uint2*>(a.u + (size_t)r * a.u_stride + c0);
    const uint2 wv = *reinterpret_cast<const uint2*>(a.v + (size_t)r * a.v_stride + c0);
    uint32_t ou[8], ov[8];
    if (a.mode == MX_KEY_CHROMA) {
        const uint32_t ch = min(c0 + 8u, Wc - 1u);
        const uint32_t hu = a.u[(size_t)r * a.u_stride + ch], hv = a.v[(size_t)r * a.v_stride + ch];
#pragma unroll
        for (uint32_t j = 0; j < 9; ++j) {
            const uint32_t u = j < 8 ? byte8(wu, j) : hu, v = j < 8 ? byte8(wv, j) : hv;
            const int32_t du = (int32_t)u - (int32_t)a.key_u, dv = (int32_t)v - (int32_t)a.key_v;
            const uint32_t d = key_dist_q4((uint32_t)(du * du + dv * dv));
            ac[j] = key_ramp(d, a.near_q4, a.far_q4, a.m_ramp);
            if (j < 8) {
                uint32_t w = 0u;
                if (a.spill_on) w = ((255u - key_ramp(d, a.far_q4, a.spill_far_q4, a.m_spill)) * a.spill_strength) / 255u;
                ou[j] = spill_sample(u, w); ov[j] = spill_sample(v, w);   // w = 0: the identity
            }
        }
    } else {
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) { ou[j] = byte8(wu, j); ov[j] = byte8(wv, j); }
    }
    if (!write) return;
    uint2 pu = make_uint2(0u, 0u), pv = make_uint2(0u, 0u);
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        const bool vis = c0 + j < Wc;
        const uint32_t bu = (vis ? ou[j] : 0x80u) << (8u * (j & 3u)), bv = (vis ? ov[j] : 0x80u) << (8u * (j & 3u));   // beyond the row: the blank frame's chroma
        if (j < 4) { pu.x |= bu; pv.x |= bv; } else { pu.y |= bu; pv.y |= bv; }
    }
    *reinterpret_cast<uint2*>(a.ou + (size_t)r * a.ou_stride + c0) = pu;
    *reinterpret_cast<uint2*>(a.ov + (size_t)r * a.ov_stride + c0) = pv;
}

// the two luma rows under chroma row r: Y copied, coverage from ac of row r (top) and of row min(r + 1, Hc - 1) (bot)
__device__ __forceinline__ void key_luma_rows(const KeyArgs& a, uint32_t c0, uint32_t r, const uint32_t (&top)[9], const uint32_t (&bot)[9]) {
    const uint32_t Wc = a.width >> 1, x0 = 2u * c0;
#pragma unroll
    for (uint32_t ry = 0; ry < 2; ++ry) {
        const uint32_t y = 2u * r + ry;
        const uint4 wy = *reinterpret_cast<const uint4*>(a.y + (size_t)y * a.y_stride + x0);
        uint4 wa = make_uint4(0u, 0u, 0u, 0u);
        if (a.a_in) wa = *reinterpret_cast<const uint4*>(a.a_in + (size_t)y * a.a_stride + x0);
        uint32_t py[4] = {0u, 0u, 0u, 0u}, pa[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t j = 0; j < 8; ++j) {
            const bool vis = c0 + j < Wc;
            const bool more = c0 + j + 1u < Wc;                           // cx1 = min(cx + 1, Wc - 1)
            const uint32_t t0 = top[j], t1 = more ? top[j + 1] : top[j];
            const uint32_t b0 = ry ? bot[j] : t0, b1 = ry ? (more ? bot[j + 1] : bot[j]) : t1;   // cy1 = cy on an even row
#pragma unroll
            for (uint32_t dx = 0; dx < 2; ++dx) {
                const uint32_t i = 2u * j + dx, yv = byte16(wy, i);
                uint32_t k;
                if (a.mode == MX_KEY_CHROMA) k = dx ? (t0 + t1 + b0 + b1 + 2u) >> 2 : (t0 + t0 + b0 + b0 + 2u) >> 2;
                else k = key_ramp(yv * 16u, a.near_q4, a.far_q4, a.m_ramp);
                if (a.invert) k = 255u - k;
                if (a.a_in) k = (k * byte16(wa, i)) / 255u;
                py[i >> 2] |= (vis ? yv : 0u) << (8u * (i & 3u));         // beyond the row: the blank frame's luma and an opaque coverage
                pa[i >> 2] |= (vis ? k : 255u) << (8u * (i & 3u));
            }
        }
        *reinterpret_cast<uint4*>(a.oy + (size_t)y * a.oy_stride + x0) = make_uint4(py[0], py[1], py[2], py[3]);
        *reinterpret_cast<uint4*>(a.oa + (size_t)y * a.oa_stride + x0) = make_uint4(pa[0], pa[1], pa[2], pa[3]);
    }
}

__global__ __launch_bounds__(KEY_THREADS) void k_video_key(const KeyArgs a) {
    const uint32_t id = blockIdx.x * KEY_THREADS + threadIdx.x;
    if (id >= a.n_threads) return;
    const uint32_t Hc = a.height >> 1;
    const uint32_t band = id / a.chunks_x, c0 = 8u * (id - band * a.chunks_x);
    const uint32_t r0 = band * a.rows_per_thread, r1 = min(Hc, r0 + a.rows_per_thread);
    uint32_t cur[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, nxt[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    key_chroma_row(a, c0, r0, true, cur);
    for (uint32_t r = r0; r < r1; ++r) {
        const bool own_next = r + 1u < r1;
        if (own_next || (a.mode == MX_KEY_CHROMA && r + 1u < Hc)) key_chroma_row(a, c0, r + 1u, own_next, nxt);   // the row below: this thread's next, or the band's halo
        else {
#pragma unroll
            for (uint32_t j = 0; j < 9; ++j) nxt[j] = cur[j];                                                      // cy1 = min(cy + 1, Hc - 1)
        }
        key_luma_rows(a, c0, r, cur, nxt);
#pragma unroll
        for (uint32_t j = 0; j < 9; ++j) cur[j] = nxt[j];
    }
}

static uint64_t key_magic(uint32_t span) { return span ? ((1ull << 40) + span - 1u) / span : 0ull; }

void launch_video_key(KeyArgs a, hipStream_t s) {
    const uint32_t W = a.width, H = a.height, Wc = W >> 1, Hc = H >> 1;
    if (!W || !H || (W & 1u) || (H & 1u) || W > 16384u || H > 16384u) throw Error(MX_ERR_INVALID, "key: frame size must be even, non-zero and at most 16384");
    // every access is one aligned 8-byte (chroma) or 16-byte (luma, coverage) word per lane, and a row's last word stays inside the row's stride
    const uint32_t cw8 = (Wc + 7u) & ~7u, lw16 = 2u * cw8;
    if (((uintptr_t)a.u | (uintptr_t)a.v | (uintptr_t)a.ou | (uintptr_t)a.ov | a.u_stride | a.v_stride | a.ou_stride | a.ov_stride) & 7u) throw Error(MX_ERR_INTERNAL, "key: chroma planes are not 8-byte aligned");
    if (((uintptr_t)a.y | (uintptr_t)a.oy | (uintptr_t)a.oa | (uintptr_t)a.a_in | a.y_stride | a.oy_stride | a.oa_stride | (a.a_in ? a.a_stride : 0u)) & 15u) throw Error(MX_ERR_INTERNAL, "key: luma / coverage planes are not 16-byte aligned");
    if (a.u_stride < cw8 || a.v_stride < cw8 || a.ou_stride < cw8 || a.ov_stride < cw8 || a.y_stride < lw16 || a.oy_stride < lw16 || a.oa_stride < lw16 || (a.a_in && a.a_stride < lw16))
        throw Error(MX_ERR_INTERNAL, "key: a row's last chunk lies beyond the stride");
    a.spill_on = (a.mode == MX_KEY_CHROMA && a.spill_strength > 0u && a.spill_far_q4 > a.far_q4) ? 1u : 0u;
    a.m_ramp = key_magic(a.far_q4 - a.near_q4);
    a.m_spill = a.spill_on ? key_magic(a.spill_far_q4 - a.far_q4) : 0ull;
    a.chunks_x = cw8 / 8u;
    // one chroma row per thread (the most parallel form: a 1080p frame is 253 workgroups) until the grid passes 2048 workgroups; then threads walk a band of rows
    const uint64_t per_row_wgs = ((uint64_t)a.chunks_x * Hc + KEY_THREADS - 1) / KEY_THREADS;
    a.rows_per_thread = (uint32_t)((per_row_wgs + 2047u) / 2048u);
    const uint32_t bands = (Hc + a.rows_per_thread - 1u) / a.rows_per_thread;
    a.n_threads = a.chunks_x * bands;
    hipLaunchKernelGGL(k_video_key, dim3((a.n_threads + KEY_THREADS - 1u) / KEY_THREADS), dim3(KEY_THREADS), 0, s, a);
}

}  // namespace mx
