// mx_k_grade.hip -- the colour corrector (mixlab_gpu.h mx_video_grade): a luma curve, a chroma matrix and a tetrahedral 3D LUT applied to
// ONE yuv420p / yuva420p frame in ONE launch, written as a new frame of the same format.  Integer arithmetic, bit-exact against tests/video_grade_model.py.
//
// The shape is the keyer's (mx_k_key.hip):
//   * a thread owns 8 consecutive chroma samples of a chroma row -- 8 bytes of U and of V -- and under them 16 luma samples of two luma rows: every plane is read
//     and written with ONE 8-byte (chroma) or 16-byte (luma, coverage) access per lane and row, at the frame's own alignment (rows are 64-byte aligned, so a row's
//     last chunk may reach into the stride padding: what is read there never reaches a visible sample, and what is written there is the value DFrame::create left);
//   * everything a sample needs is inside its thread: a luma sample takes the chroma of its own 2 x 2 block, a chroma sample the mean of its block's four curved
//     luma samples.  No halo, no cross-lane traffic, and on the path without a LUT no barrier and no LDS;
//   * the curve is read out of the kernel arguments with a per-lane index (256 bytes the whole chip shares: they stay in the caches);
//   * the stages are compiled in or out: k_video_grade<GATHER_NONE, 0> holds no LUT code, so a frame with only the curve, only the matrix or both does not pay for it;
//   * the lattice is split into a Y' table (uint16 per node) and a U' | V' << 16 table (uint32 per node): a luma sample gathers 4 x 2 bytes, a chroma sample 4 x 4.
//     GATHER_GLOBAL reads both through the caches (either lattice size; the 33-lattice's 216 KB do not fit a CU's LDS, so it always runs this way).  GATHER_LDS
//     (17-lattice only: 29 504 bytes) stages them into LDS once per workgroup, ONE barrier, and the workgroup then walks its tiles of 256 threads: one tile while
//     the frame has no more tiles than the chip has CUs, several beyond that.  It is the default of the 17-lattice: 8.5 us against 16.2 us per 1080p frame.
// Division-free: cells and fractions are shifts and masks of compile-time width (the lattice size is a template parameter).
#include "mx_common.hpp"
#include "mx_dev.hpp"
#include "mx_video.hpp"

#include <cstdlib>
#include <cstring>

namespace mx {

static constexpr uint32_t GRADE_THREADS = 256;
enum { GATHER_NONE = 0, GATHER_GLOBAL = 1, GATHER_LDS = 2 };
static constexpr uint32_t GRADE_LDS_Y_BYTES = (17u * 17u * 17u * 2u + 15u) & ~15u, GRADE_LDS_UV_BYTES = (17u * 17u * 17u * 4u + 15u) & ~15u;   // LutTables' layout of the 17-lattice
// The staging workgroups: one per tile up to one per CU of an MI355X (at 256 VGPRs a CU holds one of them), and from there on each walks tiles 256 apart.  Measured on
// a 1080p frame (254 tiles): one tile per workgroup 8.5 us, two 13.2, four 22.4 -- re-reading the lattice out of L2 costs less than leaving CUs idle
static constexpr uint32_t GRADE_LDS_MAX_WGS = 256;

__device__ __forceinline__ uint32_t g_byte8(const uint2& w, uint32_t i) { return ((i < 4 ? w.x : w.y) >> (8u * (i & 3u))) & 255u; }
__device__ __forceinline__ uint32_t g_byte16(const uint4& w, uint32_t i) {
    const uint32_t d = i < 4 ? w.x : (i < 8 ? w.y : (i < 12 ? w.z : w.w));
    return (d >> (8u * (i & 3u))) & 255u;
}
__device__ __forceinline__ uint32_t g_clip8(int32_t x) { return (uint32_t)min(255, max(0, x)); }

// The tetrahedron of (a, b, c) in a lattice of 2^K + 1 nodes per axis: node indices n[0..3] and weights w[0..3] (sum 2^(8-K)).  The vertex after the low corner lies
// one step along the axis of the largest fraction, the vertex before the high corner one step short of it along the axis of the smallest: the walk f1, f2, f3 of the
// header.  With equal fractions the choice falls on a vertex of weight 0; largest and smallest never name the same axis (all equal: Y first, V last).
template <int K> __device__ __forceinline__ void tetra(uint32_t a, uint32_t b, uint32_t c, uint32_t (&n)[4], uint32_t (&w)[4]) {
    constexpr uint32_t SH = 8u - K, S = 1u << SH, N = (1u << K) + 1u, SA = N * N, SB = N, SC = 1u;
    const uint32_t fa = a & (S - 1u), fb = b & (S - 1u), fc = c & (S - 1u);
    const uint32_t base = ((a >> SH) * N + (b >> SH)) * N + (c >> SH);
    const uint32_t fmax = max(fa, max(fb, fc)), fmin = min(fa, min(fb, fc)), fmid = fa + fb + fc - fmax - fmin;
    const uint32_t smax = (fa >= fb && fa >= fc) ? SA : (fb >= fc ? SB : SC);
    const uint32_t smin = (fc <= fa && fc <= fb) ? SC : (fb <= fa ? SB : SA);
    n[0] = base; n[1] = base + smax; n[3] = base + SA + SB + SC; n[2] = n[3] - smin;
    w[0] = S - fmax; w[1] = fmax - fmid; w[2] = fmid - fmin; w[3] = fmin;
}
template <int K> __device__ __forceinline__ uint32_t lut_round(uint32_t acc) {   // min(255, (acc + 8 S) >> (sh + 4))
    constexpr uint32_t SH = 8u - K;
    return min(255u, (acc + (8u << SH)) >> (SH + 4u));
}

// one thread's unit: chroma samples [c0, c0 + 8) of chroma row r and the two luma rows under them
template <int MODE, int K>
__device__ __forceinline__ void grade_unit(const GradeArgs& a, uint32_t c0, uint32_t r, const uint16_t* __restrict__ ty, const uint32_t* __restrict__ tuv) {
    const uint32_t Wc = a.width >> 1, x0 = 2u * c0;
    const uint2 wu = *reinterpret_cast<const uint2*>(a.u + (size_t)r * a.u_stride + c0);
    const uint2 wv = *reinterpret_cast<const uint2*>(a.v + (size_t)r * a.v_stride + c0);
    uint4 wy[2];
#pragma unroll
    for (uint32_t ry = 0; ry < 2; ++ry) wy[ry] = *reinterpret_cast<const uint4*>(a.y + (size_t)(2u * r + ry) * a.y_stride + x0);
    if (a.a_in) {   // the coverage plane: byte for byte, and an opaque byte beyond the row
#pragma unroll
        for (uint32_t ry = 0; ry < 2; ++ry) {
            const uint32_t y = 2u * r + ry;
            const uint4 wa = *reinterpret_cast<const uint4*>(a.a_in + (size_t)y * a.a_stride + x0);
            uint32_t pa[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) pa[i >> 2] |= ((c0 + (i >> 1) < Wc) ? g_byte16(wa, i) : 255u) << (8u * (i & 3u));
            *reinterpret_cast<uint4*>(a.oa + (size_t)y * a.oa_stride + x0) = make_uint4(pa[0], pa[1], pa[2], pa[3]);
        }
    }
    uint32_t u1[8], v1[8];
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        const uint32_t u = g_byte8(wu, j), v = g_byte8(wv, j);
        if (a.flags & MX_GRADE_CHROMA) {
            const int32_t du = (int32_t)u - 128, dv = (int32_t)v - 128;
            u1[j] = g_clip8(128 + ((a.m_uu * du + a.m_uv * dv + a.off_u + 2048) >> 12));
            v1[j] = g_clip8(128 + ((a.m_vu * du + a.m_vv * dv + a.off_v + 2048) >> 12));
        } else { u1[j] = u; v1[j] = v; }
    }
    uint32_t py[2][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
    uint2 pu = make_uint2(0u, 0u), pv = make_uint2(0u, 0u);
#pragma unroll
    for (uint32_t j = 0; j < 8; ++j) {
        const bool vis = c0 + j < Wc;
        uint32_t y1[4];   // the block's four luma samples: (row 0, col 0), (0, 1), (1, 0), (1, 1)
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t yv = g_byte16(wy[q >> 1], 2u * j + (q & 1u));
            y1[q] = (a.flags & MX_GRADE_CURVE) ? (uint32_t)a.curve[yv] : yv;
        }
        uint32_t uo = u1[j], vo = v1[j];
        if constexpr (MODE != GATHER_NONE) {
            uint32_t n[4], w[4];
            const uint32_t ym = (y1[0] + y1[1] + y1[2] + y1[3] + 2u) >> 2;
            tetra<K>(ym, u1[j], v1[j], n, w);
            uint32_t au = 0u, av = 0u;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) { const uint32_t node = tuv[n[i]]; au += w[i] * (node & 0xffffu); av += w[i] * (node >> 16); }
            uo = lut_round<K>(au); vo = lut_round<K>(av);
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) {
                tetra<K>(y1[q], u1[j], v1[j], n, w);
                uint32_t ay = 0u;
#pragma unroll
                for (uint32_t i = 0; i < 4; ++i) ay += w[i] * (uint32_t)ty[n[i]];
                y1[q] = lut_round<K>(ay);
            }
        }
#pragma unroll
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t i = 2u * j + (q & 1u);
            py[q >> 1][i >> 2] |= (vis ? y1[q] : 0u) << (8u * (i & 3u));   // beyond the row: the blank frame's luma
        }
        const uint32_t bu = (vis ? uo : 0x80u) << (8u * (j & 3u)), bv = (vis ? vo : 0x80u) << (8u * (j & 3u));   // ... and its chroma
        if (j < 4) { pu.x |= bu; pv.x |= bv; } else { pu.y |= bu; pv.y |= bv; }
    }
#pragma unroll
    for (uint32_t ry = 0; ry < 2; ++ry)
        *reinterpret_cast<uint4*>(a.oy + (size_t)(2u * r + ry) * a.oy_stride + x0) = make_uint4(py[ry][0], py[ry][1], py[ry][2], py[ry][3]);
    *reinterpret_cast<uint2*>(a.ou + (size_t)r * a.ou_stride + c0) = pu;
    *reinterpret_cast<uint2*>(a.ov + (size_t)r * a.ov_stride + c0) = pv;
}

template <int MODE, int K>
__global__ __launch_bounds__(GRADE_THREADS) void k_video_grade(const GradeArgs a) {
    if constexpr (MODE == GATHER_LDS) {
        // the whole lattice, LutTables' layout, 16 bytes per lane and step; then every tile this workgroup owns reads it from here
        __shared__ uint4 lds[(GRADE_LDS_Y_BYTES + GRADE_LDS_UV_BYTES) / 16u];
        const uint4* src = reinterpret_cast<const uint4*>(a.lut_y);
        for (uint32_t i = threadIdx.x; i < (GRADE_LDS_Y_BYTES + GRADE_LDS_UV_BYTES) / 16u; i += GRADE_THREADS) lds[i] = src[i];
        __syncthreads();
        const uint16_t* ty = reinterpret_cast<const uint16_t*>(lds);
        const uint32_t* tuv = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(lds) + GRADE_LDS_Y_BYTES);
        for (uint32_t id = blockIdx.x * GRADE_THREADS + threadIdx.x; id < a.n_threads; id += gridDim.x * GRADE_THREADS) {
            const uint32_t r = id / a.chunks_x;
            grade_unit<MODE, K>(a, 8u * (id - r * a.chunks_x), r, ty, tuv);
        }
    } else {
        const uint32_t id = blockIdx.x * GRADE_THREADS + threadIdx.x;
        if (id >= a.n_threads) return;
        const uint32_t r = id / a.chunks_x;
        grade_unit<MODE, K>(a, 8u * (id - r * a.chunks_x), r, a.lut_y, a.lut_uv);
    }
}

// the gather form of the 17-lattice: staged in LDS unless MX_GRADE_GATHER=global asks for the cached reads (tools/grade_cost.py times one against the other)
static bool grade_lds_gather() {
    const char* e = std::getenv("MX_GRADE_GATHER");
    return !(e && std::strcmp(e, "global") == 0);
}

void launch_video_grade(GradeArgs a, hipStream_t s) {
    const uint32_t W = a.width, H = a.height, Wc = W >> 1, Hc = H >> 1;
    if (!W || !H || (W & 1u) || (H & 1u) || W > 16384u || H > 16384u) throw Error(MX_ERR_INVALID, "grade: frame size must be even, non-zero and at most 16384");
    // every access is one aligned 8-byte (chroma) or 16-byte (luma, coverage) word per lane, and a row's last word stays inside the row's stride
    const uint32_t cw8 = (Wc + 7u) & ~7u, lw16 = 2u * cw8;
    if (((uintptr_t)a.u | (uintptr_t)a.v | (uintptr_t)a.ou | (uintptr_t)a.ov | a.u_stride | a.v_stride | a.ou_stride | a.ov_stride) & 7u) throw Error(MX_ERR_INTERNAL, "grade: chroma planes are not 8-byte aligned");
    if (((uintptr_t)a.y | (uintptr_t)a.oy | (uintptr_t)a.oa | (uintptr_t)a.a_in | a.y_stride | a.oy_stride | (a.a_in ? (a.a_stride | a.oa_stride) : 0u)) & 15u) throw Error(MX_ERR_INTERNAL, "grade: luma / coverage planes are not 16-byte aligned");
    if (a.u_stride < cw8 || a.v_stride < cw8 || a.ou_stride < cw8 || a.ov_stride < cw8 || a.y_stride < lw16 || a.oy_stride < lw16 || (a.a_in && (a.a_stride < lw16 || a.oa_stride < lw16)))
        throw Error(MX_ERR_INTERNAL, "grade: a row's last chunk lies beyond the stride");
    if ((a.a_in == nullptr) != (a.oa == nullptr)) throw Error(MX_ERR_INTERNAL, "grade: input and output differ in carrying a coverage plane");
    a.chunks_x = cw8 / 8u;
    a.n_threads = a.chunks_x * Hc;   // <= 1024 x 8192
    const uint32_t tiles = (a.n_threads + GRADE_THREADS - 1u) / GRADE_THREADS;
    if (!(a.flags & MX_GRADE_LUT)) { hipLaunchKernelGGL((k_video_grade<GATHER_NONE, 0>), dim3(tiles), dim3(GRADE_THREADS), 0, s, a); return; }
    if (!a.lut_y || !a.lut_uv || ((uintptr_t)a.lut_y & 15u) || ((uintptr_t)a.lut_uv & 3u)) throw Error(MX_ERR_INTERNAL, "grade: the lattice is missing or misaligned");
    if (a.lut_k == 5u) { hipLaunchKernelGGL((k_video_grade<GATHER_GLOBAL, 5>), dim3(tiles), dim3(GRADE_THREADS), 0, s, a); return; }
    if (a.lut_k != 4u) throw Error(MX_ERR_INTERNAL, "grade: lattice_log2 is neither 4 nor 5");
    if (grade_lds_gather()) {
        if ((const uint8_t*)a.lut_uv != (const uint8_t*)a.lut_y + GRADE_LDS_Y_BYTES) throw Error(MX_ERR_INTERNAL, "grade: the lattice does not have LutTables' layout");
        hipLaunchKernelGGL((k_video_grade<GATHER_LDS, 4>), dim3(min(tiles, GRADE_LDS_MAX_WGS)), dim3(GRADE_THREADS), 0, s, a);
    } else {
        hipLaunchKernelGGL((k_video_grade<GATHER_GLOBAL, 4>), dim3(tiles), dim3(GRADE_THREADS), 0, s, a);
    }
}

}  // namespace mx
