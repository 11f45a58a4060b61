// mx_k_place.hip -- the placer (mixlab_gpu.h mx_video_place): a crop of ONE yuv420p / yuva420p frame resampled into a rectangle of a
// canvas, in ONE launch that writes every byte of the canvas' four planes (Y, coverage, U, V) exactly once -- the rectangle, the transparent surround and the
// stride padding.  Integer arithmetic of the scaler (DESIGN.md "Scaler"), bit-exact against tests/video_place_model.py.
//
// The shape:
//   * a workgroup of 256 owns one 64 x 16 byte tile of one canvas plane (rows are 64-byte aligned, so the tiles of a plane cover its stride exactly and the
//     tile leaves as 64 aligned 16-byte stores, padding included).  The tile is assembled in LDS: first the surround / padding bytes, then the part of the
//     rectangle that falls into it;
//   * LDS-tiled form (tap counts up to MX_PLACE_TAP_BOUND on both axes): the source window of the tile's outputs -- first tap of the first output to last tap
//     of the last one, clamped to the CROP -- is staged once with aligned 4-byte loads (at most 3 bytes either side of the window are fetched and never used);
//     the H pass filters every window row into 16-bit t values in LDS (t + 8192 as u16: the tables' overshoot keeps t within [-8192, 57343], checked on the
//     host per table); the V pass filters down the t columns.  22.5 KB window + 10 KB t rows + 1 KB tile = 33.5 KB: four workgroups a CU (16 waves);
//   * gather form (more taps, or a window beyond the LDS budget): every output sample sums its vn x hn taps straight from the plane.  Slow per sample and
//     rare: a downscale beyond 4:1.
//   * no input coverage: the resampled coverage is 255 (the tables sum to 16384, so resampling a constant 255 gives 255) and nothing is read.
#include "mx_common.hpp"
#include "mx_dev.hpp"
#include "mx_video.hpp"

namespace mx {

static constexpr uint32_t PL_THREADS = 256;
static constexpr uint32_t PL_TW = MX_PLACE_TILE_W, PL_TH = MX_PLACE_TILE_H;
static constexpr uint32_t PL_S_BYTES = 22528;   // the staged window
static constexpr uint32_t PL_T_ROWS = 80;       // window rows the t buffer holds
static constexpr int32_t PL_T_BIAS = 8192;
static_assert(PL_TW == 64 && PL_TH == 16 && PL_THREADS == 256, "the index arithmetic below assumes a 64 x 16 tile and 256 threads");

__device__ __forceinline__ int32_t pl_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint32_t pl_clip8(int32_t acc) { return (uint32_t)pl_clamp((acc + (1 << 20)) >> 21, 0, 255); }

__global__ __launch_bounds__(PL_THREADS) void k_video_place(const PlaceArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t S[PL_S_BYTES];
    __shared__ uint16_t T[PL_T_ROWS * PL_TW];
    __shared__ __attribute__((aligned(16))) uint8_t O[PL_TH * PL_TW];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint32_t pi = (b >= a.p[1].tile_start ? 1u : 0u) + (b >= a.p[2].tile_start ? 1u : 0u) + (b >= a.p[3].tile_start ? 1u : 0u);
    const PlacePlane& p = a.p[pi];
    const uint32_t t = b - p.tile_start, tyi = t / p.tiles_x, txi = t - tyi * p.tiles_x;
    const int32_t X0 = (int32_t)(txi * PL_TW), Y0 = (int32_t)(tyi * PL_TH);

    {   // the surround and the padding
        const uint32_t col = (tid * 4u) & (PL_TW - 1u);
        uint32_t w4 = 0u;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) w4 |= (((uint32_t)X0 + col + k < p.w) ? p.fill : p.pad) << (8u * k);
        reinterpret_cast<uint32_t*>(O)[tid] = w4;
    }
    __syncthreads();

    // the part of the rectangle inside this tile (and inside the canvas), in canvas coordinates
    const int32_t xa = max(max(X0, p.rx), 0), xb = min(min(X0 + (int32_t)PL_TW, p.rx + (int32_t)p.rw), (int32_t)p.w);
    const int32_t ya = max(max(Y0, p.ry), 0), yb = min(min(Y0 + (int32_t)PL_TH, p.ry + (int32_t)p.rh), (int32_t)p.h);
    if (p.rw != 0u && xa < xb && ya < yb) {
        const int32_t oxa = xa - p.rx, oya = ya - p.ry;                       // first output column / row of the rectangle in this tile
        const uint32_t ncols = (uint32_t)(xb - xa), nrows = (uint32_t)(yb - ya);
        uint8_t* const Ot = O + (uint32_t)(ya - Y0) * PL_TW + (uint32_t)(xa - X0);
        const uint32_t j = tid & (PL_TW - 1u);
        if (p.src == nullptr) {
            for (uint32_t r = tid >> 6; r < nrows; r += PL_THREADS / PL_TW)
                if (j < ncols) Ot[r * PL_TW + j] = 255u;
        } else {
            const int32_t cw1 = (int32_t)p.cw - 1, ch1 = (int32_t)p.ch - 1;
            // the source window, clamped to the crop (the first-tap index never decreases along an axis)
            const int32_t sx0 = pl_clamp(p.hfirst[oxa], 0, cw1), sx1 = pl_clamp(p.hfirst[oxa + (int32_t)ncols - 1] + (int32_t)p.hn - 1, 0, cw1);
            const int32_t sy0 = pl_clamp(p.vfirst[oya], 0, ch1), sy1 = pl_clamp(p.vfirst[oya + (int32_t)nrows - 1] + (int32_t)p.vn - 1, 0, ch1);
            const uint32_t wc = (uint32_t)(sx1 - sx0 + 1), wr = (uint32_t)(sy1 - sy0 + 1);
            const uint32_t al = (p.cx + (uint32_t)sx0) & 3u, pitch = (wc + al + 3u) & ~3u;
            const uint8_t* const srow = p.src + (size_t)(p.cy + (uint32_t)sy0) * p.src_stride;   // window row 0, plane column 0
            if (p.tiled && sx1 >= sx0 && sy1 >= sy0 && wr <= PL_T_ROWS && pitch * wr <= PL_S_BYTES) {
                // stage: aligned words from (cx + sx0) & ~3; a row's last word ends at most at the plane width rounded up to 4, inside the stride
                const uint32_t wpr = pitch >> 2, n_words = wpr * wr;
                const uint8_t* const wbase = srow + ((p.cx + (uint32_t)sx0) & ~3u);
                for (uint32_t i = tid; i < n_words; i += PL_THREADS) {
                    const uint32_t r = i / wpr, c = i - r * wpr;
                    reinterpret_cast<uint32_t*>(S)[i] = *reinterpret_cast<const uint32_t*>(wbase + (size_t)r * p.src_stride + 4u * c);
                }
                __syncthreads();
                // H pass: thread (j, r mod 4) filters column j of window rows r, r + 4, ...
                if (j < ncols) {
                    const int32_t f = p.hfirst[oxa + (int32_t)j];
                    const int32_t* const hc = p.hcoef + (size_t)(oxa + (int32_t)j) * p.hn;
                    const int32_t off = (int32_t)al - sx0;
                    for (uint32_t r = tid >> 6; r < wr; r += PL_THREADS / PL_TW) {
                        const uint8_t* const row = S + r * pitch;
                        int32_t acc = 0;
                        for (uint32_t k = 0; k < p.hn; ++k) acc += hc[k] * (int32_t)row[pl_clamp(f + (int32_t)k, sx0, sx1) + off];
                        T[r * PL_TW + j] = (uint16_t)(((acc + 64) >> 7) + PL_T_BIAS);
                    }
                }
                __syncthreads();
                // V pass
                if (j < ncols) {
                    for (uint32_t r = tid >> 6; r < nrows; r += PL_THREADS / PL_TW) {
                        const int32_t f = p.vfirst[oya + (int32_t)r];
                        const int32_t* const vc = p.vcoef + (size_t)(oya + (int32_t)r) * p.vn;
                        int32_t acc = 0;
                        for (uint32_t k = 0; k < p.vn; ++k) acc += vc[k] * ((int32_t)T[(uint32_t)(pl_clamp(f + (int32_t)k, sy0, sy1) - sy0) * PL_TW + j] - PL_T_BIAS);
                        Ot[r * PL_TW + j] = (uint8_t)pl_clip8(acc);
                    }
                }
            } else if (j < ncols) {
                const int32_t hf = p.hfirst[oxa + (int32_t)j];
                const int32_t* const hc = p.hcoef + (size_t)(oxa + (int32_t)j) * p.hn;
                const uint8_t* const plane = p.src + (size_t)p.cy * p.src_stride + p.cx;   // the crop's origin
                for (uint32_t r = tid >> 6; r < nrows; r += PL_THREADS / PL_TW) {
                    const int32_t vf = p.vfirst[oya + (int32_t)r];
                    const int32_t* const vc = p.vcoef + (size_t)(oya + (int32_t)r) * p.vn;
                    int32_t acc = 0;
                    for (uint32_t kv = 0; kv < p.vn; ++kv) {
                        const uint8_t* const row = plane + (size_t)pl_clamp(vf + (int32_t)kv, 0, ch1) * p.src_stride;
                        int32_t h = 0;
                        for (uint32_t kh = 0; kh < p.hn; ++kh) h += hc[kh] * (int32_t)row[pl_clamp(hf + (int32_t)kh, 0, cw1)];
                        acc += vc[kv] * ((h + 64) >> 7);
                    }
                    Ot[r * PL_TW + j] = (uint8_t)pl_clip8(acc);
                }
            }
        }
    }
    __syncthreads();
    if (tid < PL_TH * PL_TW / 16u) {
        const uint32_t row = tid >> 2, q = tid & 3u, y = (uint32_t)Y0 + row;
        if (y < p.h) *reinterpret_cast<uint4*>(p.dst + (size_t)y * p.dst_stride + (uint32_t)X0 + 16u * q) = reinterpret_cast<const uint4*>(O)[tid];
    }
}

void launch_video_place(PlaceArgs a, hipStream_t s) {
    uint32_t total = 0;
    for (int i = 0; i < 4; ++i) {
        PlacePlane& p = a.p[i];
        if (!p.dst || !p.w || !p.h) throw Error(MX_ERR_INTERNAL, "place: a canvas plane is missing");
        // the tiles of a plane cover its stride exactly, and every tile row leaves as aligned 16-byte stores
        if (((uintptr_t)p.dst & 15u) || (p.dst_stride % PL_TW) || p.dst_stride < p.w) throw Error(MX_ERR_INTERNAL, "place: canvas rows are not 64-byte aligned");
        if (p.src && (((uintptr_t)p.src | p.src_stride) & 3u)) throw Error(MX_ERR_INTERNAL, "place: input rows are not 4-byte aligned");
        if (p.rw) {
            if (p.rx >= (int32_t)p.w || p.ry >= (int32_t)p.h || p.rx + (int64_t)p.rw <= 0 || p.ry + (int64_t)p.rh <= 0 || p.rw > 16384u || p.rh > 16384u || !p.rh)
                throw Error(MX_ERR_INTERNAL, "place: the rectangle does not meet the canvas");
            if (!p.hfirst || !p.hcoef || !p.vfirst || !p.vcoef || !p.hn || !p.vn || !p.cw || !p.ch) throw Error(MX_ERR_INTERNAL, "place: tap tables are missing");
            // the staged window reads whole aligned words: the crop's last word stays inside the row's stride
            if (p.src && ((p.cx + p.cw + 3u) & ~3u) > p.src_stride) throw Error(MX_ERR_INTERNAL, "place: the crop lies beyond the input's stride");
        }
        p.tiles_x = p.dst_stride / PL_TW;
        p.tile_start = total;
        total += p.tiles_x * ((p.h + PL_TH - 1u) / PL_TH);
    }
    hipLaunchKernelGGL(k_video_place, dim3(total), dim3(PL_THREADS), 0, s, a);
}

}  // namespace mx
