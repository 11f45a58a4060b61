// mx_k_multiview.hip -- the multiviewer (mixlab_gpu.h mx_video_multiview): up to 16 yuv420p frames, each resampled into its own
// rectangle of ONE opaque canvas with a tally frame round it, in ONE launch that writes every byte of the canvas' three planes exactly once -- pictures,
// blanks, frames, background and stride padding.  Integer arithmetic of the scaler (DESIGN.md "Scaler"), bit-exact against tests/video_multiview_model.py.
//
// The shape is the placer's (mx_k_place.hip), and the differences are the work:
//   * a workgroup of 256 owns one 64 x 16 byte tile of one canvas plane and assembles it in LDS; thread (tid & 63, tid >> 6) owns column tid & 63 of rows
//     tid >> 6, + 4, + 8, + 12 of the tile and is the only one that ever writes those four bytes -- background, then frame / blank, then picture, in program
//     order -- so the views of a tile need no barrier between their fills;
//   * the workgroup walks the views (descriptors in device memory: 16 views x 3 planes do not fit by-value kernel arguments; every test on them is
//     workgroup-uniform) and resamples the part of each picture rectangle that falls into its tile;
//   * LDS-tiled form (tap counts up to MX_MULTIVIEW_TAP_BOUND on both axes): the source window of the tile's outputs is staged once with aligned 4-byte
//     loads, the tile's COEFFICIENTS are staged too (as i16: the host checks every coefficient of a table it marks `tiled`) -- the
//     horizontal ones transposed [tap][column] behind three zeros and in front of three, so a lane can walk its window row in aligned WORDS, four taps per
//     LDS read, whatever the alignment of its first tap; lanes whose taps clamp at the plane's edge take the byte walk of the placer.  H pass into 16-bit
//     t rows (t + 8192 as u16), then the V pass down the t columns.  The bound is 20 taps, not the placer's 18: a 4 x 4 of 1080p sources on a 1080p canvas is
//     4:1 = 18 taps only without tally frames; with them the pictures are a little smaller (4.1 - 4.2:1, 20 taps), and that is the common case.  23.5 KB window +
//     10.5 KB t + 1 KB tile + 4.2 KB coefficients = 40 128 bytes: still four workgroups a CU (a tile whose window does not fit -- beyond about 4.2:1 -- gathers);
//   * gather form (more taps, or a window beyond the LDS budget -- tested per tile before any LDS index is formed): every output sample sums its vn x hn
//     taps straight from the plane.  Slow by construction: a downscale beyond 4:1.
#include <cstring>
#include <map>
#include <mutex>

#include "mx_common.hpp"
#include "mx_dev.hpp"
#include "mx_video.hpp"

namespace mx {

static constexpr uint32_t MV_THREADS = 256;
static constexpr int32_t MV_TW = MX_MULTIVIEW_TILE_W, MV_TH = MX_MULTIVIEW_TILE_H;
static constexpr uint32_t MV_TB = MX_MULTIVIEW_TAP_BOUND;
static constexpr uint32_t MV_S_BYTES = 24064;   // the staged window
static constexpr uint32_t MV_T_ROWS = 84;       // window rows the t buffer holds
static constexpr uint32_t MV_HC_ROWS = MV_TB + 6;   // three zeros, the taps, three zeros
static constexpr int32_t MV_T_BIAS = 8192;
static_assert(MV_TW == 64 && MV_TH == 16 && MV_THREADS == 256, "the index arithmetic below assumes a 64 x 16 tile and 256 threads");

static constexpr uint32_t MV_MAX_WORDS = (3 + MV_TB + 3) / 4;   // aligned words a lane's taps can touch
typedef short mv_s16x2 __attribute__((ext_vector_type(2)));
// two source bytes (as 16-bit halves of `bytes`) times two coefficients, added to acc: one V_DOT2_I32_I16
__device__ __forceinline__ int32_t mv_dot2(uint32_t bytes, mv_s16x2 c, int32_t acc) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(mv_s16x2, bytes), c, acc, false);
}
__device__ __forceinline__ int32_t mv_clamp(int32_t v, int32_t lo, int32_t hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ uint32_t mv_clip8(int32_t acc) { return (uint32_t)mv_clamp((acc + (1 << 20)) >> 21, 0, 255); }

__global__ __launch_bounds__(MV_THREADS) void k_video_multiview(const MvArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t S[MV_S_BYTES];
    __shared__ uint16_t T[MV_T_ROWS * MV_TW];
    __shared__ __attribute__((aligned(16))) uint8_t O[MV_TH * MV_TW];
    __shared__ int16_t HC[MV_HC_ROWS * MV_TW];   // [3 + tap][column of the picture part]
    __shared__ int16_t VC[MV_TH * MV_TB];        // [row of the picture part][tap]
    __shared__ int32_t HF[MV_TW];
    __shared__ int32_t VF[MV_TH];
    const uint32_t tid = threadIdx.x, b = blockIdx.x;
    const uint32_t pi = (b >= a.p[1].tile_start ? 1u : 0u) + (b >= a.p[2].tile_start ? 1u : 0u);
    const MvPlane& p = a.p[pi];
    const uint32_t t = b - p.tile_start, tyi = t / p.tiles_x, txi = t - tyi * p.tiles_x;
    const int32_t X0 = (int32_t)txi * MV_TW, Y0 = (int32_t)tyi * MV_TH;
    const int32_t col = (int32_t)(tid & 63u), row0 = (int32_t)(tid >> 6);
    const int32_t x = X0 + col;
    uint8_t* const Oc = O + row0 * MV_TW + col;   // this thread's bytes: Oc[4 i * MV_TW]

    {   // the background and the padding
        const uint8_t fill = (uint8_t)(x < (int32_t)p.w ? p.bg : p.pad);
#pragma unroll
        for (int32_t i = 0; i < 4; ++i) Oc[4 * i * MV_TW] = fill;
    }

    for (uint32_t vi = 0; vi < a.n_views; ++vi) {
        const MvView& v = a.views[vi * 3u + pi];
        if (max(X0, v.rx) >= min(X0 + MV_TW, v.rx + v.rw) || max(Y0, v.ry) >= min(Y0 + MV_TH, v.ry + v.rh)) continue;
        // the frame and the blank of the inner rectangle
        if (x >= v.rx && x < v.rx + v.rw) {
            const bool in_x = x >= v.rx + v.bt && x < v.rx + v.rw - v.bt;
#pragma unroll
            for (int32_t i = 0; i < 4; ++i) {
                const int32_t y = Y0 + row0 + 4 * i;
                if (y >= v.ry && y < v.ry + v.rh) Oc[4 * i * MV_TW] = (uint8_t)((in_x && y >= v.ry + v.bt && y < v.ry + v.rh - v.bt) ? p.blank : v.border);
            }
        }
        if (v.src == nullptr || v.pw <= 0) continue;
        // the part of the picture rectangle inside this tile, in canvas coordinates
        const int32_t xa = max(X0, v.px), xb = min(X0 + MV_TW, v.px + v.pw), ya = max(Y0, v.py), yb = min(Y0 + MV_TH, v.py + v.ph);
        if (xa >= xb || ya >= yb) continue;
        const int32_t oxa = xa - v.px, oya = ya - v.py;                  // first output column / row of the picture in this tile
        const int32_t ncols = xb - xa, nrows = yb - ya;
        const bool mine = x >= xa && x < xb;
        const int32_t j = x - xa;                                        // this thread's column of the picture part (when mine)
        const int32_t sw1 = (int32_t)v.sw - 1, sh1 = (int32_t)v.sh - 1, hn = (int32_t)v.hn, vn = (int32_t)v.vn;
        // the source window, clamped to the plane (the first-tap index never decreases along an axis)
        const int32_t sx0 = mv_clamp(v.hfirst[oxa], 0, sw1), sx1 = mv_clamp(v.hfirst[oxa + ncols - 1] + hn - 1, 0, sw1);
        const int32_t sy0 = mv_clamp(v.vfirst[oya], 0, sh1), sy1 = mv_clamp(v.vfirst[oya + nrows - 1] + vn - 1, 0, sh1);
        const uint32_t wc = (uint32_t)(sx1 - sx0 + 1), wr = (uint32_t)(sy1 - sy0 + 1);
        const uint32_t al = (uint32_t)sx0 & 3u, pitch = (wc + al + 3u) & ~3u;
        if (v.tiled && hn <= (int32_t)MV_TB && vn <= (int32_t)MV_TB && sx1 >= sx0 && sy1 >= sy0 && wr <= MV_T_ROWS && pitch * wr <= MV_S_BYTES) {
            __syncthreads();   // the view before this one is done with the buffers
            {   // stage the window: aligned words from sx0 & ~3; a row's last word ends at most at the plane width rounded up to 4, inside the stride
                const uint32_t wpr = pitch >> 2, n_words = wpr * wr;
                const uint8_t* const wbase = v.src + (size_t)sy0 * v.src_stride + ((uint32_t)sx0 & ~3u);
                for (uint32_t i = tid; i < n_words; i += MV_THREADS) {
                    const uint32_t r = i / wpr, c = i - r * wpr;
                    reinterpret_cast<uint32_t*>(S)[i] = *reinterpret_cast<const uint32_t*>(wbase + (size_t)r * v.src_stride + 4u * c);
                }
            }
            // ... and the coefficients
            for (uint32_t i = tid; i < ((uint32_t)hn + 6u) * MV_TW; i += MV_THREADS) {
                const int32_t k = (int32_t)(i >> 6) - 3, c = (int32_t)(i & 63u);
                HC[i] = (int16_t)((c < ncols && k >= 0 && k < hn) ? v.hcoef[(size_t)(oxa + c) * v.hn + (uint32_t)k] : 0);
            }
            for (uint32_t i = tid; i < (uint32_t)(nrows * vn); i += MV_THREADS) {
                const uint32_t r = i / v.vn, k = i - r * v.vn;
                VC[r * MV_TB + k] = (int16_t)v.vcoef[(size_t)(oya + (int32_t)r) * v.vn + k];
            }
            if ((int32_t)tid < ncols) HF[tid] = v.hfirst[oxa + (int32_t)tid];
            if ((int32_t)tid < nrows) VF[tid] = v.vfirst[oya + (int32_t)tid];
            __syncthreads();
            // H pass: thread (j, r mod 4) filters column j of window rows r, r + 4, ...
            if (mine) {
                const int32_t f = HF[j];
                const int32_t off = (int32_t)al - sx0;
                const int16_t* const hc = HC + j;
                if (f >= sx0 && f + hn - 1 <= sx1) {   // no tap clamps: the row is read in aligned words; the zeros round the taps take the bytes that are none of them
                    const int32_t start = f + off, q0 = start & ~3, kb = 3 - (start & 3);
                    const int32_t nw = ((start & 3) + hn + 3) >> 2;
                    // the lane's coefficients leave LDS once, not once per window row: per word the pairs (byte 0, byte 2) and (byte 1, byte 3), two 16-bit
                    // dot products a word; a word beyond the lane's last has no coefficients and is not read
                    mv_s16x2 c02[MV_MAX_WORDS], c13[MV_MAX_WORDS];
#pragma unroll
                    for (int32_t wi = 0; wi < (int32_t)MV_MAX_WORDS; ++wi) {
                        c02[wi] = mv_s16x2{0, 0}; c13[wi] = mv_s16x2{0, 0};
                        if (wi < nw) {
                            const int16_t* const c4 = hc + (kb + 4 * wi) * MV_TW;
                            c02[wi] = mv_s16x2{c4[0], c4[2 * MV_TW]}; c13[wi] = mv_s16x2{c4[MV_TW], c4[3 * MV_TW]};
                        }
                    }
                    for (uint32_t r = (uint32_t)row0; r < wr; r += MV_THREADS / MV_TW) {
                        const uint8_t* const row = S + r * pitch + q0;
                        int32_t acc = 0;
#pragma unroll
                        for (int32_t wi = 0; wi < (int32_t)MV_MAX_WORDS; ++wi) {
                            if (wi < nw) {
                                const uint32_t w = *reinterpret_cast<const uint32_t*>(row + 4 * wi);
                                acc = mv_dot2(w & 0x00ff00ffu, c02[wi], acc);
                                acc = mv_dot2((w >> 8) & 0x00ff00ffu, c13[wi], acc);
                            }
                        }
                        T[r * MV_TW + (uint32_t)j] = (uint16_t)(((acc + 64) >> 7) + MV_T_BIAS);
                    }
                } else {
                    for (uint32_t r = (uint32_t)row0; r < wr; r += MV_THREADS / MV_TW) {
                        const uint8_t* const row = S + r * pitch;
                        int32_t acc = 0;
                        for (int32_t k = 0; k < hn; ++k) acc += (int32_t)hc[(k + 3) * MV_TW] * (int32_t)row[mv_clamp(f + k, sx0, sx1) + off];
                        T[r * MV_TW + (uint32_t)j] = (uint16_t)(((acc + 64) >> 7) + MV_T_BIAS);
                    }
                }
            }
            __syncthreads();
            // V pass
            if (mine) {
#pragma unroll
                for (int32_t i = 0; i < 4; ++i) {
                    const int32_t y = Y0 + row0 + 4 * i;
                    if (y < ya || y >= yb) continue;
                    const int32_t r = y - ya, f = VF[r];
                    const int16_t* const vc = VC + r * (int32_t)MV_TB;
                    int32_t acc = 0;
                    for (int32_t k = 0; k < vn; ++k) acc += (int32_t)vc[k] * ((int32_t)T[(uint32_t)(mv_clamp(f + k, sy0, sy1) - sy0) * MV_TW + (uint32_t)j] - MV_T_BIAS);
                    Oc[4 * i * MV_TW] = (uint8_t)mv_clip8(acc);
                }
            }
        } else if (mine) {
            const int32_t hf = v.hfirst[oxa + j];
            const int32_t* const hc = v.hcoef + (size_t)(oxa + j) * v.hn;
#pragma unroll 1
            for (int32_t i = 0; i < 4; ++i) {
                const int32_t y = Y0 + row0 + 4 * i;
                if (y < ya || y >= yb) continue;
                const int32_t vf = v.vfirst[y - v.py];
                const int32_t* const vc = v.vcoef + (size_t)(y - v.py) * v.vn;
                int32_t acc = 0;
                for (int32_t kv = 0; kv < vn; ++kv) {
                    const uint8_t* const row = v.src + (size_t)mv_clamp(vf + kv, 0, sh1) * v.src_stride;
                    int32_t h = 0;
                    for (int32_t kh = 0; kh < hn; ++kh) h += hc[kh] * (int32_t)row[mv_clamp(hf + kh, 0, sw1)];
                    acc += vc[kv] * ((h + 64) >> 7);
                }
                Oc[4 * i * MV_TW] = (uint8_t)mv_clip8(acc);
            }
        }
    }
    __syncthreads();
    if (tid < (uint32_t)(MV_TH * MV_TW) / 16u) {
        const uint32_t row = tid >> 2, q = tid & 3u, y = (uint32_t)Y0 + row;
        if (y < p.h) *reinterpret_cast<uint4*>(p.dst + (size_t)y * p.dst_stride + (uint32_t)X0 + 16u * q) = reinterpret_cast<const uint4*>(O)[tid];
    }
}

// Descriptor staging per (device, stream): a small ring of page-locked blocks with their device copies.  A slot is rewritten only after the launch that
// read it has finished; the copy goes out on the launch's own stream, in front of it.
namespace {
constexpr size_t MV_DESC_BYTES = sizeof(MvView) * 3 * 16;
struct MvSlot { uint8_t* host = nullptr; uint8_t* dev = nullptr; hipEvent_t done = nullptr; bool used = false; };
struct MvRing { MvSlot slot[4]; uint32_t next = 0; };
std::mutex g_mv_mu;
std::map<std::pair<int, hipStream_t>, MvRing> g_mv;
}  // namespace

void multiview_stream_retired(hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_mv_mu);
    for (auto it = g_mv.begin(); it != g_mv.end();) {
        if (it->first.second != s) { ++it; continue; }
        for (MvSlot& c : it->second.slot) {
            if (c.used) (void)hipEventSynchronize(c.done);
            if (c.host) (void)hipHostFree(c.host);
            if (c.dev) (void)hipFree(c.dev);
            if (c.done) (void)hipEventDestroy(c.done);
        }
        it = g_mv.erase(it);
    }
}

void launch_video_multiview(MvArgs a, const MvView* views, hipStream_t s) {
    if (!views || a.n_views == 0 || a.n_views > 16u) throw Error(MX_ERR_INTERNAL, "multiview: 1 .. 16 views");
    uint32_t total = 0;
    for (int i = 0; i < 3; ++i) {
        MvPlane& p = a.p[i];
        if (!p.dst || !p.w || !p.h) throw Error(MX_ERR_INTERNAL, "multiview: a canvas plane is missing");
        // the tiles of a plane cover its stride exactly, and every tile row leaves as aligned 16-byte stores
        if (((uintptr_t)p.dst & 15u) || (p.dst_stride % (uint32_t)MV_TW) || p.dst_stride < p.w) throw Error(MX_ERR_INTERNAL, "multiview: canvas rows are not 64-byte aligned");
        for (uint32_t k = 0; k < a.n_views; ++k) {
            const MvView& v = views[k * 3u + (uint32_t)i];
            if (v.rw <= 0 || v.rh <= 0 || v.rx < 0 || v.ry < 0 || v.rx + (int64_t)v.rw > (int64_t)p.w || v.ry + (int64_t)v.rh > (int64_t)p.h || v.bt < 0 || 2 * (int64_t)v.bt >= v.rw || 2 * (int64_t)v.bt >= v.rh)
                throw Error(MX_ERR_INTERNAL, "multiview: a view does not lie inside the canvas");
            if (!v.src || v.pw <= 0) continue;
            if (v.ph <= 0 || v.px < v.rx + v.bt || v.py < v.ry + v.bt || v.px + (int64_t)v.pw > (int64_t)v.rx + v.rw - v.bt || v.py + (int64_t)v.ph > (int64_t)v.ry + v.rh - v.bt)
                throw Error(MX_ERR_INTERNAL, "multiview: a picture rectangle does not lie inside its view");
            if (!v.hfirst || !v.hcoef || !v.vfirst || !v.vcoef || !v.hn || !v.vn || !v.sw || !v.sh) throw Error(MX_ERR_INTERNAL, "multiview: tap tables are missing");
            // the staged window reads whole aligned words: the plane's last word stays inside the row's stride
            if ((((uintptr_t)v.src | v.src_stride) & 3u) || ((v.sw + 3u) & ~3u) > v.src_stride) throw Error(MX_ERR_INTERNAL, "multiview: input rows are not 4-byte aligned");
        }
        p.tiles_x = p.dst_stride / (uint32_t)MV_TW;
        p.tile_start = total;
        total += p.tiles_x * ((p.h + (uint32_t)MV_TH - 1u) / (uint32_t)MV_TH);
    }
    int dev = 0;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    std::lock_guard<std::mutex> lk(g_mv_mu);
    MvRing& ring = g_mv[{dev, s}];
    MvSlot& sl = ring.slot[ring.next];
    ring.next = (ring.next + 1u) % 4u;
    if (!sl.host) {
        hip_check(hipHostMalloc((void**)&sl.host, MV_DESC_BYTES, hipHostMallocDefault), "hipHostMalloc(multiview descriptors)");
        hip_check(hipMalloc((void**)&sl.dev, MV_DESC_BYTES), "hipMalloc(multiview descriptors)");
        hip_check(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming), "hipEventCreate");
    }
    if (sl.used) hip_check(hipEventSynchronize(sl.done), "hipEventSynchronize(multiview descriptors)");   // the last launch that read it
    const size_t bytes = sizeof(MvView) * 3u * a.n_views;
    std::memcpy(sl.host, views, bytes);
    hip_check(hipMemcpyAsync(sl.dev, sl.host, bytes, hipMemcpyHostToDevice, s), "hipMemcpyAsync(multiview descriptors)");
    a.views = reinterpret_cast<const MvView*>(sl.dev);
    hipLaunchKernelGGL(k_video_multiview, dim3(total), dim3(MV_THREADS), 0, s, a);
    hip_check(hipEventRecord(sl.done, s), "hipEventRecord");
    sl.used = true;
}

}  // namespace mx
