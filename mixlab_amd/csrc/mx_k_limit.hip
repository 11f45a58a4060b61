// mx_k_limit.hip -- look-ahead limiter taps on audio output ports (mixlab_gpu.h mx_graph_set_limiters): once per run,
// for every tap, a limited copy of the port delayed by the lookahead D, and one record per tick.
//
// k_limit_init  one thread per (tap, tick): the record before any frame has been counted -- min_gain 1.0, peak_out +0.0, the counts 0, frames
//               and channels.  k_limit's workgroups add to it with integer atomics, so it must run first on the same stream.
// k_limit       one workgroup per (tap, tile of LIMIT_TILE frames of the run).  Output frame n needs the input frames n - 2 D .. n, so the
//               workgroup stages the tile behind a run-in of 2 D frames: frames of the run come from the port, whose ticks lie back to back in
//               its buffer, frames before the run's first from the tap's carried history.  In LDS:
//                 A  r[] of the run-in and the tile; then, in place, the minimum over the last 2^b frames (b = floor(log2(D + 1)), b passes of
//                    a[i] = min(a[i], a[i - s]), s = 1, 2, 4, ..: every lane reads its LIMIT_TILE / 256 + 4 elements, the workgroup meets, every
//                    lane writes);
//                 B  m[] = min(a[i], a[i - (D + 1 - 2^b)]): two overlapping windows of 2^b cover D + 1 frames.  A minimum is exact in any order.
//               Then every lane takes frames lane, lane + 256, ..: the (D + 1)-tap sum in the spec's order with 8 independent accumulators, the
//               weight read uniformly, m[] conflict-free (consecutive lanes, consecutive words) -- skipped by a wave none of whose frames has
//               anything to limit within 2 D frames (q == 1: the result would not be used).  r[n - D] is evaluated again from the delayed input
//               frame, which the output needs anyway.  The copy is written in the port's logical layout (a dup-stored port as interleaved
//               stereo).  Record: a wave whose 64 consecutive frames lie in one tick reduces across its lanes and adds once; a wave across
//               a tick boundary (or ticks shorter than a wave) adds per lane.  The identity is never added.  The workgroup of a tap's last
//               tile writes the history the next run reads, out of place: the last 2 D frames of the stream, which for a run shorter than that
//               are the old history shifted.
//
// Arithmetic: every product and sum is one f32 operation rounded on its own (-ffp-contract=off); the division is the correctly rounded
// f32 division (the default of the compiler for HIP; the quotient is normal by the spec's cap).  f32 subnormals reach the kernel unflushed.
#include "mx_dev.hpp"

namespace mx {

static constexpr uint32_t LIMIT_THREADS = 256, LIMIT_PER_LANE = LIMIT_TILE / LIMIT_THREADS;                          // 8 frames per lane
static constexpr uint32_t LIMIT_A = LIMIT_TILE + LIMIT_HIST_FRAMES, LIMIT_B = LIMIT_TILE + LIMIT_MAX_LOOKAHEAD;      // LDS floats
static constexpr uint32_t LIMIT_A_PER_LANE = LIMIT_A / LIMIT_THREADS;                                                // 12
static_assert(LIMIT_TILE % LIMIT_THREADS == 0 && LIMIT_A % LIMIT_THREADS == 0, "whole elements per lane");

// frame j of the run (j >= -H: the history holds frame -H + h at h) as (L, R); a mono or dup-stored port gives its one float twice
__device__ __forceinline__ float2 limit_frame(const LimitDesc& d, const float2* __restrict__ hin, uint32_t H, int64_t j) {
    if (j < 0) return hin[(int64_t)H + j];
    if (d.layout == METER_STEREO) return reinterpret_cast<const float2*>(d.p)[j];   // 8-byte aligned, as k_meter_reduce's
    const float v = d.p[j];
    return make_float2(v, v);
}

// the spec's required gain of one frame
__device__ __forceinline__ float limit_r(float2 x, float c) {
    const uint32_t a = max(__float_as_uint(x.x) & 0x7fffffffu, __float_as_uint(x.y) & 0x7fffffffu);
    if (a >= 0x7f800000u) return 0.0f;
    const float af = __uint_as_float(a);
    if (af <= c) return 1.0f;
    return c / fminf(af, 65536.0f);
}

__global__ __launch_bounds__(256) void k_limit_init(const LimitRun r) {
    const uint64_t total = (uint64_t)r.n * r.n_ticks;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * 256u) {
        const uint32_t i = (uint32_t)(idx / r.n_ticks), t = (uint32_t)(idx - (uint64_t)i * r.n_ticks);
        const LimitDesc d = r.desc[i];
        r.rec[(size_t)t * r.stride + d.slot] = LimitTick{1.0f, 0.0f, 0u, 0u, d.frames, d.channels};
    }
}

__global__ __launch_bounds__(LIMIT_THREADS) void k_limit(const LimitRun r, uint32_t tiles_per_tap) {
    __shared__ float A[LIMIT_A];
    __shared__ float B[LIMIT_B];
    const uint32_t tid = threadIdx.x;
    const uint32_t D = r.lookahead, H = 2u * D, W = D + 1u;
    const uint32_t b = 31u - (uint32_t)__clz((int)W), rem = W - (1u << b);
    const float c = r.ceiling;
    const uint64_t total = (uint64_t)r.n * tiles_per_tap;
    for (uint64_t w = blockIdx.x; w < total; w += gridDim.x) {   // workgroup-uniform
        const uint32_t i = (uint32_t)(w / tiles_per_tap), tile = (uint32_t)(w - (uint64_t)i * tiles_per_tap);
        const LimitDesc d = r.desc[i];
        const uint32_t F = d.frames, C = d.channels;
        const uint64_t N = (uint64_t)F * r.n_ticks, t0 = (uint64_t)tile * LIMIT_TILE;
        const float2* __restrict__ hin = r.hist_in + (size_t)d.slot * LIMIT_HIST_FRAMES;
        float2* __restrict__ hout = r.hist_out + (size_t)d.slot * LIMIT_HIST_FRAMES;
        if (N == 0) {   // a tap without frames: the history stays what it is
            if (tile == 0) for (uint32_t h = tid; h < H; h += LIMIT_THREADS) hout[h] = hin[h];
            continue;
        }
        if (t0 >= N) continue;
        const uint32_t len = N - t0 < LIMIT_TILE ? (uint32_t)(N - t0) : LIMIT_TILE, L = len + H;
        __syncthreads();   // the previous tile of this workgroup is done with A and B
        for (uint32_t idx = tid; idx < L; idx += LIMIT_THREADS) A[idx] = limit_r(limit_frame(d, hin, H, (int64_t)t0 - H + idx), c);
        __syncthreads();
        for (uint32_t s = 1; s < (1u << b); s <<= 1) {
            float v[LIMIT_A_PER_LANE];
#pragma unroll
            for (uint32_t u = 0; u < LIMIT_A_PER_LANE; ++u) {
                const uint32_t idx = tid + LIMIT_THREADS * u;
                if (idx < L) v[u] = idx >= s ? fminf(A[idx], A[idx - s]) : A[idx];
            }
            __syncthreads();
#pragma unroll
            for (uint32_t u = 0; u < LIMIT_A_PER_LANE; ++u) {
                const uint32_t idx = tid + LIMIT_THREADS * u;
                if (idx < L) A[idx] = v[u];
            }
            __syncthreads();
        }
        for (uint32_t idx = tid; idx < len + D; idx += LIMIT_THREADS) B[idx] = fminf(A[idx + D], A[idx + D - rem]);   // m of frame t0 - D + idx
        __syncthreads();

        // the tile's first frame in ticks; a lane's frame is e = rem0 + f frames behind that tick's first (F <= 2^30: no overflow)
        const uint64_t tick0 = t0 / F;
        const uint32_t rem0 = (uint32_t)(t0 - tick0 * F);
        float q[LIMIT_PER_LANE], acc[LIMIT_PER_LANE];
        bool any = false;
#pragma unroll
        for (uint32_t u = 0; u < LIMIT_PER_LANE; ++u) {
            const uint32_t f = tid + LIMIT_THREADS * u;
            q[u] = f < len ? fminf(B[f + D], B[f]) : 1.0f;
            acc[u] = 0.0f;
            any = any || q[u] != 1.0f;
        }
        if (any) {
            const float* __restrict__ wt = r.weights;
            for (uint32_t k = 0; k <= D; ++k) {
                const float wk = wt[k];   // uniform
#pragma unroll
                for (uint32_t u = 0; u < LIMIT_PER_LANE; ++u) {
                    const float p = wk * B[tid + LIMIT_THREADS * u + D - k];
                    acc[u] = acc[u] + p;
                }
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < LIMIT_PER_LANE; ++u) {
            if (LIMIT_THREADS * u >= len) break;   // workgroup-uniform: every lane's frame lies past the tile
            const uint32_t f = tid + LIMIT_THREADS * u;
            const bool valid = f < len;
            uint32_t gb = 0x3f800000u, pk = 0u, lim = 0u, bad = 0u, tk = 0u;
            if (valid) {
                const float2 x = limit_frame(d, hin, H, (int64_t)t0 + f - D);
                const float g = q[u] == 1.0f ? 1.0f : fminf(acc[u], limit_r(x, c));
                const bool okl = (__float_as_uint(x.x) & 0x7f800000u) != 0x7f800000u, okr = (__float_as_uint(x.y) & 0x7f800000u) != 0x7f800000u;
                const float yl = okl ? fmaxf(-c, fminf(c, x.x * g)) : 0.0f;
                const float yr = okr ? fmaxf(-c, fminf(c, x.y * g)) : 0.0f;
                const uint32_t e = rem0 + f, dt = e / F, fi = e - dt * F;
                tk = (uint32_t)(tick0 + dt);
                float* o = r.out + (size_t)tk * r.tick_floats + d.off + (size_t)fi * C;
                o[0] = yl;
                if (C == 2) o[1] = yr;   // (two stores: a tap's copy starts on any float)
                gb = __float_as_uint(g);
                pk = __float_as_uint(yl) & 0x7fffffffu;
                bad = okl ? 0u : 1u;
                if (C == 2) { pk = max(pk, __float_as_uint(yr) & 0x7fffffffu); bad += okr ? 0u : 1u; }
                lim = g < 1.0f ? 1u : 0u;
            }
            // lanes with a frame are the first of their wave, so lane 0 has one when any lane has
            const uint32_t tk_first = (uint32_t)__shfl((int)tk, 0, 64);
            if (!__any(valid)) continue;   // wave-uniform
            if (__all(!valid || tk == tk_first)) {
                for (int k = 32; k >= 1; k >>= 1) {
                    gb = min(gb, (uint32_t)__shfl_xor((int)gb, k, 64)); pk = max(pk, (uint32_t)__shfl_xor((int)pk, k, 64));
                    lim += (uint32_t)__shfl_xor((int)lim, k, 64); bad += (uint32_t)__shfl_xor((int)bad, k, 64);
                }
                if ((tid & 63u) != 0) continue;
            } else if (!valid) continue;
            LimitTick* rec = r.rec + (size_t)tk * r.stride + d.slot;
            if (gb != 0x3f800000u) atomicMin(reinterpret_cast<uint32_t*>(&rec->min_gain), gb);   // g is in [+0.0, 1.0]: its bits order as it does
            if (pk) atomicMax(reinterpret_cast<uint32_t*>(&rec->peak_out), pk);
            if (lim) atomicAdd(&rec->limited, lim);
            if (bad) atomicAdd(&rec->nonfinite, bad);
        }
        if (t0 + len == N)   // the tap's last tile: what the next run reads as its history
            for (uint32_t h = tid; h < H; h += LIMIT_THREADS) hout[h] = limit_frame(d, hin, H, (int64_t)N - H + h);
    }
}

// ticks [0, n_ticks) of one tap's copy, `width` floats each and `pitch` floats apart, back to back (the read-backs' staging)
__global__ __launch_bounds__(256) void k_limit_gather(const float* __restrict__ src, size_t pitch, uint32_t width, uint32_t n_ticks, float* __restrict__ dst) {
    const uint64_t total = (uint64_t)width * n_ticks;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * 256u) {
        const uint32_t t = (uint32_t)(idx / width), k = (uint32_t)(idx - (uint64_t)t * width);
        dst[idx] = src[(size_t)t * pitch + k];
    }
}

void launch_limit_gather(const float* src, size_t pitch, uint32_t width, uint32_t n_ticks, float* dst, hipStream_t s) {
    const size_t total = (size_t)width * n_ticks;
    if (!total) return;
    hipLaunchKernelGGL(k_limit_gather, dim3(grid_x(total, 256, 4096)), dim3(256), 0, s, src, pitch, width, n_ticks, dst);
}

void launch_taps(const LimitRun& r, hipStream_t s) {
    if (!r.n || !r.n_ticks) return;
    hipLaunchKernelGGL(k_limit_init, dim3(grid_x((size_t)r.n * r.n_ticks, 256, 4096)), dim3(256), 0, s, r);
    const uint64_t tiles = std::max<uint64_t>(1, ((uint64_t)r.max_frames * r.n_ticks + LIMIT_TILE - 1) / LIMIT_TILE);   // of the tap with the most frames
    const uint64_t total = (uint64_t)r.n * tiles;
    hipLaunchKernelGGL(k_limit, dim3((uint32_t)std::min<uint64_t>(total, 1u << 20)), dim3(LIMIT_THREADS), 0, s, r, (uint32_t)tiles);
}

// w[k] = h[k] / sum h, h[k] = 1 - cos(2 pi (k + 1) / (D + 2)), k = 0 .. D.  The sum is D + 2 exactly (the cosines of all D + 2 roots of
// unity add to 0, and the one left out is 1), and 1 - cos(2 t) = 2 sin^2(t) has no cancellation: in x87 long double the error is near
// 2^-62 relative against the 2^-25 half-spacing of an f32 (tests/test_cpu_limiter.py checks every entry at 60 digits).
bool limiter_weights(uint32_t lookahead, float* w) {
    if (lookahead > LIMIT_MAX_LOOKAHEAD || !w) return false;
    const long double pil = 3.14159265358979323846264338327950288L, n = (long double)(lookahead + 2u);
    for (uint32_t k = 0; k <= lookahead; ++k) {
        const long double sn = sinl(pil * (long double)(k + 1u) / n);
        w[k] = lookahead ? (float)(2.0L * sn * sn / n) : 1.0f;
    }
    return true;
}

}  // namespace mx
