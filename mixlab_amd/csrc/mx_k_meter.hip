// mx_k_meter.hip -- level meters on output ports (mixlab_gpu.h mx_graph_set_meters): once per run, for every tap and tick.
//
// k_meter_reduce  one wave per (tap, tick): lane l reads frames l, l + 64, l + 128, ... in ascending order -- exactly partial l of the
//                 sum-of-squares spec -- with UNROLL independent loads in flight, then reduces peak (integer max of the magnitude bits), over
//                 (integer add) and the f64 partials (the spec's butterfly, s[j] + s[j ^ k] for k = 32 .. 1) across the wave.  Frames past
//                 the tick read as +0.0, which changes none of the three: 0 is no larger magnitude, no over, and s + 0.0 == s for every
//                 s >= +0 and NaN.  Algorithmic bytes per frame: 4 (mono, dup) or 8 (stereo) read, 48 per record written.
// k_meter_hold    one block per tap: one lane per channel walks the run's ticks in order through the peak-hold recurrence over peaks the
//                 block staged in LDS, the block writes each tick's hold back, the lane the state the next run starts from.  Same pattern as
//                 k_out_scan.
//
// Arithmetic: (double)x * (double)x is exact in f64 (24 + 24 bits), so fused or not it rounds nowhere; f32 subnormals must reach the widening
// unflushed -- the kernels are built with the default f32 denormal mode (float_denorm_mode_32 = 3, kept), tests/test_gpu_meters.py feeds them.
#include "mx_dev.hpp"

namespace mx {

static constexpr uint32_t METER_WAVES = 4;   // waves per block of k_meter_reduce

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    for (int k = 32; k >= 1; k >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, k, 64));
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
    for (int k = 32; k >= 1; k >>= 1) v += (uint32_t)__shfl_xor((int)v, k, 64);
    return v;
}
__device__ __forceinline__ double wave_butterfly(double s) {   // s[j] = s[j] + s[j ^ k]; addition commutes bit for bit, so lane 0 holds the spec's s[0]
    for (int k = 32; k >= 1; k >>= 1) s = s + __shfl_xor(s, k, 64);
    return s;
}

struct ChanAcc {
    uint32_t peak = 0u, over = 0u; double s = 0.0;
    __device__ __forceinline__ void add(float x) {
        peak = max(peak, __float_as_uint(x) & 0x7fffffffu);
        over += (x < -1.0f || x > 1.0f) ? 1u : 0u;
        const double d = (double)x;
        s = s + d * d;
    }
};

// one tick of a mono / dup port (one float per frame)
template <uint32_t UNROLL>
__device__ __forceinline__ void reduce_one(const float* __restrict__ p, uint32_t F, uint32_t lane, ChanAcc& a) {
    for (uint32_t f0 = lane; f0 < F; f0 += 64u * UNROLL) {
        float x[UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) { const uint32_t f = f0 + 64u * u; x[u] = f < F ? p[f] : 0.0f; }
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) a.add(x[u]);   // ascending f: the loads above are all in flight before the first add
    }
}
// one tick of an interleaved stereo port (8-byte aligned: a 735-frame tick starts 5 880 bytes after the last)
template <uint32_t UNROLL>
__device__ __forceinline__ void reduce_two(const float2* __restrict__ p, uint32_t F, uint32_t lane, ChanAcc& l, ChanAcc& r) {
    for (uint32_t f0 = lane; f0 < F; f0 += 64u * UNROLL) {
        float2 x[UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) { const uint32_t f = f0 + 64u * u; x[u] = f < F ? p[f] : make_float2(0.0f, 0.0f); }
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) { l.add(x[u].x); r.add(x[u].y); }
    }
}

__global__ __launch_bounds__(64 * METER_WAVES) void k_meter_reduce(const MeterDesc* __restrict__ desc, uint32_t n, uint32_t n_ticks, uint32_t stride,
                                                                    MeterTick* __restrict__ rec) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t pairs = (uint64_t)n * n_ticks;
    const uint64_t waves = (uint64_t)gridDim.x * METER_WAVES;
    for (uint64_t w = (uint64_t)blockIdx.x * METER_WAVES + (threadIdx.x >> 6); w < pairs; w += waves) {   // wave-uniform
        const uint32_t i = (uint32_t)(w / n_ticks), t = (uint32_t)(w - (uint64_t)i * n_ticks);   // consecutive waves: consecutive ticks of one tap
        const MeterDesc d = desc[i];
        const uint32_t F = d.frames;
        ChanAcc a, b;
        if (d.layout == METER_STEREO) reduce_two<8>(reinterpret_cast<const float2*>(d.p) + (size_t)t * F, F, lane, a, b);
        else reduce_one<16>(d.p + (size_t)t * F, F, lane, a);
        MeterTick r;
        r.peak[0] = __uint_as_float(wave_max_u32(a.peak));
        r.over[0] = wave_sum_u32(a.over);
        r.sum_sq[0] = wave_butterfly(a.s);
        if (d.layout == METER_STEREO) {
            r.peak[1] = __uint_as_float(wave_max_u32(b.peak)); r.over[1] = wave_sum_u32(b.over); r.sum_sq[1] = wave_butterfly(b.s);
        } else if (d.layout == METER_DUP) {
            r.peak[1] = r.peak[0]; r.over[1] = r.over[0]; r.sum_sq[1] = r.sum_sq[0];   // L == R: the unfused port's right channel, bit for bit
        } else {
            r.peak[1] = 0.0f; r.over[1] = 0u; r.sum_sq[1] = 0.0;
        }
        r.hold[0] = r.hold[1] = 0.0f;   // k_meter_hold
        r.frames = F;
        r.channels = d.layout == METER_MONO ? 1u : 2u;
        if (lane == 0) rec[(size_t)t * stride + d.slot] = r;
    }
}

__device__ __forceinline__ void hold_step(uint32_t pk_bits, uint32_t hold_ticks, float release, float& h, uint32_t& a) {
    a = a == 0xffffffffu ? a : a + 1u;
    if (a > hold_ticks) h = isfinite(h) ? h * release : 0.0f;
    if (pk_bits >= __float_as_uint(h)) { h = __uint_as_float(pk_bits); a = 0u; }
}

// one block per tap: the block stages HOLD_CHUNK ticks' peaks in LDS (each record's peak pair is one 8-byte load; the records are read
// back to back), one lane per channel walks them in tick order and leaves each tick's hold in their place, the block writes the holds back
static constexpr uint32_t HOLD_CHUNK = 2048;
__global__ __launch_bounds__(256) void k_meter_hold(const MeterDesc* __restrict__ desc, uint32_t n_ticks, uint32_t stride, MeterTick* __restrict__ rec,
                                                    MeterHold* __restrict__ state) {
    __shared__ uint32_t s_v[2][HOLD_CHUNK];
    const MeterDesc d = desc[blockIdx.x];
    const uint32_t tid = threadIdx.x, ch = tid >> 6;
    const uint32_t nch = d.layout == METER_MONO ? 1u : 2u;
    const bool walker = (tid & 63u) == 0 && ch < nch;   // lane 0 of wave 0 (left / mono) and of wave 1 (right)
    MeterHold* st = state + 2 * (size_t)d.slot;
    float h = 0.0f;
    uint32_t a = 0u;
    if (walker) { h = st[ch].h; a = st[ch].a; }
    for (uint32_t t0 = 0; t0 < n_ticks; t0 += HOLD_CHUNK) {
        const uint32_t cnt = min(HOLD_CHUNK, n_ticks - t0);
        for (uint32_t k = tid; k < cnt; k += 256u) {
            const float2 pk = *reinterpret_cast<const float2*>(rec[(size_t)(t0 + k) * stride + d.slot].peak);
            s_v[0][k] = __float_as_uint(pk.x); s_v[1][k] = __float_as_uint(pk.y);
        }
        __syncthreads();
        if (walker) {
            uint32_t* v = s_v[ch];
            uint32_t k = 0;
            for (; k + 8 <= cnt; k += 8) {   // the LDS reads of a batch go out ahead of the dependent steps
                uint32_t pk[8];
#pragma unroll
                for (uint32_t u = 0; u < 8; ++u) pk[u] = v[k + u];
#pragma unroll
                for (uint32_t u = 0; u < 8; ++u) { hold_step(pk[u], d.hold_ticks, d.release, h, a); v[k + u] = __float_as_uint(h); }
            }
            for (; k < cnt; ++k) { hold_step(v[k], d.hold_ticks, d.release, h, a); v[k] = __float_as_uint(h); }
        }
        __syncthreads();
        for (uint32_t k = tid; k < cnt; k += 256u)   // a mono tap's [1] stays 0
            *reinterpret_cast<float2*>(rec[(size_t)(t0 + k) * stride + d.slot].hold) = make_float2(__uint_as_float(s_v[0][k]), nch == 2 ? __uint_as_float(s_v[1][k]) : 0.0f);
        __syncthreads();   // the next chunk overwrites the arrays
    }
    if (walker) st[ch] = MeterHold{h, a};
}

void launch_taps(const MeterRun& r, hipStream_t s) {
    if (!r.n || !r.n_ticks) return;
    const uint64_t pairs = (uint64_t)r.n * r.n_ticks;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((pairs + METER_WAVES - 1) / METER_WAVES, 256u * 16u);   // grid-stride beyond 16 blocks per CU
    hipLaunchKernelGGL(k_meter_reduce, dim3(blocks), dim3(64 * METER_WAVES), 0, s, r.desc, r.n, r.n_ticks, r.stride, r.rec);
    hipLaunchKernelGGL(k_meter_hold, dim3(r.n), dim3(256), 0, s, r.desc, r.n_ticks, r.stride, r.rec, r.state);
}

}  // namespace mx
