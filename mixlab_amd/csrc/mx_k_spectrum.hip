// mx_k_spectrum.hip -- spectrum analyser taps on output ports (mixlab_gpu.h mx_graph_set_spectra): once per run, for
// every tap and tick a windowed n_fft-point transform of the port's last n_fft frames, reduced to band powers.
//
// k_spectrum          one workgroup per (tap, tick).  The frame is read coalesced (from the tap's history for the part before the run's first
//                     frame, else from the port buffer, which holds every tick of the run), multiplied by the window and scattered to its
//                     bit-reversed place in LDS.  The transform is the spec's radix-2 decimation-in-time data flow, two stages per pass: a
//                     thread holds the four values of a radix-4 group in registers, performs the two stages' four butterflies with every
//                     f32 operation rounded on its own (the build's -ffp-contract=off), and writes them back -- the same roundings as two
//                     radix-2 passes, half the LDS traffic and barriers.  An odd log2(n_fft) ends with one radix-2 pass.  The LDS array is
//                     padded by one complex value per 32 (256 bytes = one row of the 64 banks), which spreads the power-of-two strides of
//                     the bit-reversed scatter and of the passes below 32 over the banks.  Split and band reduction: one wave per band,
//                     its lanes are the spec's 64 partials, summed with the meters' butterfly.
// k_spectrum_history  one block per tap, after the transforms: history = concat(history, run)[-n_fft:], out of place (the two history
//                     buffers alternate per run), so that a run shorter than n_fft frames shifts correctly.
//
// Arithmetic: f32 subnormals are kept (float_denorm_mode_32 at its default, as mx_k_meter.hip); (double)c * (double)c is exact in f64, so the
// power of a bin rounds once, in its addition.
#include "mx_dev.hpp"

#include <cmath>

namespace mx {

static constexpr uint32_t SPEC_THREADS = 256;

__device__ __forceinline__ uint32_t spec_idx(uint32_t i) { return i + (i >> 5); }
// t = w * b: (b.re*w.re - b.im*w.im, b.re*w.im + b.im*w.re), each product and each sum rounded
__device__ __forceinline__ float2 spec_cmul(float2 b, float2 w) { return make_float2(b.x * w.x - b.y * w.y, b.x * w.y + b.y * w.x); }
__device__ __forceinline__ void spec_bfly(float2& a, float2& b, float2 w) {
    const float2 t = spec_cmul(b, w);
    const float2 u = a;
    a = make_float2(u.x + t.x, u.y + t.y);
    b = make_float2(u.x - t.x, u.y - t.y);
}
__device__ __forceinline__ double spec_wave_sum(double s) {   // s[q] = s[q] + s[q ^ m], m = 32 .. 1: lane 0 holds the spec's s[0]
    for (int m = 32; m >= 1; m >>= 1) s = s + __shfl_xor(s, m, 64);
    return s;
}
__device__ __forceinline__ double spec_power(float re, float im) {
    const double a = (double)re, b = (double)im;
    return a * a + b * b;
}

template <uint32_t LOG2N>
__global__ __launch_bounds__(SPEC_THREADS) void k_spectrum(const SpecRun r) {
    constexpr uint32_t N = 1u << LOG2N;
    __shared__ float2 z[N + N / 32];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint64_t pairs = (uint64_t)r.n * r.n_ticks;
    const float2* __restrict__ tw = r.twiddle;
    const double scale = 4.0 / ((double)N * (double)N);   // a power of two: exact
    for (uint64_t pr = blockIdx.x; pr < pairs; pr += gridDim.x) {   // block-uniform
        const uint32_t i = (uint32_t)(pr / r.n_ticks), t = (uint32_t)(pr - (uint64_t)i * r.n_ticks);
        const TapDesc d = r.desc[i];
        const float* __restrict__ hist = r.hist_in + (size_t)d.slot * 2u * N;
        // stream position of the frame's first sample relative to the run's first: >= -N, since the frame ends inside the run
        const int64_t q0 = (int64_t)(t + 1u) * d.frames - (int64_t)N;
        for (uint32_t k = tid; k < N; k += SPEC_THREADS) {
            const int64_t q = q0 + k;
            float xl, xr;
            if (d.layout == METER_STEREO) {   // 8-byte aligned: a 735-frame tick starts 5 880 bytes after the last
                const float2 v = q < 0 ? reinterpret_cast<const float2*>(hist)[(int64_t)N + q] : reinterpret_cast<const float2*>(d.p)[q];
                xl = v.x; xr = v.y;
            } else {
                xl = q < 0 ? hist[(int64_t)N + q] : d.p[q];
                xr = xl;
            }
            const float w = r.window[k];
            // a mono port has imaginary part +0.0; a dup port is the stereo port with L == R
            z[spec_idx(__brev(k) >> (32u - LOG2N))] = make_float2(xl * w, d.layout == METER_MONO ? 0.0f : xr * w);
        }
        __syncthreads();
        uint32_t s = 0;
#pragma unroll
        for (; s + 1 < LOG2N; s += 2) {   // stages of half-size h = 2^s and 2h
            const uint32_t h = 1u << s;
            for (uint32_t j = tid; j < N / 4; j += SPEC_THREADS) {
                const uint32_t lo = j & (h - 1u), base = ((j >> s) << (s + 2u)) | lo;
                float2 a0 = z[spec_idx(base)], a1 = z[spec_idx(base + h)], a2 = z[spec_idx(base + 2u * h)], a3 = z[spec_idx(base + 3u * h)];
                const float2 w1 = tw[lo << (LOG2N - 1u - s)];
                spec_bfly(a0, a1, w1);
                spec_bfly(a2, a3, w1);
                const float2 w2 = tw[lo << (LOG2N - 2u - s)], w3 = tw[(lo + h) << (LOG2N - 2u - s)];
                spec_bfly(a0, a2, w2);
                spec_bfly(a1, a3, w3);
                z[spec_idx(base)] = a0; z[spec_idx(base + h)] = a1; z[spec_idx(base + 2u * h)] = a2; z[spec_idx(base + 3u * h)] = a3;
            }
            __syncthreads();
        }
        if (s < LOG2N) {   // the last stage of an odd log2 N: h = N / 2
            for (uint32_t j = tid; j < N / 2; j += SPEC_THREADS) {
                float2 a = z[spec_idx(j)], b = z[spec_idx(j + N / 2)];
                spec_bfly(a, b, tw[j]);
                z[spec_idx(j)] = a; z[spec_idx(j + N / 2)] = b;
            }
            __syncthreads();
        }
        // split into the two real channels' bins, power, bands: one wave per band, lane q is partial q
        float* __restrict__ out = r.rec + ((size_t)t * r.stride + d.slot) * 2u * r.n_bands;
        for (uint32_t j = wave; j < r.n_bands; j += SPEC_THREADS / 64u) {
            const uint32_t e0 = r.edges[j], e1 = r.edges[j + 1u];
            double sl = 0.0, sr = 0.0;
            for (uint32_t k = e0 + lane; k < e1; k += 64u) {
                const float2 zk = z[spec_idx(k)], zn = z[spec_idx((N - k) & (N - 1u))];
                sl = sl + spec_power(zk.x + zn.x, zk.y - zn.y);
                sr = sr + spec_power(zk.y + zn.y, zn.x - zk.x);
            }
            sl = spec_wave_sum(sl);
            sr = spec_wave_sum(sr);
            if (lane == 0) {
                out[j] = (float)(sl * scale);
                out[r.n_bands + j] = d.layout == METER_MONO ? 0.0f : (float)(sr * scale);
            }
        }
        __syncthreads();   // the next pair overwrites z
    }
}

__global__ __launch_bounds__(SPEC_THREADS) void k_spectrum_history(const SpecRun r) {
    const TapDesc d = r.desc[blockIdx.x];
    const uint32_t N = r.n_fft;
    const float* __restrict__ in = r.hist_in + (size_t)d.slot * 2u * N;
    float* __restrict__ out = r.hist_out + (size_t)d.slot * 2u * N;
    const int64_t q0 = (int64_t)r.n_ticks * d.frames - (int64_t)N;   // >= -N
    for (uint32_t k = threadIdx.x; k < N; k += SPEC_THREADS) {
        const int64_t q = q0 + k;
        if (d.layout == METER_STEREO)
            reinterpret_cast<float2*>(out)[k] = q < 0 ? reinterpret_cast<const float2*>(in)[(int64_t)N + q] : reinterpret_cast<const float2*>(d.p)[q];
        else
            out[k] = q < 0 ? in[(int64_t)N + q] : d.p[q];
    }
}

void launch_taps(const SpecRun& r, hipStream_t s) {
    if (!r.n || !r.n_ticks) return;
    const uint64_t pairs = (uint64_t)r.n * r.n_ticks;
    const dim3 grid((uint32_t)std::min<uint64_t>(pairs, 256u * 16u)), block(SPEC_THREADS);   // block-stride beyond 16 per CU
    switch (r.n_fft) {
    case 256:  hipLaunchKernelGGL(k_spectrum<8>, grid, block, 0, s, r); break;
    case 512:  hipLaunchKernelGGL(k_spectrum<9>, grid, block, 0, s, r); break;
    case 1024: hipLaunchKernelGGL(k_spectrum<10>, grid, block, 0, s, r); break;
    case 2048: hipLaunchKernelGGL(k_spectrum<11>, grid, block, 0, s, r); break;
    case 4096: hipLaunchKernelGGL(k_spectrum<12>, grid, block, 0, s, r); break;
    default: return;   // (set_spectra admits no other size)
    }
    hipLaunchKernelGGL(k_spectrum_history, dim3(r.n), block, 0, s, r);
}

// The tables, correctly rounded to f32.  The angle is reduced to [0, pi/4] with integers, so that the exact values (0, 1) are exact and every
// other entry is computed without cancellation in extended precision (x87 long double, 64-bit significand: an error near 2^-63 relative against
// the 2^-25 half-spacing of an f32 -- no entry of these sizes lies that close to a rounding boundary; tests/test_cpu_spectrum.py checks every
// entry against a 60-digit evaluation).
bool spectrum_tables(uint32_t n_fft, float* window, float* twiddle_re, float* twiddle_im) {
    if (n_fft != 256 && n_fft != 512 && n_fft != 1024 && n_fft != 2048 && n_fft != 4096) return false;
    const long double pi = 3.14159265358979323846264338327950288L;
    const uint32_t N = n_fft;
    auto ang = [&](uint32_t j, uint32_t den) { return pi * (long double)j / (long double)den; };   // pi * j / den
    // cos and sin of 2 pi k / N, k < N / 2, from an angle 2 pi j / N with j <= N / 8
    for (uint32_t k = 0; k < N / 2; ++k) {
        long double c, sn;
        if (k <= N / 8) { c = cosl(ang(2 * k, N)); sn = sinl(ang(2 * k, N)); }
        else if (k <= N / 4) { const uint32_t j = N / 4 - k; c = sinl(ang(2 * j, N)); sn = cosl(ang(2 * j, N)); }
        else if (k <= 3 * N / 8) { const uint32_t j = k - N / 4; c = -sinl(ang(2 * j, N)); sn = cosl(ang(2 * j, N)); }
        else { const uint32_t j = N / 2 - k; c = -cosl(ang(2 * j, N)); sn = sinl(ang(2 * j, N)); }
        if (twiddle_re) twiddle_re[k] = (float)c;
        if (twiddle_im) twiddle_im[k] = (float)-sn;
    }
    // 0.5 - 0.5 cos(2 pi i / N) = sin^2(pi i / N) (no cancellation), symmetric about N / 2
    if (window)
        for (uint32_t i = 0; i < N; ++i) {
            const long double sn = sinl(ang(i <= N / 2 ? i : N - i, N));
            window[i] = (float)(sn * sn);
        }
    return true;
}

}  // namespace mx
