// mx_k_loudness.hip -- loudness taps on output ports (mixlab_gpu.h mx_graph_set_loudness): once per run, for every tap
// and tick the K-weighted sum of squares per channel, the momentary / short-term window sums and the true peak.
//
// The K-weighting is a recurrence in time (two f64 biquads); the spec cuts it at tick boundaries so that ticks run in parallel:
// k_loud_peak    one wave per (tap, tick): lane l takes frames l, l + 64, ...; three 12-tap interpolator phases in f64 (exact products,
//                ascending j), integer max of the magnitude bits across the wave; writes true_peak / frames / channels.  The wave of the
//                run's last tick also writes the 11-frame history the next run starts from (out of place, as the spectrum taps').
// k_loud_walk    one lane per (tap, channel, tick); a block is one wave that takes 64 (32 for a stereo port) consecutive ticks of one tap
//                and stages them through LDS LOUD_CHUNK frames at a time with coalesced loads (a lane would otherwise read at a stride
//                of one tick), rows padded to an odd stride so that the lanes' reads hit distinct banks.
//                  <ZERO>        walks from the zero state and leaves Z_k in the walk buffer           (k_loud_zero)
//                  <TRUE>        walks from S_k (the walk buffer, after the scan), eight partials in registers, writes ksq (k_loud_energy)
//                  <ZERO, TRUE>  a one-tick run: both chains interleaved in one lane from the carried state, then S' = Z + P S; two
//                                independent chains fill each other's latency instead of two dependent launches
// k_loud_scan    one lane per (tap, channel): S_{k+1} = Z_k + P S_k over the run's ticks, Z_k replaced by S_k in the walk buffer, the loads
//                of eight ticks issued ahead of the dependent steps.
// k_loud_window  one lane per (tap, tick): both window sums afresh in ascending tick over e = ksq[0] + ksq[1] (history for ticks before the
//                run), and per tap the 1023-tick history for the next run (out of place).
//
// Arithmetic: every f64 operation is rounded on its own (the build's -ffp-contract=off; the ISA of this file holds no v_fma_f64 and no
// scratch).  (double)a * (double)b of two f32 is exact, so the interpolator rounds only in its additions.  f32 subnormals reach the widening
// unflushed (float_denorm_mode_32 at its default, as mx_k_meter.hip).
#include "mx_dev.hpp"

#include <cmath>

namespace mx {

static constexpr uint32_t LOUD_CHUNK = 32;        // frames per staged chunk; a multiple of 8, so that frame i's partial is (i - chunk start) & 7
static constexpr uint32_t LOUD_ROW = LOUD_CHUNK + 1;
static constexpr uint32_t LOUD_PEAK_WAVES = 4;

struct LoudBq { double b0, b1, b2, a1, a2; };
// one sample through one biquad, transposed direct form II: y = b0 x + s1; s1 = (b1 x - a1 y) + s2; s2 = b2 x - a2 y
__device__ __forceinline__ double loud_step(const LoudBq& q, double x, double& s1, double& s2) {
    const double y = q.b0 * x + s1;
    s1 = (q.b1 * x - q.a1 * y) + s2;
    s2 = q.b2 * x - q.a2 * y;
    return y;
}
__device__ __forceinline__ LoudBq loud_bq(const double* __restrict__ c) { return LoudBq{c[0], c[1], c[2], c[3], c[4]}; }
__device__ __forceinline__ uint32_t loud_nch(uint32_t layout) { return layout == METER_STEREO ? 2u : 1u; }   // channels computed (a dup port's right channel is its left)

template <bool ZERO, bool TRUE>
__global__ __launch_bounds__(64) void k_loud_walk(const LoudRun r, uint32_t groups) {
    __shared__ float buf[64 * LOUD_ROW];
    const uint32_t lane = threadIdx.x;
    const uint32_t i = blockIdx.x / groups, g = blockIdx.x - i * groups;
    const TapDesc d = r.desc[i];
    const uint32_t nch = loud_nch(d.layout), tg = 64u / nch;   // ticks of this block
    const uint32_t t0 = g * tg;
    if (t0 >= r.n_ticks) return;   // block-uniform (the grid is sized for 32-tick groups)
    const uint32_t nt = min(tg, r.n_ticks - t0), F = d.frames;
    const uint32_t c = nch == 2 ? (lane & 1u) : 0u, tl = nch == 2 ? (lane >> 1) : lane;
    const bool live = tl < nt;
    const LoudCoef* __restrict__ co = r.coef + d.slot;
    const LoudBq qa = loud_bq(co->bq), qb = loud_bq(co->bq + 5);
    double* __restrict__ wk = r.walk + (((size_t)d.slot * 2u + c) * r.walk_ticks + (t0 + tl)) * 4u;
    double* __restrict__ st = r.state + ((size_t)d.slot * 2u + c) * 4u;
    double z0 = 0.0, z1 = 0.0, z2 = 0.0, z3 = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (TRUE && live) {
        const double* __restrict__ from = ZERO ? st : wk;   // a one-tick run starts from the carried state itself
        s0 = from[0]; s1 = from[1]; s2 = from[2]; s3 = from[3];
    }
    const double start0 = s0, start1 = s1, start2 = s2, start3 = s3;
    double part[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (uint32_t f0 = 0; f0 < F; f0 += LOUD_CHUNK) {
        const uint32_t cnt = min(LOUD_CHUNK, F - f0);
        __syncthreads();   // the last chunk has been read
        for (uint32_t k = lane; k < nt * LOUD_CHUNK; k += 64u) {   // 32 consecutive lanes read 32 consecutive frames of one tick
            const uint32_t row = k / LOUD_CHUNK, col = k - row * LOUD_CHUNK;
            if (col < cnt) {
                const size_t at = (size_t)(t0 + row) * F + f0 + col;
                if (nch == 2) {   // 8-byte aligned: a 735-frame tick starts 5 880 bytes after the last
                    const float2 v = reinterpret_cast<const float2*>(d.p)[at];
                    buf[(2u * row) * LOUD_ROW + col] = v.x; buf[(2u * row + 1u) * LOUD_ROW + col] = v.y;
                } else {
                    buf[row * LOUD_ROW + col] = d.p[at];
                }
            }
        }
        __syncthreads();
        if (live) {
            const float* __restrict__ x = buf + lane * LOUD_ROW;
            for (uint32_t i8 = 0; i8 < cnt; i8 += 8u) {
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) {
                    if (i8 + u < cnt) {   // block-uniform
                        const double xv = (double)x[i8 + u];
                        if (ZERO) (void)loud_step(qb, loud_step(qa, xv, z0, z1), z2, z3);
                        if (TRUE) {
                            const double y = loud_step(qb, loud_step(qa, xv, s0, s1), s2, s3);
                            part[u] = part[u] + y * y;   // the product rounds, then the sum
                        }
                    }
                }
            }
        }
    }
    if (!live) return;
    if (TRUE) {
#pragma unroll
        for (uint32_t m = 4; m >= 1; m >>= 1)
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j)
                if (!(j & m)) part[j] = part[j] + part[j ^ m];   // s[j] += s[j ^ m] for the j that reach s[0] (addition commutes bit for bit)
        LoudTick* rec = r.rec + (size_t)(t0 + tl) * r.stride + d.slot;
        rec->ksq[c] = part[0];
        if (nch == 1) rec->ksq[1] = d.layout == METER_DUP ? part[0] : 0.0;   // L == R: the unfused port's right channel, bit for bit; mono: 0
    }
    if (ZERO && !TRUE) { wk[0] = z0; wk[1] = z1; wk[2] = z2; wk[3] = z3; }
    if (ZERO && TRUE) {   // S' = Z + P S from the state the tick started with
        const double* __restrict__ P = co->carry;
        st[0] = z0 + (((P[0] * start0 + P[1] * start1) + P[2] * start2) + P[3] * start3);
        st[1] = z1 + (((P[4] * start0 + P[5] * start1) + P[6] * start2) + P[7] * start3);
        st[2] = z2 + (((P[8] * start0 + P[9] * start1) + P[10] * start2) + P[11] * start3);
        st[3] = z3 + (((P[12] * start0 + P[13] * start1) + P[14] * start2) + P[15] * start3);
    }
}

__global__ __launch_bounds__(64) void k_loud_scan(const LoudRun r) {
    const uint32_t idx = blockIdx.x * 64u + threadIdx.x;
    const uint32_t i = idx >> 1, c = idx & 1u;
    if (i >= r.n) return;
    const TapDesc d = r.desc[i];
    if (c >= loud_nch(d.layout)) return;
    const double* __restrict__ Pm = r.coef[d.slot].carry;
    double P[16];
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) P[k] = Pm[k];
    double* __restrict__ st = r.state + ((size_t)d.slot * 2u + c) * 4u;
    double* __restrict__ wk = r.walk + ((size_t)d.slot * 2u + c) * r.walk_ticks * 4u;
    double s0 = st[0], s1 = st[1], s2 = st[2], s3 = st[3];
    auto advance = [&](double* __restrict__ w, double za, double zb, double zc, double zd) {
        w[0] = s0; w[1] = s1; w[2] = s2; w[3] = s3;   // the tick's start state, where its Z was
        const double n0 = za + (((P[0] * s0 + P[1] * s1) + P[2] * s2) + P[3] * s3);
        const double n1 = zb + (((P[4] * s0 + P[5] * s1) + P[6] * s2) + P[7] * s3);
        const double n2 = zc + (((P[8] * s0 + P[9] * s1) + P[10] * s2) + P[11] * s3);
        const double n3 = zd + (((P[12] * s0 + P[13] * s1) + P[14] * s2) + P[15] * s3);
        s0 = n0; s1 = n1; s2 = n2; s3 = n3;
    };
    uint32_t k = 0;
    for (; k + 8u <= r.n_ticks; k += 8u) {   // the loads of a batch go out ahead of the dependent steps
        double z[8][4];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u)
#pragma unroll
            for (uint32_t q = 0; q < 4u; ++q) z[u][q] = wk[(size_t)(k + u) * 4u + q];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) advance(wk + (size_t)(k + u) * 4u, z[u][0], z[u][1], z[u][2], z[u][3]);
    }
    for (; k < r.n_ticks; ++k) {
        double* w = wk + (size_t)k * 4u;
        advance(w, w[0], w[1], w[2], w[3]);
    }
    st[0] = s0; st[1] = s1; st[2] = s2; st[3] = s3;
}

__device__ __forceinline__ uint32_t loud_wave_max(uint32_t v) {
    for (int k = 32; k >= 1; k >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, k, 64));
    return v;
}

__global__ __launch_bounds__(64 * LOUD_PEAK_WAVES) void k_loud_peak(const LoudRun r) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t pairs = (uint64_t)r.n * r.n_ticks;
    const uint64_t waves = (uint64_t)gridDim.x * LOUD_PEAK_WAVES;
    float tab[36];
#pragma unroll
    for (uint32_t k = 0; k < 36u; ++k) tab[k] = r.interp[k];
    for (uint64_t w = (uint64_t)blockIdx.x * LOUD_PEAK_WAVES + (threadIdx.x >> 6); w < pairs; w += waves) {   // wave-uniform
        const uint32_t i = (uint32_t)(w / r.n_ticks), t = (uint32_t)(w - (uint64_t)i * r.n_ticks);
        const TapDesc d = r.desc[i];
        const uint32_t F = d.frames, nch = loud_nch(d.layout);
        const float* __restrict__ hin = r.xhist_in + (size_t)d.slot * 2u * LOUD_HIST_FRAMES;   // [channel][11]
        // frame q of the run (q >= -11): before the run from the history, else from the port, which holds every tick of the run
        auto sample = [&](int64_t q, float& l, float& rr) {
            if (q < 0) { l = hin[(int64_t)LOUD_HIST_FRAMES + q]; rr = hin[2 * (int64_t)LOUD_HIST_FRAMES + q]; }
            else if (nch == 2) { const float2 v = reinterpret_cast<const float2*>(d.p)[q]; l = v.x; rr = v.y; }
            else { l = d.p[q]; rr = 0.0f; }
        };
        uint32_t pk0 = 0u, pk1 = 0u;
        for (uint32_t m = lane; m < F; m += 64u) {
            const int64_t q = (int64_t)t * F + m;
            double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
            float xl = 0.0f, xr = 0.0f;
#pragma unroll
            for (uint32_t j = 0; j < 12u; ++j) {   // ascending j: x[m - 11 + j]
                sample(q - 11 + (int64_t)j, xl, xr);
#pragma unroll
                for (uint32_t p = 0; p < 3u; ++p) {
                    a[p] = a[p] + (double)tab[12u * p + j] * (double)xl;
                    if (nch == 2) b[p] = b[p] + (double)tab[12u * p + j] * (double)xr;
                }
            }
            pk0 = max(pk0, __float_as_uint(xl) & 0x7fffffffu);   // j = 11 left x[m] itself
            pk1 = max(pk1, __float_as_uint(xr) & 0x7fffffffu);
#pragma unroll
            for (uint32_t p = 0; p < 3u; ++p) {
                pk0 = max(pk0, __float_as_uint((float)a[p]) & 0x7fffffffu);
                pk1 = max(pk1, __float_as_uint((float)b[p]) & 0x7fffffffu);
            }
        }
        pk0 = loud_wave_max(pk0);
        pk1 = nch == 2 ? loud_wave_max(pk1) : (d.layout == METER_DUP ? pk0 : 0u);
        if (lane == 0) {
            LoudTick* rec = r.rec + (size_t)t * r.stride + d.slot;
            rec->true_peak[0] = __uint_as_float(pk0); rec->true_peak[1] = __uint_as_float(pk1);
            rec->frames = F; rec->channels = d.layout == METER_MONO ? 1u : 2u;
        }
        if (t + 1u == r.n_ticks && lane < 2u * LOUD_HIST_FRAMES) {   // the last 11 frames of the stream so far, for the next run
            const uint32_t ch = lane / LOUD_HIST_FRAMES, k = lane - ch * LOUD_HIST_FRAMES;
            float l, rr;
            sample((int64_t)r.n_ticks * F - (int64_t)LOUD_HIST_FRAMES + k, l, rr);
            r.xhist_out[(size_t)d.slot * 2u * LOUD_HIST_FRAMES + lane] = ch ? rr : l;
        }
    }
}

__global__ __launch_bounds__(256) void k_loud_window(const LoudRun r) {
    const uint32_t per_tap = r.n_ticks + LOUD_HIST_TICKS;
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)r.n * per_tap) return;
    const uint32_t i = (uint32_t)(idx / per_tap), j = (uint32_t)(idx - (uint64_t)i * per_tap);
    const uint32_t slot = r.desc[i].slot;
    const double* __restrict__ hin = r.ehist_in + (size_t)slot * LOUD_HIST_TICKS;
    // e of tick u of the run (u >= -1023): ksq[0] + ksq[1], from the history before the run
    auto e = [&](int64_t u) {
        if (u < 0) return hin[(int64_t)LOUD_HIST_TICKS + u];
        const LoudTick* rec = r.rec + (size_t)u * r.stride + slot;
        return rec->ksq[0] + rec->ksq[1];
    };
    if (j >= r.n_ticks) {   // the history the next run reads
        const uint32_t k = j - r.n_ticks;
        r.ehist_out[(size_t)slot * LOUD_HIST_TICKS + k] = e((int64_t)r.n_ticks - (int64_t)LOUD_HIST_TICKS + k);
        return;
    }
    const uint32_t M = r.momentary_ticks, S = r.short_ticks;
    double ms = 0.0, ss = 0.0;
    for (uint32_t back = max(M, S); back-- > 0;) {   // ascending tick: j - back
        const double v = e((int64_t)j - back);
        if (back < M) ms = ms + v;
        if (back < S) ss = ss + v;
    }
    LoudTick* rec = r.rec + (size_t)j * r.stride + slot;
    rec->momentary_sq = ms;
    rec->short_sq = ss;
}

void launch_taps(const LoudRun& r, hipStream_t s) {
    if (!r.n || !r.n_ticks) return;
    const uint64_t pairs = (uint64_t)r.n * r.n_ticks;
    const uint32_t pk_blocks = (uint32_t)std::min<uint64_t>((pairs + LOUD_PEAK_WAVES - 1) / LOUD_PEAK_WAVES, 256u * 16u);   // grid-stride beyond 16 blocks per CU
    hipLaunchKernelGGL(k_loud_peak, dim3(pk_blocks), dim3(64 * LOUD_PEAK_WAVES), 0, s, r);
    const uint32_t groups = (r.n_ticks + 31u) / 32u;   // of 32 ticks, a stereo port's; a block of a mono or dup port takes 64 and every second one leaves
    const dim3 grid(r.n * groups), block(64);
    if (r.n_ticks == 1) {
        hipLaunchKernelGGL((k_loud_walk<true, true>), grid, block, 0, s, r, groups);
    } else {
        hipLaunchKernelGGL((k_loud_walk<true, false>), grid, block, 0, s, r, groups);
        hipLaunchKernelGGL(k_loud_scan, dim3((2u * r.n + 63u) / 64u), block, 0, s, r);
        hipLaunchKernelGGL((k_loud_walk<false, true>), grid, block, 0, s, r, groups);
    }
    const uint64_t items = (uint64_t)r.n * (r.n_ticks + LOUD_HIST_TICKS);
    hipLaunchKernelGGL(k_loud_window, dim3((uint32_t)((items + 255u) / 256u)), dim3(256), 0, s, r);
}

// ---- host: the tables of the spec ----

static const double SHELF_F0 = 1681.974450955533, SHELF_G = 3.999843853973347, SHELF_Q = 0.7071752369554196, SHELF_VB_EXP = 0.4996667741545416;
static const double HP_F0 = 38.13547087602444, HP_Q = 0.5003270373238773;

static void host_step(const double* bq, double x, double* s) {   // both biquads, the kernels' order (this file is built with -ffp-contract=off)
    for (int k = 0; k < 2; ++k) {
        const double* q = bq + 5 * k;
        const double y = q[0] * x + s[2 * k];
        s[2 * k] = (q[1] * x - q[3] * y) + s[2 * k + 1];
        s[2 * k + 1] = q[2] * x - q[4] * y;
        x = y;
    }
}

bool loudness_tables(double rate, uint32_t frames, double* biquads, double* carry, float* interp) {
    if (!(rate > 2.0 * SHELF_F0) || !std::isfinite(rate) || frames < 1 || frames > LOUD_MAX_FRAMES) return false;
    const double pi = 3.14159265358979323846;
    double bq[10];
    {
        const double K = std::tan(pi * SHELF_F0 / rate), Vh = std::pow(10.0, SHELF_G / 20.0), Vb = std::pow(Vh, SHELF_VB_EXP);
        const double a0 = 1.0 + K / SHELF_Q + K * K;
        bq[0] = (Vh + Vb * K / SHELF_Q + K * K) / a0;
        bq[1] = 2.0 * (K * K - Vh) / a0;
        bq[2] = (Vh - Vb * K / SHELF_Q + K * K) / a0;
        bq[3] = 2.0 * (K * K - 1.0) / a0;
        bq[4] = (1.0 - K / SHELF_Q + K * K) / a0;
    }
    {
        const double K = std::tan(pi * HP_F0 / rate), a0 = 1.0 + K / HP_Q + K * K;
        bq[5] = 1.0; bq[6] = -2.0; bq[7] = 1.0;
        bq[8] = 2.0 * (K * K - 1.0) / a0;
        bq[9] = (1.0 - K / HP_Q + K * K) / a0;
    }
    if (biquads) std::copy(bq, bq + 10, biquads);
    if (carry)
        for (int c = 0; c < 4; ++c) {   // column c: `frames` zero samples from unit state c
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            s[c] = 1.0;
            for (uint32_t f = 0; f < frames; ++f) host_step(bq, 0.0, s);
            for (int rr = 0; rr < 4; ++rr) carry[4 * rr + c] = s[rr];
        }
    // sinc(d) (0.5 + 0.5 cos(pi d / 6)) = sin(pi d) / (pi d) * cos^2(pi d / 12) (no cancellation), d = j - 5 - p / 4, in extended precision (x87 long
    // double: an error near 2^-62 relative against the 2^-25 half-spacing of an f32; tests/test_cpu_loudness.py checks every entry at 60 digits)
    if (interp) {
        const long double pil = 3.14159265358979323846264338327950288L;
        for (int p = 1; p <= 3; ++p)
            for (int j = 0; j < 12; ++j) {
                const long double dd = (long double)(4 * (j - 5) - p) / 4.0L;   // exact
                const long double cw = cosl(pil * dd / 12.0L);
                interp[12 * (p - 1) + j] = (float)(sinl(pil * dd) / (pil * dd) * cw * cw);
            }
    }
    return true;
}

}  // namespace mx
