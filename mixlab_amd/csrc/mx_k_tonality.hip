// mx_k_tonality.hip -- tonality taps on audio output ports (mixlab_gpu.h mx_graph_set_tonality): once per run, for every tap.
//
// k_ton_emit      one thread per (tap, emission), one per tap in a run that emits nothing.  Writes the record's header -- the emitting tick, the
//                 hops completed since the previous emission from the frame counts, and as nonfinite what the ticks before this run left
//                 (first record; it clears that count) or zero -- and starts C[0 .. B) at what the hops before this run left (first record;
//                 it clears those sums) or zero.  The thread of emission 0 hands on the hops the run leaves behind its last emission.
// k_ton_decimate  per tap three kinds of thread in one launch.  (a) One per stretch of D frames of the run: it counts the stretch's
//                 non-finite frames -- rare, so one atomic each, into the record of the frame's tick's emission or the carried count; every
//                 frame lies in one stretch, so it is counted once and in the tick it arrives -- and, where the run completes decimated frame
//                 n0 + j, forms d: 8 D taps over quantised frames, read from the port (quantised on the fly) or from the carried tail, written
//                 behind the carried history in the tap's linear array and, where it is among the newest, into the next run's.  (b) One per
//                 carried decimated frame that stays carried.  (c) One per frame of the next run's quantised tail.
//                 Nothing is read that the launch writes: both arrays are kept twice.
// k_ton_cq        one workgroup of 256 per (tap, completed hop).  The 2048 decimated frames that end in the hop's last are staged in LDS
//                 (4 KB).  Wave w takes bins w, w + 4, ...; lane l takes n = l, l + 64, ... of the bin's kernel, right-aligned on the hop's last
//                 frame: consecutive lanes read consecutive int16 in LDS and consecutive {re, im} pairs of the table (one dword each, from L2).
//                 Accumulation is in 64 bits (v_mad_i64_i32): |K| <= 2^14 and |d| < 2^15 bound a product by 2^29, so an int32 holds any three
//                 but not four of them, and a stretch of three saves nothing over the 64-bit multiply-add.  A shfl_xor reduction follows; lane
//                 0 shifts, squares, takes the exact root and adds it with one 64-bit atomic to C[b] of the record whose emission the hop's
//                 tick belongs to, or to the carried sums.  Integer sums: no order matters.
//
// Arithmetic: m = L + R is the one f32 operation that rounds; the clamp and the product by 2^13 are exact; everything after is integer.  An m
// below 2^-13 quantises to 0 flushed or not, so f32 subnormals cannot show.  The tables are made on the host in f64 (tonality_tables).
#include "mx_dev.hpp"

#include <cmath>
#include <vector>

namespace mx {

static constexpr uint32_t TON_WAVES = 4;
// (pos < 2^63 frames; a run's decimated frames and hops fit 32 bits: the host sizes the arrays by them and refuses more)
__device__ __forceinline__ uint64_t ton_pos(const TonRun& r, const TonDesc& d) { return d.pos0 + r.ticks0 * (uint64_t)d.frames; }
__device__ __forceinline__ uint64_t ton_decimated(const TonRun& r, uint64_t frames) { return (frames + (1u << r.log2_d) - 1u) >> r.log2_d; }   // n with n D < frames

__device__ __forceinline__ int32_t ton_quantise(float l, float rr, bool& bad) {
    const float m = l + rr;
    bad = (__float_as_uint(m) & 0x7f800000u) == 0x7f800000u;
    return bad ? 0 : (int32_t)(fminf(fmaxf(m, -2.0f), 2.0f) * 8192.0f);
}
__device__ __forceinline__ int32_t ton_frame(const TonDesc& d, uint64_t f, bool& bad) {   // frame f of the run, quantised
    float a, b;
    if (d.layout == METER_STEREO) { const float2 x = reinterpret_cast<const float2*>(d.p)[f]; a = x.x; b = x.y; }
    else a = b = d.p[f];
    return ton_quantise(a, b, bad);
}

// where a count or a sum of tick `tick` of the run goes: the record of the tick's emission, or what is carried behind the run's last one
__device__ __forceinline__ uint32_t* ton_record(const TonRun& r, const TonDesc& d, uint64_t tick) {
    const uint64_t grp = ((uint64_t)r.phase + tick) / r.emit_ticks;
    return grp < r.n_emit ? r.rec + ((size_t)grp * r.stride + d.slot) * r.rec_words : nullptr;
}

__global__ __launch_bounds__(256) void k_ton_emit(const TonRun r) {
    const uint32_t per_tap = max(r.n_emit, 1u);
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)r.n * per_tap) return;
    const uint32_t i = (uint32_t)(idx / per_tap), e = (uint32_t)(idx - (uint64_t)i * per_tap);
    const TonDesc d = r.desc[i];
    const uint64_t pos = ton_pos(r, d), end = pos + (uint64_t)r.n_ticks * d.frames;
    const uint64_t h0 = ton_decimated(r, pos) >> r.log2_hop, h1 = ton_decimated(r, end) >> r.log2_hop;
    if (!r.n_emit) { r.hops_out[d.slot] = r.hops_in[d.slot] + (uint32_t)(h1 - h0); return; }
    const uint32_t tick = r.emit_ticks - 1u - r.phase + e * r.emit_ticks;   // the emitting tick
    const uint64_t h_end = ton_decimated(r, pos + ((uint64_t)tick + 1u) * d.frames) >> r.log2_hop;
    uint32_t* w = r.rec + ((size_t)e * r.stride + d.slot) * r.rec_words;
    uint64_t* c = reinterpret_cast<uint64_t*>(w + 8);
    uint32_t hops, bad = 0u;
    if (e == 0) {
        hops = r.hops_in[d.slot] + (uint32_t)(h_end - h0);
        bad = r.nonfinite[d.slot]; r.nonfinite[d.slot] = 0u;
        uint64_t* carried = r.csum + (size_t)d.slot * r.bins;
        for (uint32_t b = 0; b < r.bins; ++b) { c[b] = carried[b]; carried[b] = 0u; }
        const uint32_t last = r.emit_ticks - 1u - r.phase + (r.n_emit - 1u) * r.emit_ticks;
        r.hops_out[d.slot] = (uint32_t)(h1 - (ton_decimated(r, pos + ((uint64_t)last + 1u) * d.frames) >> r.log2_hop));
    } else {
        hops = (uint32_t)(h_end - (ton_decimated(r, pos + ((uint64_t)tick + 1u - r.emit_ticks) * d.frames) >> r.log2_hop));
        for (uint32_t b = 0; b < r.bins; ++b) c[b] = 0u;
    }
    w[0] = tick; w[1] = hops; w[2] = bad; w[3] = 1u << r.log2_d; w[4] = 1u << r.log2_hop; w[5] = r.bins / 12u; w[6] = r.f_lo_mhz; w[7] = 0u;
}

__global__ __launch_bounds__(256) void k_ton_decimate(const TonRun r) {
    const uint32_t D = 1u << r.log2_d, Tf = 8u * D, QT = Tf + D - 2u, HD = TON_MAX_KERNEL - 1u + (1u << r.log2_hop) - 1u;
    const uint64_t per_tap = (uint64_t)r.max_groups + HD + QT;
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)r.n * per_tap) return;
    const uint32_t i = (uint32_t)(idx / per_tap);
    uint32_t j = (uint32_t)(idx - (uint64_t)i * per_tap);
    const TonDesc d = r.desc[i];
    const uint64_t pos = ton_pos(r, d), run_frames = (uint64_t)r.n_ticks * d.frames, end = pos + run_frames;
    const uint64_t n0 = ton_decimated(r, pos);
    const uint32_t nd = (uint32_t)(ton_decimated(r, end) - n0);   // decimated frames the run completes
    int16_t* lin = r.lin + (size_t)d.slot * r.lin_stride;
    int16_t* next = r.lin_next + (size_t)d.slot * r.lin_stride;
    const int16_t* qt = r.qt + (size_t)d.slot * QT;
    if (j < r.max_groups) {
        const uint64_t g0 = (uint64_t)j << r.log2_d;   // (a) the stretch's frames, counted from the run's first
        for (uint64_t f = g0; f < min(g0 + D, run_frames); ++f) {
            bool bad;
            (void)ton_frame(d, f, bad);
            if (bad) {
                uint32_t* w = ton_record(r, d, f / d.frames);
                atomicAdd(w ? w + 2 : r.nonfinite + d.slot, 1u);
            }
        }
        if (j >= nd) return;
        const int16_t* fir = reinterpret_cast<const int16_t*>(r.tab + (size_t)d.tab * r.tab_stride);
        const uint64_t at = ((n0 + j) << r.log2_d) - pos;   // input frame n D, counted from the run's first: in [0, run_frames)
        int32_t acc = 0;                                    // |sum| <= 65534 x 2^14 < 2^30
        for (uint32_t k = 0; k < Tf; ++k) {
            int32_t q;
            if (at >= k) { bool bad; q = ton_frame(d, at - k, bad); }
            else q = qt[QT - (k - (uint32_t)at)];           // frame pos - (k - at) of the stream: k - at <= Tf - 1 < QT
            acc += (int32_t)fir[k] * q;
        }
        const int16_t v = (int16_t)(acc >> 15);
        lin[HD + j] = v;
        if ((uint64_t)j + HD >= nd) next[j + HD - nd] = v;
        return;
    }
    j -= r.max_groups;
    if (j < HD) {   // (b) a carried decimated frame that stays among the newest HD
        if ((uint64_t)j + nd < HD) next[j] = lin[j + nd];
        return;
    }
    j -= HD;        // (c) frame end - QT + j of the stream, for the next run's tail
    int16_t* qn = r.qt_next + (size_t)d.slot * QT;
    if ((uint64_t)j + run_frames >= QT) { bool bad; qn[j] = (int16_t)ton_frame(d, (uint64_t)j + run_frames - QT, bad); }
    else qn[j] = qt[j + run_frames];
}

__global__ __launch_bounds__(64 * TON_WAVES) void k_ton_cq(const TonRun r) {
    __shared__ int16_t s[TON_MAX_KERNEL];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t HD = TON_MAX_KERNEL - 1u + (1u << r.log2_hop) - 1u;
    const uint64_t pairs = (uint64_t)r.n * r.max_hops;
    for (uint64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {   // workgroup-uniform
        const uint32_t i = (uint32_t)(pair / r.max_hops), k = (uint32_t)(pair - (uint64_t)i * r.max_hops);
        const TonDesc d = r.desc[i];
        const uint64_t pos = ton_pos(r, d), end = pos + (uint64_t)r.n_ticks * d.frames;
        const uint64_t n0 = ton_decimated(r, pos), n1 = ton_decimated(r, end);
        const uint64_t h0 = n0 >> r.log2_hop;
        if (k >= (uint32_t)((n1 >> r.log2_hop) - h0)) continue;
        const uint64_t e_h = ((h0 + k + 1u) << r.log2_hop) - 1u;   // the hop's last decimated frame: n0 <= e_h < n1
        // lin[HD + e_h - n0] is d[e_h]; the 2048 frames that end there start at or behind lin[Hc - 1]
        const int16_t* __restrict__ src = r.lin + (size_t)d.slot * r.lin_stride + HD + (uint32_t)(e_h - n0) - (TON_MAX_KERNEL - 1u);
        for (uint32_t t = tid; t < TON_MAX_KERNEL; t += 64u * TON_WAVES) s[t] = src[t];
        __syncthreads();
        const unsigned char* tab = r.tab + (size_t)d.tab * r.tab_stride;
        const uint32_t* len = reinterpret_cast<const uint32_t*>(tab + 16u * (1u << r.log2_d));   // behind int16 fir[8 D]
        const uint32_t* off = len + r.bins;
        const short2* kern = reinterpret_cast<const short2*>(off + r.bins);
        uint32_t* w = ton_record(r, d, ((e_h << r.log2_d) - pos) / d.frames);   // the hop is complete in the tick of input frame e_h D
        unsigned long long* c = reinterpret_cast<unsigned long long*>(w ? (void*)(w + 8) : (void*)(r.csum + (size_t)d.slot * r.bins));
        for (uint32_t b = wave; b < r.bins; b += TON_WAVES) {   // wave-uniform
            const uint32_t N = len[b];
            const short2* __restrict__ kb = kern + off[b];
            const int16_t* sb = s + (TON_MAX_KERNEL - N);        // n = N - 1 is the newest frame
            long long re = 0, im = 0;
            for (uint32_t n = lane; n < N; n += 64u) {
                const short2 kv = kb[n];
                const int32_t x = sb[n];
                re += (long long)((int32_t)kv.x * x);            // |product| <= 2^29
                im += (long long)((int32_t)kv.y * x);
            }
            for (int x = 32; x >= 1; x >>= 1) { re += __shfl_xor(re, x, 64); im += __shfl_xor(im, x, 64); }
            if (lane == 0) {
                const long long a = re >> 10, bq = im >> 10;     // floor; |a|, |bq| <= 2^30
                atomicAdd(c + b, (unsigned long long)ton_root((uint64_t)(a * a) + (uint64_t)(bq * bq)));
            }
        }
        __syncthreads();   // before the next pair overwrites s
    }
}

void launch_taps(const TonRun& r, hipStream_t s) {
    if (!r.n || !r.n_ticks) return;
    const uint64_t recs = (uint64_t)r.n * std::max(r.n_emit, 1u);
    hipLaunchKernelGGL(k_ton_emit, dim3((uint32_t)((recs + 255u) / 256u)), dim3(256), 0, s, r);
    const uint64_t items = (uint64_t)r.n * ((uint64_t)r.max_groups + ton_dhist(1u << r.log2_hop) + ton_qtail(1u << r.log2_d));
    hipLaunchKernelGGL(k_ton_decimate, dim3((uint32_t)((items + 255u) / 256u)), dim3(256), 0, s, r);
    if (!r.max_hops) return;
    const uint64_t pairs = (uint64_t)r.n * r.max_hops;
    hipLaunchKernelGGL(k_ton_cq, dim3((uint32_t)std::min<uint64_t>(pairs, 256u * 8u)), dim3(64 * TON_WAVES), 0, s, r);   // grid-stride beyond eight workgroups per CU
}

// ---- the tables (host, f64) ----

int tonality_tables(double rate, uint32_t decim, uint32_t octaves, uint32_t f_lo_mhz, int16_t* fir, uint32_t* len, int16_t* kern, size_t* kern_pairs) {
    if (!(std::isfinite(rate) && rate > 0.0)) return 4;
    const double pi = 3.14159265358979323846, fs_d = rate / decim, f_lo = f_lo_mhz / 1000.0;
    const uint32_t B = 12 * octaves, Tf = 8 * decim;
    auto f_bin = [&](uint32_t b) { return f_lo * std::exp2((double)b / 12.0); };
    if (std::ceil(TON_Q * fs_d / f_lo) > (double)TON_MAX_KERNEL) return 1;
    if (f_bin(B - 1) * std::exp2(1.0 / 24.0) >= 0.45 * fs_d) return 2;
    // the decimator: a Hann-windowed sinc, cutoff 0.45 fs_d = 0.45 / D cycles per input frame, centred at (Tf - 1) / 2 (never on a tap: Tf is even)
    std::vector<double> h(Tf);
    double sum = 0.0;
    for (uint32_t k = 0; k < Tf; ++k) {
        const double t = (double)k - 0.5 * (double)(Tf - 1);
        h[k] = std::sin(2.0 * pi * (0.45 / decim) * t) / (pi * t) * (0.5 - 0.5 * std::cos(2.0 * pi * (double)(k + 1) / (double)(Tf + 1)));
        sum += h[k];
    }
    long mag = 0;
    for (uint32_t k = 0; k < Tf; ++k) { const long c = std::lround(32768.0 * h[k] / sum); fir[k] = (int16_t)c; mag += std::labs(c); }
    if (mag > 65534) return 3;
    size_t pairs = 0;
    for (uint32_t b = 0; b < B; ++b) {
        const double f = f_bin(b);
        const uint32_t N = (uint32_t)std::ceil(TON_Q * fs_d / f);
        len[b] = N;
        if (kern)
            for (uint32_t n = 0; n < N; ++n) {
                const double w = 0.5 - 0.5 * std::cos(2.0 * pi * (double)(n + 1) / (double)(N + 1));
                const double phi = 2.0 * pi * f * ((double)n - (double)(N - 1)) / fs_d;
                kern[2 * (pairs + n)] = (int16_t)std::lround(16384.0 * w * std::cos(phi));
                kern[2 * (pairs + n) + 1] = (int16_t)std::lround(-16384.0 * w * std::sin(phi));
            }
        pairs += N;
    }
    if (kern_pairs) *kern_pairs = pairs;
    return 0;
}

}  // namespace mx
