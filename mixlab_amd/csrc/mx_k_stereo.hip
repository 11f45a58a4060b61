// mx_k_stereo.hip -- stereo field taps on stereo output ports (mixlab_gpu.h mx_graph_set_stereo): once per run, for
// every tap and tick.
//
// k_stereo_emit    only in a run that emits goniometer records: writes every record of the launch's taps -- the header, and as counts the
//                  tap's carried grid in the run's first record and zero in the others -- and clears the carried grid.  One thread per word,
//                  which reads and clears only its own word of the carry.
// k_stereo_reduce  one wave per (tap, tick), k_meter_reduce's shape: lane l reads frames l, l + 64, ... in ascending order -- partial l of the
//                  spec -- with UNROLL independent loads in flight, keeps the three f64 partials in registers, counts the non-finite frames
//                  with a ballot, and reduces with the spec's butterfly across the wave.  Frames past the tick read as +0.0 and add
//                  (+0.0)(+0.0) = +0.0, which changes no partial: a partial is never -0.0 (it starts as +0.0, and a sum of two numbers is -0.0
//                  only when both are), s + 0.0 == s for every other s, NaN included.  With a goniometer the same wave plots the frames it
//                  has just loaded: non-returning u32 atomics straight into the record of the tick's emission group (or into the carried
//                  grid, for the group the run ends in), after the lanes of the wave that hit the same cell have been merged into one add
//                  for up to GON_MERGE distinct cells -- silence, a mono signal at low level and a hard-panned one put a whole wave into one
//                  or two cells.  A tick is `frames` hits against grid^2 cells, so a grid staged in LDS would be cleared and flushed at 5 to
//                  20 words per hit; DESIGN.md section 0.6 has the argument and the measurement.
// k_stereo_window  one lane per (tap, tick) sums the three windows afresh in ascending tick, k_loud_window's shape; the further lanes of the
//                  same launch write the history the next run reads, out of place.
//
// Arithmetic: (double)x * (double)y is exact in f64 (24 + 24 bits), so fused or not it rounds nowhere; every add is one f64 rounding.  m = L + R,
// s = L - R and their products with the power of two z are single f32 operations; f32 subnormals must reach them unflushed (default f32
// denormal mode, as for the meters).  Counts are integers: the order of the atomics cannot matter.
#include "mx_dev.hpp"

namespace mx {

static constexpr uint32_t STEREO_WAVES = 4;   // waves per block of k_stereo_reduce
static constexpr int GON_MERGE = 4;           // distinct cells per wave-load whose lanes are merged into one atomic each

__device__ __forceinline__ double stereo_butterfly(double s) {   // s[j] = s[j] + s[j ^ k]; addition commutes bit for bit, so lane 0 holds the spec's s[0]
    for (int k = 32; k >= 1; k >>= 1) s = s + __shfl_xor(s, k, 64);
    return s;
}
__device__ __forceinline__ bool finite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

struct GonTarget { uint32_t* tab; float z, half; uint32_t grid; };

// the cell of one coordinate: floorf(v * z) clamped to [-grid / 2, grid / 2 - 1], moved to 0 .. grid - 1
__device__ __forceinline__ uint32_t gon_cell(float v, const GonTarget& g) {
    const float t = fminf(fmaxf(floorf(v * g.z), -g.half), g.half - 1.0f);
    return (uint32_t)((int)t + (int)g.half);
}

__device__ __forceinline__ void gon_plot(const GonTarget& g, bool ok, float l, float r, uint32_t lane) {
    l = ok ? l : 0.0f; r = ok ? r : 0.0f;
    const float m = l + r, s = l - r;
    const uint32_t idx = min(gon_cell(m, g) * g.grid + gon_cell(s, g), g.grid * g.grid - 1u);
    unsigned long long todo = __ballot(ok);
    for (int round = 0; round < GON_MERGE && todo; ++round) {   // wave-uniform
        const int lead = __ffsll((long long)todo) - 1;
        const uint32_t c = (uint32_t)__shfl((int)idx, lead, 64);
        const unsigned long long same = __ballot(ok && idx == c);
        if (lane == (uint32_t)lead) atomicAdd(g.tab + c, (uint32_t)__popcll(same));
        todo &= ~same;
        ok = ok && idx != c;
    }
    if (ok) atomicAdd(g.tab + idx, 1u);
}

struct StereoAcc {
    double ll = 0.0, rr = 0.0, lr = 0.0;
    __device__ __forceinline__ void add(float l, float r) {
        const double a = (double)l, b = (double)r;
        ll = ll + a * a; rr = rr + b * b; lr = lr + a * b;
    }
};

template <bool GON, bool DUP, uint32_t UNROLL>
__device__ __forceinline__ uint32_t stereo_tick(const float* __restrict__ p, uint32_t F, uint32_t lane, StereoAcc& acc, const GonTarget& g) {
    uint32_t bad = 0;
    for (uint32_t f0 = lane; f0 < F; f0 += 64u * UNROLL) {   // f0 - lane is wave-uniform
        float2 x[UNROLL];
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) {
            const uint32_t f = f0 + 64u * u;
            if (DUP) { const float v = f < F ? p[f] : 0.0f; x[u] = make_float2(v, v); }
            else x[u] = f < F ? reinterpret_cast<const float2*>(p)[f] : make_float2(0.0f, 0.0f);   // 8-byte aligned, as k_meter_reduce's
        }
#pragma unroll
        for (uint32_t u = 0; u < UNROLL; ++u) {   // ascending f: the loads above are all in flight before the first add
            if (f0 - lane + 64u * u >= F) break;   // (wave-uniform: a load of which every lane lies past the tick)
            const bool in = f0 + 64u * u < F, fin = finite_bits(x[u].x) && finite_bits(x[u].y);
            bad += (uint32_t)__popcll(__ballot(in && !fin));
            acc.add(x[u].x, x[u].y);
            if (GON) gon_plot(g, in && fin, x[u].x, x[u].y, lane);
        }
    }
    return bad;
}

template <bool GON>
__global__ __launch_bounds__(64 * STEREO_WAVES) void k_stereo_reduce(const StereoRun r) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t pairs = (uint64_t)r.n * r.n_ticks;
    const uint64_t waves = (uint64_t)gridDim.x * STEREO_WAVES;
    for (uint64_t w = (uint64_t)blockIdx.x * STEREO_WAVES + (threadIdx.x >> 6); w < pairs; w += waves) {   // wave-uniform
        const uint32_t i = (uint32_t)(w / r.n_ticks), t = (uint32_t)(w - (uint64_t)i * r.n_ticks);   // consecutive waves: consecutive ticks of one tap
        const TapDesc d = r.desc[i];
        const uint32_t F = d.frames;
        GonTarget g{nullptr, 0.0f, 0.0f, 0u};
        uint32_t* head = nullptr;
        if (GON) {
            const uint32_t grp = (r.phase + t) / r.hop;   // <= n_emit
            head = grp < r.n_emit ? r.gon_rec + ((size_t)grp * r.stride + d.slot) * r.rec_words : r.gon_carry + (size_t)d.slot * r.rec_words;
            g = GonTarget{head + 8, (float)((r.grid >> 2) << r.zoom_log2), (float)(r.grid >> 1), r.grid};
        }
        StereoAcc acc;
        const uint32_t bad = d.layout == METER_DUP ? stereo_tick<GON, true, 8>(d.p + (size_t)t * F, F, lane, acc, g)
                                                   : stereo_tick<GON, false, 8>(d.p + (size_t)t * 2u * F, F, lane, acc, g);
        const double ll = stereo_butterfly(acc.ll), rr = stereo_butterfly(acc.rr), lr = stereo_butterfly(acc.lr);
        if (lane == 0) {
            StereoTick* rec = r.rec + (size_t)t * r.stride + d.slot;   // win_*: k_stereo_window
            rec->sum_ll = ll; rec->sum_rr = rr; rec->sum_lr = lr;
            rec->frames = F; rec->nonfinite = bad;
            if (GON) { if (F - bad) atomicAdd(head + 2, F - bad); if (bad) atomicAdd(head + 3, bad); }
        }
    }
}

__global__ __launch_bounds__(256) void k_stereo_emit(const StereoRun r) {
    const uint64_t per_tap = (uint64_t)r.n_emit * r.rec_words, total = (uint64_t)r.n * per_tap;
    for (uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x; idx < total; idx += (uint64_t)gridDim.x * 256u) {
        const uint32_t i = (uint32_t)(idx / per_tap);
        const uint64_t rem = idx - (uint64_t)i * per_tap;
        const uint32_t e = (uint32_t)(rem / r.rec_words), w = (uint32_t)(rem - (uint64_t)e * r.rec_words);
        const uint32_t slot = r.desc[i].slot;
        uint32_t v = 0u;
        if (w == 0) v = r.hop - 1u - r.phase + e * r.hop;   // the emitting tick
        else if (w == 1) v = r.hop;
        else if (w == 4) v = r.grid;
        else if (w == 5) v = r.zoom_log2;
        else if (w != 6 && w != 7 && e == 0) {              // frames, skipped and the counts: what the ticks before this run left
            uint32_t* c = r.gon_carry + (size_t)slot * r.rec_words + w;
            v = *c; *c = 0u;
        }
        r.gon_rec[((size_t)e * r.stride + slot) * r.rec_words + w] = v;
    }
}

__global__ __launch_bounds__(256) void k_stereo_window(const StereoRun r) {
    const uint32_t per_tap = r.n_ticks + STEREO_HIST_TICKS;
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)r.n * per_tap) return;
    const uint32_t i = (uint32_t)(idx / per_tap), j = (uint32_t)(idx - (uint64_t)i * per_tap);
    const uint32_t slot = r.desc[i].slot;
    const double* __restrict__ hin = r.hist_in + (size_t)slot * STEREO_HIST_TICKS * 3u;
    // the three sums of tick u of the run (u >= -1023), from the history before the run
    auto sums = [&](int64_t u, double& a, double& b, double& c) {
        if (u < 0) { const double* h = hin + ((int64_t)STEREO_HIST_TICKS + u) * 3; a = h[0]; b = h[1]; c = h[2]; return; }
        const StereoTick* rec = r.rec + (size_t)u * r.stride + slot;
        a = rec->sum_ll; b = rec->sum_rr; c = rec->sum_lr;
    };
    if (j >= r.n_ticks) {   // the history the next run reads
        const uint32_t k = j - r.n_ticks;
        double a, b, c;
        sums((int64_t)r.n_ticks - (int64_t)STEREO_HIST_TICKS + k, a, b, c);
        double* h = r.hist_out + ((size_t)slot * STEREO_HIST_TICKS + k) * 3u;
        h[0] = a; h[1] = b; h[2] = c;
        return;
    }
    double wl = 0.0, wr = 0.0, wx = 0.0;
    for (uint32_t back = r.window_ticks; back-- > 0;) {   // ascending tick: j - back
        double a, b, c;
        sums((int64_t)j - back, a, b, c);
        wl = wl + a; wr = wr + b; wx = wx + c;
    }
    StereoTick* rec = r.rec + (size_t)j * r.stride + slot;
    rec->win_ll = wl; rec->win_rr = wr; rec->win_lr = wx;
}

void launch_taps(const StereoRun& r, hipStream_t s) {
    if (!r.n || !r.n_ticks) return;
    if (r.grid && r.n_emit) {
        const uint64_t words = (uint64_t)r.n * r.n_emit * r.rec_words;
        hipLaunchKernelGGL(k_stereo_emit, dim3((uint32_t)std::min<uint64_t>((words + 255u) / 256u, 256u * 16u)), dim3(256), 0, s, r);
    }
    const uint64_t pairs = (uint64_t)r.n * r.n_ticks;
    const dim3 grid((uint32_t)std::min<uint64_t>((pairs + STEREO_WAVES - 1) / STEREO_WAVES, 256u * 16u)), block(64 * STEREO_WAVES);   // grid-stride beyond 16 blocks per CU
    if (r.grid) hipLaunchKernelGGL(k_stereo_reduce<true>, grid, block, 0, s, r);
    else hipLaunchKernelGGL(k_stereo_reduce<false>, grid, block, 0, s, r);
    const uint64_t items = (uint64_t)r.n * (r.n_ticks + STEREO_HIST_TICKS);
    hipLaunchKernelGGL(k_stereo_window, dim3((uint32_t)((items + 255u) / 256u)), dim3(256), 0, s, r);
}

}  // namespace mx
