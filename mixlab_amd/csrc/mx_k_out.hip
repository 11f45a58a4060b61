// mx_k_out.hip -- OutputDevice (src/module/output_device.rs:174-246): what run_tick computes on the tick thread, for every tick of a span.
//
// k_out_route  routes the stereo input into the device's C-channel interleaved frame (scratch[C i + left] = L[i], then
//              scratch[C i + right] = R[i]: right wins when left == right, :188-208) for every tick of the span at once.  A position
//              without an assigned channel takes the persistent scratch: between two updates only the assigned positions of the scratch
//              change from tick to tick, so every tick of a span reads the same scratch there.  The blocks of the span's LAST tick write
//              the assigned positions back into the scratch -- the positions they read are the other ones, so no block reads what another
//              writes.  The clip test (:192-194, :202-204) looks at the samples WRITTEN only; every block leaves one partial per tick.
//              Algorithmic bytes per frame: 8 read (L, R) + 4 C written.
// k_out_scan   one workgroup: ORs the partials of each tick and scans the ticks in order against the node's device state
//              (last clip / last lag / statuses): util::temporal_warning on the graph's sample clock, the per-tick indication
//              record, then the state the next span starts from.
#include "mx_dev.hpp"

namespace mx {

static constexpr uint32_t OUT_CHUNK = 2048;   // floats of one tick's hand-off per block (256 lanes x 8)

uint32_t out_route_blocks(size_t frames_per_tick, uint32_t channels) {
    return (uint32_t)(((size_t)frames_per_tick * channels + OUT_CHUNK - 1) / OUT_CHUNK);
}

__global__ __launch_bounds__(256) void k_out_route(const float* __restrict__ in, uint32_t dup, uint32_t F, uint32_t C, int32_t left, int32_t right,
                                                   uint32_t nb, uint32_t n_ticks, float* scratch, float* __restrict__ out, uint32_t* __restrict__ partial) {
    const uint32_t t = blockIdx.x / nb, b = blockIdx.x - t * nb;
    const uint32_t per_tick = F * C;
    const uint32_t p0 = b * OUT_CHUNK, p1 = min(per_tick, p0 + OUT_CHUNK);
    const float* src = in + (size_t)t * F * (dup ? 1u : 2u);
    float* dst = out + (size_t)t * per_tick;
    const bool last = t + 1 == n_ticks;
    int clip = 0;
    for (uint32_t p = p0 + threadIdx.x; p < p1; p += 256) {
        const uint32_t i = p / C;
        const int32_t c = (int32_t)(p - i * C);
        float v = 0.f;
        bool assigned = false;
        if (c == left) {
            const float x = dup ? src[i] : src[2 * i];
            clip |= (x < -1.0f || x > 1.0f);   // NaN and +-1.0 do not clip
            v = x; assigned = true;
        }
        if (c == right) {
            const float x = dup ? src[i] : src[2 * i + 1];
            clip |= (x < -1.0f || x > 1.0f);
            v = x; assigned = true;
        }
        if (!assigned) v = scratch[p];
        else if (last) scratch[p] = v;
        dst[p] = v;
    }
    clip = __syncthreads_or(clip);
    if (threadIdx.x == 0) partial[blockIdx.x] = clip ? 1u : 0u;
}

// util.rs temporal_warning on sample counts: Active when (now - last) * 10 < rate (100 ms), Recent when now - last < 5 rate (5 s).
// Signed: a run whose first tick lies before a recorded event (a host that restarted its tick count) sees a negative distance, which is
// Active -- as the numpy model computes it; the reference's Instant never goes back (mixlab_gpu.h, MX_KIND_OUTPUT_DEVICE's clock).
__device__ __forceinline__ uint32_t out_status(uint64_t now, int64_t last, uint32_t rate) {
    if (last < 0) return 0u;
    const int64_t d = (int64_t)now - last;
    if (d * 10 < (int64_t)rate) return 2u;
    if (d < 5ll * rate) return 1u;
    return 0u;
}

__global__ __launch_bounds__(256) void k_out_scan(const uint32_t* __restrict__ partial, uint32_t nb, uint32_t n_ticks, OutState* st, uint64_t t0, uint32_t spt,
                                                  uint32_t rate, uint32_t lag, uint32_t C, OutTick* __restrict__ rec) {
    __shared__ int64_t s_last[256];
    __shared__ uint32_t s_cs[256], s_ls[256];
    const uint32_t tid = threadIdx.x;
    const OutState S = *st;
    int64_t carry_clip = S.last_clip;
    const int64_t last_lag = lag ? (int64_t)t0 : S.last_lag;   // the flag is swapped at the span's first tick (:219)
    uint32_t prev_cs = S.clip_status, prev_ls = S.lag_status;
    for (uint32_t base = 0; base < n_ticks; base += 256) {
        const uint32_t k = base + tid;
        const bool valid = k < n_ticks;
        uint32_t clip = 0;
        if (valid) for (uint32_t j = 0; j < nb; ++j) clip |= partial[(size_t)k * nb + j];
        const uint64_t now = t0 + (uint64_t)k * spt;
        s_last[tid] = (valid && clip) ? (int64_t)now : -1;
        __syncthreads();
        for (uint32_t off = 1; off < 256; off <<= 1) {   // inclusive prefix max: the latest clipping tick up to k
            const int64_t o = tid >= off ? s_last[tid - off] : -1;
            __syncthreads();
            if (o > s_last[tid]) s_last[tid] = o;
            __syncthreads();
        }
        const int64_t lc = s_last[tid] > carry_clip ? s_last[tid] : carry_clip;
        const uint32_t cs = out_status(now, lc, rate), ls = out_status(now, last_lag, rate);
        s_cs[tid] = cs; s_ls[tid] = ls;
        __syncthreads();
        const uint32_t pcs = tid ? s_cs[tid - 1] : prev_cs, pls = tid ? s_ls[tid - 1] : prev_ls;
        if (valid) {
            OutTick r;
            r.clip = (uint8_t)clip; r.clip_status = (uint8_t)cs; r.lag_status = (uint8_t)ls;
            r.changed = (uint8_t)((cs != pcs || ls != pls) ? 1 : 0); r.channels = C;
            rec[k] = r;
        }
        const uint32_t lastv = min(255u, n_ticks - 1 - base);
        if (s_last[lastv] > carry_clip) carry_clip = s_last[lastv];
        prev_cs = s_cs[lastv]; prev_ls = s_ls[lastv];
        __syncthreads();   // the next chunk overwrites the arrays
    }
    if (tid == 0) {
        OutState o;
        o.last_clip = carry_clip; o.last_lag = last_lag; o.clip_status = prev_cs; o.lag_status = prev_ls;
        *st = o;
    }
}

void launch_output_device(const OutRun& r, hipStream_t s) {
    if (!r.n_ticks) return;
    uint32_t nb = 0;
    if (r.channels) {
        nb = out_route_blocks(r.frames, r.channels);
        hipLaunchKernelGGL(k_out_route, dim3(nb * r.n_ticks), dim3(256), 0, s, r.in, r.dup, r.frames, r.channels, r.left, r.right,
                           nb, r.n_ticks, r.scratch, r.out, r.partial);
    }
    hipLaunchKernelGGL(k_out_scan, dim3(1), dim3(256), 0, s, r.partial, nb, r.n_ticks, r.state, r.t0, r.spt, r.rate, r.lag, r.channels, r.rec);
}

}  // namespace mx
