// mx_k_tempo.hip -- tempo taps on audio output ports (mixlab_gpu.h mx_graph_set_tempo): once per run, for every tap.
//
// k_tempo_emit    only in a run that emits: one thread per (tap, emission) writes the record's header -- the emitting tick, hops_complete from
//                 the frame counts, and as nonfinite what the ticks before this run left (first record; it clears that count) or zero.
// k_tempo_energy  one wave per (tap, hop the run touches).  The run's ticks lie back to back in the port buffer and the stream position of its
//                 first frame is known, so a hop is a stretch of the buffer: lane l takes frames l, l + 64, ... of it (H / 64 each), forms
//                 m = L + R, quantises, squares, and the wave adds up with shfl_xor -- 64-bit integer sums, so no order matters.  The run's
//                 first hop adds the carried partial on; the hop the run ends in hands its sum on as the next partial (or zero, where the
//                 run ends on a hop's last frame); a complete hop stores E.  A non-finite frame -- rare -- is added with one atomic to the
//                 record of its tick's emission, or to the carried count for the ticks behind the run's last emission.
// k_tempo_onsets  one thread per completed hop of a tap: the exact integer root of E[h] and of E[h - 1] (or the carried A), their clamped
//                 difference, the shift; written behind the tap's W + L - 1 carried onsets so that every emission of the run sees one linear
//                 array, and -- where it belongs to the last W + L - 1 -- into the next run's array.  Further threads of the same launch
//                 move the carried onsets that stay.  Nothing is read that the launch writes: the arrays, A and the partial are kept twice.
// k_tempo_acf     only in a run that emits: one workgroup of 256 per (tap, emission).  The W + L - 1 onsets that end in the emission's o[hl]
//                 are staged in LDS (at most 20 476 bytes).  A lane owns the lags l, l + 256, ... (one, two or four of them: L <= 256, 512,
//                 1024).  The loop over j takes 64 values of the uniform operand o[hl - j] per LDS read (lane b holds j0 + b), ballots the
//                 non-zero ones -- onsets are sparse -- and for each broadcasts it from its lane (v_readlane, no LDS) against o[hl - j - l],
//                 which consecutive lanes read at consecutive addresses: conflict-free.  One v_mad_u64_u32 per product.
//
// Arithmetic: m = L + R is the one f32 operation that rounds; |m| x 2^20 is exact; everything after is integer.  f32 subnormals cannot show:
// an m below 2^-20 quantises to 0 flushed or not.  No float accumulation anywhere.
#include "mx_dev.hpp"

namespace mx {

static constexpr uint32_t TEMPO_WAVES = 4;       // waves per block of k_tempo_energy
static constexpr uint32_t TEMPO_MAX_HIST = 4096 + 1024 - 1;

struct TempoTap { uint64_t pos, end; uint32_t h_first; uint32_t n_done; };   // the run of one tap: first frame, one past its last, the hop of pos, hops it completes
// (pos < 2^63 frames and a run's hops fit 32 bits: a run is at most 2^32 ticks of at most 2^30 frames ... / 64; the host refuses more)
__device__ __forceinline__ uint64_t tempo_pos(const TempoRun& r, const TempoDesc& d) { return d.pos0 + r.ticks0 * (uint64_t)d.frames; }

__device__ __forceinline__ uint32_t tempo_quantise(float l, float rr, bool& bad) {
    const float m = l + rr;
    bad = (__float_as_uint(m) & 0x7f800000u) == 0x7f800000u;
    return bad ? 0u : (uint32_t)(fminf(fabsf(m), 4.0f) * 1048576.0f);
}

__global__ __launch_bounds__(256) void k_tempo_emit(const TempoRun r) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)r.n * r.n_emit) return;
    const uint32_t i = (uint32_t)(idx / r.n_emit), e = (uint32_t)(idx - (uint64_t)i * r.n_emit);
    const TempoDesc d = r.desc[i];
    const uint32_t tick = r.emit_ticks - 1u - r.phase + e * r.emit_ticks;   // the emitting tick
    const uint64_t hops = (tempo_pos(r, d) + ((uint64_t)tick + 1u) * d.frames) >> r.log2_hop;
    uint32_t* w = r.rec + ((size_t)e * r.stride + d.slot) * r.rec_words;
    uint32_t bad = 0u;
    if (e == 0) { bad = r.nonfinite[d.slot]; r.nonfinite[d.slot] = 0u; }
    w[0] = tick; w[1] = (uint32_t)min(hops, (uint64_t)0xffffffffu); w[2] = bad; w[3] = 1u << r.log2_hop;
    w[4] = r.window_hops; w[5] = r.max_lag; w[6] = 0u; w[7] = 0u;
}

__global__ __launch_bounds__(64 * TEMPO_WAVES) void k_tempo_energy(const TempoRun r) {
    const uint32_t lane = threadIdx.x & 63u, H = 1u << r.log2_hop;
    const uint64_t pairs = (uint64_t)r.n * r.max_touched;
    const uint64_t waves = (uint64_t)gridDim.x * TEMPO_WAVES;
    for (uint64_t w = (uint64_t)blockIdx.x * TEMPO_WAVES + (threadIdx.x >> 6); w < pairs; w += waves) {   // wave-uniform
        const uint32_t i = (uint32_t)(w / r.max_touched), k = (uint32_t)(w - (uint64_t)i * r.max_touched);   // consecutive waves: consecutive hops of one tap
        const TempoDesc d = r.desc[i];
        const uint32_t F = d.frames;
        const uint64_t pos = tempo_pos(r, d), run_frames = (uint64_t)r.n_ticks * F, end = pos + run_frames;
        const uint64_t h_first = pos >> r.log2_hop;
        if (run_frames == 0) {   // (a port without frames: the partial is handed on as it is)
            if (k == 0 && lane == 0) r.part_out[d.slot] = r.part_in[d.slot];
            continue;
        }
        const uint32_t touched = (uint32_t)(((end - 1u) >> r.log2_hop) - h_first) + 1u, n_done = (uint32_t)((end >> r.log2_hop) - h_first);
        if (k >= touched) continue;
        // the hop's frames inside the run, counted from the run's first frame
        const uint64_t s0 = (h_first + k) << r.log2_hop;
        const uint64_t begin = s0 > pos ? s0 - pos : 0u, stop = min(run_frames, s0 + H - pos);
        uint64_t sum = 0u;
#pragma unroll
        for (uint32_t u = 0; u < 4u; ++u) {
            if (64u * u >= H) break;   // (wave-uniform)
            const uint64_t f = begin + lane + 64u * u;
            if (f < stop) {
                float a, b;
                if (d.layout == METER_STEREO) { const float2 x = reinterpret_cast<const float2*>(d.p)[f]; a = x.x; b = x.y; }
                else a = b = d.p[f];
                bool bad;
                const uint32_t q = tempo_quantise(a, b, bad);
                sum += (uint64_t)q * q;
                if (bad) {
                    const uint64_t grp = ((uint64_t)r.phase + f / F) / r.emit_ticks;   // the emission its tick belongs to
                    atomicAdd(grp < r.n_emit ? r.rec + ((size_t)grp * r.stride + d.slot) * r.rec_words + 2 : r.nonfinite + d.slot, 1u);
                }
            }
        }
        for (int x = 32; x >= 1; x >>= 1) sum += __shfl_xor(sum, x, 64);
        if (lane == 0) {
            if (k == 0) sum += r.part_in[d.slot];
            if (k < n_done) r.energy[(size_t)d.slot * r.e_stride + k] = sum;
            if (k == touched - 1u) r.part_out[d.slot] = k < n_done ? 0u : sum;
        }
    }
}

__global__ __launch_bounds__(256) void k_tempo_onsets(const TempoRun r) {
    const uint32_t hist = r.window_hops + r.max_lag - 1u;
    const uint64_t per_tap = (uint64_t)r.max_done + hist;
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= (uint64_t)r.n * per_tap) return;
    const uint32_t i = (uint32_t)(idx / per_tap), j = (uint32_t)(idx - (uint64_t)i * per_tap);
    const TempoDesc d = r.desc[i];
    const uint64_t pos = tempo_pos(r, d), end = pos + (uint64_t)r.n_ticks * d.frames;
    const uint32_t n_done = (uint32_t)((end >> r.log2_hop) - (pos >> r.log2_hop));
    uint32_t* lin = r.lin + (size_t)d.slot * r.lin_stride;
    uint32_t* next = r.lin_next + (size_t)d.slot * r.lin_stride;
    if (j >= r.max_done) {   // a carried onset that stays among the last W + L - 1
        const uint32_t k = j - r.max_done;
        if ((uint64_t)k + n_done < hist) next[k] = lin[k + n_done];
        if (k == 0 && n_done == 0) r.amp_out[d.slot] = r.amp_in[d.slot];
        return;
    }
    if (j >= n_done) return;
    const uint64_t* e = r.energy + (size_t)d.slot * r.e_stride;
    const uint32_t a = tempo_root(e[j]), before = j ? tempo_root(e[j - 1]) : r.amp_in[d.slot];
    const uint32_t o = (a > before ? a - before : 0u) >> 6;
    lin[hist + j] = o;
    if ((uint64_t)j + hist >= n_done) next[j + hist - n_done] = o;
    if (j == n_done - 1u) r.amp_out[d.slot] = a;
}

template <uint32_t LPT>
__global__ __launch_bounds__(256) void k_tempo_acf(const TempoRun r) {
    __shared__ uint32_t s[TEMPO_MAX_HIST + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t W = r.window_hops, L = r.max_lag, hist = W + L - 1u, top = hist - 1u;   // s[top] = o[hl]
    const uint64_t pairs = (uint64_t)r.n * r.n_emit;
    for (uint64_t pair = blockIdx.x; pair < pairs; pair += gridDim.x) {   // workgroup-uniform
        const uint32_t i = (uint32_t)(pair / r.n_emit), e = (uint32_t)(pair - (uint64_t)i * r.n_emit);
        const TempoDesc d = r.desc[i];
        const uint64_t pos = tempo_pos(r, d);
        const uint32_t tick = r.emit_ticks - 1u - r.phase + e * r.emit_ticks;
        // hops complete at the end of the emitting tick, counted from the hop of the run's first frame: o[hl] is lin[hist + done - 1]
        const uint32_t done = (uint32_t)(((pos + ((uint64_t)tick + 1u) * d.frames) >> r.log2_hop) - (pos >> r.log2_hop));
        const uint32_t* __restrict__ src = r.lin + (size_t)d.slot * r.lin_stride + done;
        for (uint32_t t = tid; t < hist; t += 256u) s[t] = src[t];
        __syncthreads();
        uint32_t back[LPT];   // the lane's lags (a lane beyond L reads lag L - 1 and stores nothing)
        uint64_t acc[LPT];
#pragma unroll
        for (uint32_t k = 0; k < LPT; ++k) { back[k] = min(tid + 256u * k, L - 1u); acc[k] = 0u; }
        for (uint32_t j0 = 0; j0 < W; j0 += 64u) {   // wave-uniform
            const uint32_t mine = j0 + lane < W ? s[top - j0 - lane] : 0u;
            unsigned long long todo = __ballot(mine != 0u);
            while (todo) {   // wave-uniform: the non-zero o[hl - j] of this stretch
                const uint32_t b = (uint32_t)__ffsll((long long)todo) - 1u;
                todo &= todo - 1u;
                const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)b);
                const uint32_t at = top - j0 - b;
#pragma unroll
                for (uint32_t k = 0; k < LPT; ++k) acc[k] += (uint64_t)a * s[at - back[k]];
            }
        }
        uint64_t* out = reinterpret_cast<uint64_t*>(r.rec + ((size_t)e * r.stride + d.slot) * r.rec_words + 8);
#pragma unroll
        for (uint32_t k = 0; k < LPT; ++k)
            if (tid + 256u * k < L) out[tid + 256u * k] = acc[k];
        __syncthreads();   // before the next pair overwrites s
    }
}

void launch_taps(const TempoRun& r, hipStream_t s) {
    if (!r.n || !r.n_ticks) return;
    const uint64_t pairs = (uint64_t)r.n * r.n_emit;
    if (r.n_emit) hipLaunchKernelGGL(k_tempo_emit, dim3((uint32_t)((pairs + 255u) / 256u)), dim3(256), 0, s, r);
    const uint64_t hops = (uint64_t)r.n * r.max_touched;
    hipLaunchKernelGGL(k_tempo_energy, dim3((uint32_t)std::min<uint64_t>((hops + TEMPO_WAVES - 1) / TEMPO_WAVES, 256u * 16u)), dim3(64 * TEMPO_WAVES), 0, s, r);   // grid-stride beyond 16 blocks per CU
    const uint64_t items = (uint64_t)r.n * ((uint64_t)r.max_done + r.window_hops + r.max_lag - 1u);
    hipLaunchKernelGGL(k_tempo_onsets, dim3((uint32_t)((items + 255u) / 256u)), dim3(256), 0, s, r);
    if (!r.n_emit) return;
    const dim3 grid((uint32_t)std::min<uint64_t>(pairs, 256u * 8u));   // 20 KB of LDS: eight workgroups per CU
    if (r.max_lag <= 256u) hipLaunchKernelGGL(k_tempo_acf<1>, grid, dim3(256), 0, s, r);
    else if (r.max_lag <= 512u) hipLaunchKernelGGL(k_tempo_acf<2>, grid, dim3(256), 0, s, r);
    else hipLaunchKernelGGL(k_tempo_acf<4>, grid, dim3(256), 0, s, r);
}

}  // namespace mx
