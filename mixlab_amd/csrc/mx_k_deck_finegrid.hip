// mx_k_deck_finegrid.hip -- the deck's fine beat grid (include/mixlab_gpu.h "the deck", FINE GRID): the tooth weights of the whole track, then a
// comb of every candidate period at every phase over them.
//
// k_fine_onsets   a workgroup of 256 writes w for FG_TILE = 256 hops.  It needs A of the two hops before them and the one after, so it sums e for 259 hops itself --
//                 nothing depends on another workgroup.  A lane per frame, consecutive lanes at consecutive frames: one 32-bit load a frame, bounds-checked against
//                 [0, n_frames).  h >= 16, so 16 aligned lanes share a hop: s^2 is summed over them by shuffles and one lane adds it to the hop's 64-bit word in LDS.
//                 Then a lane per hop takes the exact root (mx_dev.hpp tempo_root, the tempo taps'), and a lane per output hop the three onsets and the weight.
//                 Hops outside [0, N) have e = 0, hence A = 0 and o = 0 without a special case: A[-1] = 0 and "o is 0 outside" are what the arithmetic gives.
// k_fine_comb     the hot path: a workgroup of FG_LANES = 256 per candidate, a lane per phase (candidates with more phases loop in strides of 256), so at tooth k a
//                 wave reads w[first_hop + phi + ((k P) >> 16)] at consecutive addresses.  k P is carried as a 64-bit sum (k < 2^24, P < 2^31 + 1: below 2^56).
//                 The loop over k is a bounded for: its trip count comes from the host (the teeth of phase 0 at the smallest period, or max_beats), and a tooth
//                 beyond the track adds nothing -- i_k never decreases with k, so that equals stopping at the first one.  The load itself is unconditional, from
//                 an index clamped into w, and only what is added depends on the comparison: the loop, unrolled by eight, then has eight loads in flight a lane.
//                 (With the load under the comparison a lane waited out one L2 access per tooth: stage two of a ten-minute track took 0.63 ms instead of 0.23;
//                 DESIGN.md section 0.19.)  S is a 64-bit sum (w <= 2^18, up to 2^24 teeth: below 2^44).  The maximum under the tie rule (largest S, smallest
//                 phi) is taken per lane in ascending phi, across the wave by shuffles, across the four waves through LDS; one 16-byte record store per
//                 candidate.  Lane 0 always has phase 0, so a candidate of nothing but zeros reports phase 0.
// Integers throughout: no order of accumulation matters.  No scratch.
#include "mx_deck_finegrid.hpp"

namespace mx {

enum { FG_HOPS = FG_TILE + FG_HALO_BEFORE + FG_HALO_AFTER };

__global__ __launch_bounds__(256) void k_fine_onsets(const uint32_t* __restrict__ track, int64_t n_frames, uint32_t log_h, uint32_t N, uint32_t* __restrict__ w) {
    __shared__ unsigned long long e[FG_HOPS];
    __shared__ uint32_t A[FG_HOPS];
    const uint32_t tid = threadIdx.x;
    const int64_t i0 = (int64_t)blockIdx.x * FG_TILE;        // the first hop written; local hop j is hop i0 - 2 + j
    for (uint32_t j = tid; j < FG_HOPS; j += 256u) e[j] = 0ull;
    __syncthreads();
    const int64_t f0 = (i0 - FG_HALO_BEFORE) * ((int64_t)1 << log_h);   // (negative in the first workgroup)
    const uint32_t frames = (uint32_t)FG_HOPS << log_h;                  // a multiple of 16: a group of 16 aligned lanes is inside or outside together
    for (uint32_t t0 = 0; t0 < frames; t0 += 256u) {                     // workgroup-uniform
        const uint32_t t = t0 + tid;
        const int64_t f = f0 + (int64_t)t;
        unsigned long long v = (t < frames && f >= 0 && f < n_frames) ? fg_square(track[f]) : 0ull;
#pragma unroll
        for (int off = 8; off; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((tid & 15u) == 0u && v) atomicAdd(e + (t >> log_h), v);      // (v != 0 only with t < frames: t >> log_h < FG_HOPS)
    }
    __syncthreads();
    for (uint32_t j = tid; j < FG_HOPS; j += 256u) A[j] = tempo_root(e[j]);
    __syncthreads();
    const int64_t i = i0 + tid;
    if (i < (int64_t)N) w[i] = fg_tooth(fg_onset(A[tid + 1u], A[tid]), fg_onset(A[tid + 2u], A[tid + 1u]), fg_onset(A[tid + 3u], A[tid + 2u]));
}

__global__ __launch_bounds__(FG_LANES) void k_fine_comb(const uint32_t* __restrict__ w, uint32_t N, uint32_t first_hop, uint64_t period0, uint64_t dperiod, uint32_t trip,
                                                        mx_deck_comb* __restrict__ rec) {
    __shared__ unsigned long long ws[FG_LANES / 64];
    __shared__ uint32_t wp[FG_LANES / 64], wn[FG_LANES / 64];
    const uint32_t tid = threadIdx.x;
    const uint64_t P = period0 + (uint64_t)blockIdx.x * dperiod;
    const uint32_t phases = fg_phases(P);
    unsigned long long best = 0ull; uint32_t best_phi = 0xffffffffu, best_n = 0u;   // a lane without a phase loses every comparison
    for (uint32_t phi = tid; phi < phases; phi += FG_LANES) {
        const uint64_t base = (uint64_t)first_hop + phi;
        unsigned long long S = 0ull, kp = 0ull; uint32_t n = 0u;
#pragma unroll 8
        for (uint32_t k = 0; k < trip; ++k) {   // uniform bound from the host
            const uint64_t i = base + (kp >> 16);
            const bool in = i < N;
            const uint32_t v = w[in ? i : (uint64_t)N - 1u];   // the index is always inside w (N >= 1), so the eight loads of a round are issued together
            S += in ? v : 0u; n += in ? 1u : 0u;
            kp += P;
        }
        if (fg_better(S, phi, best, best_phi)) { best = S; best_phi = phi; best_n = n; }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const unsigned long long s2 = __shfl_xor(best, off, 64);
        const uint32_t p2 = (uint32_t)__shfl_xor((int)best_phi, off, 64), n2 = (uint32_t)__shfl_xor((int)best_n, off, 64);
        if (fg_better(s2, p2, best, best_phi)) { best = s2; best_phi = p2; best_n = n2; }
    }
    if ((tid & 63u) == 0u) { ws[tid >> 6] = best; wp[tid >> 6] = best_phi; wn[tid >> 6] = best_n; }
    __syncthreads();
    if (tid == 0u) {
        for (uint32_t v = 1; v < FG_LANES / 64; ++v)
            if (fg_better(ws[v], wp[v], best, best_phi)) { best = ws[v]; best_phi = wp[v]; best_n = wn[v]; }
        mx_deck_comb r; r.score = best; r.phase = best_phi; r.beats = best_n;
        rec[blockIdx.x] = r;   // (blockIdx.x < n_periods: the grid is n_periods)
    }
}

uint32_t launch_deck_fine_onsets(const uint32_t* track, int64_t n_frames, uint32_t log_hop, uint32_t N, uint32_t* w, hipStream_t s) {
    const uint32_t onset_wgs = (N + FG_TILE - 1u) / FG_TILE;   // (N <= 2^26: at most 2^18)
    hipLaunchKernelGGL(k_fine_onsets, dim3(onset_wgs), dim3(256), 0, s, track, n_frames, log_hop, N, w);
    return onset_wgs;
}

void launch_deck_finegrid(const DkFineArgs& a, uint32_t forms[4], hipStream_t s) {
    const uint32_t onset_wgs = launch_deck_fine_onsets(a.track, a.n_frames, a.log_hop, a.N, a.w, s);
    hipLaunchKernelGGL(k_fine_comb, dim3(a.n_periods), dim3(FG_LANES), 0, s, (const uint32_t*)a.w, a.N, a.first_hop, a.period0, a.dperiod, a.trip, a.rec);
    forms[DK_FINE_FORM_ONE_PASS] = forms[DK_FINE_FORM_STRIDED] = 0u;
    for (uint32_t j = 0; j < a.n_periods; ++j) ++forms[fg_phases(a.period0 + (uint64_t)j * a.dperiod) <= FG_LANES ? DK_FINE_FORM_ONE_PASS : DK_FINE_FORM_STRIDED];
    forms[DK_FINE_FORM_ONSET] = onset_wgs; forms[DK_FINE_FORM_TRIP] = a.trip;
}

}  // namespace mx
