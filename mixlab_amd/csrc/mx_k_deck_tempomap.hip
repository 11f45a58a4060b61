// mx_k_deck_tempomap.hip -- the deck's tempo map (include/mixlab_gpu.h "the deck", TEMPO MAP): FINE GRID's tooth weights of the whole track
// (k_fine_onsets, launched as it is), then a comb of every candidate period at every phase inside every window of them.
//
// k_tempo_comb    the hot path: a workgroup of TM_LANES = 256 takes one window v and TM_GROUP = 8 neighbouring candidates of it, one after the other; a lane per
//                 phase (candidates with more phases loop in strides of 256), so at tooth k a wave reads the window's w at consecutive addresses.  Two forms of one
//                 body:
//                   STAGED  the workgroup first copies its window's slice w[v T .. E_v) into LDS (dynamic, sized to the window: at most TM_STAGED_MAX words under the
//                           host's rule below, 16384 = 64 KB when a cost tool forces the form) and every candidate of the group walks that copy: the slice crosses
//                           from L2 once a workgroup instead of once a candidate;
//                   GLOBAL  every tooth is read from w itself, as k_fine_comb does.
//                 Either way the loop over k is a bounded for whose trip count comes from the host (the teeth of phase 0 at the smallest period in a full window),
//                 the load is unconditional from an index clamped into the window (E_v - v T >= 1), and only what is added depends on the comparison with the
//                 window's end -- i_k never decreases with k, so a tooth beyond the end adding nothing equals stopping at the first one.  Unrolled by eight.  The
//                 index inside a window is below 2^15 + 2^12 * 2^15: 32 bits.  S is a 64-bit sum.  The maximum under the tie rule (largest S, smallest phi) is taken
//                 per lane in ascending phi and across the wave by shuffles; the four waves' results of all candidates of the group go through LDS once, after one
//                 barrier, and lane g finishes candidate g with one 16-byte record store.  Lane 0 always has phase 0, so a candidate of nothing but zeros reports
//                 phase 0 and phase 0's teeth.
// Integers throughout: no order of accumulation matters.  No scratch.
#include "mx_deck_tempomap.hpp"

namespace mx {

template <bool STAGED>
__global__ __launch_bounds__(TM_LANES) void k_tempo_comb(const uint32_t* __restrict__ w, uint32_t N, uint32_t W, uint32_t T, uint32_t n_periods, uint32_t groups,
                                                         uint64_t period0, uint64_t dperiod, uint32_t trip, mx_deck_comb* __restrict__ rec) {
    extern __shared__ uint32_t slice[];                        // STAGED: the window's w
    __shared__ unsigned long long ws[TM_GROUP][TM_LANES / 64];
    __shared__ uint32_t wp[TM_GROUP][TM_LANES / 64], wn[TM_GROUP][TM_LANES / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t v = blockIdx.x / groups, j0 = (blockIdx.x - v * groups) * TM_GROUP;   // (the grid is V * groups: v < V, so v T < N)
    const uint32_t len = tm_window_len(v, W, T, N);            // >= 1
    const uint32_t* __restrict__ src = w + (size_t)v * T;      // src[0 .. len) lies inside w
    if (STAGED) {
        for (uint32_t i = tid; i < len; i += TM_LANES) slice[i] = src[i];
        __syncthreads();
    }
    const uint32_t cands = n_periods - j0 < (uint32_t)TM_GROUP ? n_periods - j0 : (uint32_t)TM_GROUP;   // workgroup-uniform; j0 < n_periods
    for (uint32_t g = 0; g < cands; ++g) {
        const uint64_t P = period0 + (uint64_t)(j0 + g) * dperiod;
        const uint32_t phases = fg_phases(P);
        unsigned long long best = 0ull; uint32_t best_phi = 0xffffffffu, best_n = 0u;   // a lane without a phase loses every comparison
        for (uint32_t phi = tid; phi < phases; phi += TM_LANES) {
            unsigned long long S = 0ull, kp = 0ull; uint32_t n = 0u;
#pragma unroll 8
            for (uint32_t k = 0; k < trip; ++k) {   // uniform bound from the host
                const uint32_t i = phi + (uint32_t)(kp >> 16);
                const bool in = i < len;
                const uint32_t at = in ? i : len - 1u;   // always inside the window
                const uint32_t x = STAGED ? slice[at] : src[at];
                S += in ? x : 0u; n += in ? 1u : 0u;
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
        if ((tid & 63u) == 0u) { ws[g][tid >> 6] = best; wp[g][tid >> 6] = best_phi; wn[g][tid >> 6] = best_n; }
    }
    __syncthreads();
    if (tid < cands) {
        unsigned long long best = ws[tid][0]; uint32_t best_phi = wp[tid][0], best_n = wn[tid][0];
        for (uint32_t q = 1; q < TM_LANES / 64; ++q)
            if (fg_better(ws[tid][q], wp[tid][q], best, best_phi)) { best = ws[tid][q]; best_phi = wp[tid][q]; best_n = wn[tid][q]; }
        mx_deck_comb r; r.score = best; r.phase = best_phi; r.beats = best_n;
        rec[(size_t)v * n_periods + j0 + tid] = r;   // (v < V, j0 + tid < n_periods)
    }
}

// The host's rule between the two forms (DESIGN.md section 0.22 has the figures).  Staging needs a second candidate to read the copy again, and it costs occupancy: a
// slice of 4 len + 512 bytes a workgroup out of a CU's 160 KiB.  Measured on a ten-minute track at h = 64: with four workgroups a CU (W = 8825) staged is 14 % ahead,
// with three (W = 11654) the two tie, with two (W = 16384) reading from memory is 23 % ahead; a single candidate is 5 % faster from memory.  So: stage when there are
// at least two candidates and four slices fit a CU -- (4 * TM_STAGED_MAX + 512) * 4 = 163840.
static_assert((4 * TM_STAGED_MAX + 512) * 4 == 160 * 1024, "four staged workgroups fill a CU's LDS exactly");
static bool tm_staged(const DkTempoArgs& a) {
    if (a.form != TM_FORM_RULE) return a.form == TM_FORM_STAGED;
    return a.n_periods >= 2u && (a.W < a.N ? a.W : a.N) <= (uint32_t)TM_STAGED_MAX;
}

void launch_deck_tempomap_comb(const DkTempoArgs& a, uint32_t forms[4], hipStream_t s) {
    const uint32_t groups = (a.n_periods + TM_GROUP - 1u) / TM_GROUP, wgs = a.V * groups;   // at most 2^20
    const bool staged = tm_staged(a);
    if (staged) {
        const uint32_t longest = a.W < a.N ? a.W : a.N;   // <= 16384 words (a forced form; the rule stops at TM_STAGED_MAX)
        const size_t bytes = (size_t)longest * sizeof(uint32_t);
        hip_check(hipFuncSetAttribute((const void*)k_tempo_comb<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes), "hipFuncSetAttribute(deck tempo map)");
        hipLaunchKernelGGL(k_tempo_comb<true>, dim3(wgs), dim3(TM_LANES), bytes, s, (const uint32_t*)a.w, a.N, a.W, a.T, a.n_periods, groups, a.period0, a.dperiod, a.trip, a.rec);
    } else {
        hipLaunchKernelGGL(k_tempo_comb<false>, dim3(wgs), dim3(TM_LANES), 0, s, (const uint32_t*)a.w, a.N, a.W, a.T, a.n_periods, groups, a.period0, a.dperiod, a.trip, a.rec);
    }
    forms[DK_TEMPO_FORM_STAGED] = staged ? wgs : 0u; forms[DK_TEMPO_FORM_GLOBAL] = staged ? 0u : wgs;
    forms[DK_TEMPO_FORM_TRIP] = a.trip;
}

void launch_deck_tempomap(const DkTempoArgs& a, uint32_t forms[4], hipStream_t s) {
    forms[DK_TEMPO_FORM_ONSET] = launch_deck_fine_onsets(a.track, a.n_frames, a.log_hop, a.N, a.w, s);
    launch_deck_tempomap_comb(a, forms, s);
}

}  // namespace mx
