// mx_k_deck_keylock.hip -- the two kernels of a key-locked deck (include/mixlab_gpu.h "the deck", KEY-LOCK).
//
// k_deck_keylock_search   one workgroup per key-locked deck walks that deck's grains of the feed in order: the chain g[j-1] -> c -> delta[j] -> g[j] is sequential by
//                         definition.  Per searched grain the V reference sums s[C + i] and the V + 2R candidate sums s[A - R + i] are staged as int32 in LDS (16 KB at
//                         the most), bounds-checked there; a lane takes the candidates delta = -R + lane, + 256, ...: the reference read is a broadcast, the candidate
//                         reads are consecutive across lanes.  The argmin is one 64-bit key, D in the high half and the tie order (2 |delta| + (delta > 0)) below it,
//                         reduced in the wave by shuffles and across the four waves through LDS.  First grains and radius 0 run no search.  rec[0], rec[1] are the two
//                         grains before the feed's first (the deck's state buffer), rec[2 + k] grain k of the feed; the last two go back into the state buffer.
// k_deck_keylock_render   the grid of k_deck_feed over the key-locked decks: a workgroup per chunk of MX_DECK_CHUNK frames of a tick, a lane per output frame.  A lane
//                         derives (grain, m) from the tick's clock by shift and mask, reads g of its grain, runs the 32 taps at g + m p, and where it fades runs them a
//                         second time at g[j-1] + (H + m) p.  Lanes differ in phase unless p is a whole number of frames, so the bank is staged in LDS there (section
//                         0.15's finding) and read from the tables otherwise.  The taps gather from the track; a chunk may hold lanes of three grains (hop 256), so no
//                         window is staged.
// The arithmetic of a grain sample is the plain deck's (mx_k_deck.hip deck_taps), restated here so that file -- and the code of a plain feed -- stays as it was.
#include "mx_deck.hpp"
#include "mx_kernels.hpp"

namespace mx {

enum { KL_COEF_STRIDE = MX_DECK_TAPS + 1, KL_MAX_OVERLAP = 1024, KL_MAX_RADIUS = 1024, KL_LANES = 256 };

// s[f] = L[f] + R[f] of the raw track, 0 outside it
__device__ inline int32_t kl_sum(const KlDeckDev& d, int64_t f) {
    if (f < 0 || f >= d.n_frames) return 0;
    const uint32_t s = d.track[f];
    return (int32_t)(int16_t)(s & 0xffffu) + (int32_t)(int16_t)(s >> 16);
}

__global__ __launch_bounds__(KL_LANES) void k_deck_keylock_search(const KlDeckDev* __restrict__ decks) {
    __shared__ int32_t ref[KL_MAX_OVERLAP];
    __shared__ int32_t cand[KL_MAX_OVERLAP + 2 * KL_MAX_RADIUS];
    __shared__ unsigned long long wave_key[KL_LANES / 64];
    const KlDeckDev d = decks[blockIdx.x];
    const uint32_t lane = threadIdx.x, V = d.overlap, R = d.radius;
    int64_t g2 = d.state[0], g1 = d.state[1];   // every lane carries the chain; lane 0 stores it
    __syncthreads();                            // (the state is read by all before lane 0 writes it back)
    if (lane == 0) { d.rec[0] = KlRec{g2, 0, 0u}; d.rec[1] = KlRec{g1, 0, 0u}; }
    for (uint32_t k = 0; k < d.n_grains; ++k) {
        const KlGrainIn in = d.grains[k];
        int64_t g = in.a;
        int32_t delta = 0;
        uint32_t dist = 0;
        if (!in.first) {
            const int64_t c = g1 + ((int64_t)1 << d.log_hop) * d.pitch, C = c >> DECK_Q, A = in.a >> DECK_Q;
            if (R) {
                for (uint32_t i = lane; i < V; i += KL_LANES) ref[i] = kl_sum(d, C + (int64_t)i);
                for (uint32_t i = lane; i < V + 2 * R; i += KL_LANES) cand[i] = kl_sum(d, A - (int64_t)R + (int64_t)i);
                __syncthreads();
                unsigned long long key = ~0ull;
                for (uint32_t e = lane; e <= 2 * R; e += KL_LANES) {   // e = delta + R
                    uint32_t D = 0;
#pragma unroll 8
                    for (uint32_t i = 0; i < V; ++i) { const int32_t x = ref[i] - cand[e + i]; D += (uint32_t)(x < 0 ? -x : x); }
                    const int32_t dl = (int32_t)e - (int32_t)R;
                    const uint32_t tie = 2u * (uint32_t)(dl < 0 ? -dl : dl) + (dl > 0 ? 1u : 0u);
                    const unsigned long long kk = ((unsigned long long)D << 32) | tie;
                    key = kk < key ? kk : key;
                }
                for (int off = 32; off; off >>= 1) {
                    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), off), lo = (uint32_t)__shfl_xor((int)(uint32_t)key, off);
                    const unsigned long long other = ((unsigned long long)hi << 32) | lo;
                    key = other < key ? other : key;
                }
                if ((lane & 63u) == 0) wave_key[lane >> 6] = key;
                __syncthreads();
                key = wave_key[0];
                for (int w = 1; w < KL_LANES / 64; ++w) key = wave_key[w] < key ? wave_key[w] : key;
                const uint32_t tie = (uint32_t)key;
                delta = (tie & 1u) ? (int32_t)(tie >> 1) : -(int32_t)(tie >> 1);
                dist = (uint32_t)(key >> 32);
            }
            g = (A + (int64_t)delta) * ((int64_t)1 << DECK_Q) + (c - C * ((int64_t)1 << DECK_Q));
        }
        if (lane == 0) d.rec[2 + k] = KlRec{g, delta, dist};
        g2 = g1; g1 = g;
    }
    if (lane == 0) { d.state[0] = g2; d.state[1] = g1; }
}

// G(u): the deck's FILTER at position u (never folded), both channels, rounded to f32; rows from LDS (stride 33) or from the tables (stride 32) -- one or the other
// per call site, never a pointer chosen at run time: such a pointer is generic, and a generic load whose address register the compiler has moved below the first
// row (it folds the row offset into the instruction) leaves the LDS aperture when the row is row 0 of an array at LDS offset 0 -- a memory fault, met on a device.
template <bool CHECK>
__device__ __forceinline__ float2 kl_taps(const float* __restrict__ r0, int stride, const KlDeckDev& d, int64_t idx, double w) {
    double al = 0.0, ar = 0.0;
#pragma unroll 8
    for (int k = 0; k < MX_DECK_TAPS; ++k) {
        const double a = (double)r0[k], b = (double)r0[stride + k];
        const double ck = a + w * (b - a);
        const int64_t f = idx - 15 + k;
        const uint32_t s = CHECK ? (f >= 0 && f < d.n_frames ? d.track[f] : 0u) : d.track[f];
        const double xl = (double)(int16_t)(s & 0xffffu) * 0x1p-15, xr = (double)(int16_t)(s >> 16) * 0x1p-15;
        al = al + ck * xl;
        ar = ar + ck * xr;
    }
    return make_float2((float)al, (float)ar);
}

__device__ __forceinline__ float2 kl_grain(const float* __restrict__ rows, int stride, const KlDeckDev& d, int64_t u) {
    const int64_t idx = u >> DECK_Q;
    const uint32_t p = (uint32_t)(u >> 24) & 255u;
    const double w = (double)(uint32_t)(u & 0xFFFFFF) * 0x1p-24;
    const float* r0 = rows + p * stride;
    if (idx + 16 < 0 || idx - 15 >= d.n_frames) return make_float2(0.0f, 0.0f);   // no tap reaches the track: the sum of +0 products
    return idx - 15 >= 0 && idx + 16 < d.n_frames ? kl_taps<false>(r0, stride, d, idx, w) : kl_taps<true>(r0, stride, d, idx, w);
}

__global__ __launch_bounds__(MX_DECK_CHUNK) void k_deck_keylock_render(const KlDeckDev* __restrict__ decks, const KlTickDev* __restrict__ ticks,
                                                                       const float* __restrict__ tables, uint32_t n_ticks, uint32_t spt, uint32_t chunks) {
    __shared__ float coef[(MX_DECK_PHASES + 1) * KL_COEF_STRIDE];
    const uint32_t item = blockIdx.x / chunks, c = blockIdx.x - item * chunks;
    const uint32_t deck = item / n_ticks, tick = item - deck * n_ticks;
    const KlDeckDev d = decks[deck];
    const KlTickDev t = ticks[item];
    const uint32_t n0 = c * MX_DECK_CHUNK, cnt = min((uint32_t)MX_DECK_CHUNK, spt - n0), lane = threadIdx.x;
    float2* const out = reinterpret_cast<float2*>(d.out + ((size_t)tick * spt + n0) * 2);
    if (!t.play) {
        if (lane < cnt) out[lane] = make_float2(0.0f, 0.0f);
        return;
    }
    const float* const T = tables + (size_t)d.bank * DECK_BANK_FLOATS;
    const bool bank_lds = (d.pitch & 0xFFFFFFFFll) != 0;
    if (bank_lds)
        for (uint32_t i = lane; i < (uint32_t)DECK_BANK_FLOATS; i += MX_DECK_CHUNK) coef[(i >> 5) * KL_COEF_STRIDE + (i & 31u)] = T[i];
    __syncthreads();
    if (lane >= cnt) return;

    const uint32_t hop_mask = (1u << d.log_hop) - 1u;
    const uint32_t tt = t.m0 + n0 + lane, dj = tt >> d.log_hop, m = tt & hop_mask;
    const KlRec* const r = d.rec + t.gi0 + dj;
    const int64_t u = r->g + (int64_t)m * d.pitch;
    float2 y = bank_lds ? kl_grain(coef, KL_COEF_STRIDE, d, u) : kl_grain(T, MX_DECK_TAPS, d, u);
    if (m < d.overlap && !(t.first0 && dj == 0)) {
        const int64_t uo = r[-1].g + (int64_t)(hop_mask + 1u + m) * d.pitch;
        const float2 old = bank_lds ? kl_grain(coef, KL_COEF_STRIDE, d, uo) : kl_grain(T, MX_DECK_TAPS, d, uo);
        const double w = (double)m / (double)d.overlap;
        const double al = (double)old.x, ar = (double)old.y;
        y = make_float2((float)(al + w * ((double)y.x - al)), (float)(ar + w * ((double)y.y - ar)));
    }
    out[lane] = y;
}

void launch_deck_keylock(const KlDeckDev* decks, const KlTickDev* ticks, const float* tables, uint32_t n, uint32_t n_ticks, uint32_t spt, hipStream_t s) {
    const uint32_t chunks = (spt + MX_DECK_CHUNK - 1) / MX_DECK_CHUNK;
    const uint64_t blocks = (uint64_t)n * n_ticks * chunks;
    if (!blocks) return;
    if (blocks > 0x7fffffffull) throw Error(MX_ERR_INVALID, "deck feed: decks x ticks x chunks exceed 2^31 workgroups");
    hipLaunchKernelGGL(k_deck_keylock_search, dim3(n), dim3(KL_LANES), 0, s, decks);
    hipLaunchKernelGGL(k_deck_keylock_render, dim3((unsigned)blocks), dim3(MX_DECK_CHUNK), 0, s, decks, ticks, tables, n_ticks, spt, chunks);
}

}  // namespace mx
