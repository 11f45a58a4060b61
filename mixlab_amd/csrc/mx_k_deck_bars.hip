// mx_k_deck_bars.hip -- the deck's bars and phrases (include/mixlab_gpu.h "the deck", BARS): three kernels on the deck's load stream.
//
// k_bars_bands     a workgroup of 256 per HALF-BEAT (2 n_beats of them) walks its own frames in tiles of 1024: k_deck_columns' arithmetic (mx_k_deck_analyse.hip) over
//                  segments that start anywhere.  Per tile the s-window -- 1024 frames and the K - 1 halo frames round them -- is staged in LDS as int32, one 32-bit load
//                  a frame, bounds-checked there; a lane owns four consecutive frames, reads ONE int4 of the window per four taps and issues 32 24-bit multiply-adds;
//                  the two tap tables are a kernel argument indexed uniformly (scalar loads).  Frames at or beyond the half-beat's end add nothing.  The three 64-bit
//                  energies are reduced by shuffles, then over the four waves through LDS; three lanes take the roots (tempo_root) and store v.  A workgroup owns its
//                  half-beat, so there is no global atomic and nothing to zero first.
// k_bars_novelty   a workgroup per MX_DECK_BARS_BLOCK beats, a wave per beat.  The vectors of the block's beats and of the 64 beats to either side are staged in LDS
//                  (rows of 7 words: an odd stride).  N_W[k] is the sum over ALL ordered pairs (i, j) of the window [k - W, k + W) of +d(i, j) when the two lie on
//                  different sides of k and -d(i, j) when on the same -- NOVELTY's three sums in one -- a lane per pair in strides of 64, reduced by shuffles.
// k_bars_fold      one workgroup: integer atomic adds of the clamped novelties into M + M Q words in LDS.
// Integers throughout but for tempo_root's f64 root: no order of accumulation matters.
#include "mx_deck_bars.hpp"

namespace mx {

enum { BR_WIN = BR_TILE + 136, BR_ROW = 7, BR_ROWS = BR_BLOCK + 2 * BR_MAX_W };
static_assert(sizeof(mx_deck_beat) == 48, "mx_deck_beat is 48 bytes");

__device__ __forceinline__ int32_t br_sum(const uint32_t* __restrict__ track, int64_t n_frames, int64_t f) {
    if (f < 0 || f >= n_frames) return 0;
    const uint32_t s = track[f];
    return (int32_t)(int16_t)(s & 0xffffu) + (int32_t)(int16_t)(s >> 16);
}
// |c| < 2^15, |s| <= 2^16: both fit 24 bits, so the 24-bit multiply-add is exact (the faster one: DESIGN.md section 0.17)
__device__ __forceinline__ int32_t br_mad(int32_t c, int32_t s, int32_t acc) { return acc + __mul24(c, s); }

__global__ __launch_bounds__(BR_LANES) void k_bars_bands(const uint32_t* __restrict__ track, int64_t n_frames, uint64_t base, uint64_t period, uint32_t lead, uint32_t n_beats,
                                                         uint32_t kpad, uint32_t D, const DeckAnalyseTaps taps, mx_deck_beat* __restrict__ rec) {
    __shared__ int4 win4[BR_WIN / 4];
    __shared__ unsigned long long part[BR_LANES / 64][3];
    int32_t* const win = reinterpret_cast<int32_t*>(win4);
    const uint32_t tid = threadIdx.x, k = blockIdx.x >> 1, half = blockIdx.x & 1u;
    if (k >= n_beats) return;   // workgroup-uniform
    const int64_t a = br_line(base, period, k, lead), c = br_line(base, period, k + 1u, lead), h = br_half(a, c);
    const int64_t lo = half ? h : a, hi = half ? c : h;
    unsigned long long en[3] = {0ull, 0ull, 0ull};
    for (int64_t f0 = lo; f0 < hi; f0 += BR_TILE) {   // workgroup-uniform
        __syncthreads();   // the tile before has been read
        for (uint32_t i = tid; i < BR_TILE + kpad + 4u; i += BR_LANES) win[i] = br_sum(track, n_frames, f0 - (int64_t)D + (int64_t)i);   // (at most 1156 of BR_WIN)
        __syncthreads();
        int32_t a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0};
        int4 w0 = win4[tid];
        for (uint32_t kk = 0; kk < kpad; kk += 4) {   // uniform: taps kk .. kk + 3 against window frames 4 tid + kk + (0 .. 6)
            const int4 w1 = win4[tid + (kk >> 2) + 1u];
            const int32_t w[7] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int32_t cl = taps.lo[kk + j], ch = taps.hi[kk + j];
#pragma unroll
                for (int i = 0; i < 4; ++i) { a1[i] = br_mad(cl, w[j + i], a1[i]); a2[i] = br_mad(ch, w[j + i], a2[i]); }
            }
            w0 = w1;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (f0 + 4 * (int64_t)tid + i < hi) {
                const int32_t s = win[4u * tid + D + (uint32_t)i], low = a1[i] >> 14, b = a2[i] >> 14, band[3] = {low, b - low, s - b};
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const uint32_t m = (uint32_t)(band[j] < 0 ? -band[j] : band[j]);
                    en[j] += (unsigned long long)m * m;
                }
            }
    }
    for (uint32_t off = 32; off; off >>= 1)
#pragma unroll
        for (int j = 0; j < 3; ++j) en[j] += __shfl_xor(en[j], (int)off, 64);
    if ((tid & 63u) == 0u)
#pragma unroll
        for (int j = 0; j < 3; ++j) part[tid >> 6][j] = en[j];
    __syncthreads();
    if (tid < 3u) rec[k].v[3u * half + tid] = tempo_root(part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid]);
    if (tid == 3u && !half) { rec[k].first_frame = (uint32_t)a; rec[k].frames = (uint32_t)(c - a); }
}

__global__ __launch_bounds__(BR_LANES) void k_bars_novelty(mx_deck_beat* __restrict__ rec, uint32_t n_beats, uint32_t w_bar, uint32_t w_phrase) {
    __shared__ uint32_t sv[BR_ROWS * BR_ROW];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, k0 = blockIdx.x * BR_BLOCK;
    // row r holds beat k0 - 64 + r (zeros where there is none: no defined novelty reads them)
    for (uint32_t i = tid; i < BR_ROWS * 6u; i += BR_LANES) {
        const uint32_t r = i / 6u, c = i % 6u;
        const int64_t beat = (int64_t)k0 - BR_MAX_W + (int64_t)r;
        sv[r * BR_ROW + c] = beat >= 0 && beat < (int64_t)n_beats ? rec[beat].v[c] : 0u;
    }
    __syncthreads();
    const uint32_t k = k0 + (tid >> 6);
    if (k >= n_beats) return;   // wave-uniform, after the only barrier
#pragma unroll 1
    for (uint32_t which = 0; which < 2u; ++which) {
        const uint32_t W = which ? w_phrase : w_bar;
        long long acc = 0;
        if (br_defined(k, W, n_beats)) {   // wave-uniform
            const uint32_t tw = 2u * W, total = tw * tw, q = 64u / tw, rem = 64u % tw;
            const uint32_t r0 = (k - k0) + BR_MAX_W - W;   // the window's first row
            uint32_t i = lane / tw, j = lane % tw;
            for (uint32_t t = lane; t < total; t += 64u) {
                const long long d = (long long)br_dist(sv + (r0 + i) * BR_ROW, sv + (r0 + j) * BR_ROW);
                acc += ((i < W) != (j < W)) ? d : -d;
                i += q; j += rem;
                if (j >= tw) { j -= tw; ++i; }
            }
            for (uint32_t off = 32; off; off >>= 1) acc += __shfl_xor(acc, (int)off, 64);
        }
        if (lane == 0u) (which ? rec[k].n_phrase : rec[k].n_bar) = (int64_t)acc;
    }
}

__global__ __launch_bounds__(BR_LANES) void k_bars_fold(const mx_deck_beat* __restrict__ rec, uint32_t n_beats, uint32_t M, uint32_t MQ, unsigned long long* __restrict__ folds) {
    __shared__ unsigned long long H[BR_MAX_FOLDS];
    const uint32_t tid = threadIdx.x;
    if (tid < BR_MAX_FOLDS) H[tid] = 0ull;
    __syncthreads();
    for (uint32_t k = tid; k < n_beats; k += BR_LANES) {
        const unsigned long long nb = br_clamp(rec[k].n_bar), np = br_clamp(rec[k].n_phrase);
        if (nb) atomicAdd(&H[k % M], nb);
        if (np) atomicAdd(&H[M + k % MQ], np);
    }
    __syncthreads();
    if (tid < M + MQ) folds[tid] = H[tid];   // (M + M Q <= 136 < 256)
}

void launch_deck_bars(const DkBarsArgs& a, const DeckAnalyseTaps& taps, uint32_t forms[4], hipStream_t s) {
    forms[0] = forms[1] = forms[2] = forms[3] = 0u;
    // a beat is floor(period) frames or one more; the beats together span line n_beats - line 0, which says how many of each there are
    const int64_t shorter = (int64_t)(a.period >> 32);
    const int64_t longer_n = br_line(a.base, a.period, a.n_beats, a.lead) - br_line(a.base, a.period, 0u, a.lead) - shorter * (int64_t)a.n_beats;
    for (int l = 0; l < 2; ++l) {
        const int64_t len = shorter + l, h = br_half(0, len);
        const uint32_t cnt = (uint32_t)(l ? longer_n : (int64_t)a.n_beats - longer_n);
        forms[h <= BR_TILE ? DK_BARS_FORM_ONE_TILE : DK_BARS_FORM_TILED] += cnt;
        forms[len - h <= BR_TILE ? DK_BARS_FORM_ONE_TILE : DK_BARS_FORM_TILED] += cnt;
    }
    for (uint32_t W : {a.w_bar, a.w_phrase})
        if (a.n_beats >= 2u * W) forms[DK_BARS_FORM_DEFINED] += a.n_beats - 2u * W + 1u;
    const uint32_t D = (a.K - 1u) / 2u, kpad = (a.K + 3u) & ~3u, wgs = (a.n_beats + BR_BLOCK - 1u) / BR_BLOCK;
    forms[DK_BARS_FORM_NOVELTY] = wgs;
    hipLaunchKernelGGL(k_bars_bands, dim3(2u * a.n_beats), dim3(BR_LANES), 0, s, a.track, a.n_frames, a.base, a.period, a.lead, a.n_beats, kpad, D, taps, a.rec);
    hipLaunchKernelGGL(k_bars_novelty, dim3(wgs), dim3(BR_LANES), 0, s, a.rec, a.n_beats, a.w_bar, a.w_phrase);
    hipLaunchKernelGGL(k_bars_fold, dim3(1), dim3(BR_LANES), 0, s, a.rec, a.n_beats, a.M, a.MQ, (unsigned long long*)a.folds);
}

}  // namespace mx
