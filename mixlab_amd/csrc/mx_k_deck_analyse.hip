// mx_k_deck_analyse.hip -- the deck's track analysis (include/mixlab_gpu.h "the deck", ANALYSIS): one pass over the resident track.
//
// k_deck_columns        a workgroup of 256 takes a span of max(C, 1024) frames in tiles of 1024.  Per tile the s-window -- 1024 frames and the K - 1 halo frames round
//                       them -- is staged in LDS as int32, one 32-bit load a frame, bounds-checked there.  A lane owns four consecutive frames: per four taps it reads
//                       ONE int4 of the window (lanes at consecutive 16 bytes: conflict-free) and issues 32 multiply-adds, the window sliding through registers.  The
//                       two tap tables are kernel arguments, indexed uniformly: scalar loads, the coefficient a scalar operand of the multiply-add.  The tap loop runs
//                       to K rounded up to four -- the taps there are 0 and the window behind the halo holds track or 0, so nothing is added.  C < 1024: the
//                       workgroup covers 1024 / C columns (form SEVERAL); C = 1024: one (form ONE); C > 1024: one column, C / 1024 tiles, the lane's partial
//                       carried in registers over them (form TILED).  The partial -- min / max of s, three peaks, four 64-bit sums -- is reduced by shuffles over the
//                       min(64, C / 4) lanes of a wave that share a column, then by integer atomics on the column's record in LDS, and the records leave as dwords.
// k_deck_columns_short  a track shorter than the halo (n_frames < K - 1, so at most 125 frames and two columns): one workgroup, a lane per frame, and the sums run over
//                       the FRAMES of the track (fewer than the taps), each tap picked by the lane; straight to the LDS records.  NOT needed for correctness:
//                       k_deck_columns' bounds-checked staging gives the same records for such a track, and a track this short is never hot.  It is the form the
//                       interface names for it (mx_deck_debug_last_analysis out[2]), and a second, differently shaped statement of the filter the tests compare.
// k_deck_onsets         a thread per column: the exact root of e[c] and of e[c - 1] (mx_dev.hpp tempo_root, the tempo taps'), the clamped difference, the shift.
// k_deck_autocorr       a workgroup per 1024 onsets, staged in LDS with the L - 1 that follow (0 beyond the last column); a lane per lag (and lag + 256, ...): the
//                       left operand is a broadcast, the right one consecutive across lanes.  One 64-bit atomic add per (workgroup, lag) into R, zeroed before.
// Integers throughout k_deck_columns: no order of accumulation matters, and no f32 / f64 appears in it.
#include "mx_deck.hpp"
#include "mx_dev.hpp"
#include "mx_kernels.hpp"

namespace mx {

enum { AN_TILE = 1024, AN_LANES = 256, AN_WIN = AN_TILE + 136, AN_REC_WORDS = 14, AN_SHORT_LANES = 128, AC_BLOCK = 1024 };
static_assert(sizeof(mx_deck_column) == 4 * AN_REC_WORDS, "mx_deck_column is 14 words");

struct AnPart { int32_t smin, smax; uint32_t pk[3]; unsigned long long en[3], e; };

__device__ __forceinline__ int32_t an_sum(const uint32_t* __restrict__ track, int64_t n_frames, int64_t f) {
    if (f < 0 || f >= n_frames) return 0;
    const uint32_t s = track[f];
    return (int32_t)(int16_t)(s & 0xffffu) + (int32_t)(int16_t)(s >> 16);
}

// one frame's bands from its two sums, into the partial
__device__ __forceinline__ void an_frame(AnPart& p, int32_t s, int32_t a1, int32_t a2) {
    const int32_t low = a1 >> 14, b = a2 >> 14, band[3] = {low, b - low, s - b};
    p.smin = min(p.smin, s); p.smax = max(p.smax, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const uint32_t m = (uint32_t)(band[k] < 0 ? -band[k] : band[k]);
        p.pk[k] = max(p.pk[k], m);
        p.en[k] += (unsigned long long)m * m;
    }
    const uint32_t m = (uint32_t)(s < 0 ? -s : s);
    p.e += (unsigned long long)m * m;
}

// a record in LDS as the header lays it out: words 0 smin, 1 smax, 2 .. 4 peak, 5 onset, then energy[3] and e as 64-bit words 3 .. 6
__device__ __forceinline__ void an_rec_init(unsigned long long* rec) {
    int32_t* w = reinterpret_cast<int32_t*>(rec);
    w[0] = 0x7fffffff; w[1] = (int32_t)0x80000000;
#pragma unroll
    for (int k = 2; k < AN_REC_WORDS; ++k) w[k] = 0;
}
__device__ __forceinline__ void an_rec_add(unsigned long long* rec, const AnPart& p) {
    int32_t* w = reinterpret_cast<int32_t*>(rec);
    atomicMin(w, p.smin); atomicMax(w + 1, p.smax);
#pragma unroll
    for (int k = 0; k < 3; ++k) { atomicMax(reinterpret_cast<uint32_t*>(w) + 2 + k, p.pk[k]); atomicAdd(rec + 3 + k, p.en[k]); }
    atomicAdd(rec + 6, p.e);
}

// |c| < 2^15, |s| <= 2^16: both fit 24 bits, so the 24-bit multiply-add is exact (measured 8 % faster here than the 32-bit multiply)
__device__ __forceinline__ int32_t an_mad(int32_t c, int32_t s, int32_t acc) { return acc + __mul24(c, s); }

__global__ __launch_bounds__(AN_LANES) void k_deck_columns(const uint32_t* __restrict__ track, int64_t n_frames, uint32_t log_c, uint32_t kpad, uint32_t D,
                                                           const DeckAnalyseTaps taps, uint32_t* __restrict__ cols, uint64_t n_cols) {
    __shared__ int4 win4[AN_WIN / 4];
    __shared__ unsigned long long rec[(AN_TILE / 64) * (AN_REC_WORDS / 2)];
    int32_t* const win = reinterpret_cast<int32_t*>(win4);
    const uint32_t tid = threadIdx.x, C = 1u << log_c;
    const uint32_t tiles = C > AN_TILE ? C / AN_TILE : 1u, per_wg = C < AN_TILE ? AN_TILE / C : 1u;   // tiles of this workgroup's span; columns in it
    const int64_t span0 = (int64_t)blockIdx.x * ((int64_t)tiles * AN_TILE);
    if (tid < per_wg) an_rec_init(rec + tid * (AN_REC_WORDS / 2));
    AnPart p{0x7fffffff, (int32_t)0x80000000, {0u, 0u, 0u}, {0ull, 0ull, 0ull}, 0ull};
    for (uint32_t t = 0; t < tiles; ++t) {   // workgroup-uniform
        const int64_t f0 = span0 + (int64_t)t * AN_TILE;
        if (f0 >= n_frames) break;
        __syncthreads();   // the tile before has been read
        for (uint32_t i = tid; i < AN_TILE + kpad + 4u; i += AN_LANES) win[i] = an_sum(track, n_frames, f0 - (int64_t)D + (int64_t)i);   // (at most 1156 of AN_WIN)
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
                for (int i = 0; i < 4; ++i) { a1[i] = an_mad(cl, w[j + i], a1[i]); a2[i] = an_mad(ch, w[j + i], a2[i]); }
            }
            w0 = w1;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (f0 + 4 * (int64_t)tid + i < n_frames) an_frame(p, win[4u * tid + D + (uint32_t)i], a1[i], a2[i]);
    }
    // the lanes of a wave that share a column: min(64, C / 4) of them, aligned
    const uint32_t G = C / 4u < 64u ? C / 4u : 64u;
    for (uint32_t off = G >> 1; off; off >>= 1) {
        p.smin = min(p.smin, __shfl_xor(p.smin, (int)off, 64)); p.smax = max(p.smax, __shfl_xor(p.smax, (int)off, 64));
#pragma unroll
        for (int k = 0; k < 3; ++k) { p.pk[k] = max(p.pk[k], (uint32_t)__shfl_xor((int)p.pk[k], (int)off, 64)); p.en[k] += __shfl_xor(p.en[k], (int)off, 64); }
        p.e += __shfl_xor(p.e, (int)off, 64);
    }
    if ((tid & (G - 1u)) == 0u) an_rec_add(rec + (C < AN_TILE ? (4u * tid) >> log_c : 0u) * (AN_REC_WORDS / 2), p);
    __syncthreads();
    if (tid < per_wg * AN_REC_WORDS) {
        const uint64_t col = (uint64_t)blockIdx.x * per_wg + tid / AN_REC_WORDS;
        if (col < n_cols) cols[col * AN_REC_WORDS + tid % AN_REC_WORDS] = reinterpret_cast<const uint32_t*>(rec)[tid];
    }
}

__global__ __launch_bounds__(AN_SHORT_LANES) void k_deck_columns_short(const uint32_t* __restrict__ track, uint32_t n_frames, uint32_t log_c, uint32_t K, uint32_t D,
                                                                       const DeckAnalyseTaps taps, uint32_t* __restrict__ cols, uint32_t n_cols) {
    __shared__ int32_t s[AN_SHORT_LANES], tl[128], th[128];
    __shared__ unsigned long long rec[2 * (AN_REC_WORDS / 2)];
    const uint32_t tid = threadIdx.x;
    s[tid] = an_sum(track, n_frames, tid);
    tl[tid] = taps.lo[tid]; th[tid] = taps.hi[tid];
    if (tid < 2u) an_rec_init(rec + tid * (AN_REC_WORDS / 2));
    __syncthreads();
    if (tid < n_frames) {
        int32_t a1 = 0, a2 = 0;
        for (uint32_t j = 0; j < n_frames; ++j) {   // frame j meets tap k = j - tid + D of frame tid
            const uint32_t k = j + D - tid;           // (wraps below 0: then k >= K)
            if (k < K) { a1 += tl[k] * s[j]; a2 += th[k] * s[j]; }
        }
        AnPart p{0x7fffffff, (int32_t)0x80000000, {0u, 0u, 0u}, {0ull, 0ull, 0ull}, 0ull};
        an_frame(p, s[tid], a1, a2);
        an_rec_add(rec + (tid >> log_c) * (AN_REC_WORDS / 2), p);
    }
    __syncthreads();
    if (tid < n_cols * AN_REC_WORDS) cols[tid] = reinterpret_cast<const uint32_t*>(rec)[tid];
}

__global__ __launch_bounds__(256) void k_deck_onsets(uint32_t* __restrict__ cols, uint32_t* __restrict__ onsets, uint64_t n_cols) {
    const uint64_t c = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (c >= n_cols) return;
    auto e = [&](uint64_t k) { return *reinterpret_cast<const unsigned long long*>(cols + k * AN_REC_WORDS + 12); };
    const uint32_t a = tempo_root(e(c)), before = c ? tempo_root(e(c - 1)) : 0u;
    const uint32_t o = (a > before ? a - before : 0u) >> 6;
    cols[c * AN_REC_WORDS + 5] = o;
    onsets[c] = o;
}

__global__ __launch_bounds__(256) void k_deck_autocorr(const uint32_t* __restrict__ onsets, uint64_t n_cols, uint32_t L, unsigned long long* __restrict__ R) {
    __shared__ uint32_t s[AC_BLOCK + 1024];
    const uint32_t tid = threadIdx.x;
    const uint64_t c0 = (uint64_t)blockIdx.x * AC_BLOCK;
    for (uint32_t i = tid; i < AC_BLOCK + L - 1u; i += 256u) s[i] = c0 + i < n_cols ? onsets[c0 + i] : 0u;   // (L <= 1024: at most 2047 words)
    __syncthreads();
    const uint32_t cnt = (uint32_t)min((uint64_t)AC_BLOCK, n_cols - c0);
    for (uint32_t l = tid; l < L; l += 256u) {
        unsigned long long acc = 0ull;
#pragma unroll 4
        for (uint32_t c = 0; c < cnt; ++c) acc += (unsigned long long)s[c] * s[c + l];
        if (acc) atomicAdd(R + l, acc);
    }
}

void launch_deck_analyse(const uint32_t* track, uint64_t n_frames, uint32_t column, uint32_t K, uint32_t max_lag, const DeckAnalyseTaps& taps, void* cols, uint32_t* onsets,
                         uint64_t* R, uint64_t n_cols, uint32_t forms[4], hipStream_t s) {
    uint32_t log_c = 0;
    while ((1u << log_c) < column) ++log_c;
    const uint32_t D = (K - 1u) / 2u;
    forms[0] = forms[1] = forms[2] = forms[3] = 0u;
    if (n_frames + 1u < K) {
        hipLaunchKernelGGL(k_deck_columns_short, dim3(1), dim3(AN_SHORT_LANES), 0, s, track, (uint32_t)n_frames, log_c, K, D, taps, (uint32_t*)cols, (uint32_t)n_cols);
        forms[DECK_AN_SHORT] = 1u;
    } else {
        const uint64_t span = std::max<uint64_t>(column, AN_TILE);
        const uint32_t wgs = (uint32_t)((n_frames + span - 1u) / span);   // (n_frames <= 2^30: at most 2^20)
        const uint32_t kpad = (K + 3u) & ~3u;
        hipLaunchKernelGGL(k_deck_columns, dim3(wgs), dim3(AN_LANES), 0, s, track, (int64_t)n_frames, log_c, kpad, D, taps, (uint32_t*)cols, n_cols);
        forms[column < AN_TILE ? DECK_AN_SEVERAL : column > AN_TILE ? DECK_AN_TILED : DECK_AN_ONE] = wgs;
    }
    hipLaunchKernelGGL(k_deck_onsets, dim3((uint32_t)((n_cols + 255u) / 256u)), dim3(256), 0, s, (uint32_t*)cols, onsets, n_cols);
    hip_check(hipMemsetAsync(R, 0, (size_t)max_lag * sizeof(uint64_t), s), "hipMemsetAsync(deck autocorrelation)");
    hipLaunchKernelGGL(k_deck_autocorr, dim3((uint32_t)((n_cols + AC_BLOCK - 1u) / AC_BLOCK)), dim3(256), 0, s, onsets, n_cols, max_lag, (unsigned long long*)R);
}

}  // namespace mx
