// mx_k_deck_loudness.hip -- the deck's whole-track loudness (include/mixlab_gpu.h "KEY AND LOUDNESS", LOUDNESS): the loudness taps' rules
// (mx_k_loudness.hip) over the blocks of one int16 track in device memory.  A sample is (float)s / 32768.0f, exact; frames at or beyond n_frames read +0.0f.
//
// k_dk_loud_peak    a workgroup of 256 takes a tile of DK_LOUD_TILE = 1024 frames of the stream, staged ONCE in LDS per channel with its 11-frame run-in (the taps' peak
//                   kernel reads every frame twelve times from memory).  A lane takes frames l, l + 256, ...: consecutive lanes read consecutive floats.  Three 12-tap
//                   phases in f64 (exact products, ascending j).  The magnitudes' integer maximum goes to the block's record by atomicMax -- one per wave and channel
//                   where the wave's 64 frames lie in one block, else one per lane; the records are zeroed first.
// k_dk_loud_walk    one lane per (block, channel); a workgroup is one wave that takes 32 consecutive blocks and stages them through LDS 32 frames at a time: 32
//                   consecutive lanes read the 128 bytes of one block's 32 frames (L and R of a frame share a dword), rows padded to an odd stride.  A chunk's
//                   16 loads a lane go into registers while the chunk before is walked.
//                     <false>  walks from the zero state and leaves Z_k in the walk buffer
//                     <true>   walks from S_k (the walk buffer, after the scan), eight partials in registers, writes ksq
// k_dk_loud_scan    one wave; one lane per channel walks S_{k+1} = Z_k + P S_k over the blocks, Z_k replaced by S_k in the walk buffer.  The whole wave stages Z through
//                   LDS, 256 blocks of both channels at a time and a chunk ahead, so that the two lanes wait for LDS and never for memory; the LDS reads of eight
//                   blocks go out ahead of the dependent steps.  Serial by specification: a tree would change the roundings.
// k_dk_loud_window  a lane per block: both window sums afresh in ascending block from +0.0 (blocks before the first read +0.0), and frames / channels.
// Arithmetic: every f64 operation is rounded on its own (the build's -ffp-contract=off).  Every global index is checked against n_frames or n_blocks before it is used.
#include "mx_deck_loudkey.hpp"
#include "mx_dev.hpp"

namespace mx {

static constexpr uint32_t DKL_CHUNK = 32, DKL_ROW = DKL_CHUNK + 1, DKL_RUNIN = 11, DKL_SCAN = 256;

__device__ __forceinline__ float2 dkl_frame(const uint32_t* __restrict__ track, int64_t n_frames, int64_t f) {
    if (f < 0 || f >= n_frames) return make_float2(0.0f, 0.0f);
    const uint32_t v = track[f];
    return make_float2((float)(int16_t)(v & 0xffffu) / 32768.0f, (float)(int16_t)(v >> 16) / 32768.0f);
}

__global__ __launch_bounds__(256) void k_dk_loud_peak(const DkLoudArgs a, const DkLoudTabs t) {
    __shared__ float xs[2][DK_LOUD_TILE + DKL_RUNIN + 1];
    const uint32_t tid = threadIdx.x;
    const int64_t f0 = (int64_t)blockIdx.x * DK_LOUD_TILE, end = (int64_t)a.n_blocks * a.F;   // the tile's first frame; the stream's length
    for (uint32_t i = tid; i < DK_LOUD_TILE + DKL_RUNIN; i += 256u) {
        const float2 v = dkl_frame(a.track, a.n_frames, f0 - (int64_t)DKL_RUNIN + (int64_t)i);
        xs[0][i] = v.x; xs[1][i] = v.y;
    }
    __syncthreads();
    uint32_t* const rec = reinterpret_cast<uint32_t*>(a.rec);   // true_peak[c] of block k is word 12 k + 8 + c
    for (uint32_t m = tid; m < DK_LOUD_TILE; m += 256u) {        // (every wave runs all four rounds: the shuffles below are among 64 lanes)
        const int64_t f = f0 + m;
        const bool live = f < end;
        uint32_t pk[2] = {0u, 0u};
        if (live) {
#pragma unroll
            for (uint32_t c = 0; c < 2u; ++c) {
                double acc[3] = {0.0, 0.0, 0.0};
                float x = 0.0f;
#pragma unroll
                for (uint32_t j = 0; j < 12u; ++j) {   // ascending j: x[m - 11 + j]
                    x = xs[c][m + j];
#pragma unroll
                    for (uint32_t p = 0; p < 3u; ++p) acc[p] = acc[p] + (double)t.interp[12u * p + j] * (double)x;
                }
                pk[c] = __float_as_uint(x) & 0x7fffffffu;   // j = 11 left x[m] itself
#pragma unroll
                for (uint32_t p = 0; p < 3u; ++p) pk[c] = max(pk[c], __float_as_uint((float)acc[p]) & 0x7fffffffu);
            }
        }
        const uint32_t k = live ? (uint32_t)(f / a.F) : 0xffffffffu;
        const uint32_t k_first = (uint32_t)__shfl((int)k, 0, 64), k_last = (uint32_t)__shfl((int)k, 63, 64);
        if (k_first == k_last) {   // wave-uniform: the 64 frames lie in one block (or all beyond the stream)
            if (k_first == 0xffffffffu) continue;
#pragma unroll
            for (uint32_t c = 0; c < 2u; ++c) {
                uint32_t v = pk[c];
                for (int x = 32; x >= 1; x >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, x, 64));
                if ((tid & 63u) == 0u) atomicMax(rec + (size_t)k * 12u + 8u + c, v);
            }
        } else if (live) {
            atomicMax(rec + (size_t)k * 12u + 8u, pk[0]);
            atomicMax(rec + (size_t)k * 12u + 9u, pk[1]);
        }
    }
}

template <bool ENERGY>
__global__ __launch_bounds__(64) void k_dk_loud_walk(const DkLoudArgs a, const DkLoudTabs t) {
    __shared__ float buf[64 * DKL_ROW];
    const uint32_t lane = threadIdx.x;
    const uint32_t k0 = blockIdx.x * 32u;                        // (the grid is ceil(n_blocks / 32): k0 < n_blocks)
    const uint32_t nb = min(32u, a.n_blocks - k0), F = a.F;
    const uint32_t c = lane & 1u, kl = lane >> 1;
    const bool live = kl < nb;
    double* __restrict__ wk = a.walk + ((size_t)c * a.n_blocks + (k0 + (live ? kl : 0u))) * 4u;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (ENERGY && live) { s0 = wk[0]; s1 = wk[1]; s2 = wk[2]; s3 = wk[3]; }
    double part[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    // a chunk is 32 rows x 32 frames: 16 dwords a lane, loaded into registers a chunk AHEAD (a chunk's 32 dependent steps hide the latency of the next one's loads;
    // loaded and stored in one loop, each of the 16 loads waited for the one before: 7 us a chunk), rows and frames that do not exist as 0
    constexpr uint32_t PER = 32u * DKL_CHUNK / 64u;
    uint32_t v[PER];
    auto fetch = [&](uint32_t f0) {
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u) {
            const uint32_t i = lane + 64u * u, row = i / DKL_CHUNK, col = i - row * DKL_CHUNK;
            const int64_t f = (int64_t)(k0 + row) * F + f0 + col;
            v[u] = (row < nb && f0 + col < F && f < a.n_frames) ? a.track[f] : 0u;
        }
    };
    fetch(0u);
    for (uint32_t f0 = 0; f0 < F; f0 += DKL_CHUNK) {
        const uint32_t cnt = min(DKL_CHUNK, F - f0);
        __syncthreads();   // the last chunk has been read
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u) {   // 32 consecutive lanes hold 32 consecutive frames of one block
            const uint32_t i = lane + 64u * u, row = i / DKL_CHUNK, col = i - row * DKL_CHUNK;
            buf[(2u * row) * DKL_ROW + col] = (float)(int16_t)(v[u] & 0xffffu) / 32768.0f;
            buf[(2u * row + 1u) * DKL_ROW + col] = (float)(int16_t)(v[u] >> 16) / 32768.0f;
        }
        __syncthreads();
        if (f0 + DKL_CHUNK < F) fetch(f0 + DKL_CHUNK);
        if (live) {
            const float* __restrict__ x = buf + lane * DKL_ROW;
            for (uint32_t i8 = 0; i8 < cnt; i8 += 8u) {
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) {
                    if (i8 + u < cnt) {   // workgroup-uniform
                        const double y = dk_biquad(t.bq + 5, dk_biquad(t.bq, (double)x[i8 + u], s0, s1), s2, s3);
                        if (ENERGY) part[u] = part[u] + y * y;   // the product rounds, then the sum
                    }
                }
            }
        }
    }
    if (!live) return;
    if (ENERGY) {
#pragma unroll
        for (uint32_t m = 4; m >= 1; m >>= 1)
#pragma unroll
            for (uint32_t j = 0; j < 8u; ++j)
                if (!(j & m)) part[j] = part[j] + part[j ^ m];   // s[j] += s[j ^ m] for the j that reach s[0] (addition commutes bit for bit)
        a.rec[k0 + kl].ksq[c] = part[0];
    } else {
        wk[0] = s0; wk[1] = s1; wk[2] = s2; wk[3] = s3;
    }
}

__global__ __launch_bounds__(64) void k_dk_loud_scan(const DkLoudArgs a, const DkLoudTabs t) {
    __shared__ double2 zs[2][2][DKL_SCAN * 2u];   // [buffer][channel][block of the chunk][2 x double2]
    const uint32_t lane = threadIdx.x, n = a.n_blocks;
    const uint32_t chunks = (n + DKL_SCAN - 1u) / DKL_SCAN;
    double P[16];
#pragma unroll
    for (uint32_t k = 0; k < 16u; ++k) P[k] = t.carry[k];
    // the wave loads a chunk of DKL_SCAN blocks' Z of both channels with coalesced 16-byte loads, a chunk ahead of the two lanes that walk it
    constexpr uint32_t PER = 2u * DKL_SCAN * 2u / 64u;   // double2 a lane: 16
    double2 r[PER];
    auto fetch = [&](uint32_t c) {
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u) {
            const uint32_t ch = u / (PER / 2u), idx = lane + 64u * (u % (PER / 2u));   // double2 idx of the chunk: block idx / 2
            const uint32_t k = c * DKL_SCAN + idx / 2u;
            r[u] = k < n ? reinterpret_cast<const double2*>(a.walk + ((size_t)ch * n + k) * 4u)[idx & 1u] : make_double2(0.0, 0.0);
        }
    };
    double* __restrict__ wk = a.walk + (size_t)(lane & 1u) * n * 4u;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;   // S_0
    auto advance = [&](double* __restrict__ w, double2 za, double2 zb) {
        w[0] = s0; w[1] = s1; w[2] = s2; w[3] = s3;   // the block's start state, where its Z was
        const double n0 = dk_carry(P, 0, za.x, s0, s1, s2, s3), n1 = dk_carry(P, 1, za.y, s0, s1, s2, s3);
        const double n2 = dk_carry(P, 2, zb.x, s0, s1, s2, s3), n3 = dk_carry(P, 3, zb.y, s0, s1, s2, s3);
        s0 = n0; s1 = n1; s2 = n2; s3 = n3;
    };
    fetch(0u);
    for (uint32_t c = 0; c < chunks; ++c) {   // (zs[c & 1] was last read two chunks ago, before the barrier of the chunk between)
#pragma unroll
        for (uint32_t u = 0; u < PER; ++u) zs[c & 1u][u / (PER / 2u)][lane + 64u * (u % (PER / 2u))] = r[u];
        __syncthreads();
        if (c + 1u < chunks) fetch(c + 1u);
        if (lane < 2u) {
            const double2* __restrict__ z = zs[c & 1u][lane];
            const uint32_t cnt = min((uint32_t)DKL_SCAN, n - c * DKL_SCAN);
            double* w = wk + (size_t)c * DKL_SCAN * 4u;
            uint32_t k = 0;
            for (; k + 8u <= cnt; k += 8u) {   // the LDS reads of a batch go out ahead of the dependent steps
                double2 b[16];
#pragma unroll
                for (uint32_t u = 0; u < 16u; ++u) b[u] = z[2u * k + u];
#pragma unroll
                for (uint32_t u = 0; u < 8u; ++u) advance(w + (size_t)(k + u) * 4u, b[2u * u], b[2u * u + 1u]);
            }
            for (; k < cnt; ++k) advance(w + (size_t)k * 4u, z[2u * k], z[2u * k + 1u]);
        }
    }
}

__global__ __launch_bounds__(256) void k_dk_loud_window(const DkLoudArgs a) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= a.n_blocks) return;
    double ms = 0.0, ss = 0.0;
    for (uint32_t back = max(a.M, a.S); back-- > 0;) {   // ascending block: j - back
        const double v = back > j ? 0.0 : a.rec[j - back].ksq[0] + a.rec[j - back].ksq[1];
        if (back < a.M) ms = ms + v;
        if (back < a.S) ss = ss + v;
    }
    LoudTick* rec = a.rec + j;
    rec->momentary_sq = ms; rec->short_sq = ss;
    rec->frames = a.F; rec->channels = 2u;
}

void launch_deck_loudness(const DkLoudArgs& a, const DkLoudTabs& t, uint32_t forms[4], hipStream_t s) {
    const uint64_t end = (uint64_t)a.n_blocks * a.F;
    const uint32_t peak_wgs = (uint32_t)((end + DK_LOUD_TILE - 1u) / DK_LOUD_TILE), walk_wgs = (a.n_blocks + 31u) / 32u, win_wgs = (a.n_blocks + 255u) / 256u;
    hip_check(hipMemsetAsync(a.rec, 0, (size_t)a.n_blocks * sizeof(LoudTick), s), "hipMemsetAsync(deck loudness)");
    hipLaunchKernelGGL(k_dk_loud_peak, dim3(peak_wgs), dim3(256), 0, s, a, t);
    hipLaunchKernelGGL(k_dk_loud_walk<false>, dim3(walk_wgs), dim3(64), 0, s, a, t);
    hipLaunchKernelGGL(k_dk_loud_scan, dim3(1), dim3(64), 0, s, a, t);
    hipLaunchKernelGGL(k_dk_loud_walk<true>, dim3(walk_wgs), dim3(64), 0, s, a, t);
    hipLaunchKernelGGL(k_dk_loud_window, dim3(win_wgs), dim3(256), 0, s, a);
    forms[DK_LOUD_FORM_PEAK] = peak_wgs; forms[DK_LOUD_FORM_WALK] = walk_wgs; forms[DK_LOUD_FORM_SCAN] = a.n_blocks; forms[DK_LOUD_FORM_WINDOW] = win_wgs;
}

}  // namespace mx
