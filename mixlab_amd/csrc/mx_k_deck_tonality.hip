// mx_k_deck_tonality.hip -- the deck's whole-track tonality (include/mixlab_gpu.h "KEY AND LOUDNESS", TONALITY): the tonality taps' rules
// (mx_k_tonality.hip) over one stream of up to 2^30 frames that lies in device memory as int16, instead of taps x ticks.
//
// k_dk_ton_head      a lane per 64-bit word of the records: the four header words { g, G | 0, D | Hc, O | f_lo_mhz, 0 } and C[0 .. B) = 0.
// k_dk_ton_decimate  a workgroup of 256 forms DK_TON_OUT = 512 decimated frames.  Its window of quantised frames -- 512 D + 8 D - 1 of them -- is staged in LDS as
//                    int16: one 32-bit load per track frame, bounds-checked, the zero padding on both sides coming out of the check; a frame is quantised ONCE (the
//                    taps' decimator re-quantises every frame eight times over).  A lane then forms two outputs from 8 D taps each; the taps are a kernel argument,
//                    indexed uniformly (scalar operands), the loop unrolled by the template on D.  int32 accumulation is exact: |sum| <= 65534 x 2^14 < 2^30.
// k_dk_ton_cq        a workgroup of 256 takes up to DK_TON_HOPS = 8 consecutive hops of ONE segment.  The decimated frames those hops look at -- 2048 + 7 Hc -- are
//                    staged in LDS once.  Wave w takes bins w, w + 4, ...; lane l takes n = l, l + 64, ... of the bin's kernel and applies every {re, im} pair it
//                    loads to all 8 hops (the table load is what a lone workgroup of the taps' kernel waits for: here it is paid once for 8 hops; nothing is issued
//                    further ahead than that).  Accumulation is in 64 bits as in k_ton_cq, whose bound argument is in DESIGN.md section 0.10.  After a shuffle
//                    reduction lane 0 takes the exact roots of the hops that exist and adds their sum with ONE 64-bit atomic to C[b] of the segment's record.
// Integers throughout: no order of accumulation matters.  Every global index is checked against the array it goes into before it is used.
#include "mx_deck_loudkey.hpp"
#include "mx_dev.hpp"

namespace mx {

__global__ __launch_bounds__(256) void k_dk_ton_head(const DkTonArgs a) {
    const uint32_t per = 4u + a.bins;   // 64-bit words of a record
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= a.n_seg * per) return;
    const uint64_t g = idx / per;
    const uint32_t w = (uint32_t)(idx - g * per);
    unsigned long long v = 0ull;
    if (w == 0u) v = (unsigned long long)g | ((unsigned long long)a.G << 32);
    else if (w == 1u) v = (unsigned long long)a.D << 32;
    else if (w == 2u) v = (unsigned long long)a.Hc | ((unsigned long long)(a.bins / 12u) << 32);
    else if (w == 3u) v = (unsigned long long)a.f_lo_mhz;
    reinterpret_cast<unsigned long long*>(a.rec)[idx] = v;
}

template <uint32_t D>
__global__ __launch_bounds__(256) void k_dk_ton_decimate(const uint32_t* __restrict__ track, int64_t n_frames, const DkFir fir, int16_t* __restrict__ dec, uint64_t n_dec) {
    constexpr uint32_t Tf = 8u * D, WIN = DK_TON_OUT * D + Tf - 1u;   // (D = 8: 4159 int16)
    __shared__ int16_t win[WIN + 1u];
    const uint32_t tid = threadIdx.x;
    const uint64_t j0 = (uint64_t)blockIdx.x * DK_TON_OUT;
    const int64_t f0 = (int64_t)(j0 * D) - (int64_t)(Tf - 1u);      // the frame of win[0]
    for (uint32_t i = tid; i < WIN; i += 256u) {
        const int64_t f = f0 + (int64_t)i;
        win[i] = (f < 0 || f >= n_frames) ? (int16_t)0 : (int16_t)dk_quant(dk_sum(track[f]));
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < DK_TON_OUT / 256u; ++r) {
        const uint32_t o = tid + 256u * r;
        if (j0 + o >= n_dec) break;
        const int16_t* __restrict__ w = win + o * D + (Tf - 1u);   // q[(j0 + o) D]
        int32_t acc = 0;
#pragma unroll
        for (uint32_t k = 0; k < Tf; ++k) acc += (int32_t)fir.c[k] * (int32_t)w[-(int32_t)k];
        dec[j0 + o] = (int16_t)(acc >> 15);
    }
}

__global__ __launch_bounds__(256) void k_dk_ton_cq(const DkTonArgs a, uint32_t chunks) {
    __shared__ int16_t s[TON_MAX_KERNEL + (DK_TON_HOPS - 1) * 512];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t g = blockIdx.x / chunks, ch = blockIdx.x - g * chunks;
    const uint32_t u0 = ch * DK_TON_HOPS, cnt = min((uint32_t)DK_TON_HOPS, a.G - u0);
    const uint64_t h0 = (uint64_t)g * a.G + u0;                                                   // the first hop of this workgroup
    const int64_t base = (int64_t)((h0 + 1u) * a.Hc) - 1 - (int64_t)(TON_MAX_KERNEL - 1u);        // the decimated frame of s[0]: 2047 before that hop's last
    const int64_t n_dec = (int64_t)(a.n_seg * a.G * a.Hc);
    const uint32_t span = TON_MAX_KERNEL + (DK_TON_HOPS - 1u) * a.Hc;
    for (uint32_t i = tid; i < span; i += 256u) {
        const int64_t n = base + (int64_t)i;
        s[i] = (n < 0 || n >= n_dec) ? (int16_t)0 : a.dec[n];   // (beyond n_dec: hops this workgroup does not have)
    }
    __syncthreads();
    const uint32_t* __restrict__ len = a.tab;
    const uint32_t* __restrict__ off = len + a.bins;
    const short2* __restrict__ kern = reinterpret_cast<const short2*>(off + a.bins);
    unsigned long long* c = reinterpret_cast<unsigned long long*>(a.rec + (size_t)g * a.rec_words + 8u);
    for (uint32_t b = wave; b < a.bins; b += 4u) {   // wave-uniform
        const uint32_t N = len[b];
        const short2* __restrict__ kb = kern + off[b];
        const int16_t* sb = s + (TON_MAX_KERNEL - N);   // n = N - 1 is the first hop's newest frame
        long long re[DK_TON_HOPS], im[DK_TON_HOPS];
#pragma unroll
        for (uint32_t u = 0; u < DK_TON_HOPS; ++u) re[u] = im[u] = 0;
        for (uint32_t n = lane; n < N; n += 64u) {
            const short2 kv = kb[n];
#pragma unroll
            for (uint32_t u = 0; u < DK_TON_HOPS; ++u) {
                const int32_t x = sb[n + u * a.Hc];
                re[u] += (long long)((int32_t)kv.x * x);   // |product| <= 2^29
                im[u] += (long long)((int32_t)kv.y * x);
            }
        }
#pragma unroll
        for (uint32_t u = 0; u < DK_TON_HOPS; ++u)
            for (int x = 32; x >= 1; x >>= 1) { re[u] += __shfl_xor(re[u], x, 64); im[u] += __shfl_xor(im[u], x, 64); }
        if (lane == 0u) {
            unsigned long long sum = 0ull;
#pragma unroll
            for (uint32_t u = 0; u < DK_TON_HOPS; ++u)
                if (u < cnt) sum += dk_magnitude(re[u], im[u]);
            atomicAdd(c + b, sum);
        }
    }
}

void launch_deck_tonality(const DkTonArgs& a, const DkFir& fir, uint32_t forms[4], hipStream_t s) {
    const uint64_t words = a.n_seg * (4u + a.bins), n_dec = a.n_seg * a.G * a.Hc;
    const uint32_t head_wgs = (uint32_t)((words + 255u) / 256u), dec_wgs = (uint32_t)((n_dec + DK_TON_OUT - 1u) / DK_TON_OUT);
    const uint32_t chunks = (a.G + DK_TON_HOPS - 1u) / DK_TON_HOPS;
    hipLaunchKernelGGL(k_dk_ton_head, dim3(head_wgs), dim3(256), 0, s, a);
    if (a.D == 4u) hipLaunchKernelGGL(k_dk_ton_decimate<4>, dim3(dec_wgs), dim3(256), 0, s, a.track, a.n_frames, fir, a.dec, n_dec);
    else hipLaunchKernelGGL(k_dk_ton_decimate<8>, dim3(dec_wgs), dim3(256), 0, s, a.track, a.n_frames, fir, a.dec, n_dec);
    hipLaunchKernelGGL(k_dk_ton_cq, dim3((uint32_t)(a.n_seg * chunks)), dim3(256), 0, s, a, chunks);
    forms[DK_TON_FORM_DECIMATE] = dec_wgs;
    forms[DK_TON_FORM_FULL] = (uint32_t)(a.n_seg * (a.G / DK_TON_HOPS));
    forms[DK_TON_FORM_PART] = a.G % DK_TON_HOPS ? (uint32_t)a.n_seg : 0u;
    forms[DK_TON_FORM_HEAD] = head_wgs;
}

}  // namespace mx
