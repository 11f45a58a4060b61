// mx_k_deck.hip -- the deck's feed kernel (include/mixlab_gpu.h "the deck").
//
// One launch writes every tick of every deck of a feed.  A workgroup of MX_DECK_CHUNK lanes writes one chunk of one tick, a lane per output frame, both channels: L and R
// of a track frame are one 32-bit word, so a tap is one load.  Per chunk (deck_chunk_plan, shared with the host):
//   zero form       the tick is not playing, or lies wholly before / past the track: the chunk is stored as zeros, nothing is read;
//   streaming form  the positions of the chunk move in one direction and stay inside one wrap of a loop: the <= 4 * chunk + 32 track frames its taps touch are staged
//                   in LDS once (bounds-checked there) and every lane's 32 taps come from LDS;
//   gather form     a loop fold or a change of direction inside the chunk: every lane folds its own position (the only place the 64-bit floor-mod runs) and reads its taps
//                   from the track one by one, bounds-checked.
// The arithmetic is the header's: per tap c = T[p][k] + w (T[p + 1][k] - T[p][k]) and acc += c x in f64, never fused (-ffp-contract=off), ascending k, one rounding to f32.
// Where a lane's two coefficient rows come from depends on the tick (DESIGN.md section 0.15 has the timings): when every lane of the tick has the same phase (a step of
// whole frames and no slew: unity, reverse, x2, x4) the two rows are read from the tables in global memory and broadcast; otherwise lanes read 64 different rows, and the
// tick's bank (32.9 KB) is staged in LDS first, rows padded to 33 words -- 3.5 times faster there, 1.2 times slower where the phase stands.  The launcher picks the kernel
// with the LDS bank only for a feed that has such a tick.  MX_DECK_FORM (read per launch) forces a candidate for an A/B: 1 the bank always in LDS, 2 every chunk gathers
// and reads global tables, 3 the bank never in LDS.
#include "mx_deck.hpp"
#include "mx_kernels.hpp"

#include <cstdlib>

namespace mx {

enum { DECK_COEF_STRIDE = MX_DECK_TAPS + 1 };

__device__ inline uint32_t deck_frame(const DeckDev& d, int64_t f) { return f >= 0 && f < d.n_frames ? d.track[f] : 0u; }

// the 32 taps of one output frame: rows r0 and r0 + stride (global or LDS -- one or the other per instantiation, so the loads keep their address space)
template <bool STREAM>
__device__ inline float2 deck_taps(const float* __restrict__ r0, int stride, const uint32_t* win, uint32_t w0, const DeckDev& d, int64_t idx, double w) {
    double al = 0.0, ar = 0.0;
#pragma unroll 8
    for (int k = 0; k < MX_DECK_TAPS; ++k) {
        const double a = (double)r0[k], b = (double)r0[stride + k];
        const double ck = a + w * (b - a);
        const uint32_t s = STREAM ? win[w0 + k] : deck_frame(d, idx - 15 + k);
        const double xl = (double)(int16_t)(s & 0xffffu) * 0x1p-15, xr = (double)(int16_t)(s >> 16) * 0x1p-15;   // (float)s / 32768.0f, exactly
        al = al + ck * xl;
        ar = ar + ck * xr;
    }
    return make_float2((float)al, (float)ar);
}

// COEF: the kernel has room for a bank in LDS; coef_mode 0: a tick stages it when its lanes differ in phase, 1: always (A/B)
template <int COEF, int GATHER_ONLY>
__global__ __launch_bounds__(MX_DECK_CHUNK) void k_deck_feed(const DeckDev* __restrict__ decks, const DeckTickDev* __restrict__ ticks, const float* __restrict__ tables,
                                                             uint32_t n_ticks, uint32_t spt, uint32_t chunks, uint32_t coef_mode) {
    __shared__ uint32_t win[DECK_WINDOW];
    __shared__ float coef[COEF ? (MX_DECK_PHASES + 1) * DECK_COEF_STRIDE : 1];
    const uint32_t item = blockIdx.x / chunks, c = blockIdx.x - item * chunks;
    const uint32_t deck = item / n_ticks, tick = item - deck * n_ticks;
    const DeckDev d = decks[deck];
    const DeckTickDev t = ticks[item];
    const uint32_t n0 = c * MX_DECK_CHUNK, cnt = min((uint32_t)MX_DECK_CHUNK, spt - n0), lane = threadIdx.x;
    float2* const out = reinterpret_cast<float2*>(d.out + ((size_t)tick * spt + n0) * 2);
    if (t.form == DECK_FORM_ZERO) {
        if (lane < cnt) out[lane] = make_float2(0.0f, 0.0f);
        return;
    }
    DeckChunkPlan plan = deck_chunk_plan(t, n0, cnt);
    if (GATHER_ONLY) plan.stream = false;
    const float* const T = tables + (size_t)t.bank * DECK_BANK_FLOATS;
    const bool bank_lds = COEF && (coef_mode == 1u || deck_phase_varies(t));
    if (plan.stream)
        for (uint32_t i = lane; i < plan.len; i += MX_DECK_CHUNK) win[i] = deck_frame(d, plan.lo + (int64_t)i);
    if (bank_lds)
        for (uint32_t i = lane; i < (uint32_t)DECK_BANK_FLOATS; i += MX_DECK_CHUNK) coef[(i >> 5) * DECK_COEF_STRIDE + (i & 31u)] = T[i];
    __syncthreads();
    if (lane >= cnt) return;

    int64_t u = deck_u(t.pos, t.step, t.dstep, (int64_t)(n0 + lane));
    if (t.loop_len) u = plan.stream ? u - plan.shift : deck_fold(u, (int64_t)t.loop_in << DECK_Q, (int64_t)t.loop_len << DECK_Q);
    const int64_t idx = u >> DECK_Q;
    const uint32_t p = (uint32_t)(u >> 24) & 255u;
    const double w = (double)(uint32_t)(u & 0xFFFFFF) * 0x1p-24;
    const uint32_t w0 = (uint32_t)(idx - 15 - plan.lo);   // streaming form: the first tap's place in the window
    float2 r;
    if (bank_lds) r = plan.stream ? deck_taps<true>(coef + p * DECK_COEF_STRIDE, DECK_COEF_STRIDE, win, w0, d, idx, w) : deck_taps<false>(coef + p * DECK_COEF_STRIDE, DECK_COEF_STRIDE, win, w0, d, idx, w);
    else r = plan.stream ? deck_taps<true>(T + p * MX_DECK_TAPS, MX_DECK_TAPS, win, w0, d, idx, w) : deck_taps<false>(T + p * MX_DECK_TAPS, MX_DECK_TAPS, win, w0, d, idx, w);
    out[lane] = r;
}

void launch_deck_feed(const DeckDev* decks, const DeckTickDev* ticks, const float* tables, uint32_t n, uint32_t n_ticks, uint32_t spt, bool phase_varies, hipStream_t s) {
    const uint32_t chunks = (spt + MX_DECK_CHUNK - 1) / MX_DECK_CHUNK;
    const uint64_t blocks = (uint64_t)n * n_ticks * chunks;
    if (!blocks) return;
    if (blocks > 0x7fffffffull) throw Error(MX_ERR_INVALID, "deck feed: decks x ticks x chunks exceed 2^31 workgroups");
    const char* const fe = getenv("MX_DECK_FORM");   // A/B only (see the head of this file)
    const int form = fe ? atoi(fe) : 0;
    const dim3 grid((unsigned)blocks), block(MX_DECK_CHUNK);
    if (form == 2) hipLaunchKernelGGL((k_deck_feed<0, 1>), grid, block, 0, s, decks, ticks, tables, n_ticks, spt, chunks, 0u);
    else if (form == 1 || (form != 3 && phase_varies)) hipLaunchKernelGGL((k_deck_feed<1, 0>), grid, block, 0, s, decks, ticks, tables, n_ticks, spt, chunks, form == 1 ? 1u : 0u);
    else hipLaunchKernelGGL((k_deck_feed<0, 0>), grid, block, 0, s, decks, ticks, tables, n_ticks, spt, chunks, 0u);
}

}  // namespace mx
