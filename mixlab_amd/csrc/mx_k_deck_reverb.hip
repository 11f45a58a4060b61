// mx_k_deck_reverb.hip -- the deck's reverb on the device (include/mixlab_gpu.h "REVERB"): a feedback delay network of four allpass diffusers
// and eight tank lines, run in place on the port buffer the feed, key-lock, filter and echo kernels have just written.
//
// Frame t reads tank line i at t - D_i - 1 .. t - D_i + 1 and diffuser j at t - d_j, and writes all twelve at t, so the frames of a block [t0, t0 + B) are
// independent of one another when each of them reads below t0 (mx_deck_reverb.hpp reverb_block_end): B is at most the reach, min(min D_i - 1, min d_j), a few
// hundred frames at real-time settings and far below a tick.  There is no one-block form here: a tick is always several dependent blocks.
// k_deck_reverb       one workgroup of REVERB_LANES lanes per reverberated deck walks the deck's blocks in order, cutting them itself by the shared rule (uniform
//                     across the lanes).  Within a block the ticks it touches are taken one after another -- the tick index is uniform, so the tick's 176-byte
//                     descriptor comes through uniform (scalar) loads and never rides the per-frame path -- and the lanes stride the block's frames of that tick;
//                     each lane runs the whole network for its frame (mx_deck_reverb.hpp reverb_frame: 4 diffuser reads, 24 tank reads, 12 line stores, one port
//                     store).  The pieces of one block need no barrier between them: they are independent by the block rule.  __syncthreads() between blocks.
// The lines are in global memory, written and read by this one workgroup: the barrier's workgroup-scope ordering is what makes a block's stores visible to the next
// block's loads (the echo walk's argument, mx_k_deck_echo.hip).  The rings are one per line, structure-of-arrays, so consecutive lanes read and write consecutive
// words of each ring.  A read below clock 0 is zero, so a restarted clock needs no cleared rings; every ring index is masked into the ring, so no clock can leave it.
// Every multiply, add and subtract is a separate f64 operation (the build sets -ffp-contract=off).
#include "mx_deck_reverb.hpp"
#include "mx_kernels.hpp"

namespace mx {

__global__ __launch_bounds__(REVERB_LANES) void k_deck_reverb(const ReverbDeckDev* __restrict__ decks, const ReverbTickDev* __restrict__ ticks, uint32_t n_ticks, uint32_t spt) {
    const ReverbDeckDev d = decks[blockIdx.x];
    const ReverbTickDev* const tk = ticks + (size_t)blockIdx.x * n_ticks;
    const uint64_t total = (uint64_t)n_ticks * spt;
    for (uint64_t f = 0; f < total;) {
        const uint32_t k0 = (uint32_t)(f / spt);
        if (!(tk[k0].flags & REVERB_TICK_ON)) { f = (uint64_t)(k0 + 1) * spt; continue; }
        const uint64_t e = reverb_block_end(f, k0, n_ticks, spt, tk);
        for (uint32_t k = k0; (uint64_t)k * spt < e; ++k) {                  // the block's piece of tick k: frames [lo, hi) of the feed
            const uint64_t a = (uint64_t)k * spt, lo = a > f ? a : f, hi = a + spt < e ? a + spt : e;
            for (uint64_t i = lo + threadIdx.x; i < hi; i += REVERB_LANES) reverb_frame(d.lines, tk[k], (uint32_t)(i - a), spt, (float*)(d.port + i));
        }
        __syncthreads();
        f = e;
    }
}

void launch_deck_reverb(const ReverbDeckDev* decks, const ReverbTickDev* ticks, uint32_t n_decks, uint32_t n_ticks, uint32_t spt, hipStream_t s) {
    if (n_decks) hipLaunchKernelGGL(k_deck_reverb, dim3(n_decks), dim3(REVERB_LANES), 0, s, decks, ticks, n_ticks, spt);
}

}  // namespace mx
