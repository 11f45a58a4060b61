// mx_k_deck_echo.hip -- the deck's beat echo on the device (include/mixlab_gpu.h "ECHO"): a feedback delay run in place on the port buffer the
// feed and key-lock kernels have just written.
//
// Frame t reads the delay line at t - D - 1 .. t - D + 1 and writes it at t, so the frames of a block [t0, t0 + B) are independent of one another when each of them
// reads below t0 (mx_deck_echo.hpp echo_block_end).  Two forms:
// k_deck_echo_block   the decks whose echo frames of the feed are ONE block (every one-tick feed with D > spt): the grid of k_deck_feed, a workgroup per chunk of
//                     MX_DECK_CHUNK frames, a lane per frame, no barrier.
// k_deck_echo_walk    every other deck: one workgroup of ECHO_LANES lanes walks the deck's blocks in order, cutting them itself by the shared rule (uniform across
//                     the lanes); lanes stride the frames of a block, __syncthreads() between blocks.  The line is in global memory, written and read by this one
//                     workgroup: the barrier's workgroup-scope ordering is what makes a block's stores visible to the next block's loads.
// The line is a ring of ECHO_RING frames, L and R adjacent: one frame is one 64-bit access.  A frame before t = 0 reads as zero, so a restarted clock needs no
// cleared ring.  Every multiply and add is a separate f64 operation (the build sets -ffp-contract=off).
#include "mx_deck_echo.hpp"
#include "mx_kernels.hpp"

namespace mx {

__device__ inline float2 echo_line(const float2* line, int64_t s) {
    return s < 0 ? make_float2(0.0f, 0.0f) : line[(uint64_t)s & (uint64_t)(ECHO_RING - 1)];
}

__device__ inline float echo_gain(float g0, float g1, bool ramp, double w) {
    return ramp ? (float)((double)g0 + ((double)g1 - (double)g0) * w) : g1;
}

// frame n of tick k: port[0] is the frame's L R pair
__device__ inline void echo_frame(float2* line, const EchoTickDev& k, uint32_t n, uint32_t spt, float2* port) {
    const uint64_t t = k.t0 + n;
    const int64_t s = (int64_t)t - (int64_t)k.delay;
    const float2 x = *port;
    float2 r0 = echo_line(line, s), rm = echo_line(line, s - 1), rp = echo_line(line, s + 1);
    if (k.flags & ECHO_TICK_PINGPONG) { r0 = make_float2(r0.y, r0.x); rm = make_float2(rm.y, rm.x); rp = make_float2(rp.y, rp.x); }
    const bool ramp = (k.flags & ECHO_TICK_RAMP) != 0;
    const double w = (double)n / (double)spt;
    const double send = (double)echo_gain(k.send0, k.send1, ramp, w), fb = (double)echo_gain(k.fb0, k.fb1, ramp, w), wet = (double)echo_gain(k.wet0, k.wet1, ramp, w);
    const double fl = k.b * (double)r0.x + k.a * (double)rm.x + k.a * (double)rp.x;
    const double fr = k.b * (double)r0.y + k.a * (double)rm.y + k.a * (double)rp.y;
    const double xl = (double)x.x, xr = (double)x.y;
    line[t & (uint64_t)(ECHO_RING - 1)] = make_float2((float)(send * xl + fb * fl), (float)(send * xr + fb * fr));
    *port = make_float2((float)(xl + wet * fl), (float)(xr + wet * fr));
}

__global__ __launch_bounds__(MX_DECK_CHUNK) void k_deck_echo_block(const EchoDeckDev* __restrict__ decks, const EchoTickDev* __restrict__ ticks, uint32_t n_ticks, uint32_t spt,
                                                                   uint32_t chunks) {
    const uint32_t item = blockIdx.x / chunks, c = blockIdx.x - item * chunks;
    const uint32_t deck = item / n_ticks, tick = item - deck * n_ticks;
    const EchoTickDev k = ticks[item];
    const uint32_t n = c * MX_DECK_CHUNK + threadIdx.x;
    if (!(k.flags & ECHO_TICK_ON) || n >= spt) return;
    const EchoDeckDev d = decks[deck];
    echo_frame(d.line, k, n, spt, d.port + (size_t)tick * spt + n);
}

__global__ __launch_bounds__(ECHO_LANES) void k_deck_echo_walk(const EchoDeckDev* __restrict__ decks, const EchoTickDev* __restrict__ ticks, uint32_t n_ticks, uint32_t spt) {
    const EchoDeckDev d = decks[blockIdx.x];
    const EchoTickDev* const tk = ticks + (size_t)blockIdx.x * n_ticks;
    const uint64_t total = (uint64_t)n_ticks * spt;
    for (uint64_t f = 0; f < total;) {
        const uint32_t k0 = (uint32_t)(f / spt);
        if (!(tk[k0].flags & ECHO_TICK_ON)) { f = (uint64_t)(k0 + 1) * spt; continue; }
        const uint64_t e = echo_block_end(f, k0, n_ticks, spt, tk);
        for (uint64_t i = f + threadIdx.x; i < e; i += ECHO_LANES) {
            const uint32_t k = (uint32_t)(i / spt);
            echo_frame(d.line, tk[k], (uint32_t)(i - (uint64_t)k * spt), spt, d.port + i);
        }
        __syncthreads();
        f = e;
    }
}

void launch_deck_echo(const EchoDeckDev* decks, const EchoTickDev* ticks, uint32_t n_block, uint32_t n_walk, uint32_t n_ticks, uint32_t spt, hipStream_t s) {
    const uint32_t chunks = (spt + MX_DECK_CHUNK - 1) / MX_DECK_CHUNK;
    const uint64_t blocks = (uint64_t)n_block * n_ticks * chunks;
    if (blocks > 0x7fffffffull) throw Error(MX_ERR_INVALID, "deck feed: echo decks x ticks x chunks exceed 2^31 workgroups");
    if (blocks) hipLaunchKernelGGL(k_deck_echo_block, dim3((unsigned)blocks), dim3(MX_DECK_CHUNK), 0, s, decks, ticks, n_ticks, spt, chunks);
    if (n_walk) hipLaunchKernelGGL(k_deck_echo_walk, dim3(n_walk), dim3(ECHO_LANES), 0, s, decks + n_block, ticks + (size_t)n_block * n_ticks, n_ticks, spt);
}

}  // namespace mx
