// mx_k_deck_filter.hip -- the deck's resonant sweep filter on the device (include/mixlab_gpu.h "FILTER"): a trapezoidal state-variable filter
// run in place on the port buffer the feed and key-lock kernels have just written, ahead of the echo.
//
// The recurrence is serial in time per (deck, channel); everything round it is not.  One wave (a workgroup of FILTER_BLOCK = 64 lanes) per filtered deck walks the
// feed in super-blocks of 64 frames, counted from the feed's first frame, so a super-block may straddle a tick boundary and each lane takes the descriptor of its
// own frame's tick:
//   A  a lane per frame: the frame's L R pair (one coalesced 512-byte row) and its tick's descriptor were fetched a super-block ahead; compute the frame's
//      coefficients (the two f64 divisions n / spt and 1 / d are here), put x and a1 a2 a3 into LDS, fetch the next super-block's row and descriptors;
//   B  lanes 0 and 1 (L and R) walk the 64 frames with s1 s2 in registers.  The LDS addresses they read do not depend on the state, so the unrolled loop issues
//      the reads ahead of use; lanes 0 and 1 read the same coefficient words (a broadcast).  v1 and v2 go back to LDS;
//   C  a lane per frame: pick the response from v1 v2, mix it with x by wet, store the row.
// The state comes from and goes to the deck's four doubles at the feed's ends.  Every multiply, add and divide is a separate f64 operation (the build sets
// -ffp-contract=off; f64 division is the correctly rounded one).
#include "mx_deck_filter.hpp"
#include "mx_kernels.hpp"

namespace mx {

// what a lane holds of its frame of a super-block: the frame's tick (flags 0 past the feed's end), its index n in the tick, the L R pair the deck wrote
struct FilterLane { FilterTickDev t; float2 x; };
__device__ inline void filter_fetch(const FilterDeckDev& d, const FilterTickDev* tk, uint64_t f, uint64_t total, uint32_t k, FilterLane& out) {
    out.t.flags = 0; out.x = make_float2(0.0f, 0.0f);
    if (f < total) { out.t = tk[k]; out.x = d.port[f]; }
}

__global__ __launch_bounds__(FILTER_BLOCK) void k_deck_filter(const FilterDeckDev* __restrict__ decks, const FilterTickDev* __restrict__ ticks, uint32_t n_ticks, uint32_t spt) {
    __shared__ double sh_a[FILTER_BLOCK][4];      // a1 a2 a3 of each frame of the super-block (zeros for a frame without a filter), one 32-byte row a frame
    __shared__ double sh_x[FILTER_BLOCK][2];      // x of L and R
    __shared__ double sh_v[FILTER_BLOCK][2][2];   // v1 v2 of L and R
    __shared__ uint32_t sh_code[FILTER_BLOCK];    // 0: no filter in this frame (or past the feed's end); 1: filter; 3: filter, the state cleared first
    const FilterDeckDev d = decks[blockIdx.x];
    const FilterTickDev* const tk = ticks + (size_t)blockIdx.x * n_ticks;
    const uint64_t total = (uint64_t)n_ticks * spt;
    const uint32_t lane = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    if (lane < 2) { s1 = d.state[2 * lane]; s2 = d.state[2 * lane + 1]; }
    // the lane's frame of the first super-block; from then on the frame of the NEXT super-block is fetched ahead of phase B, whose walk hides the two loads
    uint32_t k = lane / spt, n = lane - k * spt;
    FilterLane cur, nxt;
    filter_fetch(d, tk, lane, total, k, cur);
    for (uint64_t f0 = 0; f0 < total; f0 += FILTER_BLOCK) {
        // ---- A ----
        const uint64_t f = f0 + lane;
        const uint32_t kind = cur.t.kind;
        uint32_t code = 0;
        double xl = 0.0, xr = 0.0, kn = 0.0, wn = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        if (cur.t.flags & FILTER_TICK_ON) {
            const FilterCoef c = filter_coef(cur.t, n, spt);
            xl = (double)cur.x.x; xr = (double)cur.x.y; kn = c.kn; wn = c.wn; a1 = c.a1; a2 = c.a2; a3 = c.a3;
            code = (n == 0 && (cur.t.flags & FILTER_TICK_CLEAR)) ? 3u : 1u;
        }
        sh_a[lane][0] = a1; sh_a[lane][1] = a2; sh_a[lane][2] = a3;
        sh_x[lane][0] = xl; sh_x[lane][1] = xr;
        sh_code[lane] = code;
        n += FILTER_BLOCK;
        if (n >= spt) { const uint32_t q = n / spt; k += q; n -= q * spt; }
        filter_fetch(d, tk, f + FILTER_BLOCK, total, k, nxt);
        __syncthreads();
        // ---- B: no branch on the frame's code, so that every LDS read of the unrolled stretch can go out ahead of the chain ----
        if (lane < 2) {
#pragma unroll 16
            for (uint32_t i = 0; i < FILTER_BLOCK; ++i) {
                const uint32_t c = sh_code[i];
                const double b1 = (c & 2u) ? 0.0 : s1, b2 = (c & 2u) ? 0.0 : s2;
                double m1 = b1, m2 = b2, v1, v2;
                filter_step(sh_x[i][lane], sh_a[i][0], sh_a[i][1], sh_a[i][2], m1, m2, v1, v2);
                s1 = c ? m1 : s1; s2 = c ? m2 : s2;
                sh_v[i][lane][0] = v1; sh_v[i][lane][1] = v2;
            }
        }
        __syncthreads();
        // ---- C ----
        if (code) d.port[f] = make_float2(filter_out(kind, xl, kn, wn, sh_v[lane][0][0], sh_v[lane][0][1]), filter_out(kind, xr, kn, wn, sh_v[lane][1][0], sh_v[lane][1][1]));
        cur = nxt;
    }
    if (lane < 2) { d.state[2 * lane] = s1; d.state[2 * lane + 1] = s2; }
}

void launch_deck_filter(const FilterDeckDev* decks, const FilterTickDev* ticks, uint32_t n_decks, uint32_t n_ticks, uint32_t spt, hipStream_t s) {
    if (n_decks) hipLaunchKernelGGL(k_deck_filter, dim3(n_decks), dim3(FILTER_BLOCK), 0, s, decks, ticks, n_ticks, spt);
}

}  // namespace mx
