// mx_deck_loudkey.hpp -- the deck's whole-track tonality and loudness (include/mixlab_gpu.h "KEY AND LOUDNESS"): the rules that the host
// functions (mx_deck_loudkey.cpp) and the kernels (mx_k_deck_tonality.hip, mx_k_deck_loudness.hip) both evaluate, stated once, the launches, and the deck's two
// analyses (internal).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "mx_common.hpp"
#include "mx_deck_analysis.hpp"
#include "mx_dev.hpp"

namespace mx {

// s = L + R of one track frame as the deck stores it (L in the low half), and the tap's q: s / 4, truncating toward zero
__host__ __device__ inline int32_t dk_sum(uint32_t frame) { return (int32_t)(int16_t)(frame & 0xffffu) + (int32_t)(int16_t)(frame >> 16); }
__host__ __device__ inline int32_t dk_quant(int32_t s) { return s / 4; }
// M_b[h] from the two sums (ton_root: mx_dev.hpp, the taps' own)
__host__ __device__ inline uint64_t dk_magnitude(long long re, long long im) {
    const long long a = re >> 10, b = im >> 10;   // floor; |a|, |b| <= 2^30
    return ton_root((uint64_t)(a * a) + (uint64_t)(b * b));
}
// one sample through one biquad of the loudness taps, transposed direct form II (q: b0 b1 b2 a1 a2); the files that use it are built with -ffp-contract=off
__host__ __device__ inline double dk_biquad(const double* q, double x, double& s1, double& s2) {
    const double y = q[0] * x + s1;
    s1 = (q[1] * x - q[3] * y) + s2;
    s2 = q[2] * x - q[4] * y;
    return y;
}
// row r of S' = Z + P S
__host__ __device__ inline double dk_carry(const double* P, uint32_t r, double z, double s0, double s1, double s2, double s3) {
    return z + (((P[4 * r] * s0 + P[4 * r + 1] * s1) + P[4 * r + 2] * s2) + P[4 * r + 3] * s3);
}

// ---- tonality: head -> decimate -> constant-Q, all on stream s ----
// tab: uint32 len[B] | uint32 off[B] (pairs before bin b) | int16 kern[sum len][2], on the device.  rec: n_seg records of rec_words uint32 each.  dec: n_seg G Hc int16.
enum { DK_TON_OUT = 512, DK_TON_HOPS = 8, DK_TON_FORM_DECIMATE = 0, DK_TON_FORM_FULL = 1, DK_TON_FORM_PART = 2, DK_TON_FORM_HEAD = 3 };
struct DkFir { int16_t c[64]; };
struct DkTonArgs {
    const uint32_t* track; int64_t n_frames;
    uint32_t D, Hc, bins, f_lo_mhz, G;
    uint64_t n_seg;
    const uint32_t* tab;
    uint32_t* rec; uint32_t rec_words;
    int16_t* dec;
};
void launch_deck_tonality(const DkTonArgs& a, const DkFir& fir, uint32_t forms[4], hipStream_t s);

// ---- loudness: zero the records -> peak, walk<ZERO>, scan, walk<ENERGY>, window, all on stream s ----
enum { DK_LOUD_TILE = 1024, DK_LOUD_FORM_PEAK = 0, DK_LOUD_FORM_WALK = 1, DK_LOUD_FORM_SCAN = 2, DK_LOUD_FORM_WINDOW = 3 };
struct DkLoudTabs { double bq[10], carry[16]; float interp[36]; };
struct DkLoudArgs {
    const uint32_t* track; int64_t n_frames;
    uint32_t F, M, S, n_blocks;
    LoudTick* rec;     // [n_blocks]
    double* walk;      // [channel][n_blocks][4]: Z_k, then S_k
};
void launch_deck_loudness(const DkLoudArgs& a, const DkLoudTabs& t, uint32_t forms[4], hipStream_t s);

// ---- host ----
void deck_tonality_check(const mx_deck_tonality& t);                                 // throws Error(MX_ERR_INVALID) naming the rule
uint64_t deck_tonality_count(uint64_t n_frames, const mx_deck_tonality& t);
void deck_tonality_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_tonality& t, uint64_t first, uint64_t n, void* dst);
void deck_loudness_check(const mx_deck_loudness& l);                                 // throws Error(MX_ERR_INVALID) naming the rule
uint64_t deck_loudness_count(uint64_t n_frames, uint32_t block_frames);
void deck_loudness_host(const int16_t* interleaved, uint64_t n_frames, const mx_deck_loudness& l, mx_loudness_tick* dst, uint64_t cap);

// one buffer -- count_ segment records of rec_bytes_, then the decimated frames -- and the table set of tab_for_ with its decimator taps fir_, kept while the settings
// that shape them stay
class DeckTonality : public DeckTrackAnalysis {
public:
    explicit DeckTonality(const DeckTrack& deck);
    void analyse(const mx_deck_tonality* t);                               // NULL: frees the results.  Asynchronous on the load stream.
    void read(uint64_t first, uint64_t n, void* dst, size_t cap_bytes);    // waits for the analysis
    static void debug_last(uint32_t out[4]);
private:
    DevBuf tab_;
    mx_deck_tonality tab_for_{}; int16_t fir_[64] = {};
    size_t rec_bytes_ = 0;
};

// one buffer -- count_ block records, then the walk states
class DeckLoudness : public DeckTrackAnalysis {
public:
    explicit DeckLoudness(const DeckTrack& deck);
    void analyse(const mx_deck_loudness* l);                               // NULL: frees the results.  Asynchronous on the load stream.
    void read(uint64_t first, uint64_t n, mx_loudness_tick* dst);          // waits for the analysis
    static void debug_last(uint32_t out[4]);
};

}  // namespace mx
