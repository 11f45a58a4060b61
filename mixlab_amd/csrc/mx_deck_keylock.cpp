// mx_deck_keylock.cpp -- the deck's key-lock, host side (include/mixlab_gpu.h "KEY-LOCK"): the setting rules, the grain search rule in plain
// C++ (mx_deck_keylock_search: the CPU test path), the setting, the read-out of the last feed's grains and the launch plan of its key-locked ticks.  The grain clock
// itself runs in the feed (mx_deck.cpp).
#include <algorithm>
#include <cstring>

#include "mx_deck.hpp"

namespace mx {

static const int64_t kOne = (int64_t)1 << DECK_Q, kMaxStep = 4 * kOne;

void deck_keylock_check(const mx_deck_keylock& k) {
    auto pow2 = [](uint32_t v) { return v && !(v & (v - 1)); };
    if (k.pitch_q32 < kOne / 4 || k.pitch_q32 > kMaxStep) throw Error(MX_ERR_INVALID, "deck key-lock: pitch_q32 outside 2^30 .. 4 * 2^32");
    if (!pow2(k.hop) || k.hop < 256 || k.hop > 8192) throw Error(MX_ERR_INVALID, "deck key-lock: hop is not a power of two in 256 .. 8192");
    if (!pow2(k.overlap) || k.overlap < 16 || k.overlap > std::min<uint32_t>(k.hop / 2, 1024)) throw Error(MX_ERR_INVALID, "deck key-lock: overlap is not a power of two in 16 .. min(hop / 2, 1024)");
    if (k.radius > 1024) throw Error(MX_ERR_INVALID, "deck key-lock: radius above 1024");
    if (k._pad) throw Error(MX_ERR_INVALID, "deck key-lock: _pad must be 0");
}

void deck_keylock_search(const int16_t* x, uint64_t n_frames, int64_t C, int64_t A, uint32_t overlap, uint32_t radius, int32_t& delta, uint32_t& dist) {
    const int64_t far = (int64_t)1 << 40;
    if (!x) throw Error(MX_ERR_INVALID, "deck key-lock search: interleaved is NULL");
    if (n_frames < 1 || n_frames > kDeckMaxFrames) throw Error(MX_ERR_INVALID, "deck key-lock search: n_frames outside 1 .. 2^30");
    if (overlap < 1 || overlap > 1024 || radius > 1024) throw Error(MX_ERR_INVALID, "deck key-lock search: overlap outside 1 .. 1024 or radius above 1024");
    if (C < -far || C > far || A < -far || A > far) throw Error(MX_ERR_INVALID, "deck key-lock search: |C| or |A| above 2^40 frames");
    auto s = [&](int64_t f) -> int32_t { return f < 0 || f >= (int64_t)n_frames ? 0 : (int32_t)x[2 * f] + (int32_t)x[2 * f + 1]; };
    bool have = false;
    // scanned in the tie order itself -- 0, -1, +1, -2, +2, ... -- so that a strictly smaller D is the only thing that replaces the best so far
    for (int64_t q = 0; q <= (int64_t)radius; ++q)
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            if (q == 0 && sgn > 0) continue;
            const int64_t dl = sgn * q;
            uint32_t D = 0;
            for (uint32_t i = 0; i < overlap; ++i) { const int32_t v = s(C + i) - s(A + dl + i); D += (uint32_t)(v < 0 ? -v : v); }
            if (!have || D < dist) { have = true; dist = D; delta = (int32_t)dl; }
        }
}

void Deck::set_keylock(const mx_deck_keylock* k) {
    DeckKeylock& kl = keylock_;
    if (k) {
        deck_keylock_check(*k);
        if (!kl.state.p) { hip_check(hipSetDevice(device_), "hipSetDevice"); kl.state.alloc(2 * sizeof(int64_t)); }
        kl.k = *k;
        kl.bank = k->pitch_q32 <= kOne ? 0u : 3 * k->pitch_q32 <= 4 * kOne ? 1u : k->pitch_q32 <= 2 * kOne ? 2u : 3u;
        kl.log_hop = 0;
        while ((1u << kl.log_hop) < k->hop) ++kl.log_hop;
    }
    kl.on = k != nullptr;
    kl.t = 0;
}

void Deck::fetch_grains() {
    DeckKeylock& kl = keylock_;
    if (kl.grains_fetched) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    std::vector<KlRec> r(kl.grains.size());
    hip_check(hipMemcpy(r.data(), (const KlRec*)kl.rec.p + 2, r.size() * sizeof(KlRec), hipMemcpyDeviceToHost), "hipMemcpy(deck grains)");
    for (size_t k = 0; k < r.size(); ++k) { kl.grains[k].g_q32 = r[k].g; kl.grains[k].delta = r[k].delta; kl.grains[k].dist = r[k].dist; }
    kl.grains_fetched = true;
}

void Deck::read_grains(uint32_t first, uint32_t n, mx_deck_grain* dst) {
    const std::vector<mx_deck_grain>& grains = keylock_.grains;
    if (first > grains.size() || n > grains.size() - first) throw Error(MX_ERR_INVALID, "deck: a window beyond the last feed's grains");
    if (n && !dst) throw Error(MX_ERR_INVALID, "deck: dst is NULL");
    if (!n) return;
    fetch_grains();
    std::memcpy(dst, grains.data() + first, (size_t)n * sizeof(mx_deck_grain));
}

void Deck::debug_last_keylock(uint32_t out[4]) {
    const DeckLastKeylock last = deck_last_keylock();
    out[0] = last.searched; out[1] = last.unsearched; out[2] = out[3] = 0;
    const uint32_t spt = last.spt;
    for (const DeckKlTick& k : last.ticks) {
        if (!k.t.play) continue;
        const uint32_t hop = 1u << k.log_hop;
        for (uint32_t n0 = 0; n0 < spt; n0 += MX_DECK_CHUNK) {
            const uint32_t a = k.t.m0 + n0, b = a + std::min<uint32_t>(MX_DECK_CHUNK, spt - n0) - 1;   // the chunk's clock, first and last lane
            if ((a >> k.log_hop) != (b >> k.log_hop)) ++out[3];
            bool fades = false;
            for (uint32_t dj = a >> k.log_hop; dj <= (b >> k.log_hop); ++dj)   // per grain of the chunk, the smallest m is that of its first lane
                if ((std::max(a, dj * hop) & (hop - 1)) < k.overlap && !(k.t.first0 && dj == 0)) fades = true;
            if (fades) ++out[2];
        }
    }
}

}  // namespace mx
