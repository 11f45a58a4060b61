// mx_deck_loudkey.cpp -- the deck's whole-track tonality and loudness, host side (include/mixlab_gpu.h "KEY AND LOUDNESS"): the setting rules,
// the rules themselves in plain C++ (mx_deck_tonality_host, mx_deck_loudness_host: the CPU test path and the single-thread baseline), and the deck's two analyses.
// (the library is built with -ffp-contract=off: every f64 operation below is rounded on its own, as the header says)
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "mx_deck_loudkey.hpp"

namespace mx {

static void frames_check(uint64_t n_frames, const char* what) {
    if (n_frames < 1 || n_frames > kDeckMaxFrames) throw Error(MX_ERR_INVALID, std::string(what) + ": n_frames outside 1 .. 2^30");
}

// ---- tonality ----
void deck_tonality_check(const mx_deck_tonality& t) {
    if (!tonality_params_ok(t.decim, t.hop_frames, t.octaves, t.f_lo_mhz, 1))
        throw Error(MX_ERR_INVALID, "deck tonality: decim must be 4 or 8, hop_frames 128, 256 or 512, octaves 2 .. 6, f_lo_mhz >= 1");
    if (t.segment_hops < 1 || t.segment_hops > 65536) throw Error(MX_ERR_INVALID, "deck tonality: segment_hops outside 1 .. 65536");
    if (t._pad) throw Error(MX_ERR_INVALID, "deck tonality: _pad must be 0");
    int16_t fir[64]; uint32_t len[72];
    const int rc = tonality_tables(t.rate, t.decim, t.octaves, t.f_lo_mhz, fir, len, nullptr, nullptr);
    if (rc == 1) throw Error(MX_ERR_INVALID, "deck tonality: the lowest bin's kernel, ceil(17 fs_d / f_lo), exceeds 2048 decimated frames");
    if (rc == 2) throw Error(MX_ERR_INVALID, "deck tonality: the highest bin reaches 0.45 fs_d, the decimator's cutoff");
    if (rc) throw Error(MX_ERR_INVALID, "deck tonality: rate must be finite and positive");
}

uint64_t deck_tonality_count(uint64_t n_frames, const mx_deck_tonality& t) {
    frames_check(n_frames, "deck tonality");
    deck_tonality_check(t);
    const uint64_t F = (uint64_t)t.segment_hops * t.hop_frames * t.decim;
    return (n_frames + F - 1) / F;
}

// the table set as both sides use it: fir, and uint32 len[B] | uint32 off[B] | int16 kern[sum len][2]
static void tonality_table_set(const mx_deck_tonality& t, DkFir& fir, std::vector<uint32_t>& tab) {
    const uint32_t B = 12 * t.octaves;
    uint32_t len[72]; size_t pairs = 0;
    std::memset(&fir, 0, sizeof fir);
    (void)tonality_tables(t.rate, t.decim, t.octaves, t.f_lo_mhz, fir.c, len, nullptr, &pairs);
    tab.assign(2 * (size_t)B + pairs, 0u);
    (void)tonality_tables(t.rate, t.decim, t.octaves, t.f_lo_mhz, fir.c, tab.data(), reinterpret_cast<int16_t*>(tab.data() + 2 * B), &pairs);
    uint32_t at = 0;
    for (uint32_t b = 0; b < B; ++b) { tab[B + b] = at; at += tab[b]; }
}

void deck_tonality_host(const int16_t* x, uint64_t n_frames, const mx_deck_tonality& t, uint64_t first, uint64_t n, void* dst) {
    if (!x) throw Error(MX_ERR_INVALID, "deck tonality: interleaved is NULL");
    const uint64_t n_seg = deck_tonality_count(n_frames, t);
    if (first > n_seg || n > n_seg - first) throw Error(MX_ERR_INVALID, "deck tonality: a window beyond the track's segments");
    if (n && !dst) throw Error(MX_ERR_INVALID, "deck tonality: dst is NULL");
    if (!n) return;
    const uint32_t D = t.decim, Hc = t.hop_frames, G = t.segment_hops, B = 12 * t.octaves, Tf = 8 * D;
    DkFir fir; std::vector<uint32_t> tab;
    tonality_table_set(t, fir, tab);
    const uint32_t* len = tab.data(); const uint32_t* off = len + B;
    const int16_t* kern = reinterpret_cast<const int16_t*>(off + B);
    auto q = [&](int64_t f) -> int32_t { return f < 0 || f >= (int64_t)n_frames ? 0 : dk_quant((int32_t)x[2 * f] + (int32_t)x[2 * f + 1]); };
    // the decimated frames the window's hops look at: [lo, hi), lo 2047 before the first hop's first
    const int64_t lo = (int64_t)(first * G * Hc) - (int64_t)(TON_MAX_KERNEL - 1), hi = (int64_t)((first + n) * G * Hc);
    std::vector<int16_t> d((size_t)(hi - lo), 0);
    for (int64_t j = std::max<int64_t>(lo, 0); j < hi; ++j) {
        int32_t acc = 0;   // |sum| <= 65534 x 2^14 < 2^30
        for (uint32_t k = 0; k < Tf; ++k) acc += (int32_t)fir.c[k] * q(j * D - (int64_t)k);
        d[(size_t)(j - lo)] = (int16_t)(acc >> 15);
    }
    const size_t rb = tonality_record_bytes(t.octaves);
    for (uint64_t g = first; g < first + n; ++g) {
        uint64_t C[72] = {};
        for (uint64_t h = g * G; h < (g + 1) * G; ++h) {
            const int64_t e = (int64_t)((h + 1) * Hc) - 1;
            for (uint32_t b = 0; b < B; ++b) {
                const uint32_t N = len[b];
                const int16_t* kb = kern + 2 * (size_t)off[b];
                const int16_t* db = d.data() + (size_t)(e - (int64_t)(N - 1) - lo);
                long long re = 0, im = 0;
                for (uint32_t i = 0; i < N; ++i) { re += (long long)((int32_t)kb[2 * i] * db[i]); im += (long long)((int32_t)kb[2 * i + 1] * db[i]); }
                C[b] += dk_magnitude(re, im);
            }
        }
        unsigned char* r = (unsigned char*)dst + (size_t)(g - first) * rb;
        const uint32_t head[8] = {(uint32_t)g, G, 0u, D, Hc, t.octaves, t.f_lo_mhz, 0u};
        std::memcpy(r, head, sizeof head);
        std::memcpy(r + 32, C, 8 * (size_t)B);
    }
}

// ---- loudness ----
void deck_loudness_check(const mx_deck_loudness& l) {
    if (l.block_frames < 64 || l.block_frames > 65536) throw Error(MX_ERR_INVALID, "deck loudness: block_frames outside 64 .. 65536");
    if (l.momentary_blocks < 1 || l.momentary_blocks > 1024 || l.short_blocks < 1 || l.short_blocks > 1024)
        throw Error(MX_ERR_INVALID, "deck loudness: a window outside 1 .. 1024 blocks");
    if (l._pad) throw Error(MX_ERR_INVALID, "deck loudness: _pad must be 0");
    if (!loudness_tables(l.rate, l.block_frames, nullptr, nullptr, nullptr)) throw Error(MX_ERR_INVALID, "deck loudness: rate must be finite and above twice the shelf frequency");
}

uint64_t deck_loudness_count(uint64_t n_frames, uint32_t block_frames) {
    frames_check(n_frames, "deck loudness");
    if (block_frames < 64 || block_frames > 65536) throw Error(MX_ERR_INVALID, "deck loudness: block_frames outside 64 .. 65536");
    return (n_frames + block_frames - 1) / block_frames;
}

void deck_loudness_host(const int16_t* x, uint64_t n_frames, const mx_deck_loudness& l, mx_loudness_tick* dst, uint64_t cap) {
    if (!x || !dst) throw Error(MX_ERR_INVALID, "deck loudness: NULL argument");
    deck_loudness_check(l);
    const uint64_t nb = deck_loudness_count(n_frames, l.block_frames);
    if (cap < nb) throw Error(MX_ERR_INVALID, "deck loudness: cap is below the track's blocks");
    const uint32_t F = l.block_frames;
    DkLoudTabs t;
    (void)loudness_tables(l.rate, F, t.bq, t.carry, t.interp);
    auto sample = [&](int64_t f, int c) -> float { return f < 0 || f >= (int64_t)n_frames ? 0.0f : (float)x[2 * f + c] / 32768.0f; };
    double S[2][4] = {};
    std::vector<double> e((size_t)nb);
    for (uint64_t k = 0; k < nb; ++k) {
        mx_loudness_tick r{};
        r.frames = F; r.channels = 2;
        for (int c = 0; c < 2; ++c) {
            double z[4] = {0.0, 0.0, 0.0, 0.0}, s[4] = {S[c][0], S[c][1], S[c][2], S[c][3]}, part[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            uint32_t pk = 0;
            for (uint32_t i = 0; i < F; ++i) {
                const int64_t f = (int64_t)(k * F + i);
                const double xv = (double)sample(f, c);
                (void)dk_biquad(t.bq + 5, dk_biquad(t.bq, xv, z[0], z[1]), z[2], z[3]);
                const double y = dk_biquad(t.bq + 5, dk_biquad(t.bq, xv, s[0], s[1]), s[2], s[3]);
                part[i & 7u] = part[i & 7u] + y * y;
                double acc[3] = {0.0, 0.0, 0.0};
                float xj = 0.0f;
                for (int j = 0; j < 12; ++j) {
                    xj = sample(f - 11 + j, c);
                    for (int p = 0; p < 3; ++p) acc[p] = acc[p] + (double)t.interp[12 * p + j] * (double)xj;
                }
                auto bits = [](float v) { uint32_t u; std::memcpy(&u, &v, 4); return u & 0x7fffffffu; };
                pk = std::max(pk, bits(xj));
                for (int p = 0; p < 3; ++p) pk = std::max(pk, bits((float)acc[p]));
            }
            for (uint32_t m = 4; m >= 1; m >>= 1)
                for (uint32_t j = 0; j < 8; ++j)
                    if (!(j & m)) part[j] = part[j] + part[j ^ m];
            r.ksq[c] = part[0];
            std::memcpy(&r.true_peak[c], &pk, 4);
            const double o0 = S[c][0], o1 = S[c][1], o2 = S[c][2], o3 = S[c][3];   // S' = Z + P S from the state the block started with
            for (uint32_t q = 0; q < 4; ++q) S[c][q] = dk_carry(t.carry, q, z[q], o0, o1, o2, o3);
        }
        e[(size_t)k] = r.ksq[0] + r.ksq[1];
        double ms = 0.0, ss = 0.0;
        for (uint32_t back = std::max(l.momentary_blocks, l.short_blocks); back-- > 0;) {   // ascending block: k - back
            const double v = back > k ? 0.0 : e[(size_t)(k - back)];
            if (back < l.momentary_blocks) ms = ms + v;
            if (back < l.short_blocks) ss = ss + v;
        }
        r.momentary_sq = ms; r.short_sq = ss;
        dst[k] = r;
    }
}

// ---- the deck's two analyses ----
namespace {
DeckLastForms last_tonality, last_loudness;   // mx_deck_debug_last_tonality / _loudness
bool same_tables(const mx_deck_tonality& a, const mx_deck_tonality& b) {
    return a.rate == b.rate && a.decim == b.decim && a.octaves == b.octaves && a.f_lo_mhz == b.f_lo_mhz;
}
}  // namespace

DeckTonality::DeckTonality(const DeckTrack& deck) : DeckTrackAnalysis(deck, last_tonality) {}

void DeckTonality::analyse(const mx_deck_tonality* t) {
    if (t) deck_tonality_check(*t);
    const uint64_t n_seg = t ? deck_tonality_count(deck_.n_frames, *t) : 0;
    const size_t rb = t ? tonality_record_bytes(t->octaves) : 0;
    const size_t rec_bytes = (size_t)n_seg * rb, need = t ? rec_bytes + (size_t)n_seg * t->segment_hops * t->hop_frames * sizeof(int16_t) : 0;   // (rb is a multiple of 8)
    const bool new_tables = t && !(tab_.p && same_tables(*t, tab_for_));
    // the record buffer goes only when it is too small or on NULL; new tables alone make the wait, since an analysis in flight reads the old ones
    if (!prepare(need, !t, new_tables)) {
        tab_.free_();   // the tables go on NULL only
        return;
    }
    DkFir fir;
    if (new_tables) {   // (the stream is idle: waited for above.  The tables cost the host more than the kernels cost the device: made once per setting)
        std::vector<uint32_t> tab;
        tonality_table_set(*t, fir, tab);
        tab_.free_();
        tab_.alloc(tab.size() * sizeof(uint32_t));
        hip_check(hipMemcpy(tab_.p, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice), "hipMemcpy(deck tonality tables)");
        tab_for_ = *t;
        std::memcpy(fir_, fir.c, sizeof fir_);
    }
    std::memcpy(fir.c, fir_, sizeof fir_);
    DkTonArgs a{deck_.track, (int64_t)deck_.n_frames, t->decim, t->hop_frames, 12 * t->octaves, t->f_lo_mhz, t->segment_hops, n_seg,
                (const uint32_t*)tab_.p, (uint32_t*)buf_.p, (uint32_t)(rb / 4), (int16_t*)((char*)buf_.p + rec_bytes)};
    uint32_t forms[4];
    launch_deck_tonality(a, fir, forms, deck_.load_stream);
    rec_bytes_ = rb;
    launched("deck tonality launch", n_seg, forms);
}

void DeckTonality::read(uint64_t first, uint64_t n, void* dst, size_t cap_bytes) {
    read_window(first, n, dst, rec_bytes_, 0, count_,
                {"deck: no tonality analysis", "deck: a window beyond the tonality analysis' segments", "deck: dst is NULL", "hipMemcpy(deck tonality)"}, cap_bytes);
}

void DeckTonality::debug_last(uint32_t out[4]) { last_tonality.get(out); }

DeckLoudness::DeckLoudness(const DeckTrack& deck) : DeckTrackAnalysis(deck, last_loudness) {}

void DeckLoudness::analyse(const mx_deck_loudness* l) {
    if (l) deck_loudness_check(*l);
    const uint64_t nb = l ? deck_loudness_count(deck_.n_frames, l->block_frames) : 0;
    if (!prepare((size_t)nb * (sizeof(LoudTick) + 2 * 4 * sizeof(double)), !l)) return;
    DkLoudTabs t;
    (void)loudness_tables(l->rate, l->block_frames, t.bq, t.carry, t.interp);
    DkLoudArgs a{deck_.track, (int64_t)deck_.n_frames, l->block_frames, l->momentary_blocks, l->short_blocks, (uint32_t)nb, (LoudTick*)buf_.p,
                 (double*)((char*)buf_.p + (size_t)nb * sizeof(LoudTick))};
    uint32_t forms[4];
    launch_deck_loudness(a, t, forms, deck_.load_stream);
    launched("deck loudness launch", nb, forms);
}

void DeckLoudness::read(uint64_t first, uint64_t n, mx_loudness_tick* dst) {
    static_assert(sizeof(mx_loudness_tick) == sizeof(LoudTick), "mx_loudness_tick is the kernels' record");
    read_window(first, n, dst, sizeof(LoudTick), 0, count_,
                {"deck: no loudness analysis", "deck: a window beyond the loudness analysis' blocks", "deck: dst is NULL", "hipMemcpy(deck loudness)"});
}

void DeckLoudness::debug_last(uint32_t out[4]) { last_loudness.get(out); }

}  // namespace mx
