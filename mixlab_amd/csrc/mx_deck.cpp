// mx_deck.cpp -- the deck's host side: parameter rules, the per-tick state machine (mx_deck_plan), the coefficient tables, the track, and the feed that turns the
// coming ticks of many decks into one descriptor block and one launch (include/mixlab_gpu.h "the deck").
#include "mx_deck.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>

#include "mx_dev.hpp"
#include "mx_engine.hpp"
#include "mx_kernels.hpp"

namespace mx {

static const int64_t kOne = (int64_t)1 << DECK_Q, kMaxStep = 4 * kOne, kMaxSlew = (int64_t)1 << 24, kMargin = (int64_t)1 << 20;
static const uint64_t kMaxFrames = (uint64_t)1 << 30;

void deck_check(const mx_deck_params& p, uint64_t n_frames) {
    if (n_frames < 1 || n_frames > kMaxFrames) throw Error(MX_ERR_INVALID, "deck: n_frames outside 1 .. 2^30");
    if (p.step_q32 > kMaxStep || p.step_q32 < -kMaxStep) throw Error(MX_ERR_INVALID, "deck: |step_q32| above 4 * 2^32");
    if (p.slew_q32 < 0 || p.slew_q32 > kMaxSlew) throw Error(MX_ERR_INVALID, "deck: slew_q32 outside 0 .. 2^24");
    if (p.flags & ~(MX_DECK_PLAY | MX_DECK_LOOP)) throw Error(MX_ERR_INVALID, "deck: a flag bit outside MX_DECK_PLAY | MX_DECK_LOOP");
    if (p._pad) throw Error(MX_ERR_INVALID, "deck: _pad must be 0");
    if ((p.flags & MX_DECK_LOOP) && !(p.loop_in >= 0 && p.loop_in < p.loop_out && p.loop_out <= (int64_t)n_frames))
        throw Error(MX_ERR_INVALID, "deck: with MX_DECK_LOOP, 0 <= loop_in < loop_out <= n_frames");
}

static inline int64_t iabs64(int64_t v) { return v < 0 ? -v : v; }

void deck_plan(const mx_deck_head& in, const mx_deck_params* params, const int64_t* seek, uint32_t spt, uint64_t n_frames, mx_deck_tick& tick, mx_deck_head& out) {
    if (spt < 1 || spt > MX_DECK_MAX_SPT) throw Error(MX_ERR_INVALID, "deck: frames per tick outside 1 .. MX_DECK_MAX_SPT");
    if (params) deck_check(*params, n_frames);
    else if (n_frames < 1 || n_frames > kMaxFrames) throw Error(MX_ERR_INVALID, "deck: n_frames outside 1 .. 2^30");
    if (in.step_q32 > kMaxStep || in.step_q32 < -kMaxStep) throw Error(MX_ERR_INVALID, "deck: the head's |step_q32| is above 4 * 2^32");
    mx_deck_head h = in;
    if (seek) h.pos_q32 = *seek;                                                                   // 1.
    if (params) h.params = *params;                                                                // 2.
    const mx_deck_params& p = h.params;
    const int64_t lo = -kMargin * kOne, hi = ((int64_t)n_frames + kMargin) * kOne;                 // 3.
    h.pos_q32 = std::min(std::max(h.pos_q32, lo), hi);
    const bool looping = (p.flags & MX_DECK_LOOP) &&                                               // 4.
        ((h.last_looping && h.last_loop_in == p.loop_in && h.last_loop_out == p.loop_out) || (h.pos_q32 >= p.loop_in * kOne && h.pos_q32 < p.loop_out * kOne));
    const bool play = (p.flags & MX_DECK_PLAY) != 0;
    int64_t dstep = 0, m = 0;
    if (play) {                                                                                    // 5.
        if (p.slew_q32 == 0) h.step_q32 = p.step_q32;
        else {
            dstep = std::min(std::max((p.step_q32 - h.step_q32) / (int64_t)spt, -p.slew_q32), p.slew_q32);
            if (dstep == 0) h.step_q32 = p.step_q32;
        }
        m = std::max(iabs64(h.step_q32), iabs64(h.step_q32 + (int64_t)(spt - 1) * dstep));
    }
    tick.pos_q32 = h.pos_q32; tick.step_q32 = h.step_q32; tick.dstep_q32 = dstep;
    tick.loop_in = looping ? p.loop_in : 0; tick.loop_len = looping ? p.loop_out - p.loop_in : 0;
    tick.bank = !play || m <= kOne ? 0u : 3 * m <= 4 * kOne ? 1u : m <= 2 * kOne ? 2u : 3u;
    tick.flags = (play ? MX_DECK_TICK_PLAY : 0u) | (looping ? MX_DECK_TICK_LOOPING : 0u);
    if (play && !looping) {
        if (h.pos_q32 + (int64_t)(spt - 1) * m < -16 * kOne) tick.flags |= MX_DECK_TICK_BEFORE;
        if (h.pos_q32 - (int64_t)(spt - 1) * m >= ((int64_t)n_frames + 15) * kOne) tick.flags |= MX_DECK_TICK_PAST;
    }
    if (play) {
        h.pos_q32 = deck_u(h.pos_q32, h.step_q32, dstep, spt);
        if (looping) h.pos_q32 = deck_fold(h.pos_q32, p.loop_in * kOne, (p.loop_out - p.loop_in) * kOne);
        h.step_q32 += (int64_t)spt * dstep;
    }
    h.last_looping = looping ? 1u : 0u; h.last_loop_in = looping ? p.loop_in : 0; h.last_loop_out = looping ? p.loop_out : 0; h._pad = 0;
    out = h;
}

int64_t deck_step(uint32_t track_rate, uint32_t graph_rate, double speed) {
    if (!track_rate || !graph_rate) throw Error(MX_ERR_INVALID, "deck: a rate of 0");
    if (!std::isfinite(speed)) throw Error(MX_ERR_INVALID, "deck: speed is not finite");
    const char* const too_fast = "deck: the step is above 4 * 2^32 in magnitude";
    if (std::fabs(speed) * (double)track_rate / (double)graph_rate > 5.0) throw Error(MX_ERR_INVALID, too_fast);
    // exactly: |speed| = M 2^e (M < 2^53), the step = M track_rate 2^(32 + e) / graph_rate rounded to nearest, ties to even
    int e = 0;
    const double fr = std::frexp(std::fabs(speed), &e);
    unsigned __int128 num = (unsigned __int128)(uint64_t)std::ldexp(fr, 53) * track_rate, den = graph_rate;
    const int sh = 32 + e - 53;
    if (sh >= 0) num <<= sh;                 // (sh <= 15 here: |speed| <= 5 * 2^32)
    else if (-sh > 90) return 0;             // below 2^-6 of a unit
    else den <<= -sh;
    unsigned __int128 q = num / den; const unsigned __int128 r = num % den;
    if (2 * r > den || (2 * r == den && (q & 1))) ++q;
    if (q > (unsigned __int128)kMaxStep) throw Error(MX_ERR_INVALID, too_fast);
    return speed < 0 ? -(int64_t)q : (int64_t)q;
}

// ---- tables (the header's TABLES), evaluated in long double so that the one rounding to f32 is the nearest f32 of the exact value ----
static long double bessel_i0(long double x) {
    long double term = 1.0L, sum = 1.0L;
    const long double q = x * x / 4.0L;
    for (int k = 1; k < 200; ++k) { term *= q / ((long double)k * k); sum += term; if (term < sum * 1e-25L) break; }
    return sum;
}
const float* deck_tables_host() {
    static std::vector<float> tab;
    static std::once_flag once;
    std::call_once(once, [] {
        tab.assign((size_t)MX_DECK_BANKS * DECK_BANK_FLOATS, 0.0f);
        const long double pi = 3.14159265358979323846264338327950288L, i0_9 = bessel_i0(9.0L);
        for (int b = 0; b < MX_DECK_BANKS; ++b) {
            const int fc4 = 4 - b;   // fc = fc4 / 4
            for (int p = 0; p <= MX_DECK_PHASES; ++p) {
                long double g[MX_DECK_TAPS], sum = 0.0L;
                for (int k = 0; k < MX_DECK_TAPS; ++k) {
                    const int x256 = (k - 15) * 256 - p;             // x = x256 / 256, fc x = N / 1024
                    const int N = fc4 * x256;
                    long double sinc = 1.0L;
                    if (N != 0) {
                        // sin(pi N / 1024) with the argument reduced exactly: N = 1024 h + r, |r| <= 512
                        int h = (N >= 0 ? N + 512 : N - 511) / 1024; int r = N - 1024 * h;
                        const long double s = r == 0 ? 0.0L : sinl(pi * (long double)r / 1024.0L);
                        sinc = ((h & 1) ? -s : s) / (pi * (long double)N / 1024.0L);
                    }
                    const long double xr = (long double)x256 / 4096.0L;   // x / 16
                    const long double in = 1.0L - xr * xr;
                    g[k] = ((long double)fc4 / 4.0L) * sinc * bessel_i0(9.0L * sqrtl(in > 0.0L ? in : 0.0L)) / i0_9;
                    sum += g[k];
                }
                for (int k = 0; k < MX_DECK_TAPS; ++k) tab[(size_t)b * DECK_BANK_FLOATS + (size_t)p * MX_DECK_TAPS + k] = (float)(g[k] / sum);
            }
        }
    });
    return tab.data();
}

// the tables on a device, uploaded on first use and kept for the life of the process
static const float* deck_tables_device(int device) {
    static std::mutex mu;
    static std::vector<std::pair<int, float*>> have;
    std::lock_guard<std::mutex> lock(mu);
    for (auto& h : have) if (h.first == device) return h.second;
    float* p = nullptr;
    const size_t bytes = (size_t)MX_DECK_BANKS * DECK_BANK_FLOATS * sizeof(float);
    hip_check(hipMalloc((void**)&p, bytes), "hipMalloc(deck tables)");
    hip_check(hipMemcpy(p, deck_tables_host(), bytes, hipMemcpyHostToDevice), "hipMemcpy(deck tables)");
    have.push_back({device, p});
    return p;
}

// ---- the deck ----
Deck::Deck(uint64_t n_frames, int device) : n_frames_(n_frames), device_(device) {
    if (n_frames < 1 || n_frames > kMaxFrames) throw Error(MX_ERR_INVALID, "deck: n_frames outside 1 .. 2^30");
    if (device_ < 0) hip_check(hipGetDevice(&device_), "hipGetDevice");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    track_.alloc(n_frames * 4);
    hip_check(hipStreamCreateWithFlags(&load_stream_, hipStreamNonBlocking), "hipStreamCreate(deck)");
    hip_check(hipEventCreateWithFlags(&loaded_, hipEventDisableTiming), "hipEventCreate");
    hip_check(hipMemsetAsync(track_.p, 0, n_frames * 4, load_stream_), "hipMemsetAsync(deck track)");
    hip_check(hipStreamSynchronize(load_stream_), "hipStreamSynchronize");
}

Deck::~Deck() {
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();   // a feed in flight may still read the track
    if (loaded_) (void)hipEventDestroy(loaded_);
    if (load_stream_) (void)hipStreamDestroy(load_stream_);
}

void Deck::load_i16(uint64_t first, const int16_t* interleaved, uint64_t n) {
    if (first > n_frames_ || n > n_frames_ - first) throw Error(MX_ERR_INVALID, "deck: the loaded range lies outside the track");
    if (!n) return;
    if (!interleaved) throw Error(MX_ERR_INVALID, "deck: interleaved is NULL");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipMemcpyAsync((char*)track_.p + first * 4, interleaved, n * 4, hipMemcpyHostToDevice, load_stream_), "hipMemcpyAsync(deck load)");
    hip_check(hipEventRecord(loaded_, load_stream_), "hipEventRecord");
    load_pending_ = true;
    hip_check(hipStreamSynchronize(load_stream_), "hipStreamSynchronize");   // the host buffer is the caller's again
}

void Deck::schedule(uint32_t tick, const mx_deck_params* params, const int64_t* seek) {
    if (params) deck_check(*params, n_frames_);
    if (!params && !seek) return;
    auto it = std::find_if(sched_.begin(), sched_.end(), [&](const Event& e) { return e.tick == tick; });
    if (it == sched_.end()) { sched_.push_back(Event{tick, false, false, mx_deck_params{}, 0}); it = sched_.end() - 1; }
    if (params) { it->has_params = true; it->params = *params; }
    if (seek) { it->has_seek = true; it->seek = *seek; }
}

void Deck::read_ticks(uint32_t first, uint32_t n, mx_deck_tick* dst) const {
    if (first > ticks_.size() || n > ticks_.size() - first) throw Error(MX_ERR_INVALID, "deck: a window beyond the last feed");
    if (n && !dst) throw Error(MX_ERR_INVALID, "deck: dst is NULL");
    if (n) std::memcpy(dst, ticks_.data() + first, (size_t)n * sizeof(mx_deck_tick));
}

// ---- the feed ----
// The descriptor block of a feed -- DeckDev[n] then DeckTickDev[n x n_ticks] -- is written into one of kSlots page-locked buffers, copied by a kernel into that slot's
// device buffer and read there by the feed kernel; the event recorded behind the feed kernel says when both are free again.  A slot is taken round-robin, so the host
// waits only when kSlots feeds are in flight at once (and then for the oldest): a steady tick-by-tick host never does.
namespace {
struct Slot { void* host = nullptr; size_t host_cap = 0; DevBuf dev; hipEvent_t done = nullptr; bool pending = false; int device = -1; hipStream_t stream = nullptr; };
constexpr int kSlots = 4;
struct FeedState {
    std::mutex mu;
    Slot slots[kSlots]; int next = 0;
    std::vector<DeckTickDev> last; uint32_t last_spt = 0;   // the last feed's ticks, for mx_deck_debug_last_feed
    struct KlTick { KlTickDev t; uint32_t log_hop, overlap; };
    std::vector<KlTick> last_kl; uint32_t kl_searched = 0, kl_unsearched = 0;   // ... and its key-locked ticks and grains, for mx_deck_debug_last_keylock
} feed_state;
}  // namespace

// A slot's event remembers the stream it was last recorded on, and the runtime looks at that stream when the event is waited for or recorded again: an event must
// not outlive it.  The graph whose stream goes away says so here (the stream still there, its work done): the slots it was the last to use give up their events.
void deck_stream_retired(hipStream_t s) {
    std::lock_guard<std::mutex> lock(feed_state.mu);
    for (Slot& sl : feed_state.slots) {
        if (!sl.done || sl.stream != s) continue;
        (void)hipSetDevice(sl.device);
        if (sl.pending) (void)hipEventSynchronize(sl.done);
        (void)hipEventDestroy(sl.done);
        sl.done = nullptr; sl.pending = false; sl.stream = nullptr;
    }
}

void Deck::feed(Deck* const* decks, const uint32_t* nodes, size_t n, Graph& g, uint32_t n_ticks) {
    auto drop = [&] { for (size_t i = 0; i < n; ++i) if (decks && decks[i]) decks[i]->sched_.clear(); };
    try {
        if (!n) return;
        if (!decks || !nodes) throw Error(MX_ERR_INVALID, "deck feed: decks / nodes is NULL");
        if (n > 0xffffffu) throw Error(MX_ERR_INVALID, "deck feed: more than 2^24 decks");
        if (!n_ticks) throw Error(MX_ERR_INVALID, "deck feed: n_ticks is 0");
        const size_t spt = g.spt();
        if (spt < 1 || spt > MX_DECK_MAX_SPT) throw Error(MX_ERR_INVALID, "deck feed: the graph's frames per tick are outside 1 .. MX_DECK_MAX_SPT");
        for (size_t i = 0; i < n; ++i) if (!decks[i]) throw Error(MX_ERR_INVALID, "deck feed: a deck is NULL");
        std::vector<float*> outs(n);
        for (size_t i = 0; i < n; ++i) {
            if (decks[i]->device_ != g.device()) throw Error(MX_ERR_INVALID, "deck feed: deck " + std::to_string(i) + " lives on another device than the graph");
            outs[i] = g.source_feed_ptr(nodes[i], (size_t)n_ticks * spt);
            for (const Event& e : decks[i]->sched_)
                if (e.tick >= n_ticks) throw Error(MX_ERR_INVALID, "deck feed: deck " + std::to_string(i) + " has an event scheduled at tick " + std::to_string(e.tick) + ", beyond this feed");
        }
        {
            std::vector<const Deck*> d(decks, decks + n); std::vector<uint32_t> nd(nodes, nodes + n);
            std::sort(d.begin(), d.end()); std::sort(nd.begin(), nd.end());
            if (std::adjacent_find(d.begin(), d.end()) != d.end()) throw Error(MX_ERR_INVALID, "deck feed: a deck is named twice");
            if (std::adjacent_find(nd.begin(), nd.end()) != nd.end()) throw Error(MX_ERR_INVALID, "deck feed: a node is named twice");
        }
        hip_check(hipSetDevice(g.device()), "hipSetDevice");
        const float* tables = deck_tables_device(g.device());

        std::lock_guard<std::mutex> lock(feed_state.mu);
        Slot& sl = feed_state.slots[feed_state.next];
        feed_state.next = (feed_state.next + 1) % kSlots;
        if (sl.pending) { hip_check(hipSetDevice(sl.device), "hipSetDevice"); hip_check(hipEventSynchronize(sl.done), "hipEventSynchronize"); sl.pending = false; hip_check(hipSetDevice(g.device()), "hipSetDevice"); }
        size_t nk = 0, grain_cap = 0;   // key-locked decks, and room for their grain starts: ceil(spt / hop) a tick at the most
        for (size_t i = 0; i < n; ++i)
            if (decks[i]->kl_on_) { ++nk; grain_cap += (size_t)n_ticks * (spt / decks[i]->kl_.hop + 1); }
        const size_t head_bytes = (n * sizeof(DeckDev) + 15) & ~(size_t)15, plain_bytes = (head_bytes + n * (size_t)n_ticks * sizeof(DeckTickDev) + 15) & ~(size_t)15;
        const size_t bytes = nk ? plain_bytes + nk * sizeof(KlDeckDev) + nk * (size_t)n_ticks * sizeof(KlTickDev) + grain_cap * sizeof(KlGrainIn)
                                : head_bytes + n * (size_t)n_ticks * sizeof(DeckTickDev);
        if (sl.host_cap < bytes) {
            if (sl.host) (void)hipHostFree(sl.host);
            sl.host = nullptr; sl.host_cap = 0;
            hip_check(hipHostMalloc(&sl.host, bytes, hipHostMallocDefault), "hipHostMalloc(deck staging)");
            sl.host_cap = bytes;
        }
        if (sl.dev.bytes < bytes || sl.device != g.device()) {
            if (sl.done) { (void)hipEventDestroy(sl.done); sl.done = nullptr; }
            sl.dev.free_(); sl.dev.alloc(bytes); sl.device = g.device();
        }
        if (!sl.done) hip_check(hipEventCreateWithFlags(&sl.done, hipEventDisableTiming), "hipEventCreate");

        // plain decks take the first n_plain entries of DeckDev / DeckTickDev, in the order given; key-locked decks have descriptors of their own behind them
        DeckDev* dd = (DeckDev*)sl.host;
        DeckTickDev* td = (DeckTickDev*)((char*)sl.host + head_bytes);
        KlDeckDev* kd = (KlDeckDev*)((char*)sl.host + plain_bytes);
        KlTickDev* kt = (KlTickDev*)(kd + nk);
        KlGrainIn* kg = (KlGrainIn*)(kt + nk * (size_t)n_ticks);
        std::vector<mx_deck_head> heads(n);
        std::vector<std::vector<mx_deck_tick>> recs(n);
        std::vector<std::vector<mx_deck_grain>> grains(nk);
        std::vector<uint64_t> clocks(nk);
        bool phase_varies = false;
        size_t ip = 0, ik = 0, grain_at = 0;
        for (size_t i = 0; i < n; ++i) {
            Deck& d = *decks[i];
            const bool kl = d.kl_on_;
            if (!kl) dd[ip] = DeckDev{(const uint32_t*)d.track_.p, outs[i], (int64_t)d.n_frames_};
            mx_deck_head h = d.head_;
            recs[i].resize(n_ticks);
            std::vector<const Event*> at(d.sched_.empty() ? 0 : n_ticks, nullptr);
            for (const Event& e : d.sched_) at[e.tick] = &e;
            uint64_t clock = kl && d.last_lineage_ == g.lineage() ? d.kl_t_ : 0;   // (another graph restarts the grain clock; one that adopted the last one's state is not another)
            const uint32_t hop = d.kl_.hop;
            uint32_t next = 2;                                           // rec[] index of the next grain to start
            for (uint32_t t = 0; t < n_ticks; ++t) {
                const Event* e = at.empty() ? nullptr : at[t];
                mx_deck_tick& r = recs[i][t];
                deck_plan(h, e && e->has_params ? &e->params : nullptr, e && e->has_seek ? &e->seek : nullptr, (uint32_t)spt, d.n_frames_, r, h);
                if (!kl) {
                    const bool zero = !(r.flags & MX_DECK_TICK_PLAY) || (r.flags & (MX_DECK_TICK_BEFORE | MX_DECK_TICK_PAST));
                    td[ip * (size_t)n_ticks + t] = DeckTickDev{r.pos_q32, r.step_q32, r.dstep_q32, (uint32_t)r.loop_in, (uint32_t)r.loop_len,
                                                              zero ? (uint32_t)DECK_FORM_ZERO : (uint32_t)DECK_FORM_PLAY, r.bank};
                    if (!zero && deck_phase_varies(td[ip * (size_t)n_ticks + t])) phase_varies = true;
                    continue;
                }
                KlTickDev& k = kt[ik * (size_t)n_ticks + t];
                if (!(r.flags & MX_DECK_TICK_PLAY)) { k = KlTickDev{0, 0, 0, 0}; clock = 0; continue; }   // (a tick that is not playing restarts the grain clock)
                const uint32_t m0 = (uint32_t)(clock & (hop - 1));
                k = KlTickDev{m0, m0 ? next - 1 : next, (clock >> d.kl_log_hop_) == 0 ? 1u : 0u, 1u};
                for (uint64_t fr = (hop - m0) & (hop - 1); fr < spt; fr += hop) {   // the grain starts of this tick
                    int64_t a = deck_u(r.pos_q32, r.step_q32, r.dstep_q32, (int64_t)fr);
                    if (r.flags & MX_DECK_TICK_LOOPING) a = deck_fold(a, r.loop_in * kOne, r.loop_len * kOne);
                    const bool first = clock + fr == 0;
                    grains[ik].push_back(mx_deck_grain{a, 0, t, (uint32_t)fr, 0, 0u, first ? (uint32_t)MX_DECK_GRAIN_FIRST : 0u, 0u});
                    kg[grain_at + grains[ik].size() - 1] = KlGrainIn{a, first ? 1u : 0u, 0u};
                    ++next;
                }
                clock += spt;
            }
            heads[i] = h;
            if (kl) {
                kd[ik] = KlDeckDev{(const uint32_t*)d.track_.p, outs[i], (int64_t)d.n_frames_, d.kl_.pitch_q32, nullptr, (int64_t*)d.kl_state_.p,
                                   (const KlGrainIn*)((const char*)sl.dev.p + ((const char*)(kg + grain_at) - (const char*)sl.host)),
                                   (uint32_t)grains[ik].size(), d.kl_log_hop_, d.kl_.overlap, d.kl_.radius, d.kl_bank_, 0u};
                clocks[ik] = clock;
                grain_at += grains[ik].size();
                ++ik;
            } else ++ip;
        }
        // the last things that can fail: room for the grain records of each key-locked deck.  A deck that changes graphs waits for the device once -- its state and
        // record buffers may still be in use on the other graph's stream.
        for (size_t i = 0, k = 0; i < n; ++i) {
            Deck& d = *decks[i];
            if (!d.kl_on_) continue;
            if (d.last_graph_ && d.last_graph_ != &g) hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
            const size_t need = (2 + grains[k].size()) * sizeof(KlRec);
            if (d.kl_rec_.bytes < need) {
                d.fetch_grains();            // the last feed's records, before their buffer goes
                d.kl_rec_.free_(); d.kl_rec_.alloc(2 * need);
            }
            kd[k++].rec = (KlRec*)d.kl_rec_.p;
        }
        for (size_t i = 0; i < n; ++i)
            if (decks[i]->load_pending_) { hip_check(hipStreamWaitEvent(g.stream(), decks[i]->loaded_, 0), "hipStreamWaitEvent"); decks[i]->load_pending_ = false; }
        launch_upload(sl.dev.p, sl.host, nk ? (size_t)((const char*)(kg + grain_at) - (const char*)sl.host) : bytes, g.stream());
        launch_deck_feed((const DeckDev*)sl.dev.p, (const DeckTickDev*)((const char*)sl.dev.p + head_bytes), tables, (uint32_t)ip, n_ticks, (uint32_t)spt, phase_varies, g.stream());
        launch_deck_keylock((const KlDeckDev*)((const char*)sl.dev.p + plain_bytes), (const KlTickDev*)((const char*)sl.dev.p + plain_bytes + nk * sizeof(KlDeckDev)), tables,
                            (uint32_t)nk, n_ticks, (uint32_t)spt, g.stream());
        hip_check(hipGetLastError(), "deck feed launch");
        hip_check(hipEventRecord(sl.done, g.stream()), "hipEventRecord");
        sl.pending = true; sl.stream = g.stream();
        feed_state.last.assign(td, td + ip * (size_t)n_ticks); feed_state.last_spt = (uint32_t)spt;
        feed_state.last_kl.clear(); feed_state.kl_searched = feed_state.kl_unsearched = 0;
        for (size_t i = 0, k = 0; i < n; ++i) {
            Deck& d = *decks[i];
            d.head_ = heads[i]; d.ticks_ = std::move(recs[i]); d.sched_.clear(); d.last_graph_ = &g; d.last_lineage_ = g.lineage();
            if (!d.kl_on_) { d.grains_.clear(); d.grains_fetched_ = true; continue; }
            for (const mx_deck_grain& gr : grains[k]) ++((gr.flags & MX_DECK_GRAIN_FIRST) || !d.kl_.radius ? feed_state.kl_unsearched : feed_state.kl_searched);
            for (uint32_t t = 0; t < n_ticks; ++t) feed_state.last_kl.push_back(FeedState::KlTick{kt[k * (size_t)n_ticks + t], d.kl_log_hop_, d.kl_.overlap});
            d.kl_t_ = clocks[k]; d.grains_ = std::move(grains[k]); d.grains_fetched_ = d.grains_.empty();
            ++k;
        }
    } catch (...) { drop(); throw; }
}

// ---- key-lock ----
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
    if (n_frames < 1 || n_frames > kMaxFrames) throw Error(MX_ERR_INVALID, "deck key-lock search: n_frames outside 1 .. 2^30");
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
    if (k) {
        deck_keylock_check(*k);
        if (!kl_state_.p) { hip_check(hipSetDevice(device_), "hipSetDevice"); kl_state_.alloc(2 * sizeof(int64_t)); }
        kl_ = *k;
        kl_bank_ = k->pitch_q32 <= kOne ? 0u : 3 * k->pitch_q32 <= 4 * kOne ? 1u : k->pitch_q32 <= 2 * kOne ? 2u : 3u;
        kl_log_hop_ = 0;
        while ((1u << kl_log_hop_) < k->hop) ++kl_log_hop_;
    }
    kl_on_ = k != nullptr;
    kl_t_ = 0;
}

void Deck::fetch_grains() {
    if (grains_fetched_) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
    std::vector<KlRec> r(grains_.size());
    hip_check(hipMemcpy(r.data(), (const KlRec*)kl_rec_.p + 2, r.size() * sizeof(KlRec), hipMemcpyDeviceToHost), "hipMemcpy(deck grains)");
    for (size_t k = 0; k < r.size(); ++k) { grains_[k].g_q32 = r[k].g; grains_[k].delta = r[k].delta; grains_[k].dist = r[k].dist; }
    grains_fetched_ = true;
}

void Deck::read_grains(uint32_t first, uint32_t n, mx_deck_grain* dst) {
    if (first > grains_.size() || n > grains_.size() - first) throw Error(MX_ERR_INVALID, "deck: a window beyond the last feed's grains");
    if (n && !dst) throw Error(MX_ERR_INVALID, "deck: dst is NULL");
    if (!n) return;
    fetch_grains();
    std::memcpy(dst, grains_.data() + first, (size_t)n * sizeof(mx_deck_grain));
}

void Deck::debug_last_keylock(uint32_t out[4]) {
    std::lock_guard<std::mutex> lock(feed_state.mu);
    out[0] = feed_state.kl_searched; out[1] = feed_state.kl_unsearched; out[2] = out[3] = 0;
    const uint32_t spt = feed_state.last_spt;
    for (const FeedState::KlTick& k : feed_state.last_kl) {
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

// ---- analysis (the header's ANALYSIS) ----
void deck_analysis_check(const mx_deck_analysis& a) {
    if (a.column < 64 || a.column > 4096 || (a.column & (a.column - 1))) throw Error(MX_ERR_INVALID, "deck analysis: column is not a power of two in 64 .. 4096");
    if (!(a.taps & 1u) || a.taps > 127) throw Error(MX_ERR_INVALID, "deck analysis: taps is not odd in 1 .. 127");
    if (a.max_lag < 16 || a.max_lag > 1024) throw Error(MX_ERR_INVALID, "deck analysis: max_lag outside 16 .. 1024");
    if (a._pad) throw Error(MX_ERR_INVALID, "deck analysis: _pad must be 0");
    for (const int16_t* t : {a.lo, a.hi}) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < 127; ++k) {
            if (k >= a.taps && t[k]) throw Error(MX_ERR_INVALID, std::string("deck analysis: ") + (t == a.lo ? "lo" : "hi") + " has a non-zero entry at index taps or above");
            sum += (uint32_t)(t[k] < 0 ? -(int32_t)t[k] : (int32_t)t[k]);
        }
        if (sum > 32767) throw Error(MX_ERR_INVALID, std::string("deck analysis: the sum of |") + (t == a.lo ? "lo" : "hi") + "[k]| is above 32767");
    }
}

uint64_t deck_column_count(uint64_t n_frames, uint32_t column) {
    if (n_frames < 1 || n_frames > kMaxFrames) throw Error(MX_ERR_INVALID, "deck analysis: n_frames outside 1 .. 2^30");
    if (column < 64 || column > 4096 || (column & (column - 1))) throw Error(MX_ERR_INVALID, "deck analysis: column is not a power of two in 64 .. 4096");
    return (n_frames + column - 1) / column;
}

void deck_analysis_bands(double rate, double f_lo, double f_hi, uint32_t taps, mx_deck_analysis& a) {
    if (!(std::isfinite(rate) && rate > 0.0)) throw Error(MX_ERR_INVALID, "deck analysis bands: rate is not finite and positive");
    if (!(f_lo > 0.0 && f_lo < f_hi && f_hi < rate / 2.0)) throw Error(MX_ERR_INVALID, "deck analysis bands: the cutoffs are not 0 < f_lo < f_hi < rate / 2");
    if (!(taps & 1u) || taps > 127) throw Error(MX_ERR_INVALID, "deck analysis bands: taps is not odd in 1 .. 127");
    const double pi = 3.14159265358979323846;
    const int K = (int)taps, D = (K - 1) / 2;
    mx_deck_analysis out = a;
    out.taps = taps;
    const double cut[2] = {f_lo, f_hi};
    int16_t* const tab[2] = {out.lo, out.hi};
    for (int b = 0; b < 2; ++b) {
        const double fc = 2.0 * cut[b] / rate;
        double g[127], sum = 0.0;
        for (int k = 0; k <= D; ++k) {   // the first half and the centre; the rest mirrors them
            const double x = fc * (double)(k - D), w = 0.5 - 0.5 * std::cos(2.0 * pi * (double)(k + 1) / (double)(K + 1));
            g[k] = g[K - 1 - k] = fc * (x == 0.0 ? 1.0 : std::sin(pi * x) / (pi * x)) * w;
        }
        for (int k = 0; k < K; ++k) sum += g[k];
        long total = 0, c[127];
        for (int k = 0; k < K; ++k) { c[k] = std::lround(16384.0 * g[k] / sum); total += c[k]; }
        c[D] += 16384 - total;
        long mag = 0;
        for (int k = 0; k < K; ++k) mag += c[k] < 0 ? -c[k] : c[k];
        if (mag > 32767) throw Error(MX_ERR_INVALID, "deck analysis bands: the sum of |c| is above 32767 at these cutoffs");
        for (int k = 0; k < 127; ++k) tab[b][k] = k < K ? (int16_t)c[k] : (int16_t)0;
    }
    a = out;
}

void deck_columns_host(const int16_t* x, uint64_t n_frames, const mx_deck_analysis& a, uint64_t first, uint64_t n, mx_deck_column* cols, uint64_t* R) {
    if (!x) throw Error(MX_ERR_INVALID, "deck columns: interleaved is NULL");
    deck_analysis_check(a);
    const uint64_t N = deck_column_count(n_frames, a.column);
    if (first > N || n > N - first) throw Error(MX_ERR_INVALID, "deck columns: a window beyond the track's columns");
    if (n && !cols) throw Error(MX_ERR_INVALID, "deck columns: cols is NULL");
    if (R && (first != 0 || n != N)) throw Error(MX_ERR_INVALID, "deck columns: the autocorrelation needs all the columns, first = 0 and n = N");
    const uint32_t C = a.column, K = a.taps, D = (K - 1) / 2;
    auto s = [&](int64_t f) -> int32_t { return f < 0 || f >= (int64_t)n_frames ? 0 : (int32_t)x[2 * f] + (int32_t)x[2 * f + 1]; };
    std::vector<int32_t> w((size_t)C + K - 1);
    uint32_t before = 0;   // A[first - 1]
    if (first) {
        uint64_t e = 0;
        for (uint64_t f = (first - 1) * C; f < first * C; ++f) { const int64_t v = s((int64_t)f); e += (uint64_t)(v * v); }
        before = tempo_root(e);
    }
    for (uint64_t c = first; c < first + n; ++c) {
        const uint64_t f0 = c * C;
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(C, n_frames - f0);
        for (uint32_t i = 0; i < cnt + K - 1; ++i) w[i] = s((int64_t)f0 - (int64_t)D + (int64_t)i);
        mx_deck_column r{INT32_MAX, INT32_MIN, {0u, 0u, 0u}, 0u, {0u, 0u, 0u}, 0u};
        for (uint32_t i = 0; i < cnt; ++i) {
            int32_t a1 = 0, a2 = 0;   // exact: |a| <= 65536 * 32767
            for (uint32_t k = 0; k < K; ++k) { a1 += (int32_t)a.lo[k] * w[i + k]; a2 += (int32_t)a.hi[k] * w[i + k]; }
            const int32_t sv = w[i + D], low = a1 >> 14, b = a2 >> 14, band[3] = {low, b - low, sv - b};
            r.smin = std::min(r.smin, sv); r.smax = std::max(r.smax, sv);
            for (int j = 0; j < 3; ++j) {
                const uint64_t m = (uint64_t)(band[j] < 0 ? -(int64_t)band[j] : (int64_t)band[j]);
                r.peak[j] = std::max(r.peak[j], (uint32_t)m);
                r.energy[j] += m * m;
            }
            r.e += (uint64_t)((int64_t)sv * sv);
        }
        const uint32_t A = tempo_root(r.e);
        r.onset = (A > before ? A - before : 0u) >> 6;
        before = A;
        cols[c - first] = r;
    }
    if (R)
        for (uint64_t l = 0; l < a.max_lag; ++l) {
            uint64_t acc = 0;
            for (uint64_t c = 0; c + l < N; ++c) acc += (uint64_t)cols[c].onset * cols[c + l].onset;
            R[l] = acc;
        }
}

// (the library is built with -ffp-contract=off: the multiply and the add of i_k are two roundings, as the header says)
void deck_beatgrid(const mx_deck_column* cols, uint64_t n_cols, const uint64_t* R, uint32_t max_lag, uint32_t column, double rate, double bpm_lo, double bpm_hi, mx_deck_grid& out) {
    if (!R || (n_cols && !cols)) throw Error(MX_ERR_INVALID, "deck beat grid: NULL argument");
    if (column < 64 || column > 4096 || (column & (column - 1)) || max_lag < 16 || max_lag > 1024)
        throw Error(MX_ERR_INVALID, "deck beat grid: column is not a power of two in 64 .. 4096, or max_lag is outside 16 .. 1024");
    if (!(std::isfinite(rate) && rate > 0.0 && std::isfinite(bpm_lo) && bpm_lo > 0.0 && std::isfinite(bpm_hi) && bpm_hi >= bpm_lo))
        throw Error(MX_ERR_INVALID, "deck beat grid: rate, bpm_lo and bpm_hi must be finite and positive, bpm_lo <= bpm_hi");
    out = mx_deck_grid{0.0, 0.0, 0.0, 0u, 0u, 0u};
    uint32_t best = 0; double d = 0.0;
    if (!tempo_lag([&](uint32_t l) { return (double)R[l]; }, max_lag, column, rate, bpm_lo, bpm_hi, best, d)) return;
    const double P = (double)best + d;
    if (!(P >= 1.0 && P <= (double)max_lag)) return;
    const uint32_t phases = (uint32_t)std::ceil(P);
    uint64_t best_sum = 0; uint32_t phi_best = 0;
    for (uint32_t phi = 0; phi < phases; ++phi) {
        uint64_t sum = 0;
        for (uint64_t k = 0;; ++k) {
            const double step = (double)k * P;
            const double at = (double)phi + step;
            const int64_t i = (int64_t)std::floor(at);
            if (i >= (int64_t)n_cols) break;
            sum += cols[i].onset;
        }
        if (phi == 0 || sum > best_sum) { best_sum = sum; phi_best = phi; }
    }
    out.bpm = 60.0 * rate / ((double)column * P); out.period_columns = P; out.confidence = (double)R[best] / (double)R[0];
    out.first_beat_frame = (uint64_t)phi_best * column; out.lag = best; out.phase_column = phi_best;
}

namespace {
std::mutex analysis_mu;
uint32_t last_analysis[4] = {0u, 0u, 0u, 0u};   // mx_deck_debug_last_analysis
}  // namespace

void Deck::analyse(const mx_deck_analysis* a) {
    if (a) deck_analysis_check(*a);
    hip_check(hipSetDevice(device_), "hipSetDevice");
    const uint64_t N = a ? deck_column_count(n_frames_, a->column) : 0;
    const size_t need = a ? (size_t)N * sizeof(mx_deck_column) + (size_t)a->max_lag * sizeof(uint64_t) + (size_t)N * sizeof(uint32_t) : 0;
    if (!a || an_.bytes < need) {
        hip_check(hipStreamSynchronize(load_stream_), "hipStreamSynchronize");   // an analysis in flight still writes the buffer that goes
        an_cols_ = 0; an_lag_ = 0;
        an_.free_();
        if (!a) return;
        an_.alloc(need);   // (MX_ERR_NOMEM leaves the deck without an analysis)
    }
    an_cols_ = 0; an_lag_ = 0;
    DeckAnalyseTaps taps{};
    for (uint32_t k = 0; k < a->taps; ++k) { taps.lo[k] = a->lo[k]; taps.hi[k] = a->hi[k]; }
    uint64_t* const R = (uint64_t*)((char*)an_.p + (size_t)N * sizeof(mx_deck_column));
    uint32_t forms[4];
    launch_deck_analyse((const uint32_t*)track_.p, n_frames_, a->column, a->taps, a->max_lag, taps, an_.p, (uint32_t*)(R + a->max_lag), R, N, forms, load_stream_);
    hip_check(hipGetLastError(), "deck analyse launch");
    an_cols_ = N; an_lag_ = a->max_lag;
    std::lock_guard<std::mutex> lock(analysis_mu);
    std::memcpy(last_analysis, forms, sizeof forms);
}

void Deck::read_columns(uint64_t first, uint64_t n, mx_deck_column* dst) {
    if (!an_cols_) throw Error(MX_ERR_INVALID, "deck: no analysis");
    if (first > an_cols_ || n > an_cols_ - first) throw Error(MX_ERR_INVALID, "deck: a window beyond the analysis' columns");
    if (n && !dst) throw Error(MX_ERR_INVALID, "deck: dst is NULL");
    if (!n) return;
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(load_stream_), "hipStreamSynchronize");
    hip_check(hipMemcpy(dst, (const mx_deck_column*)an_.p + first, (size_t)n * sizeof(mx_deck_column), hipMemcpyDeviceToHost), "hipMemcpy(deck columns)");
}

void Deck::read_autocorr(uint64_t* R, uint32_t cap) {
    if (!an_cols_) throw Error(MX_ERR_INVALID, "deck: no analysis");
    if (cap < an_lag_) throw Error(MX_ERR_INVALID, "deck: cap is below the analysis' max_lag");
    if (!R) throw Error(MX_ERR_INVALID, "deck: R is NULL");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    hip_check(hipStreamSynchronize(load_stream_), "hipStreamSynchronize");
    hip_check(hipMemcpy(R, (const char*)an_.p + (size_t)an_cols_ * sizeof(mx_deck_column), (size_t)an_lag_ * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(deck autocorrelation)");
}

void Deck::debug_last_analysis(uint32_t out[4]) {
    std::lock_guard<std::mutex> lock(analysis_mu);
    std::memcpy(out, last_analysis, sizeof last_analysis);
}

void Deck::debug_last_feed(uint32_t out[6]) {
    std::lock_guard<std::mutex> lock(feed_state.mu);
    for (int k = 0; k < 6; ++k) out[k] = 0;
    const uint32_t spt = feed_state.last_spt, chunks = (spt + MX_DECK_CHUNK - 1) / MX_DECK_CHUNK;
    for (const DeckTickDev& t : feed_state.last) {
        if (t.form == DECK_FORM_ZERO) { ++out[0]; out[3] += chunks; continue; }
        uint32_t gathered = 0;
        for (uint32_t c = 0; c < chunks; ++c)
            if (!deck_chunk_plan(t, c * MX_DECK_CHUNK, std::min<uint32_t>(MX_DECK_CHUNK, spt - c * MX_DECK_CHUNK)).stream) ++gathered;
        ++out[gathered ? 2 : 1]; out[4] += chunks - gathered; out[5] += gathered;
    }
}

}  // namespace mx
