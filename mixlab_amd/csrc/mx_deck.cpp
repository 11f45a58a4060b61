// mx_deck.cpp -- the deck's host side: parameter rules, the per-tick state machine (mx_deck_plan), the coefficient tables, the track, and the feed that turns the
// coming ticks of many decks into one descriptor block and one launch (include/mixlab_gpu.h "the deck").  Key-lock beside the feed is
// mx_deck_keylock.cpp's, the echo behind it mx_deck_echo.cpp's (the feed asks each deck's DeckEcho for its ticks, uploads them with its own, launches, commits),
// the sweep filter between the two mx_deck_filter.cpp's (DeckFilter, the same protocol), the reverb behind the echo mx_deck_reverb.cpp's (DeckReverb), and each whole-track analysis has a file of its own (mx_deck_analysis.hpp).
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

void deck_check(const mx_deck_params& p, uint64_t n_frames) {
    if (n_frames < 1 || n_frames > kDeckMaxFrames) throw Error(MX_ERR_INVALID, "deck: n_frames outside 1 .. 2^30");
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
    else if (n_frames < 1 || n_frames > kDeckMaxFrames) throw Error(MX_ERR_INVALID, "deck: n_frames outside 1 .. 2^30");
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
    if (n_frames < 1 || n_frames > kDeckMaxFrames) throw Error(MX_ERR_INVALID, "deck: n_frames outside 1 .. 2^30");
    if (device_ < 0) hip_check(hipGetDevice(&device_), "hipGetDevice");
    hip_check(hipSetDevice(device_), "hipSetDevice");
    track_.alloc(n_frames * 4);
    hip_check(hipStreamCreateWithFlags(&load_stream_, hipStreamNonBlocking), "hipStreamCreate(deck)");
    hip_check(hipEventCreateWithFlags(&loaded_, hipEventDisableTiming), "hipEventCreate");
    hip_check(hipMemsetAsync(track_.p, 0, n_frames * 4, load_stream_), "hipMemsetAsync(deck track)");
    hip_check(hipStreamSynchronize(load_stream_), "hipStreamSynchronize");
    for_analyses_ = DeckTrack{(const uint32_t*)track_.p, n_frames_, device_, load_stream_};
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
    typedef DeckKlTick KlTick;
    std::vector<KlTick> last_kl; uint32_t kl_searched = 0, kl_unsearched = 0;   // ... and its key-locked ticks and grains, for mx_deck_debug_last_keylock
    std::vector<std::vector<uint32_t>> last_echo;                                // ... and per deck with an echo the delays of its ticks, for mx_deck_debug_last_echo
    DeckLastFilter last_filter;                                                  // ... and the filter's four counters, for mx_deck_debug_last_filter
    std::vector<std::vector<uint32_t>> last_reverb;                              // ... and per deck with a reverb the reaches of its ticks, for mx_deck_debug_last_reverb
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
    auto drop = [&] { for (size_t i = 0; i < n; ++i) if (decks && decks[i]) { decks[i]->sched_.clear(); decks[i]->echo.drop_schedule(); decks[i]->filter.drop_schedule(); decks[i]->reverb.drop_schedule(); } };
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
            uint32_t beyond = 0;
            if (decks[i]->echo.scheduled_beyond(n_ticks, beyond))
                throw Error(MX_ERR_INVALID, "deck feed: deck " + std::to_string(i) + " has an echo scheduled at tick " + std::to_string(beyond) + ", beyond this feed");
            if (decks[i]->filter.scheduled_beyond(n_ticks, beyond))
                throw Error(MX_ERR_INVALID, "deck feed: deck " + std::to_string(i) + " has a filter scheduled at tick " + std::to_string(beyond) + ", beyond this feed");
            if (decks[i]->reverb.scheduled_beyond(n_ticks, beyond))
                throw Error(MX_ERR_INVALID, "deck feed: deck " + std::to_string(i) + " has a reverb scheduled at tick " + std::to_string(beyond) + ", beyond this feed");
        }
        {
            std::vector<const Deck*> d(decks, decks + n); std::vector<uint32_t> nd(nodes, nodes + n);
            std::sort(d.begin(), d.end()); std::sort(nd.begin(), nd.end());
            if (std::adjacent_find(d.begin(), d.end()) != d.end()) throw Error(MX_ERR_INVALID, "deck feed: a deck is named twice");
            if (std::adjacent_find(nd.begin(), nd.end()) != nd.end()) throw Error(MX_ERR_INVALID, "deck feed: a node is named twice");
        }
        hip_check(hipSetDevice(g.device()), "hipSetDevice");
        const float* tables = deck_tables_device(g.device());
        // the echo of every deck over the coming ticks (host state only): echoes[] names the decks with an echo in any tick, those of the one-block form first
        struct EchoPlan { size_t deck; std::vector<EchoTickDev> ticks; std::vector<uint32_t> delays; bool one_block; };
        std::vector<EchoPlan> echoes;
        std::vector<DeckEcho::State> echo_after(n);
        for (size_t i = 0; i < n; ++i) {
            std::vector<EchoTickDev> et;
            if (!decks[i]->echo.plan(n_ticks, (uint32_t)spt, et, echo_after[i])) continue;
            std::vector<uint32_t> dl(n_ticks);
            for (uint32_t t = 0; t < n_ticks; ++t) dl[t] = echo_delay_of(et[t]);
            const bool one = deck_echo_one_block((uint32_t)spt, dl.data(), n_ticks);
            echoes.push_back(EchoPlan{i, std::move(et), std::move(dl), one});
        }
        std::stable_partition(echoes.begin(), echoes.end(), [](const EchoPlan& e) { return e.one_block; });
        const size_t ne = echoes.size(), ne_block = (size_t)std::count_if(echoes.begin(), echoes.end(), [](const EchoPlan& e) { return e.one_block; });
        const size_t echo_bytes = ne * sizeof(EchoDeckDev) + ne * (size_t)n_ticks * sizeof(EchoTickDev);
        // ... and the sweep filter's, the same way: filters[] names the decks with a filter in any tick
        struct FilterPlan { size_t deck; std::vector<FilterTickDev> ticks; };
        std::vector<FilterPlan> filters;
        std::vector<DeckFilter::State> filter_after(n);
        for (size_t i = 0; i < n; ++i) {
            std::vector<FilterTickDev> ft;
            if (decks[i]->filter.plan(n_ticks, ft, filter_after[i])) filters.push_back(FilterPlan{i, std::move(ft)});
        }
        const size_t nf = filters.size(), filter_bytes = nf * sizeof(FilterDeckDev) + nf * (size_t)n_ticks * sizeof(FilterTickDev);
        // ... and the reverb's: reverbs[] names the decks with a reverb in any tick
        struct ReverbPlan { size_t deck; std::vector<ReverbTickDev> ticks; };
        std::vector<ReverbPlan> reverbs;
        std::vector<DeckReverb::State> reverb_after(n);
        for (size_t i = 0; i < n; ++i) {
            std::vector<ReverbTickDev> rt;
            if (decks[i]->reverb.plan(n_ticks, (uint32_t)spt, rt, reverb_after[i])) reverbs.push_back(ReverbPlan{i, std::move(rt)});
        }
        const size_t nr = reverbs.size(), reverb_bytes = nr * sizeof(ReverbDeckDev) + nr * (size_t)n_ticks * sizeof(ReverbTickDev);

        std::lock_guard<std::mutex> lock(feed_state.mu);
        Slot& sl = feed_state.slots[feed_state.next];
        feed_state.next = (feed_state.next + 1) % kSlots;
        if (sl.pending) { hip_check(hipSetDevice(sl.device), "hipSetDevice"); hip_check(hipEventSynchronize(sl.done), "hipEventSynchronize"); sl.pending = false; hip_check(hipSetDevice(g.device()), "hipSetDevice"); }
        size_t nk = 0, grain_cap = 0;   // key-locked decks, and room for their grain starts: ceil(spt / hop) a tick at the most
        for (size_t i = 0; i < n; ++i)
            if (decks[i]->keylock_.on) { ++nk; grain_cap += (size_t)n_ticks * (spt / decks[i]->keylock_.k.hop + 1); }
        const size_t head_bytes = (n * sizeof(DeckDev) + 15) & ~(size_t)15, plain_bytes = (head_bytes + n * (size_t)n_ticks * sizeof(DeckTickDev) + 15) & ~(size_t)15;
        const size_t feed_bytes = nk ? plain_bytes + nk * sizeof(KlDeckDev) + nk * (size_t)n_ticks * sizeof(KlTickDev) + grain_cap * sizeof(KlGrainIn)
                                     : head_bytes + n * (size_t)n_ticks * sizeof(DeckTickDev);
        const size_t with_echo = ne ? ((feed_bytes + 15) & ~(size_t)15) + echo_bytes : feed_bytes;   // (the echo's descriptors lie behind what the two feed kernels read)
        const size_t with_filter = nf ? ((with_echo + 15) & ~(size_t)15) + filter_bytes : with_echo;  // (... and the filter's behind the echo's)
        const size_t bytes = nr ? ((with_filter + 15) & ~(size_t)15) + reverb_bytes : with_filter;    // (... and the reverb's behind the filter's)
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
            const bool kl = d.keylock_.on;
            if (!kl) dd[ip] = DeckDev{(const uint32_t*)d.track_.p, outs[i], (int64_t)d.n_frames_};
            mx_deck_head h = d.head_;
            recs[i].resize(n_ticks);
            std::vector<const Event*> at(d.sched_.empty() ? 0 : n_ticks, nullptr);
            for (const Event& e : d.sched_) at[e.tick] = &e;
            uint64_t clock = kl && d.keylock_.last_lineage == g.lineage() ? d.keylock_.t : 0;   // (another graph restarts the grain clock; one that adopted the last one's state is not another)
            const uint32_t hop = d.keylock_.k.hop;
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
                k = KlTickDev{m0, m0 ? next - 1 : next, (clock >> d.keylock_.log_hop) == 0 ? 1u : 0u, 1u};
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
                kd[ik] = KlDeckDev{(const uint32_t*)d.track_.p, outs[i], (int64_t)d.n_frames_, d.keylock_.k.pitch_q32, nullptr, (int64_t*)d.keylock_.state.p,
                                   (const KlGrainIn*)((const char*)sl.dev.p + ((const char*)(kg + grain_at) - (const char*)sl.host)),
                                   (uint32_t)grains[ik].size(), d.keylock_.log_hop, d.keylock_.k.overlap, d.keylock_.k.radius, d.keylock_.bank, 0u};
                clocks[ik] = clock;
                grain_at += grains[ik].size();
                ++ik;
            } else ++ip;
        }
        // the last things that can fail: room for the grain records of each key-locked deck.  A deck that changes graphs waits for the device once -- its state and
        // record buffers may still be in use on the other graph's stream.
        for (size_t i = 0, k = 0; i < n; ++i) {
            Deck& d = *decks[i];
            if (!d.keylock_.on) continue;
            if (d.keylock_.last_graph && d.keylock_.last_graph != &g) hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");
            const size_t need = (2 + grains[k].size()) * sizeof(KlRec);
            if (d.keylock_.rec.bytes < need) {
                d.fetch_grains();            // the last feed's records, before their buffer goes
                d.keylock_.rec.free_(); d.keylock_.rec.alloc(2 * need);
            }
            kd[k++].rec = (KlRec*)d.keylock_.rec.p;
        }
        for (size_t i = 0; i < n; ++i)
            if (decks[i]->load_pending_) { hip_check(hipStreamWaitEvent(g.stream(), decks[i]->loaded_, 0), "hipStreamWaitEvent"); decks[i]->load_pending_ = false; }
        const size_t feed_used = nk ? (size_t)((const char*)(kg + grain_at) - (const char*)sl.host) : feed_bytes, echo_at = (feed_used + 15) & ~(size_t)15;
        if (ne) {
            EchoDeckDev* ed = (EchoDeckDev*)((char*)sl.host + echo_at);
            EchoTickDev* et = (EchoTickDev*)(ed + ne);
            for (size_t k = 0; k < ne; ++k) {
                Deck& d = *decks[echoes[k].deck];
                if (d.echo.last_graph && d.echo.last_graph != &g) hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // (its line may still be in use on the other graph's stream)
                ed[k] = EchoDeckDev{(float2*)outs[echoes[k].deck], d.echo.line()};
                std::copy(echoes[k].ticks.begin(), echoes[k].ticks.end(), et + k * (size_t)n_ticks);
            }
        }
        const size_t echo_used = ne ? echo_at + echo_bytes : feed_used, filter_at = (echo_used + 15) & ~(size_t)15;
        if (nf) {
            FilterDeckDev* fd = (FilterDeckDev*)((char*)sl.host + filter_at);
            FilterTickDev* ft = (FilterTickDev*)(fd + nf);
            for (size_t k = 0; k < nf; ++k) {
                Deck& d = *decks[filters[k].deck];
                if (d.filter.last_graph && d.filter.last_graph != &g) hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // (its state may still be in use on the other graph's stream)
                fd[k] = FilterDeckDev{(float2*)outs[filters[k].deck], d.filter.dev_state()};
                std::copy(filters[k].ticks.begin(), filters[k].ticks.end(), ft + k * (size_t)n_ticks);
            }
        }
        const size_t filter_used = nf ? filter_at + filter_bytes : echo_used, reverb_at = (filter_used + 15) & ~(size_t)15;
        if (nr) {
            ReverbDeckDev* rd = (ReverbDeckDev*)((char*)sl.host + reverb_at);
            ReverbTickDev* rt = (ReverbTickDev*)(rd + nr);
            for (size_t k = 0; k < nr; ++k) {
                Deck& d = *decks[reverbs[k].deck];
                if (d.reverb.last_graph && d.reverb.last_graph != &g) hip_check(hipDeviceSynchronize(), "hipDeviceSynchronize");   // (its lines may still be in use on the other graph's stream)
                rd[k] = ReverbDeckDev{(float2*)outs[reverbs[k].deck], d.reverb.lines()};
                std::copy(reverbs[k].ticks.begin(), reverbs[k].ticks.end(), rt + k * (size_t)n_ticks);
            }
        }
        launch_upload(sl.dev.p, sl.host, nr ? reverb_at + reverb_bytes : filter_used, g.stream());
        launch_deck_feed((const DeckDev*)sl.dev.p, (const DeckTickDev*)((const char*)sl.dev.p + head_bytes), tables, (uint32_t)ip, n_ticks, (uint32_t)spt, phase_varies, g.stream());
        launch_deck_keylock((const KlDeckDev*)((const char*)sl.dev.p + plain_bytes), (const KlTickDev*)((const char*)sl.dev.p + plain_bytes + nk * sizeof(KlDeckDev)), tables,
                            (uint32_t)nk, n_ticks, (uint32_t)spt, g.stream());
        if (nf) launch_deck_filter((const FilterDeckDev*)((const char*)sl.dev.p + filter_at), (const FilterTickDev*)((const char*)sl.dev.p + filter_at + nf * sizeof(FilterDeckDev)),
                                   (uint32_t)nf, n_ticks, (uint32_t)spt, g.stream());
        if (ne) launch_deck_echo((const EchoDeckDev*)((const char*)sl.dev.p + echo_at), (const EchoTickDev*)((const char*)sl.dev.p + echo_at + ne * sizeof(EchoDeckDev)),
                                 (uint32_t)ne_block, (uint32_t)(ne - ne_block), n_ticks, (uint32_t)spt, g.stream());
        if (nr) launch_deck_reverb((const ReverbDeckDev*)((const char*)sl.dev.p + reverb_at), (const ReverbTickDev*)((const char*)sl.dev.p + reverb_at + nr * sizeof(ReverbDeckDev)),
                                   (uint32_t)nr, n_ticks, (uint32_t)spt, g.stream());
        hip_check(hipGetLastError(), "deck feed launch");
        hip_check(hipEventRecord(sl.done, g.stream()), "hipEventRecord");
        sl.pending = true; sl.stream = g.stream();
        feed_state.last.assign(td, td + ip * (size_t)n_ticks); feed_state.last_spt = (uint32_t)spt;
        feed_state.last_kl.clear(); feed_state.kl_searched = feed_state.kl_unsearched = 0;
        feed_state.last_echo.clear();
        for (EchoPlan& e : echoes) { decks[e.deck]->echo.last_graph = &g; feed_state.last_echo.push_back(std::move(e.delays)); }
        // mx_deck_debug_last_filter: decks with a filter, their ticks with and without a ramp, the super-blocks the kernel walked (every one of the feed, per deck)
        feed_state.last_filter = DeckLastFilter{};
        for (const FilterPlan& f : filters) {
            decks[f.deck]->filter.last_graph = &g;
            ++feed_state.last_filter.out[0];
            for (const FilterTickDev& t : f.ticks) if (t.flags & FILTER_TICK_ON) ++feed_state.last_filter.out[(t.flags & FILTER_TICK_RAMP) ? 1 : 2];
            feed_state.last_filter.out[3] += (uint32_t)(((uint64_t)n_ticks * spt + FILTER_BLOCK - 1) / FILTER_BLOCK);
        }
        // mx_deck_debug_last_reverb: per deck with a reverb the reaches of its ticks
        feed_state.last_reverb.clear();
        for (const ReverbPlan& r : reverbs) {
            decks[r.deck]->reverb.last_graph = &g;
            std::vector<uint32_t> reach(n_ticks);
            for (uint32_t t = 0; t < n_ticks; ++t) reach[t] = reverb_reach_of(r.ticks[t]);
            feed_state.last_reverb.push_back(std::move(reach));
        }
        for (size_t i = 0, k = 0; i < n; ++i) {
            Deck& d = *decks[i];
            d.echo.commit(echo_after[i]);
            d.filter.commit(filter_after[i]);
            d.reverb.commit(reverb_after[i]);
            d.head_ = heads[i]; d.ticks_ = std::move(recs[i]); d.sched_.clear(); d.keylock_.last_graph = &g; d.keylock_.last_lineage = g.lineage();
            if (!d.keylock_.on) { d.keylock_.grains.clear(); d.keylock_.grains_fetched = true; continue; }
            for (const mx_deck_grain& gr : grains[k]) ++((gr.flags & MX_DECK_GRAIN_FIRST) || !d.keylock_.k.radius ? feed_state.kl_unsearched : feed_state.kl_searched);
            for (uint32_t t = 0; t < n_ticks; ++t) feed_state.last_kl.push_back(FeedState::KlTick{kt[k * (size_t)n_ticks + t], d.keylock_.log_hop, d.keylock_.k.overlap});
            d.keylock_.t = clocks[k]; d.keylock_.grains = std::move(grains[k]); d.keylock_.grains_fetched = d.keylock_.grains.empty();
            ++k;
        }
    } catch (...) { drop(); throw; }
}

DeckLastKeylock deck_last_keylock() {
    std::lock_guard<std::mutex> lock(feed_state.mu);
    return DeckLastKeylock{feed_state.last_kl, feed_state.last_spt, feed_state.kl_searched, feed_state.kl_unsearched};
}

DeckLastEcho deck_last_echo() {
    std::lock_guard<std::mutex> lock(feed_state.mu);
    return DeckLastEcho{feed_state.last_echo, feed_state.last_spt};
}

DeckLastReverb deck_last_reverb() {
    std::lock_guard<std::mutex> lock(feed_state.mu);
    return DeckLastReverb{feed_state.last_reverb, feed_state.last_spt};
}

DeckLastFilter deck_last_filter() {
    std::lock_guard<std::mutex> lock(feed_state.mu);
    return feed_state.last_filter;
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
