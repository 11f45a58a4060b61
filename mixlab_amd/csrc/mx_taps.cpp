// mx_taps.cpp -- the audio tap sets.  See mx_taps.hpp.  What the seven share comes first, written for "a tap set"; then each set's own part.
#include "mx_taps.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

namespace mx {

// own_check: a set's own check of one tap, behind the shared ones of that tap
void AudioTapSet::check_ports(const mx_port_ref* ports_, size_t n, const std::function<void(size_t, const TapPort&)>& own_check) const {
    const std::string tag_ = std::string(tag) + ": ";
    std::vector<uint64_t> keys(n);
    for (size_t i = 0; i < n; ++i) {
        const mx_port_ref pr = ports_[i]; TapPort t;
        if (!host_.tap_port(pr, t)) throw Error(MX_ERR_INVALID, tag_ + "output terminal out of range");
        if (stereo_only ? t.type != MX_STEREO : t.type == MX_VIDEO) throw Error(MX_ERR_TYPE, tag_ + no_type);
        if (t.elided) throw Error(MX_ERR_INVALID, "port is not materialised: it only feeds a fused consumer (build with MX_FLAG_NO_FUSE to observe it)");
        if (own_check) own_check(i, t);
        keys[i] = (uint64_t)pr.node << 32 | pr.port;
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) throw Error(MX_ERR_INVALID, tag_ + "duplicate (node, port)");
}

// The descriptors of every tap for both buffer parities (the second only differs for a port the tail reads, while the second-stream mode is
// on), in launch order: the taps read on the graph's stream (n_head of them), then those on the tail's outputs.
std::vector<TapDesc> AudioTapSet::tap_descs(size_t fpc) {
    const size_t n = ports.size();
    std::vector<uint32_t> order, tail;
    std::vector<TapPort> tp(n);
    for (uint32_t i = 0; i < (uint32_t)n; ++i) { tp[i] = port(i); (tp[i].on_tail ? tail : order).push_back(i); }
    n_head = (uint32_t)order.size();
    order.insert(order.end(), tail.begin(), tail.end());
    std::vector<TapDesc> d(2 * n);
    for (uint32_t par = 0; par < 2; ++par)
        for (size_t k = 0; k < n; ++k) {
            const TapPort& t = tp[order[k]];
            TapDesc& m = d[par * n + k];
            m.p = t.p[par];
            m.frames = (uint32_t)(fpc * t.dom_num / t.dom_den);
            m.layout = t.dup ? METER_DUP : (t.type == MX_MONO ? METER_MONO : METER_STEREO);
            m.slot = order[k]; m._pad = 0;
        }
    return d;
}

// ... to the device, and room for a whole submission's records of tick_bytes per tick.  The stream is quiescent.  Whatever a set carries from
// run to run is untouched: it holds frames and ticks, whatever the call length.
void AudioTapSet::upload_tap_descs(const void* d, size_t bytes, size_t fpc, size_t tick_bytes) {
    tick_bytes_ = tick_bytes;
    desc.alloc(bytes);
    hip_check(hipMemcpy(desc.p, d, bytes, hipMemcpyHostToDevice), (std::string("hipMemcpy(") + tag + " descriptors)").c_str());
    const size_t need = std::max<size_t>(1, host_.cap_frames() / fpc) * tick_bytes;
    if (!rec.p || rec.bytes < need) rec.alloc(need);
}

void AudioTapSet::alloc_zeroed(DevBuf& b, size_t bytes, const char* what) { b.alloc(bytes); hip_check(hipMemsetAsync(b.p, 0, bytes, host_.stream()), what); }

void AudioTapSet::read(uint32_t first, uint32_t n, void* dst, size_t cap) {
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    if (empty()) throw Error(MX_ERR_INVALID, std::string("no ") + noun + " are set");
    if ((uint64_t)first + n > run_ticks) throw Error(MX_ERR_INVALID, std::string("the window lies beyond the last run (or no run since the ") + noun + " were set)");
    const size_t count = (size_t)n * (tick_bytes_ / item_bytes_);
    if (cap < count) throw Error(MX_ERR_INVALID, std::string("cap is smaller than ") + cap_what_);
    if (count && !dst) throw Error(MX_ERR_INVALID, "dst is NULL");
    if (!count) return;
    host_.join_tail();
    hip_check(hipMemcpyAsync(dst, (const char*)rec.p + (size_t)first * tick_bytes_, count * item_bytes_, hipMemcpyDeviceToHost, host_.stream()), "hipMemcpyAsync(D2H)");
    host_.sync();
}

// ---- level meters ----

void MeterTaps::set(const mx_port_ref* ports_, size_t n, const mx_meter_params* params) {
    DevBuf st;
    set_taps(ports_, n, params, [&] {
        check_ports(ports_, n, [&](size_t i, const TapPort&) {
            const float rel = params[i].release;
            if (!(std::isfinite(rel) && rel > 0.0f && rel <= 1.0f)) throw Error(MX_ERR_INVALID, "mx_meter_params: release must be finite, 0 < release <= 1");
        });
    }, [&] { par_.assign(params, params + n); state_ = std::move(st); }, [&] {
        if (!n) return;
        alloc_zeroed(st, n * 2 * sizeof(MeterHold), "hipMemsetAsync(meter state)");
        for (size_t i = 0; i < n; ++i)   // a surviving tap keeps its hold
            for (size_t j = 0; j < ports.size(); ++j)
                if (ports[j].node == ports_[i].node && ports[j].port == ports_[i].port)
                    hip_check(hipMemcpyAsync((MeterHold*)st.p + 2 * i, (const MeterHold*)state_.p + 2 * j, 2 * sizeof(MeterHold), hipMemcpyDeviceToDevice, host_.stream()),
                              "hipMemcpyAsync(meter state)");
        hip_check(hipStreamSynchronize(host_.stream()), "hipStreamSynchronize");
    });
}

// the shared fields of every descriptor from its TapDesc, then the tap's own parameters
void MeterTaps::upload(size_t fpc) {
    const std::vector<TapDesc> t = tap_descs(fpc);
    std::vector<MeterDesc> d(t.size());
    for (size_t k = 0; k < t.size(); ++k)
        d[k] = MeterDesc{t[k].p, t[k].frames, t[k].layout, t[k].slot, par_[t[k].slot].hold_ticks, par_[t[k].slot].release, 0};
    upload_tap_descs(d.data(), d.size() * sizeof(MeterDesc), fpc, ports.size() * sizeof(MeterTick));
}

void MeterTaps::begin_run(uint32_t n_ticks) { run_ = MeterRun{(const MeterDesc*)desc.p, size(), n_ticks, size(), (MeterTick*)rec.p, (MeterHold*)state_.p}; }

// ---- spectrum taps ----

void SpectrumTaps::set(const mx_port_ref* ports_, size_t n, const mx_spectrum_params* params) {
    std::vector<float> win, tre, tim;
    set_taps(ports_, n, params, [&] {
        if (n) {
            const uint32_t N = params->n_fft, B = params->n_bands;
            win.resize(N <= 4096 ? N : 0); tre.resize(win.size() / 2); tim.resize(win.size() / 2);
            if (N > 4096 || !spectrum_tables(N, win.data(), tre.data(), tim.data())) throw Error(MX_ERR_INVALID, "mx_spectrum_params: n_fft must be 256, 512, 1024, 2048 or 4096");
            if (B < 1 || B > 128) throw Error(MX_ERR_INVALID, "mx_spectrum_params: n_bands must be 1 .. 128");
            if (!params->edges) throw Error(MX_ERR_INVALID, "mx_spectrum_params: edges is NULL");
            for (uint32_t j = 0; j < B; ++j)
                if (params->edges[j] >= params->edges[j + 1]) throw Error(MX_ERR_INVALID, "mx_spectrum_params: edges must be strictly ascending");
            if (params->edges[B] > N / 2 + 1) throw Error(MX_ERR_INVALID, "mx_spectrum_params: edges[n_bands] exceeds n_fft / 2 + 1");
        }
        check_ports(ports_, n);
    }, [&] {
        const uint32_t N = n_fft_ = params->n_fft, B = n_bands_ = params->n_bands;
        // tables: window[N] | twiddle (re, im)[N / 2] | edges[B + 1] (u16, padded to whole floats)
        std::vector<float> tab(2 * (size_t)N + (B + 2) / 2, 0.0f);
        std::copy(win.begin(), win.end(), tab.begin());
        for (uint32_t k = 0; k < N / 2; ++k) { tab[N + 2 * k] = tre[k]; tab[N + 2 * k + 1] = tim[k]; }
        memcpy(tab.data() + 2 * (size_t)N, params->edges, (B + 1) * sizeof(uint16_t));
        tab_.alloc(tab.size() * sizeof(float));
        hip_check(hipMemcpy(tab_.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(spectrum tables)");
        // every tap's history starts as +0.0: frames before this call read as silence
        alloc_zeroed(hist_, 2 * n * 2 * (size_t)N * sizeof(float), "hipMemsetAsync(spectrum history)");
    });
}

void SpectrumTaps::upload(size_t fpc) {
    const std::vector<TapDesc> d = tap_descs(fpc);
    upload_tap_descs(d.data(), d.size() * sizeof(TapDesc), fpc, ports.size() * 2 * n_bands_ * sizeof(float));
}

// Each run reads the history buffer the previous one wrote: the history flips once per run.
void SpectrumTaps::begin_run(uint32_t n_ticks) {
    const uint32_t n = size(), N = n_fft_;
    const float* tab = (const float*)tab_.p; const uint32_t cur = flip_hist();
    float* h0 = (float*)hist_.p + (size_t)cur * n * 2 * N, * h1 = (float*)hist_.p + (size_t)(cur ^ 1u) * n * 2 * N;
    run_ = SpecRun{(const TapDesc*)desc.p, n, n_ticks, n, N, n_bands_, tab, (const float2*)(tab + N), (const uint16_t*)(tab + 2 * (size_t)N), h0, h1, (float*)rec.p};
}

// ---- loudness taps ----

void LoudnessTaps::set(const mx_port_ref* ports_, size_t n, const mx_loudness_params* params) {
    set_taps(ports_, n, params, [&] {
        if (n) {
            if (params->momentary_ticks < 1 || params->momentary_ticks > 1024) throw Error(MX_ERR_INVALID, "mx_loudness_params: momentary_ticks must be 1 .. 1024");
            if (params->short_ticks < 1 || params->short_ticks > 1024) throw Error(MX_ERR_INVALID, "mx_loudness_params: short_ticks must be 1 .. 1024");
        }
        check_ports(ports_, n, [&](size_t, const TapPort& t) {
            if (!loudness_tables(host_.sample_rate() * t.dom_num / t.dom_den, 1, nullptr, nullptr, nullptr)) throw Error(MX_ERR_INVALID, "loudness: the port's rate is not above twice the shelf frequency (3 364 Hz)");
        });
    }, [&] {
        par_ = *params;
        // filter state, window history and interpolator history all start as +0.0: the stream before this call reads as silence
        alloc_zeroed(carry_, n * (8 + 2 * (size_t)LOUD_HIST_TICKS) * sizeof(double) + 2 * n * 2 * LOUD_HIST_FRAMES * sizeof(float), "hipMemsetAsync(loudness state)");
    });
}

// beside the descriptors: room for the walk states and -- what depends on the call length here -- each tap's coefficients, the biquads of its
// port's own rate and the carry matrix of its tick length
void LoudnessTaps::upload(size_t fpc) {
    const size_t n = ports.size();
    const std::vector<TapDesc> d = tap_descs(fpc);
    upload_tap_descs(d.data(), d.size() * sizeof(TapDesc), fpc, n * sizeof(LoudTick));
    // LoudCoef[n] by slot | interp[36]; taps of one rate domain share one evaluation
    std::vector<unsigned char> tab(n * sizeof(LoudCoef) + 36 * sizeof(float));
    std::map<std::pair<uint32_t, uint32_t>, LoudCoef> by_dom;
    for (size_t i = 0; i < n; ++i) {
        const TapPort t = port(i);
        auto it = by_dom.find({t.dom_num, t.dom_den});
        if (it == by_dom.end()) {
            LoudCoef c;
            if (!loudness_tables(host_.sample_rate() * t.dom_num / t.dom_den, (uint32_t)(fpc * t.dom_num / t.dom_den), c.bq, c.carry, nullptr))
                throw Error(MX_ERR_INVALID, "loudness: the call length gives a tick the taps cannot measure");
            it = by_dom.emplace(std::make_pair(t.dom_num, t.dom_den), c).first;
        }
        memcpy(tab.data() + i * sizeof(LoudCoef), &it->second, sizeof(LoudCoef));
    }
    (void)loudness_tables(host_.sample_rate(), 1, nullptr, nullptr, reinterpret_cast<float*>(tab.data() + n * sizeof(LoudCoef)));   // (the interpolator depends on neither)
    tab_.alloc(tab.size());
    hip_check(hipMemcpy(tab_.p, tab.data(), tab.size(), hipMemcpyHostToDevice), "hipMemcpy(loudness tables)");
    max_ticks_ = (uint32_t)std::max<size_t>(1, host_.cap_frames() / fpc);
    const size_t need_walk = (size_t)max_ticks_ * n * 2 * 4 * sizeof(double);
    if (!walk_.p || walk_.bytes < need_walk) walk_.alloc(need_walk);
}

// The filter state is updated in place by the one lane that owns it; each run reads the history buffers the previous one wrote
// (the history flips once per run).
void LoudnessTaps::begin_run(uint32_t n_ticks) {
    const uint32_t n = size();
    double* state = (double*)carry_.p, * eh = state + (size_t)n * 8;
    float* xh = (float*)(eh + 2 * (size_t)n * LOUD_HIST_TICKS);
    const uint32_t cur = flip_hist();
    run_ = LoudRun{(const TapDesc*)desc.p, n, n_ticks, n, par_.momentary_ticks, par_.short_ticks,
                   (const LoudCoef*)tab_.p, (const float*)((const LoudCoef*)tab_.p + n), state, (double*)walk_.p, max_ticks_,
                   eh + (size_t)cur * n * LOUD_HIST_TICKS, eh + (size_t)(cur ^ 1u) * n * LOUD_HIST_TICKS,
                   xh + (size_t)cur * n * 2 * LOUD_HIST_FRAMES, xh + (size_t)(cur ^ 1u) * n * 2 * LOUD_HIST_FRAMES, (LoudTick*)rec.p};
}

// ---- stereo field taps ----

void StereoTaps::set(const mx_port_ref* ports_, size_t n, const mx_stereo_params* params) {
    set_taps(ports_, n, params, [&] {
        if (n) {
            if (params->window_ticks < 1 || params->window_ticks > 1024) throw Error(MX_ERR_INVALID, "mx_stereo_params: window_ticks must be 1 .. 1024");
            if (params->grid != 0 && params->grid != 64 && params->grid != 128) throw Error(MX_ERR_INVALID, "mx_stereo_params: grid must be 0, 64 or 128");
            if (params->zoom_log2 > 8) throw Error(MX_ERR_INVALID, "mx_stereo_params: zoom_log2 must be 0 .. 8");
            if (params->grid && params->hop == 0) throw Error(MX_ERR_INVALID, "mx_stereo_params: hop must be >= 1 with a goniometer");
        }
        check_ports(ports_, n);
        if (n && params->grid) gon_room(host_.tap_fpc(), n, params->grid, params->hop);   // (throws before anything changed)
    }, [&] {
        par_ = *params;
        if (!par_.grid) par_.hop = 1;   // (ignored without a goniometer)
        // window history and carried grids start as zero: the stream before this call reads as +0.0, c = 0
        alloc_zeroed(carry_, 2 * n * (size_t)STEREO_HIST_TICKS * 3 * sizeof(double), "hipMemsetAsync(stereo history)");
        if (par_.grid) alloc_zeroed(gon_carry_, n * stereo_gonio_record_bytes(par_.grid), "hipMemsetAsync(goniometer grids)");
    });
}

// the most goniometer records one run can emit at this call length (a run of T ticks that starts anywhere in a hop emits at most
// ceil(T / hop)), refused beyond 4 GiB
size_t StereoTaps::gon_room(size_t fpc, size_t n, uint32_t grid, uint32_t hop) const {
    const size_t max_ticks = std::max<size_t>(1, host_.cap_frames() / fpc), cap = (max_ticks + hop - 1) / hop;
    if ((unsigned __int128)cap * n * stereo_gonio_record_bytes(grid) > ((unsigned __int128)4 << 30))
        throw Error(MX_ERR_NOMEM, "stereo: the goniometer records of one run (ceil(max_ticks_per_run / hop) x taps x record bytes) exceed 4 GiB: raise hop");
    return cap;
}

// beside the descriptors: room for the goniometer records a run can emit (refused before anything is touched)
void StereoTaps::upload(size_t fpc) {
    const size_t n = ports.size();
    const size_t need_gon = par_.grid ? gon_room(fpc, n, par_.grid, par_.hop) * n * stereo_gonio_record_bytes(par_.grid) : 0;
    const std::vector<TapDesc> d = tap_descs(fpc);
    upload_tap_descs(d.data(), d.size() * sizeof(TapDesc), fpc, n * sizeof(StereoTick));
    if (need_gon && (!gon_rec_.p || gon_rec_.bytes < need_gon)) gon_rec_.alloc(need_gon);
}

// Each run reads the window history the previous one wrote (the history flips once per run).  A tap's carried grid and its goniometer
// records are touched by that tap's group alone -- which is why k_stereo_emit and not a memset on the graph's stream clears the records.
// The counter c lives on the host: the run's phase and emissions are launch arguments.
void StereoTaps::begin_run(uint32_t n_ticks) {
    const uint32_t n = size();
    double* hist = (double*)carry_.p; const size_t hist_words = (size_t)n * STEREO_HIST_TICKS * 3;
    const uint32_t cur = flip_hist();
    const uint32_t grid = par_.grid, hop = par_.hop, phase = (uint32_t)(c_ % hop);
    const uint32_t n_emit = grid ? (uint32_t)(((uint64_t)phase + n_ticks) / hop) : 0u;
    c_ += n_ticks; gon_n_ = n_emit; run_seen_ = true;
    run_ = StereoRun{(const TapDesc*)desc.p, n, n_ticks, n, par_.window_ticks, hist + (size_t)cur * hist_words, hist + (size_t)(cur ^ 1u) * hist_words, (StereoTick*)rec.p,
                     grid, par_.zoom_log2, hop, phase, n_emit, 8u + grid * grid, (uint32_t*)gon_rec_.p, (uint32_t*)gon_carry_.p};
}

size_t StereoTaps::read_goniometers(void* dst, size_t cap_bytes) {
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    if (empty()) throw Error(MX_ERR_INVALID, "no stereo taps are set");
    if (!par_.grid) throw Error(MX_ERR_INVALID, "the stereo taps were set without a goniometer (grid = 0)");
    if (!run_seen_) throw Error(MX_ERR_INVALID, "no run since the stereo taps were set");
    const size_t count = (size_t)gon_n_ * ports.size(), bytes = count * stereo_gonio_record_bytes(par_.grid);
    if (cap_bytes < bytes) throw Error(MX_ERR_INVALID, "cap_bytes is smaller than emissions x taps x record bytes");
    if (bytes && !dst) throw Error(MX_ERR_INVALID, "dst is NULL");
    if (bytes) {
        host_.join_tail();
        hip_check(hipMemcpyAsync(dst, gon_rec_.p, bytes, hipMemcpyDeviceToHost, host_.stream()), "hipMemcpyAsync(D2H)");
        host_.sync();
    }
    return count;
}

// ---- limiter taps ----

void LimiterTaps::set(const mx_port_ref* ports_, size_t n, const mx_limiter_params* params) {
    set_taps(ports_, n, params, [&] {
        if (n) {
            const float c = params->ceiling;
            if (!(std::isfinite(c) && c >= 0x1p-20f && c <= 1.0f)) throw Error(MX_ERR_INVALID, "mx_limiter_params: ceiling must be finite, 2^-20 <= ceiling <= 1");
            if (params->lookahead > LIMIT_MAX_LOOKAHEAD) throw Error(MX_ERR_INVALID, "mx_limiter_params: lookahead must be 0 .. 512");
        }
        check_ports(ports_, n);
    }, [&] {
        par_ = *params;
        std::vector<float> w(par_.lookahead + 1u);
        (void)limiter_weights(par_.lookahead, w.data());
        w_.alloc(w.size() * sizeof(float));
        hip_check(hipMemcpy(w_.p, w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy(limiter weights)");
        // every tap's history starts as +0.0: frames before this call read as silence
        alloc_zeroed(hist_, 2 * n * (size_t)LIMIT_HIST_FRAMES * sizeof(float2), "hipMemsetAsync(limiter history)");
    });
}

// beside the descriptors: where each tap's copy starts inside a tick of copies, and room for a whole submission's copies
void LimiterTaps::upload(size_t fpc) {
    const size_t n = ports.size();
    const std::vector<TapDesc> t = tap_descs(fpc);
    off_.assign(n, 0); floats_.assign(n, 0);
    size_t sum = 0; uint32_t max_frames = 0;
    for (size_t i = 0; i < n; ++i) {   // set order
        const TapPort tp = port(i);
        const size_t frames = fpc * tp.dom_num / tp.dom_den;
        if (frames > LIMIT_MAX_FRAMES) throw Error(MX_ERR_INVALID, "limiter: a tick of more than 2^30 frames");
        off_[i] = sum; floats_[i] = frames * (tp.type == MX_MONO ? 1u : 2u);
        sum += floats_[i]; max_frames = std::max(max_frames, (uint32_t)frames);
    }
    const size_t max_ticks = std::max<size_t>(1, host_.cap_frames() / fpc);
    if ((unsigned __int128)max_ticks * sum * sizeof(float) > ((unsigned __int128)1 << 46)) throw Error(MX_ERR_NOMEM, "limiter: the limited copies of one run (max_ticks_per_run x the taps' frames x channels) exceed the device");
    std::vector<LimitDesc> d(t.size());
    for (size_t k = 0; k < t.size(); ++k)
        d[k] = LimitDesc{t[k].p, t[k].frames, t[k].layout, t[k].slot, t[k].layout == METER_MONO ? 1u : 2u, (uint64_t)off_[t[k].slot]};
    const size_t need = max_ticks * sum * sizeof(float);
    if (!out_.p || out_.bytes < need) out_.alloc(need);
    upload_tap_descs(d.data(), d.size() * sizeof(LimitDesc), fpc, n * sizeof(LimitTick));
    tick_floats_ = sum; max_frames_ = max_frames;
}

// Each run reads the frame history the previous one wrote (the history flips once per run).  A tap's copy, records and history are touched
// by that tap's workgroups alone.
void LimiterTaps::begin_run(uint32_t n_ticks) {
    const uint32_t n = size();
    float2* hist = (float2*)hist_.p; const size_t hist_items = (size_t)n * LIMIT_HIST_FRAMES;
    const uint32_t cur = flip_hist();
    run_ = LimitRun{(const LimitDesc*)desc.p, n, n_ticks, n, par_.ceiling, par_.lookahead, (const float*)w_.p,
                    hist + (size_t)cur * hist_items, hist + (size_t)(cur ^ 1u) * hist_items, (float*)out_.p, tick_floats_, (LimitTick*)rec.p, max_frames_};
}

void LimiterTaps::read_limited(size_t tap, uint32_t first, uint32_t n, float* dst, int16_t* dst_i16, size_t cap, size_t* n_samples) {
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    if (empty()) throw Error(MX_ERR_INVALID, "no limiter taps are set");
    if (tap >= ports.size()) throw Error(MX_ERR_INVALID, "limiter: tap out of range");
    if ((uint64_t)first + n > run_ticks) throw Error(MX_ERR_INVALID, "the window lies beyond the last run (or no run since the limiter taps were set)");
    const size_t width = floats_[tap], count = (size_t)n * width;
    if (n_samples) *n_samples = count;
    if (!dst && !dst_i16 && cap == 0) return;   // the count alone
    if (cap < count) throw Error(MX_ERR_INVALID, "cap is smaller than n_ticks x frames x channels");
    if (count && !dst && !dst_i16) throw Error(MX_ERR_INVALID, "samples is NULL");
    if (!count) return;
    host_.join_tail();
    const size_t need = count * (sizeof(float) + sizeof(int16_t));   // f32 staging, then the i16 form
    if (stage_.bytes < need) { host_.sync(); stage_.alloc(need); }
    float* stage = (float*)stage_.p;
    launch_limit_gather((const float*)out_.p + (size_t)first * tick_floats_ + off_[tap], tick_floats_, (uint32_t)width, n, stage, host_.stream());
    if (dst_i16) {
        launch_f32_to_i16(stage, (int16_t*)(stage + count), count, 0, host_.stream());
        hip_check(hipMemcpyAsync(dst_i16, stage + count, count * sizeof(int16_t), hipMemcpyDeviceToHost, host_.stream()), "hipMemcpyAsync(D2H i16)");
    } else
        hip_check(hipMemcpyAsync(dst, stage, count * sizeof(float), hipMemcpyDeviceToHost, host_.stream()), "hipMemcpyAsync(D2H)");
    host_.sync();
}

float* LimiterTaps::limited_ptr(size_t tap, size_t* floats_per_tick) {
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    if (empty()) throw Error(MX_ERR_INVALID, "no limiter taps are set");
    if (tap >= ports.size()) throw Error(MX_ERR_INVALID, "limiter: tap out of range");
    if (floats_per_tick) *floats_per_tick = tick_floats_;
    host_.join_tail();   // the graph's stream is ordered behind a held-back tail's limiter launches too
    return (float*)out_.p + off_[tap];
}

// ---- tempo taps ----

void TempoTaps::set(const mx_port_ref* ports_, size_t n, const mx_tempo_params* params) {
    set_taps(ports_, n, params, [&] {
        if (n && !tempo_params_ok(params->hop_frames, params->window_hops, params->max_lag, params->emit_ticks))
            throw Error(MX_ERR_INVALID, "mx_tempo_params: hop_frames must be 64, 128 or 256, window_hops 64 .. 4096, max_lag 16 .. 1024 and <= window_hops, emit_ticks >= 1");
        check_ports(ports_, n);
        if (n) room(host_.tap_fpc(), n, *params);   // (throws before anything changed)
    }, [&] {
        par_ = *params;
        // every tap's stream starts at frame 0 with nothing carried, c = 0; the onset arrays are sized and zeroed by the upload that follows
        alloc_zeroed(state_, n * (2 * sizeof(uint64_t) + 3 * sizeof(uint32_t)), "hipMemsetAsync(tempo state)");
    });
}

size_t TempoTaps::room(size_t fpc, size_t n, const mx_tempo_params& p) const {
    const size_t max_ticks = std::max<size_t>(1, host_.cap_frames() / fpc), cap = (max_ticks + p.emit_ticks - 1) / p.emit_ticks;
    if ((unsigned __int128)cap * n * tempo_record_bytes(p.max_lag) > ((unsigned __int128)4 << 30))
        throw Error(MX_ERR_NOMEM, "tempo: the records of one run (ceil(max_ticks_per_run / emit_ticks) x taps x record bytes) exceed 4 GiB: raise emit_ticks");
    return cap;
}

// beside the descriptors: every rate domain's stream position so far (the frames per tick change with the call length, the stream goes on),
// room for the run's records, and the onset arrays -- whose length depends on the hops of the longest run the graph has room for, so a graph
// that has grown moves the carried onsets into arrays of the new length (a changed call length alone leaves them where they are)
void TempoTaps::upload(size_t fpc) {
    const size_t n = ports.size();
    const size_t need_rec = room(fpc, n, par_) * n * tempo_record_bytes(par_.max_lag);
    const uint32_t hist = par_.window_hops + par_.max_lag - 1;
    for (Domain& d : dom_) { d.pos0 += ticks0_ * d.frames; d.frames = 0; }
    ticks0_ = 0;
    uint64_t most_hops = 0;
    for (size_t i = 0; i < n; ++i) {
        const TapPort t = port(i);
        auto it = std::find_if(dom_.begin(), dom_.end(), [&](const Domain& d) { return d.num == t.dom_num && d.den == t.dom_den; });
        if (it == dom_.end()) it = dom_.insert(dom_.end(), Domain{t.dom_num, t.dom_den, 0, 0});
        it->frames = fpc * t.dom_num / t.dom_den;
        if (it->frames > LIMIT_MAX_FRAMES) throw Error(MX_ERR_INVALID, "tempo: a tick of more than 2^30 frames");
        // a run of the most frames, which starts anywhere in a hop; max_ticks x frames <= cap_frames x num / den whatever the call length
        most_hops = std::max<uint64_t>(most_hops, (uint64_t)((unsigned __int128)host_.cap_frames() * t.dom_num / t.dom_den / par_.hop_frames) + 1);
    }
    if (most_hops + hist > 0x7fffffffu) throw Error(MX_ERR_NOMEM, "tempo: the hops of one run exceed the device");
    const uint32_t lin_stride = (uint32_t)most_hops + hist, e_stride = (uint32_t)most_hops;
    if (lin_stride != lin_stride_) {
        DevBuf lin;
        alloc_zeroed(lin, 2 * n * (size_t)lin_stride * sizeof(uint32_t), "hipMemsetAsync(tempo onsets)");
        if (lin_.p)   // the carried onsets: the front of each tap's array in the buffer the next run reads
            hip_check(hipMemcpy2DAsync((uint32_t*)lin.p + (size_t)hist_cur_ * n * lin_stride, (size_t)lin_stride * sizeof(uint32_t),
                                       (const uint32_t*)lin_.p + (size_t)hist_cur_ * n * lin_stride_, (size_t)lin_stride_ * sizeof(uint32_t),
                                       (size_t)hist * sizeof(uint32_t), n, hipMemcpyDeviceToDevice, host_.stream()), "hipMemcpy2DAsync(tempo onsets)");
        hip_check(hipStreamSynchronize(host_.stream()), "hipStreamSynchronize");
        lin_ = std::move(lin); lin_stride_ = lin_stride;
    }
    if (!energy_.p || e_stride != e_stride_) { energy_.alloc(n * (size_t)e_stride * sizeof(uint64_t)); e_stride_ = e_stride; }
    const std::vector<TapDesc> t = tap_descs(fpc);
    std::vector<TempoDesc> d(t.size());
    for (size_t k = 0; k < t.size(); ++k) {
        const TapPort tp = port(t[k].slot);
        const Domain& dm = *std::find_if(dom_.begin(), dom_.end(), [&](const Domain& x) { return x.num == tp.dom_num && x.den == tp.dom_den; });
        d[k] = TempoDesc{t[k].p, t[k].frames, t[k].layout, t[k].slot, 0u, dm.pos0};
    }
    upload_tap_descs(d.data(), d.size() * sizeof(TempoDesc), fpc, 0);
    if (rec.bytes < need_rec) rec.alloc(need_rec);
}

// Each run reads the partial, the amplitude and the onset array the previous one wrote (they flip once per run).  The emission schedule and
// every hop count follow from frame counts alone: the counter c and the stream positions live on the host, and the run's phase, emissions
// and grid sizes are launch arguments.
void TempoTaps::begin_run(uint32_t n_ticks) {
    const uint32_t n = size(), emit = par_.emit_ticks, phase = (uint32_t)(c_ % emit);
    const uint32_t n_emit = (uint32_t)(((uint64_t)phase + n_ticks) / emit);
    uint32_t max_touched = 1, max_done = 0;
    for (const Domain& d : dom_) {
        if (!d.frames) continue;
        const uint64_t pos = d.pos0 + ticks0_ * d.frames, end = pos + (uint64_t)n_ticks * d.frames, H = par_.hop_frames;
        max_touched = std::max(max_touched, (uint32_t)((end - 1) / H - pos / H + 1));
        max_done = std::max(max_done, (uint32_t)(end / H - pos / H));
    }
    uint64_t* part = (uint64_t*)state_.p; uint32_t* amp = (uint32_t*)(part + 2 * (size_t)n); uint32_t* bad = amp + 2 * (size_t)n;
    uint32_t* lin = (uint32_t*)lin_.p; const size_t lin_words = (size_t)n * lin_stride_;
    const uint32_t cur = flip_hist();
    uint32_t log2_hop = 6; while ((1u << log2_hop) < par_.hop_frames) ++log2_hop;
    run_ = TempoRun{(const TempoDesc*)desc.p, n, n_ticks, n, log2_hop, par_.window_hops, par_.max_lag, emit, phase, n_emit, ticks0_, max_touched, max_done,
                    lin_stride_, e_stride_, lin + (size_t)cur * lin_words, lin + (size_t)(cur ^ 1u) * lin_words, (uint64_t*)energy_.p,
                    part + (size_t)cur * n, part + (size_t)(cur ^ 1u) * n, amp + (size_t)cur * n, amp + (size_t)(cur ^ 1u) * n, bad,
                    (uint32_t*)rec.p, 8u + 2u * par_.max_lag};
    c_ += n_ticks; ticks0_ += n_ticks; n_rec_ = n_emit; run_seen_ = true;
}

size_t TempoTaps::read_records(void* dst, size_t cap_bytes) {
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    if (empty()) throw Error(MX_ERR_INVALID, "no tempo taps are set");
    if (!run_seen_) throw Error(MX_ERR_INVALID, "no run since the tempo taps were set");
    const size_t count = (size_t)n_rec_ * ports.size(), bytes = count * tempo_record_bytes(par_.max_lag);
    if (cap_bytes < bytes) throw Error(MX_ERR_INVALID, "cap_bytes is smaller than emissions x taps x record bytes");
    if (bytes && !dst) throw Error(MX_ERR_INVALID, "dst is NULL");
    if (bytes) {
        host_.join_tail();
        hip_check(hipMemcpyAsync(dst, rec.p, bytes, hipMemcpyDeviceToHost, host_.stream()), "hipMemcpyAsync(D2H)");
        host_.sync();
    }
    return count;
}

// ---- tonality taps ----

static const char* const TON_PARAMS_MSG = "mx_tonality_params: decim must be 4 or 8, hop_frames 128, 256 or 512, octaves 2 .. 6, f_lo_mhz >= 1, emit_ticks >= 1";

// the tables' refusals as errors (tonality_tables' codes)
static void tonality_tables_check(int rc) {
    if (rc == 1) throw Error(MX_ERR_INVALID, "tonality: the lowest bin's kernel, ceil(17 fs_d / f_lo), exceeds 2048 decimated frames (raise f_lo_mhz or decim)");
    if (rc == 2) throw Error(MX_ERR_INVALID, "tonality: the highest bin reaches 0.45 fs_d, the decimator's cutoff (fewer octaves, a lower f_lo_mhz or decim 4)");
    if (rc) throw Error(MX_ERR_INVALID, "tonality: no tables at this rate");
}

void TonalityTaps::set(const mx_port_ref* ports_, size_t n, const mx_tonality_params* params) {
    set_taps(ports_, n, params, [&] {
        if (n && !tonality_params_ok(params->decim, params->hop_frames, params->octaves, params->f_lo_mhz, params->emit_ticks)) throw Error(MX_ERR_INVALID, TON_PARAMS_MSG);
        check_ports(ports_, n, [&](size_t, const TapPort& t) {   // the kernels must exist at the port's own rate
            int16_t fir[64]; uint32_t len[72];
            tonality_tables_check(tonality_tables(host_.sample_rate() * t.dom_num / t.dom_den, params->decim, params->octaves, params->f_lo_mhz, fir, len, nullptr, nullptr));
        });
        if (n) room(host_.tap_fpc(), n, *params);   // (throws before anything changed)
    }, [&] {
        par_ = *params;
        // every tap's stream starts at frame 0 with nothing carried, c = 0; the decimated arrays are sized and zeroed by the upload that follows
        const uint32_t B = 12 * par_.octaves;
        alloc_zeroed(qt_, 2 * n * (size_t)ton_qtail(par_.decim) * sizeof(int16_t), "hipMemsetAsync(tonality tail)");
        alloc_zeroed(hops_, 2 * n * sizeof(uint32_t), "hipMemsetAsync(tonality hops)");
        alloc_zeroed(acc_, n * ((size_t)B * sizeof(uint64_t) + sizeof(uint32_t)), "hipMemsetAsync(tonality sums)");
    });
}

size_t TonalityTaps::room(size_t fpc, size_t n, const mx_tonality_params& p) const {
    const size_t max_ticks = std::max<size_t>(1, host_.cap_frames() / fpc), cap = (max_ticks + p.emit_ticks - 1) / p.emit_ticks;
    if ((unsigned __int128)cap * n * tonality_record_bytes(p.octaves) > ((unsigned __int128)4 << 30))
        throw Error(MX_ERR_NOMEM, "tonality: the records of one run (ceil(max_ticks_per_run / emit_ticks) x taps x record bytes) exceed 4 GiB: raise emit_ticks");
    return cap;
}

// beside the descriptors: every rate domain's stream position so far and its table set (made when the domain is first seen: the rate of a
// domain never changes), room for the run's records, and the decimated arrays -- whose length depends on the frames of the longest run the
// graph has room for, so a graph that has grown moves the carried frames into arrays of the new length
void TonalityTaps::upload(size_t fpc) {
    const size_t n = ports.size();
    const size_t need_rec = room(fpc, n, par_) * n * tonality_record_bytes(par_.octaves);
    const uint32_t hist = ton_dhist(par_.hop_frames), B = 12 * par_.octaves, Tf = 8 * par_.decim;
    for (Domain& d : dom_) { d.pos0 += ticks0_ * d.frames; d.frames = 0; }
    ticks0_ = 0;
    const size_t n_dom = dom_.size();
    uint64_t most = 0;
    for (size_t i = 0; i < n; ++i) {
        const TapPort t = port(i);
        auto it = std::find_if(dom_.begin(), dom_.end(), [&](const Domain& d) { return d.num == t.dom_num && d.den == t.dom_den; });
        if (it == dom_.end()) it = dom_.insert(dom_.end(), Domain{t.dom_num, t.dom_den, 0, 0});
        it->frames = fpc * t.dom_num / t.dom_den;
        if (it->frames > LIMIT_MAX_FRAMES) throw Error(MX_ERR_INVALID, "tonality: a tick of more than 2^30 frames");
        // a run of the most frames, which starts anywhere between two decimated frames
        most = std::max<uint64_t>(most, (uint64_t)((unsigned __int128)host_.cap_frames() * t.dom_num / t.dom_den / par_.decim) + 1);
    }
    if (most + hist > 0x7fffffffu) throw Error(MX_ERR_NOMEM, "tonality: the decimated frames of one run exceed the device");
    if (dom_.size() != n_dom || !tab_.p) {   // a table set per domain, each padded to the longest
        std::vector<std::vector<int16_t>> kern(dom_.size());
        std::vector<std::vector<uint32_t>> len(dom_.size(), std::vector<uint32_t>(B));
        std::vector<int16_t> fir(dom_.size() * Tf);
        size_t most_pairs = 0;
        for (size_t k = 0; k < dom_.size(); ++k) {
            const double rate = host_.sample_rate() * dom_[k].num / dom_[k].den;
            size_t pairs = 0;
            tonality_tables_check(tonality_tables(rate, par_.decim, par_.octaves, par_.f_lo_mhz, fir.data() + k * Tf, len[k].data(), nullptr, &pairs));
            kern[k].resize(2 * pairs);
            tonality_tables(rate, par_.decim, par_.octaves, par_.f_lo_mhz, fir.data() + k * Tf, len[k].data(), kern[k].data(), &pairs);
            most_pairs = std::max(most_pairs, pairs);
        }
        const size_t head = Tf * sizeof(int16_t) + 2 * (size_t)B * sizeof(uint32_t), stride = head + most_pairs * 2 * sizeof(int16_t);
        std::vector<unsigned char> tab(dom_.size() * stride, 0);
        for (size_t k = 0; k < dom_.size(); ++k) {
            unsigned char* at = tab.data() + k * stride;
            std::memcpy(at, fir.data() + k * Tf, Tf * sizeof(int16_t));
            std::memcpy(at + Tf * sizeof(int16_t), len[k].data(), B * sizeof(uint32_t));
            std::vector<uint32_t> off(B, 0);
            for (uint32_t b = 1; b < B; ++b) off[b] = off[b - 1] + len[k][b - 1];
            std::memcpy(at + Tf * sizeof(int16_t) + B * sizeof(uint32_t), off.data(), B * sizeof(uint32_t));
            std::memcpy(at + head, kern[k].data(), kern[k].size() * sizeof(int16_t));
        }
        tab_.alloc(tab.size());
        hip_check(hipMemcpy(tab_.p, tab.data(), tab.size(), hipMemcpyHostToDevice), "hipMemcpy(tonality tables)");
        tab_stride_ = (uint32_t)stride;
    }
    const uint32_t lin_stride = ((uint32_t)most + hist + 1u) & ~1u;
    if (lin_stride != lin_stride_) {
        DevBuf lin;
        alloc_zeroed(lin, 2 * n * (size_t)lin_stride * sizeof(int16_t), "hipMemsetAsync(tonality decimated frames)");
        if (lin_.p)   // the carried frames: the front of each tap's array in the buffer the next run reads
            hip_check(hipMemcpy2DAsync((int16_t*)lin.p + (size_t)hist_cur_ * n * lin_stride, (size_t)lin_stride * sizeof(int16_t),
                                       (const int16_t*)lin_.p + (size_t)hist_cur_ * n * lin_stride_, (size_t)lin_stride_ * sizeof(int16_t),
                                       (size_t)hist * sizeof(int16_t), n, hipMemcpyDeviceToDevice, host_.stream()), "hipMemcpy2DAsync(tonality decimated frames)");
        hip_check(hipStreamSynchronize(host_.stream()), "hipStreamSynchronize");
        lin_ = std::move(lin); lin_stride_ = lin_stride;
    }
    const std::vector<TapDesc> t = tap_descs(fpc);
    std::vector<TonDesc> d(t.size());
    for (size_t k = 0; k < t.size(); ++k) {
        const TapPort tp = port(t[k].slot);
        const auto dm = std::find_if(dom_.begin(), dom_.end(), [&](const Domain& x) { return x.num == tp.dom_num && x.den == tp.dom_den; });
        d[k] = TonDesc{t[k].p, t[k].frames, t[k].layout, t[k].slot, (uint32_t)(dm - dom_.begin()), dm->pos0};
    }
    upload_tap_descs(d.data(), d.size() * sizeof(TonDesc), fpc, 0);
    if (rec.bytes < need_rec) rec.alloc(need_rec);
}

// Each run reads the quantised tail, the decimated array and the hop count the previous one wrote (they flip once per run).  The emission
// schedule, every decimated frame and every hop follow from frame counts alone: the counter c and the stream positions live on the host, and
// the run's phase, emissions and grid sizes are launch arguments.
void TonalityTaps::begin_run(uint32_t n_ticks) {
    const uint32_t n = size(), emit = par_.emit_ticks, phase = (uint32_t)(c_ % emit), B = 12 * par_.octaves;
    const uint32_t n_emit = (uint32_t)(((uint64_t)phase + n_ticks) / emit);
    uint32_t max_groups = 0, max_hops = 0;
    const uint64_t D = par_.decim, Hc = par_.hop_frames;
    for (const Domain& d : dom_) {
        if (!d.frames) continue;
        const uint64_t pos = d.pos0 + ticks0_ * d.frames, run = (uint64_t)n_ticks * d.frames, end = pos + run;
        max_groups = std::max(max_groups, (uint32_t)((run + D - 1) / D));
        max_hops = std::max(max_hops, (uint32_t)((end + D - 1) / D / Hc - (pos + D - 1) / D / Hc));
    }
    const uint32_t cur = flip_hist(), QT = ton_qtail(par_.decim);
    int16_t* qt = (int16_t*)qt_.p; int16_t* lin = (int16_t*)lin_.p; uint32_t* hops = (uint32_t*)hops_.p;
    const size_t qt_words = (size_t)n * QT, lin_words = (size_t)n * lin_stride_;
    uint32_t log2_d = 2; while ((1u << log2_d) < par_.decim) ++log2_d;
    uint32_t log2_hop = 7; while ((1u << log2_hop) < par_.hop_frames) ++log2_hop;
    run_ = TonRun{(const TonDesc*)desc.p, n, n_ticks, n, log2_d, log2_hop, B, emit, par_.f_lo_mhz, phase, n_emit, ticks0_, max_groups, max_hops, lin_stride_,
                  qt + (size_t)cur * qt_words, qt + (size_t)(cur ^ 1u) * qt_words, lin + (size_t)cur * lin_words, lin + (size_t)(cur ^ 1u) * lin_words,
                  hops + (size_t)cur * n, hops + (size_t)(cur ^ 1u) * n, (uint64_t*)acc_.p, (uint32_t*)((uint64_t*)acc_.p + (size_t)n * B),
                  (const unsigned char*)tab_.p, tab_stride_, (uint32_t*)rec.p, 8u + 2u * B};
    c_ += n_ticks; ticks0_ += n_ticks; n_rec_ = n_emit; run_seen_ = true;
}

size_t TonalityTaps::read_records(void* dst, size_t cap_bytes) {
    hip_check(hipSetDevice(host_.device()), "hipSetDevice");
    if (empty()) throw Error(MX_ERR_INVALID, "no tonality taps are set");
    if (!run_seen_) throw Error(MX_ERR_INVALID, "no run since the tonality taps were set");
    const size_t count = (size_t)n_rec_ * ports.size(), bytes = count * tonality_record_bytes(par_.octaves);
    if (cap_bytes < bytes) throw Error(MX_ERR_INVALID, "cap_bytes is smaller than emissions x taps x record bytes");
    if (bytes && !dst) throw Error(MX_ERR_INVALID, "dst is NULL");
    if (bytes) {
        host_.join_tail();
        hip_check(hipMemcpyAsync(dst, rec.p, bytes, hipMemcpyDeviceToHost, host_.stream()), "hipMemcpyAsync(D2H)");
        host_.sync();
    }
    return count;
}

}  // namespace mx
