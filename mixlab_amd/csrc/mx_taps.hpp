// mx_taps.hpp -- the audio tap sets: level meters, spectrum, loudness, stereo field, limiter, tempo and tonality taps on audio output ports (mixlab_gpu.h
// mx_graph_set_meters, _spectra, _loudness, _stereo, _limiters, _tempo, _tonality; DESIGN.md sections 0.2, 0.3, 0.5, 0.6, 0.8, 0.9, 0.10).  What the seven share is
// written once, in AudioTapSet; a set is one subclass that holds its own state, and one entry of Graph's list of sets (mx_engine.hpp), which
// fixes the launch order.  The kernels, descriptors and run structs are mx_kernels.hpp's.
#pragma once
#include <functional>
#include <vector>

#include "mx_common.hpp"
#include "mx_kernels.hpp"

namespace mx {

struct VOut;   // mx_video_graph.hpp

// One output port as a tap sees it ...
struct TapPort {
    uint8_t type = 0;                        // mx_line
    bool dup = false, elided = false;        // stereo with L == R stored as one float per frame; not materialised (it only feeds a fused consumer)
    bool on_tail = false;                    // the second-stream mode is on and the launch that writes the port belongs to the tail
    uint32_t dom_num = 1, dom_den = 1;       // the port's rate domain relative to the graph's rate
    const float* p[2] = {nullptr, nullptr};  // the port at tick 0 of the run, by buffer parity (the second only differs for a port the tail reads)
};
// ... and, with it, everything a tap set reads of its graph or asks of it: the whole coupling.  Graph implements it.
struct TapHost {
    virtual bool tap_port(mx_port_ref r, TapPort& t) const = 0;   // false: there is no such output terminal
    virtual size_t tap_fpc() const = 0;      // frames per call every set's descriptors are built for (the tick length until a run says otherwise)
    virtual size_t cap_frames() const = 0;   // the most frames of one run
    virtual double sample_rate() const = 0;
    virtual hipStream_t stream() const = 0;
    virtual int device() const = 0;
    virtual void sync() = 0;                 // everything queued is done, a held-back tail launch included
    virtual void join_tail() = 0;            // stream() waits for the tail launches that have not been waited for, a held-back one released first
    // what the taps on video ports ask beside (mx_video_graph.hpp)
    virtual size_t spt() const = 0;                               // base-rate frames per tick
    virtual int out_line(mx_port_ref r) const = 0;                // the mx_line of an output terminal, -1: there is no such terminal
    virtual const VOut& video_out(mx_port_ref r) const = 0;       // the frame of the tick being run on a video output terminal
};

// One audio tap set: the taps in set order (= record slots).  Launch order puts the taps read on the graph's stream first (n_head of them),
// then the taps on outputs of the tail (behind the Mixer bank on its stream while the second-stream mode is on).  desc: the descriptors
// [2][n] in launch order, one row per buffer parity; rec: the records [max ticks][n].  tag, noun, no_type: how the messages name the set
struct AudioTapSet {
    const char* tag; const char* noun; const char* no_type;
    bool stereo_only = false;               // the ports must be stereo (else: anything but video)
    std::vector<mx_port_ref> ports;
    uint32_t n_head = 0;
    uint32_t run_ticks = 0;                 // ticks of the last run that measured the current taps (0: none since they were set)
    DevBuf desc, rec;
    bool empty() const { return ports.empty(); } uint32_t size() const { return (uint32_t)ports.size(); }

    // each set's own part.  upload: the descriptors, and what it uploads or sizes beside them (the ports moved, or the call length did), on a
    // quiescent stream.  begin_run: the run struct of a run of n_ticks ticks, with whatever flips or counts once per run; launch: taps
    // [from, from + n) in launch order of that run, through the descriptors of one buffer parity.  clear: no taps, nothing held.
    // The run struct stays as begin_run left it until the next run's: a part held back with the tail is launched from it later (there is only
    // ever one held-back tail, released before the next is collected).
    virtual void upload(size_t fpc) = 0;
    virtual void begin_run(uint32_t n_ticks) = 0;
    virtual void launch(uint32_t from, uint32_t n, uint32_t parity, hipStream_t s) const = 0;
    virtual void clear() = 0;
    virtual void empty_run() { run_ticks = 0; }   // a run of zero ticks happened
    // ticks [first, first + n) of the last run's records (the set's own record type), cap counted in items of item_bytes
    void read(uint32_t first, uint32_t n, void* dst, size_t cap);

protected:
    AudioTapSet(TapHost& host, const char* tag_, const char* noun_, const char* no_type_, size_t item_bytes, const char* cap_what, bool stereo_only_ = false)
        : tag(tag_), noun(noun_), no_type(no_type_), stereo_only(stereo_only_), host_(host), item_bytes_(item_bytes), cap_what_(cap_what) {}
    ~AudioTapSet() = default;
    void clear_shared() { ports.clear(); n_head = run_ticks = hist_cur_ = 0; desc.free_(); rec.free_(); }
    uint32_t flip_hist() { hist_cur_ ^= 1u; return hist_cur_ ^ 1u; }   // of a history kept twice: the buffer this run reads (it writes the other); once per run
    void alloc_zeroed(DevBuf& b, size_t bytes, const char* what);      // ... queued on the stream (set_taps waits for it)
    void check_ports(const mx_port_ref* ports_, size_t n, const std::function<void(size_t, const TapPort&)>& own_check = nullptr) const;
    TapPort port(size_t i) const { TapPort t; (void)host_.tap_port(ports[i], t); return t; }   // of tap i (checked when it was set)
    std::vector<TapDesc> tap_descs(size_t fpc);     // launch order and n_head; TapDesc[2][n] in launch order, one row per buffer parity
    void upload_tap_descs(const void* d, size_t bytes, size_t fpc, size_t tick_bytes);   // ... to the device, and room for a whole submission's records

    // Every set's set(): the shared argument check and the set's own checks (check_ports among them) throw before anything changed; then,
    // like a read-back, the last run's launches (held-back tail included) are done with the records and whatever the set carries.  The
    // second-stream mode stays on: the taps read the ports through descriptors of both parities, in stream order with their producers
    // (Graph::launch_tap_set).  keep: what the new taps take over from the old, which are still in place; install: the set's state for the
    // new taps (ports holds them).  A throw from there on (out of device memory) leaves no taps rather than half a set.
    template <class Checks, class Install, class Keep = void (*)()>
    void set_taps(const mx_port_ref* ports_, size_t n, const void* params, Checks checks, Install install, Keep keep = [] {}) {
        hip_check(hipSetDevice(host_.device()), "hipSetDevice");
        if (n && (!ports_ || !params)) throw Error(MX_ERR_INVALID, "ports / params is NULL");
        if (n > 0xffffffu) throw Error(MX_ERR_INVALID, std::string("more than 2^24 ") + noun);
        checks();
        host_.sync();
        keep();
        clear();
        if (!n) return;
        try { ports.assign(ports_, ports_ + n); install(); hip_check(hipStreamSynchronize(host_.stream()), "hipStreamSynchronize"); upload(host_.tap_fpc()); }
        catch (...) { clear(); throw; }
    }

    TapHost& host_;
    uint32_t hist_cur_ = 0;
    size_t tick_bytes_ = 0, item_bytes_; const char* cap_what_;   // the records: bytes per tick (upload_tap_descs), per item, and how read's message names a cap of one run
};

// ... with the run struct of its kernels (mx_kernels.hpp: they begin alike -- desc, n, n_ticks, stride -- and launch_taps is overloaded on them)
template <class Run> struct TapSetOf : AudioTapSet {
    void launch(uint32_t from, uint32_t n, uint32_t parity, hipStream_t s) const final { Run r = run_; r.desc += (size_t)(parity & 1u) * size() + from; r.n = n; launch_taps(r, s); }
protected:
    using AudioTapSet::AudioTapSet;
    Run run_{};   // of the whole set, its descriptors those of parity 0 (begin_run)
};

// level meters (mx_graph_set_meters / mx_graph_read_meters): measured once per run after its last span.  desc: MeterDesc; rec: MeterTick;
// par_: each tap's hold_ticks and release; state_: MeterHold[n][2]
struct MeterTaps final : TapSetOf<MeterRun> {
    explicit MeterTaps(TapHost& h) : TapSetOf(h, "meter", "meters", "a video port has no level", sizeof(MeterTick), "n_ticks x meters") {}
    void set(const mx_port_ref* ports, size_t n, const mx_meter_params* params);
    void upload(size_t fpc) override; void begin_run(uint32_t n_ticks) override; void clear() override { clear_shared(); par_.clear(); state_.free_(); }
private:
    std::vector<mx_meter_params> par_; DevBuf state_;
};

// spectrum taps (mx_graph_set_spectra / mx_graph_read_spectra): a windowed transform of every tap's last n_fft frames per tick, as band
// powers.  rec: float[2][bands] per tap; hist_: float[2][n][2 * n_fft], of which a run reads one buffer and writes the other; tab_:
// window, twiddles and band edges on the device
struct SpectrumTaps final : TapSetOf<SpecRun> {
    explicit SpectrumTaps(TapHost& h) : TapSetOf(h, "spectrum", "spectrum taps", "a video port has no spectrum", sizeof(float), "n_ticks x taps x 2 x n_bands") {}
    void set(const mx_port_ref* ports, size_t n, const mx_spectrum_params* params);
    void upload(size_t fpc) override; void begin_run(uint32_t n_ticks) override; void clear() override { clear_shared(); hist_.free_(); tab_.free_(); n_fft_ = n_bands_ = 0; }
private:
    uint32_t n_fft_ = 0, n_bands_ = 0;
    DevBuf hist_, tab_;
};

// loudness taps (mx_graph_set_loudness / mx_graph_read_loudness): K-weighted energy, momentary / short-term window sums and true peak per
// tick.  rec: LoudTick; walk_: double[n][2][max ticks][4], the run's Z_k / S_k; tab_: LoudCoef[n] by slot, then interp[36]; carry_: what a
// run hands to the next -- state double[n][2][4] | window history double[2][n][1023] | frame history float[2][n][2][11], of which a run
// reads one buffer and writes the other
struct LoudnessTaps final : TapSetOf<LoudRun> {
    explicit LoudnessTaps(TapHost& h) : TapSetOf(h, "loudness", "loudness taps", "a video port has no loudness", sizeof(LoudTick), "n_ticks x taps") {}
    void set(const mx_port_ref* ports, size_t n, const mx_loudness_params* params);
    void upload(size_t fpc) override; void begin_run(uint32_t n_ticks) override; void clear() override { clear_shared(); walk_.free_(); tab_.free_(); carry_.free_(); par_ = mx_loudness_params{0, 0}; max_ticks_ = 0; }
private:
    mx_loudness_params par_{0, 0}; uint32_t max_ticks_ = 0;
    DevBuf walk_, tab_, carry_;
};

// stereo field taps (mx_graph_set_stereo / mx_graph_read_stereo / mx_graph_read_goniometers): the sums behind correlation, balance and
// width per tick, and the goniometer.  rec: StereoTick; carry_: window history double[2][n][1023][3], of which a run reads one buffer
// and writes the other; gon_rec_: the last run's goniometer records [emission][n], gon_n_ emissions; gon_carry_: one record-shaped grid per
// tap with the ticks since the last emission.  c_ is the hop counter c (0 when the taps are set, + the ticks of every run)
struct StereoTaps final : TapSetOf<StereoRun> {
    explicit StereoTaps(TapHost& h) : TapSetOf(h, "stereo", "stereo taps", "a video or mono port has no stereo field", sizeof(StereoTick), "n_ticks x taps", true) {}
    void set(const mx_port_ref* ports, size_t n, const mx_stereo_params* params);
    size_t read_goniometers(void* dst, size_t cap_bytes);   // the last run's emitted records; returns how many
    void upload(size_t fpc) override; void begin_run(uint32_t n_ticks) override; void clear() override { clear_shared(); carry_.free_(); gon_rec_.free_(); gon_carry_.free_(); par_ = mx_stereo_params{0, 0, 0, 0}; gon_n_ = 0; c_ = 0; run_seen_ = false; }
    void empty_run() override { run_ticks = 0; gon_n_ = 0; }
private:
    size_t gon_room(size_t fpc, size_t n, uint32_t grid, uint32_t hop) const;   // goniometer records a run can emit; MX_ERR_NOMEM beyond 4 GiB
    mx_stereo_params par_{0, 0, 0, 0};
    uint32_t gon_n_ = 0; uint64_t c_ = 0; bool run_seen_ = false;
    DevBuf carry_, gon_rec_, gon_carry_;
};

// limiter taps (mx_graph_set_limiters / mx_graph_read_limiters / mx_graph_read_limited): a look-ahead peak limiter's copy of every tapped
// port, and one record per tick.  rec: LimitTick; out_: the limited copies float[max ticks][tick_floats_], a tick being every tap's frames x
// channels floats in set order (tap i's start at off_[i], floats_[i] of them); hist_: float2[2][n][LIMIT_HIST_FRAMES], of which a run reads
// one buffer and writes the other; w_: the smoothing weights; stage_: the read-backs' staging
struct LimiterTaps final : TapSetOf<LimitRun> {
    explicit LimiterTaps(TapHost& h) : TapSetOf(h, "limiter", "limiter taps", "a video port has no level to limit", sizeof(LimitTick), "n_ticks x taps") {}
    void set(const mx_port_ref* ports, size_t n, const mx_limiter_params* params);
    // ticks [first, first + n) of tap `tap`'s limited copy as f32 (dst_i16 null) or in the sinks' i16 format; both null with cap 0: the count only
    void read_limited(size_t tap, uint32_t first, uint32_t n, float* dst, int16_t* dst_i16, size_t cap, size_t* n_samples);
    float* limited_ptr(size_t tap, size_t* floats_per_tick);   // the tap's copy of tick 0 on the device; ticks are floats_per_tick apart
    void upload(size_t fpc) override; void begin_run(uint32_t n_ticks) override; void clear() override { clear_shared(); out_.free_(); hist_.free_(); w_.free_(); stage_.free_(); off_.clear(); floats_.clear(); tick_floats_ = 0; max_frames_ = 0; par_ = mx_limiter_params{0.0f, 0}; }
private:
    mx_limiter_params par_{0.0f, 0};
    uint32_t max_frames_ = 0; size_t tick_floats_ = 0; std::vector<size_t> off_, floats_;
    DevBuf out_, hist_, w_, stage_;
};

// tempo taps (mx_graph_set_tempo / mx_graph_read_tempo): the autocorrelation of an onset function, one record per tap every emit_ticks ticks.
// rec: the last run's records [emission][n], n_rec_ emissions.  state_: what a run hands to the next beside the onsets -- partial hop energy
// uint64[2][n] | A of the last complete hop uint32[2][n] | non-finite frames since the last emission uint32[n]; lin_: uint32[2][n][lin_stride_],
// a tap's W + L - 1 carried onsets and behind them the run's; of the three kept twice a run reads one buffer and writes the other.
// energy_: uint64[n][e_stride_], E of the hops a run completes.  c_ is the emission counter c (0 when the taps are set, + the ticks of every
// run).  The stream position of a tap follows from frame counts alone: dom_ holds, per rate domain of the set, the frames per tick and the
// position when the descriptors were last uploaded; ticks0_ the ticks since.
struct TempoTaps final : TapSetOf<TempoRun> {
    explicit TempoTaps(TapHost& h) : TapSetOf(h, "tempo", "tempo taps", "a video port has no tempo", 1, "emissions x taps x record bytes") {}
    void set(const mx_port_ref* ports, size_t n, const mx_tempo_params* params);
    size_t read_records(void* dst, size_t cap_bytes);   // the last run's emitted records; returns how many
    void upload(size_t fpc) override; void begin_run(uint32_t n_ticks) override;
    void clear() override { clear_shared(); state_.free_(); lin_.free_(); energy_.free_(); dom_.clear(); par_ = mx_tempo_params{0, 0, 0, 0}; n_rec_ = 0; c_ = ticks0_ = 0; lin_stride_ = e_stride_ = 0; run_seen_ = false; }
    void empty_run() override { run_ticks = 0; n_rec_ = 0; }
private:
    struct Domain { uint32_t num, den; uint64_t frames, pos0; };   // frames: per tick at the uploaded call length
    size_t room(size_t fpc, size_t n, const mx_tempo_params& p) const;   // emissions a run can have; MX_ERR_NOMEM beyond 4 GiB of records
    mx_tempo_params par_{0, 0, 0, 0};
    uint32_t n_rec_ = 0, lin_stride_ = 0, e_stride_ = 0; uint64_t c_ = 0, ticks0_ = 0; bool run_seen_ = false;
    std::vector<Domain> dom_;
    DevBuf state_, lin_, energy_;
};

// tonality taps (mx_graph_set_tonality / mx_graph_read_tonality): constant-Q magnitudes of a decimated stream, summed per bin between emissions,
// one record per tap every emit_ticks ticks.  rec: the last run's records [emission][n], n_rec_ emissions.  qt_: int16[2][n][TON_QTAIL], the newest
// quantised frames; lin_: int16[2][n][lin_stride_], a tap's TON_DHIST carried decimated frames and behind them the run's; hops_: uint32[2][n],
// hops since the last emission -- of these three a run reads one buffer and writes the other.  acc_: the sums C uint64[n][B] | non-finite frames
// uint32[n] since the last emission, updated in place.  tab_: one table set per rate domain of the set (TonRun), tab_stride_ bytes each.
// c_, dom_ and ticks0_ as for the tempo taps; a domain also holds the index of its table set.
struct TonalityTaps final : TapSetOf<TonRun> {
    explicit TonalityTaps(TapHost& h) : TapSetOf(h, "tonality", "tonality taps", "a video port has no tonality", 1, "emissions x taps x record bytes") {}
    void set(const mx_port_ref* ports, size_t n, const mx_tonality_params* params);
    size_t read_records(void* dst, size_t cap_bytes);   // the last run's emitted records; returns how many
    void upload(size_t fpc) override; void begin_run(uint32_t n_ticks) override;
    void clear() override { clear_shared(); qt_.free_(); lin_.free_(); hops_.free_(); acc_.free_(); tab_.free_(); dom_.clear(); par_ = mx_tonality_params{0, 0, 0, 0, 0}; n_rec_ = 0; c_ = ticks0_ = 0; lin_stride_ = tab_stride_ = 0; run_seen_ = false; }
    void empty_run() override { run_ticks = 0; n_rec_ = 0; }
private:
    struct Domain { uint32_t num, den; uint64_t frames, pos0; };   // frames: per tick at the uploaded call length; the index in dom_ is the table set's
    size_t room(size_t fpc, size_t n, const mx_tonality_params& p) const;   // emissions a run can have; MX_ERR_NOMEM beyond 4 GiB of records
    mx_tonality_params par_{0, 0, 0, 0, 0};
    uint32_t n_rec_ = 0, lin_stride_ = 0, tab_stride_ = 0; uint64_t c_ = 0, ticks0_ = 0; bool run_seen_ = false;
    std::vector<Domain> dom_;
    DevBuf qt_, lin_, hops_, acc_, tab_;
};

}  // namespace mx
