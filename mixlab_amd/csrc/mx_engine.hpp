// mx_engine.hpp -- device-resident graph executor (internal C++ API behind include/mixlab_gpu.h).
//
// Mirrors what Engine::run_tick (reference src/engine.rs:400-510) does per tick -- topological
// order, fresh outputs, Disconnected => zeros, t = tick * SPT -- but freezes the topology once,
// keeps every port buffer resident in one HBM slab, batches all instances of a module kind at one
// dependency level into one launch, and runs n_ticks ticks per submission.
#pragma once
#include <algorithm>
#include <array>
#include <atomic>
#include <functional>
#include <hip/hip_runtime.h>

#include <cstdint>
#include <memory>
#include <string>
#include <deque>
#include <vector>

#include "mx_common.hpp"
#include "mx_kernels.hpp"
#include "mx_plan.hpp"
#include "mx_taps.hpp"
#include "mx_video.hpp"
#include "mx_video_graph.hpp"

namespace mx {

// OUTPUT_DEVICE (output_device.rs): what the module carries from run to run, held by the nodes of that kind only.  Every call below wants a quiescent stream.
struct OutputDeviceState {
    // the open stream's channel count (0: none), the stored left / right (filtered; -1: None), the largest channel count seen (what the
    // buffers are sized for) and the input's frames per tick
    uint32_t channels = 0, cmax = 0; int32_t left = -1, right = -1; const uint32_t frames;
    DevBuf scratch;                 // the persistent scratch: frames * cmax floats, only ever grows (:185)
    DevBuf state;                   // OutState
    DevBuf out, rec, part;          // the last run's hand-off, per-tick records (OutTick) and the route kernel's clip partials
    std::atomic<bool> lag{false};   // set by the cpal callback (mx_graph_audio_out_lag), swapped by the next run
    bool lag_run = false;           // ... taken by the current run
    struct Span { uint32_t first, n, channels; };
    std::vector<Span> spans;        // the last run's spans, in order (the hand-off is their ticks back to back)
    // `ticks`: the ticks of a whole submission, what the per-run buffers are sized for
    OutputDeviceState(uint32_t frames_per_tick, size_t ticks);                    // the empty state (no stream, nothing assigned)
    void grow(uint32_t channels, size_t ticks, hipStream_t stream);               // buffers for a channel count above any seen before
    void update(const void* params, size_t ticks, hipStream_t stream);            // ModuleT::update (output_device.rs:152-169) with mx_output_device_params
    size_t offset(uint32_t tick) const;                                           // float offset of tick `tick` of the last run in the hand-off
    void adopt(OutputDeviceState& old, size_t ticks, hipStream_t stream);         // a topology edit: the module persists
};

// A node of a built graph: what the compiler said about it (mx_plan.hpp; Graph rewrites in_src alone, in set_input_enabled), where layout_slab put
// its ports, and the state it carries while the graph runs.
struct Node : PlanNode {
    std::vector<uint8_t> params;
    std::vector<size_t> out_off;              // float offset of each output port in the slab (layout_slab)
    std::vector<size_t> out_off2;             // MX_FLAG_OVERLAP_TAIL: second buffer of a port the tail group reads (SIZE_MAX: none); dropped when the mode ends
    const float* bound = nullptr;             // SOURCE_*: caller-bound device buffer
    std::vector<uint8_t> parked;              // the carried state of a module no launch of this graph serves (it is outside the run order): kept on the host from one topology edit to the next
    // parameter updates queued for ticks inside the next run (Engine::client_update between two ticks, src/engine.rs:192-214)
    struct SchedEv { uint32_t tick; std::vector<uint8_t> params; };
    std::vector<SchedEv> sched;
    std::vector<std::pair<uint32_t, uint32_t>> gate_sched;   // Trigger: (tick, gate_open) -- a bench step queues ~70 000 of these, no allocation each
    // plotter
    uint64_t plot_count = 0;
    std::vector<uint8_t> plot_fired;          // per call of the last run
    std::vector<int32_t> plot_slot;           // staging slot per call (-1 = not fired)
    // video nodes (run tick by tick inside Graph::run): each kind's state is an object of its own (mx_video_graph.hpp), held by the nodes of that kind only
    using VOut = mx::VOut;
    using MonTick = MonitorState::Tick;
    std::unique_ptr<VideoMixer> vmixer;       // VIDEO_MIXER
    std::vector<VOut> vout;                   // this tick's video outputs (empty FrameRef = None)
    std::unique_ptr<VideoSourceState> vsrc;   // SOURCE_VIDEO
    std::unique_ptr<RgbaSinkState> rgba;      // VIDEO_TO_RGBA
    std::unique_ptr<MonitorState> mon;        // MONITOR
    std::unique_ptr<OutputDeviceState> od;    // OUTPUT_DEVICE
    explicit Node(const PlanNode& p) : PlanNode(p) {}
};

struct Group : PlanGroup {
    uint32_t max_taps = 0;   // Fir / Resample: most taps; Mixer: most channels
    uint32_t rs_common_taps = 0, rs_common_down = 0;   // ... and their taps per phase / decimation factor, likewise
    uint32_t rs_common_up = 0;   // Resample: the nodes' interpolation factor when they all have the same (the staged kernel's table stride becomes a constant)
    uint32_t rs_tab_doubles = 0, rs_win_frames = 0;   // Resample: LDS plan of the staged kernel (largest table / input window of the group)
    DevBuf desc;     // kind-specific descriptor array
    DevBuf desc_alt, extra_alt;   // MX_FLAG_OVERLAP_TAIL: the same for the other parity of the double-buffered ports (extra_alt: Mixer only)
    DevBuf state;    // EnvState[] / EqState[]
    DevBuf extra;    // Mixer: MixChan arrays
    DevBuf state2;   // EqThree: EnvState[] of Envelopes folded into the epilogue
    int dup_mode = 0; // Mixer: 0 no input stored mono-dup, 1 all, 2 mixed
    // Trigger gates per tick of the run (GateBits rows, one per node of the group): Trigger groups, Envelope groups with a folded
    // Trigger, EqThree groups with a folded Envelope.  Re-uploaded only when a gate, a schedule or the run length changed.
    bool has_gates = false;
    DevBuf gates; uint32_t gate_words = 0; uint64_t gates_version = ~0ull; uint32_t gates_calls = 0;
    DevBuf tick_desc;   // EqThree: EnvTickDesc[] of the folded Envelopes
    DevBuf env_ticks;   // EqThree: EnvTick[n][n_calls] of the current launch
    DevBuf spec;        // EqThree: chunk records of the speculative exact kernel; Envelope: marker bitmaps and per-segment states of a long stream (mx_k_envelope.hip)
    int eq_mode = -1;   // EqThree: the one epilogue every instance has (eq_epilogue_mode), or -1 when they differ
    explicit Group(const PlanGroup& g) : PlanGroup(g) {}
};

class Graph final : public TapHost {
public:
    Graph(const mx_node* nodes, size_t n_nodes, const mx_edge* edges, size_t n_edges, const mx_graph_opts& opts,
          size_t cap_frames_override = 0);
    ~Graph();

    double sample_rate() const override { return sample_rate_; }
    size_t cap_frames() const override { return cap_frames_; }
    const std::vector<uint32_t>& run_order() const { return plan_.order; }
    hipStream_t stream() const override { return stream_; }
    // what a deck takes for "the same graph": unique per built graph, and taken over by the graph that adopts this one's state (a topology edit)
    uint64_t lineage() const { return lineage_; }
    int device() const override { return device_; }
    uint32_t ticks_per_second() const { return tps_; }
    hipStream_t tail_stream() { if (tail_gi_ >= 0) flush_deferred_tail(false); return tail_gi_ >= 0 ? tail_stream_ : nullptr; }   // MX_FLAG_OVERLAP_TAIL; asking for it releases a held tail launch: what the caller orders after the stream then includes the last run's
    // debug: the chunk records of the first EqThree group's last speculative launch (device pointer, bytes; nullptr when there is none)
    void* debug_eq_records(size_t* bytes) const;
    void join_tail() override { if (tail_gi_ >= 0) wait_tail(-1); }   // the graph's stream waits for a Mixer bank still running on the tail stream (consumers that read the buses on stream())
    size_t n_nodes() const { return nodes_.size(); }
    bool eq_exact() const { return (flags_ & MX_FLAG_EQ_EXACT) || !(flags_ & MX_FLAG_EQ_FAST); }   // the default is the reference's order
    bool fp_contract() const { return (flags_ & MX_FLAG_FP_CONTRACT) != 0; }                       // the contracted order (mixlab_gpu.h)
    const Node& node(uint32_t i) const { return nodes_.at(i); }

    void update_params(uint32_t node, const void* params, size_t len);
    // ModuleT::update at the boundary before tick `tick_in_run` of the NEXT run (client_update between ticks, src/engine.rs:192-214)
    void schedule_params(uint32_t node, uint32_t tick_in_run, const void* params, size_t len);
    void check_schedule(uint32_t node, const void* params, size_t len) const;   // schedule_params' validation alone
    void drop_schedules();                                                      // forget every queued update (a run that failed must not leave them for the next)
    // counters of the speculative exact EqThree kernel since the graph was built: [0] chunks run, [1] chunks the repair pass had to re-run
    void eq_spec_stats(uint64_t out[8]);   // see k_eq_three_repair
    void write_source(uint32_t node, const float* host, size_t frames);
    void bind_source(uint32_t node, const void* dev);
    // n_calls ModuleT::run_tick calls of frames_per_call mono samples each, back to back
    void run(uint64_t t0, size_t frames_per_call, uint32_t n_calls, float* ms_by_kind = nullptr, float* ms_total = nullptr);
    void sync() override;
    // accumulate per-group hipEvent timings across runs without synchronising (bench: kernel time over the timed region)
    void profile_enable(bool on);
    uint32_t profile_collect(float* ms_by_kind, float* ms_total);   // syncs; returns number of runs collected
    void read_output(uint32_t node, uint32_t port, float* host, size_t frames, size_t first_frame = 0);   // frames [first_frame, first_frame + frames) of the last run
    // OUTPUT_DEVICE: ticks [first, first + n) of the last run (mx_graph_read_audio_out); samples / ticks may be null
    void read_audio_out(uint32_t node, uint32_t first, uint32_t n, float* samples, size_t samples_cap, OutTick* ticks, size_t* n_samples);
    void audio_out_lag(uint32_t node);
    // the audio tap sets (mx_taps.hpp): taps on audio output ports, measured once per run after its last span
    MeterTaps& meters() { return meters_; } SpectrumTaps& spectra() { return spectra_; } LoudnessTaps& loudness() { return loudness_; }
    StereoTaps& stereo() { return stereos_; } LimiterTaps& limiters() { return limiters_; } TempoTaps& tempo() { return tempos_; } TonalityTaps& tonality() { return tonalities_; }
    bool tap_port(mx_port_ref r, TapPort& t) const override; size_t tap_fpc() const override { return tap_fpc_; }   // (TapHost: with the accessors marked override, all a set sees of the graph)
    // the taps on video ports (mx_video_graph.hpp): the scope taps and the multiviewer, measured tick by tick inside the run
    VideoScopeTaps& video_scopes() { return scopes_; } MultiviewTap& multiview() { return multiview_; }
    size_t spt() const override { return spt_; }
    int out_line(mx_port_ref r) const override { return r.node < nodes_.size() && r.port < nodes_[r.node].out_type.size() ? (int)nodes_[r.node].out_type[r.port] : -1; }
    const VOut& video_out(mx_port_ref r) const override { return nodes_[r.node].vout[r.port]; }
    void read_output_i16(uint32_t node, uint32_t port, int16_t* host, size_t frames);   // sink hand-off format
    void write_source_i16(uint32_t node, const int16_t* host, size_t frames);            // ingest format
    float* output_ptr(uint32_t node, uint32_t port, size_t* floats_per_tick, bool stream_ordered_consumer = true /* false: a caller inside the library that orders itself
                      after the tail stream (mx_exchange): the automatic second-stream mode stays on */);
    // A Mixer bank of the last run that is being held back for the next run's EqThree launch (flush_deferred_tail)?  `hook` then runs ONCE, right after that launch has been
    // queued, with the stream it was queued on -- what mx_exchange uses to pack the buses behind the bank instead of joining the streams.
    bool tail_held() const { return deferred_.pending; }
    void tail_releases(uint64_t* gated, uint64_t* at_once) const { if (gated) *gated = n_gated_; if (at_once) *at_once = n_at_once_; }
    void eq_launch(uint32_t out[5]) const { for (int k = 0; k < 5; ++k) out[k] = eq_launch_[k]; }
    bool eq_env_rows();   // mx_graph_debug_eq_env_rows (synchronises)
    uint32_t eq_lean();   // mx_graph_debug_eq_lean (synchronises)
    void set_tail_hook(std::function<void(hipStream_t)> hook) { tail_hook_ = std::move(hook); }
    // The NEXT run's first launch waits for `ev` (once).  What mx_exchange asks for its collectives and its combine of step k, which went out behind the bank that run k + 1
    // released: they normally end inside run k + 1's EqThree launch; when the bank outlasts that launch they would run into run k + 2's EqThree workgroups being placed --
    // thousands of small workgroups around which the dispatcher places those unevenly (every other launch 6.1 instead of 4.7 ms, rocprofv3 --kernel-trace).
    void wait_before_next_run(hipEvent_t ev) { head_waits_.push_back(ev); }
    void forget_wait_before_next_run(hipEvent_t ev) { head_waits_.erase(std::remove(head_waits_.begin(), head_waits_.end(), ev), head_waits_.end()); }   // (its owner is going away; other owners' waits stay)
    int read_plotter(uint32_t node, uint32_t call, float* left, float* right);
    void ensure_capacity(size_t frames);   // module compat path: grow the slab (state is kept)
    // topology edit (client_update, src/engine.rs:277-398): modules persist while the connection set changes.
    // Takes over the carried state of every surviving module: old_of_new[i] = node of `old` that is node i here, or -1.
    void adopt_state(Graph& old, const int32_t* old_of_new, size_t n);
    // per-module time of the last profiled run in the reference's PerformanceInfo shape (src/engine/timing.rs:46-60)
    struct Perf { bool realtime; int lag; uint32_t tick_rate; uint64_t tick_budget_us, engine_us; };
    Perf performance_info(uint64_t* module_us, size_t cap);
    // module compat path: an InputRef may be Disconnected on one call and connected on the next
    void set_input_enabled(uint32_t node, uint32_t port, bool enabled);
    // video nodes
    void set_video_source(uint32_t node, DFrame* frame, Rational dur, Rational off, bool repeat);
    void set_video_source_band(uint32_t node, uint32_t in_w, uint32_t in_full_h, uint32_t src_row0, uint32_t slice_rows, uint32_t full_w, uint32_t full_h, uint32_t row0, uint32_t band_rows);
    void set_video_source_ring(uint32_t node, DFrame* const* frames, size_t n, Rational dur, Rational off);
    void set_video_source_key(uint32_t node, const mx_video_key_params* params);   // nullptr removes
    void set_video_source_place(uint32_t node, const mx_video_place_params* params);   // nullptr removes
    void set_video_source_grade(uint32_t node, const mx_video_grade_params* params, std::shared_ptr<const LutTables> lut);   // nullptr removes
    void set_video_source_matte(uint32_t node, const mx_video_matte_params* params);   // nullptr removes
    void queue_video_source(uint32_t node, uint64_t tick, DFrame* frame, Rational dur, Rational off);
    // what a feed checks BEFORE it takes frames out of a pacing state machine (a rejected feed must not lose media):
    void check_video_queue(uint32_t node, uint64_t first_tick) const;   // queue_video_source(node, first_tick, ...) would be accepted
    void check_source_write(uint32_t node, size_t frames) const;        // write_source[_i16](node, ..., frames) would be accepted
    float* source_feed_ptr(uint32_t node, size_t frames);               // ... of a SOURCE_STEREO: the buffer it would fill, for a device-side feeder that writes it on stream() (mx_deck_feed)
    const Node::MonTick& monitor_tick(uint32_t node, uint32_t tick_in_run);
    void monitor_consume(uint32_t node, uint32_t n_ticks);
    void read_monitor_audio_i16(uint32_t node, int16_t* host, uint32_t n_ticks);
    using MonitorLayout = MonitorState::Layout;
    MonitorLayout monitor_layout(uint32_t node);
    void read_monitor_video(uint32_t node, uint32_t first_tick, uint32_t n_ticks, uint8_t* frames, uint8_t* present);
    FrameRef video_output(uint32_t node, uint32_t port);
    void rgba_output(uint32_t node, void** dev, int32_t* stride, uint32_t* w, uint32_t* h);

private:
    struct StateLoc { void* p; size_t bytes; };
    std::vector<StateLoc> state_locs(uint32_t node) const;
    uint64_t lineage_ = next_lineage();
    static uint64_t next_lineage() { static std::atomic<uint64_t> n{0}; return ++n; }
    size_t state_bytes(uint32_t node) const;   // what state_locs(node) holds where a launch serves the node, from its kind and params alone
    void open_device(const mx_graph_opts& opts);     // the device, the stream, what the environment says about the kernels' forms, the EqThree tables
    void upload_eq_tables();                         // time-parallel EqThree tables (unused in MX_FLAG_EQ_EXACT mode)
    bool accept_tail();                              // the plan's overlap-tail candidate: taken (second stream and events created) or rejected (an automatic one that is not affordable)
    void layout_slab();                              // mx::layout_slab for cap_frames_, the offsets into the nodes, the slab allocated and cleared
    void build_descriptors();
    void upload_group(Group& g);          // descriptors of one group (both parities under MX_FLAG_OVERLAP_TAIL)
    void upload_group_one(Group& g, uint32_t parity);   // ... of one parity: desc / extra, or desc_alt / extra_alt
    void run_video_tick(uint64_t t, uint32_t tick_in_run);
    const Node& node_of_kind(uint32_t node, uint32_t kind, const char* what) const;   // nodes_[node], or MX_ERR_INVALID "node is not a <what>" (a kind's video state is reached through its pointer)
    // one launch sequence over ticks [call_off, call_off + n_calls) of the current run
    void run_span(uint64_t t0, size_t fpc, uint32_t call_off, uint32_t n_calls, uint32_t run_calls);
    void apply_params(uint32_t node, const void* params, size_t len);   // update_params without the synchronisation
    size_t od_ticks() const { return std::max<size_t>(1, cap_frames_ / spt_); }   // OUTPUT_DEVICE: the ticks of a whole submission
    struct ProfSpan;
    void launch_outputs(uint64_t t0, uint32_t call_off, uint32_t n_calls, ProfSpan* prof);   // the span's OutputDevice launches
    void launch_tap_set(AudioTapSet& s, uint32_t n_calls, ProfSpan* prof);   // the run's launches of one audio tap set: on stream_, or held back with the tail
    void reupload_taps(size_t fpc);                                      // every set's descriptors, tables and room again (the ports moved, or the call length did), on a quiescent stream
    void refresh_gates(Group& g, uint32_t run_calls);
    uint32_t trigger_of_row(const Group& g, uint32_t row) const;        // node id of the Trigger behind row `row` of a gated group, or ~0u
    void stage_upload(void* dst, const void* src, size_t bytes);         // H2D on the graph's stream through page-locked staging
    // a port's buffer for buffer parity `parity` (the second buffer of a double-buffered port when it is 1), from the span's first tick
    const float* in_ptr(const Node& n, uint32_t port, bool null_if_disconnected, uint32_t parity) const;
    float* out_ptr(const Node& n, uint32_t port, uint32_t parity) const;

    const Plan plan_;             // what compile_plan said, untouched: the nodes' and groups' plan parts start as copies of it
    std::vector<Node> nodes_;
    std::vector<Group> groups_;   // sorted by (level, kind)
    uint32_t flags_ = 0;
    uint32_t tps_ = 60;
    double sample_rate_ = 44100.0;
    size_t spt_ = 735;
    size_t cap_frames_ = 735;
    int device_ = 0;
    hipStream_t stream_ = nullptr;
    bool own_stream_ = false;
    DevBuf slab_;
    // MX_FLAG_OVERLAP_TAIL (see mixlab_gpu.h): the last launch group on a second stream, beside the next run's earlier groups
    int tail_gi_ = -1;                    // index of the FIRST tail group in groups_ (every group from it on is a Mixer group), -1 = mode off
    bool eq_mode_warned_ = false;         // the grouping / descriptor mode mismatch was reported (build_descriptors)
    bool tail_auto_ = false;              // the mode was chosen by the library (short submissions), not asked for with MX_FLAG_OVERLAP_TAIL
    int sin_mode_ = 0;                    // MX_SIN_MODE at build time (0: the reference's float through Ziv's strategy)
    uint32_t parity_ = 0;                 // which buffer of the double-buffered ports the current / last run uses
    hipStream_t tail_stream_ = nullptr;
    hipEvent_t ev_head_done_ = nullptr;   // recorded on stream_ when a run's earlier groups are queued
    hipEvent_t ev_tail_done_[2] = {nullptr, nullptr};   // recorded on tail_stream_ after the tail of a run (by parity)
    bool tail_pending_[2] = {false, false};
    bool overlap_this_run_ = false;
    // The tail launch of run k is HELD BACK until run k + 1 has queued its speculative EqThree launch, and goes behind a gate (k_tail_gate, one wave) that opens when that
    // launch's last workgroup has started: the next run's k_env_ticks runs alone (beside a Mixer bank it took 140 us instead of 9 and the EqThree launch behind it started
    // when the bank was nearly done: no overlap at all), the EqThree workgroups are placed on an empty chip, and the Mixer's waves fill what is left.  Every join
    // (mx_graph_sync, read-backs, mx_graph_tail_stream, an exchange's submit, a cut run) releases a held launch at once.  The measurements: profiles/r05/short_submission_regime.md.
    // The tail: every Mixer group from tail_gi_ on (a bank, or a bank and the buses above it), in order; outs: OutputDevices that read the tail's outputs, behind it;
    // taps: the audio tap sets' launches on the tail's outputs, behind those, in the sets' order.  prof: the span's profile record (nullptr: not profiled), whose tail events the release records.
    struct TailLaunch { const void* desc = nullptr; uint32_t n = 0, max_ch = 0; size_t frames = 0; int dup_mode = 0; hipEvent_t prof_ev = nullptr; };
    struct DeferredTail { bool pending = false; std::vector<TailLaunch> items; uint32_t parity = 0; ProfSpan* prof = nullptr;
                          std::vector<OutRun> outs; std::vector<AudioTapSet*> taps; } deferred_;
    std::function<void(hipStream_t)> tail_hook_;
    std::vector<hipEvent_t> head_waits_;
    uint64_t n_gated_ = 0, n_at_once_ = 0;
    DevBuf gate_flag_; uint32_t gate_seq_ = 0; bool gate_armed_ = false;
    bool gate_test_ = false;              // MX_TAIL_GATE_TEST at build time: arm the gate even for a launch that never opens it (tests of its bounded spin)
    void flush_deferred_tail(bool gated);
    void end_auto_tail();                 // the library-chosen second-stream mode ends for good (a host took a raw pointer that mode would not keep fresh)
    void wait_tail(int parity_or_all);    // stream_ waits for the tail launches that have not been waited for (-1: both)
    const void* desc_of(const Group& g) const { return (parity_ && g.desc_alt.p) ? g.desc_alt.p : g.desc.p; }
    size_t run_off_frames_ = 0;   // base-rate frames before the span being launched (a run cut at scheduled parameter updates)
    uint64_t gates_version_ = 0;  // bumped whenever a Trigger's params or schedule change
    DevBuf eq_stats_;             // [8] u64 counters of the speculative EqThree kernel's proof / repair pass
    uint32_t eq_launch_[5] = {MX_EQ_LAUNCH_NONE, 0, 0, 0, 0};   // mx_graph_debug_eq_launch: the first EqThree group's last launch
    bool eq_env_rows_ = true;             // MX_EQ_ENV_ROWS at build time (0: the inline Envelope keeps the lockstep form; A/B)
    bool eq_lean_ = true;                 // MX_EQ_LEAN at build time (0: the EqThree hot loops keep the input tracker and the multiply by an amplitude of 1.0; A/B)
    DevBuf eq_rows_flag_; uint32_t eq_rows_seq_ = 0;   // mx_graph_debug_eq_env_rows: a wave of the first EqThree group's last launch that took the row form stores the launch's number
    struct Stage { void* host = nullptr; size_t cap = 0; hipEvent_t done = nullptr; bool pending = false; };
    Stage stage_[4]; uint32_t stage_next_ = 0;
    uint32_t prof_runs_count_ = 0;
    std::vector<uint32_t> sched_nodes_;     // nodes with a pending schedule (a 60 000-node graph must not be walked per tick)
    size_t tap_fpc_ = 0;                        // frames per call every set's descriptors were built for (the tick length until a run says otherwise)
    MeterTaps meters_{*this}; SpectrumTaps spectra_{*this}; LoudnessTaps loudness_{*this}; StereoTaps stereos_{*this}; LimiterTaps limiters_{*this}; TempoTaps tempos_{*this}; TonalityTaps tonalities_{*this};
    const std::array<AudioTapSet*, 7> taps_{&meters_, &spectra_, &loudness_, &stereos_, &limiters_, &tempos_, &tonalities_};   // in launch order
    VideoScopeTaps scopes_{*this}; MultiviewTap multiview_{*this};
    float perf_od_ms_ = 0.f;                // OutputDevice launches of the last collected run
    bool prof_this_run_ = false;
    size_t plot_job_off_ = 0;
    size_t zero_off_ = 0;
    size_t slab_floats_ = 0;
    double lo_f_ = 0, hi_f_ = 0;
    DevBuf eq_tabs_;              // EqScanTab[4] for L = 4, 8, 16, 32
    // plotter staging
    DevBuf plot_stage_, plot_jobs_;
    DevBuf conv_stage_;           // i16 staging for sink / ingest conversions
    size_t last_frames_per_call_ = 0;
    bool prof_on_ = false;
    // the events of one profiled span (pooled: created once, reused), and which of them the span recorded
    struct ProfSpan {
        hipEvent_t begin = nullptr;                                     // stream_, before the span's launches
        std::vector<hipEvent_t> group_end;                              // per launch group, on the stream it ran on
        hipEvent_t video_end = nullptr, tail_begin = nullptr;           // the per-tick video section (stream_); a held-back tail's start (tail stream)
        hipEvent_t od_end = nullptr, od_tail_end = nullptr;             // OutputDevice launches on stream_ / behind the tail
        hipEvent_t meters_end = nullptr, meters_tail_end = nullptr;     // meter, spectrum, loudness, stereo field and limiter launches on stream_ / behind the tail (and its OutputDevices)
        bool tail_held = false, od = false, od_tail = false, meters = false, meters_tail = false;
        explicit ProfSpan(size_t n_groups);
        ProfSpan(const ProfSpan&) = delete; ProfSpan& operator=(const ProfSpan&) = delete;
        ~ProfSpan();
    };
    std::vector<std::unique_ptr<ProfSpan>> prof_runs_, prof_pool_;   // one record per profiled span since the last collect; the records to reuse
    uint32_t last_calls_ = 0;
    // PerformanceInfo bookkeeping (last profiled run)
    std::vector<float> perf_group_ms_;   // per group (+1: video section) of the last collected run
    float perf_total_ms_ = 0.f; uint32_t perf_calls_ = 0;
    double perf_last_lag_s_ = -1.0;      // steady-clock seconds of the last over-budget tick; < 0: never
};

}  // namespace mx
