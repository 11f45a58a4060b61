// mx_engine.cpp -- device-resident graph executor.  See mx_engine.hpp.
#include <chrono>

#include "mx_engine.hpp"
#include "mx_deck.hpp"

#include <cstdio>

#include <algorithm>
#include <cmath>
#include <cstring>

namespace mx {

void hip_check(hipError_t e, const char* what) {
    if (e != hipSuccess) throw Error(MX_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

void DevBuf::alloc(size_t n) {
    free_();
    if (n == 0) n = 256;
    hipError_t e = hipMalloc(&p, n);
    if (e == hipErrorOutOfMemory) { p = nullptr; throw Error(MX_ERR_NOMEM, "hipMalloc: out of device memory"); }
    hip_check(e, "hipMalloc");
    bytes = n;
}
void DevBuf::free_() {
    if (p) (void)hipFree(p);
    p = nullptr; bytes = 0;
}

// first column of A^n for the 4-pole cascade's one-sample matrix A (lower-triangular Toeplitz,
// first column f^k (1-f)): binary exponentiation on polynomials mod x^4, in long double
static void toeplitz_pow_ld(long double f, uint64_t n, long double res[4]) {
    long double base[4] = {1.0L - f, f * (1.0L - f), f * f * (1.0L - f), f * f * f * (1.0L - f)};
    res[0] = 1.0L; res[1] = res[2] = res[3] = 0.0L;
    auto mul = [](const long double a[4], const long double b[4], long double c[4]) {
        long double t[4] = {0, 0, 0, 0};
        for (int i = 0; i < 4; ++i) for (int j = 0; i + j < 4; ++j) t[i + j] += a[i] * b[j];
        for (int i = 0; i < 4; ++i) c[i] = t[i];
    };
    while (n) {
        if (n & 1) mul(res, base, res);
        mul(base, base, base);
        n >>= 1;
    }
}
static void toeplitz_pow(long double f, uint64_t n, double out[4]) {
    long double r[4];
    toeplitz_pow_ld(f, n, r);
    for (int i = 0; i < 4; ++i) out[i] = (double)r[i];
}
// y = T(a) v for the lower-triangular Toeplitz matrix with first column a
static void toeplitz_apply_ld(const long double a[4], const long double v[4], long double y[4]) {
    for (int i = 0; i < 4; ++i) { y[i] = 0.0L; for (int k = 0; k <= i; ++k) y[i] += a[k] * v[i - k]; }
}

static inline size_t floats_per_frame(uint8_t lt) { return lt == MX_MONO ? 1 : (lt == MX_STEREO ? 2 : 0); }

static PlanEnv plan_env(size_t cap_frames) {
    const char* const ae = getenv("MX_OVERLAP_AUTO");   // read per graph: tests build both kinds in one process
    PlanEnv env; env.overlap_auto = !(ae && atoi(ae) == 0); env.cap_frames = cap_frames;
    return env;
}

// The compiler first (mx_plan.hpp: every topology decision, no device), then the device: stream, the tail candidate taken or not, slab, descriptors, per-kind state.
Graph::Graph(const mx_node* nodes, size_t n_nodes, const mx_edge* edges, size_t n_edges, const mx_graph_opts& o, size_t cap_frames_override)
    : plan_(compile_plan(nodes, n_nodes, edges, n_edges, o, plan_env(cap_frames_override))) {
    flags_ = plan_.flags; tps_ = plan_.tps; sample_rate_ = (double)plan_.sample_rate;
    spt_ = plan_.spt; tap_fpc_ = spt_; cap_frames_ = plan_.cap_frames;
    open_device(o);
    nodes_.reserve(n_nodes);
    for (size_t i = 0; i < n_nodes; ++i) {
        nodes_.emplace_back(plan_.nodes[i]);
        nodes_[i].params.assign((const uint8_t*)nodes[i].params, (const uint8_t*)nodes[i].params + nodes[i].params_len);
    }
    groups_.reserve(plan_.groups.size());
    for (const PlanGroup& g : plan_.groups) groups_.emplace_back(g);
    // video nodes: per-node state lives on the host, pixels on the graph's stream
    for (Node& n : nodes_) {
        if (n.kind == MX_KIND_VIDEO_MIXER) {
            mx_video_mixer_params p; std::memcpy(&p, n.params.data(), sizeof p);
            n.vmixer.reset(new VideoMixer(p, plan_.sample_rate, stream_));
            if (!(flags_ & MX_FLAG_NO_FUSE)) n.vmixer->set_lazy_program(n.vlazy, tps_);
        }
        if (n.kind == MX_KIND_MONITOR) {
            mx_monitor_params p; std::memcpy(&p, n.params.data(), sizeof p);
            n.mon = std::make_unique<MonitorState>();
            n.mon->scaler = std::make_shared<Scaler>(p.width, p.height, stream_);
            if (n.params.size() == sizeof(mx_monitor_params_ex)) { mx_monitor_params_ex px; std::memcpy(&px, n.params.data(), sizeof px); n.mon->depth = px.queue_depth; }
        }
        if (n.kind == MX_KIND_SOURCE_VIDEO) n.vsrc = std::make_unique<VideoSourceState>();
        if (n.kind == MX_KIND_VIDEO_TO_RGBA) n.rgba = std::make_unique<RgbaSinkState>();
        n.vout.resize(n.out_type.size());
    }
    upload_eq_tables();
    if (accept_tail()) tail_gi_ = plan_.tail_first;
    layout_slab();
    build_descriptors();
    // OutputDevice: created from the empty state, its params applied as the adapter's first update
    for (Node& n : nodes_) {
        if (n.kind != MX_KIND_OUTPUT_DEVICE) continue;
        n.od = std::make_unique<OutputDeviceState>((uint32_t)(spt_ * n.in_dom_num / n.in_dom_den), od_ticks());
        n.od->update(n.params.data(), od_ticks(), stream_);
        hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    }
}

void Graph::open_device(const mx_graph_opts& o) {
    if (o.device >= 0) { hip_check(hipSetDevice(o.device), "hipSetDevice"); device_ = o.device; }
    else hip_check(hipGetDevice(&device_), "hipGetDevice");
    if (o.stream) { stream_ = (hipStream_t)o.stream; own_stream_ = false; }
    else { hip_check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate"); own_stream_ = true; }
    { const char* const sm = getenv("MX_SIN_MODE"); sin_mode_ = sm ? atoi(sm) : 0; }   // (A/B and tests: mx_k_stream.hip SIN_MODE)
    { const char* const gt = getenv("MX_TAIL_GATE_TEST"); gate_test_ = gt && atoi(gt); }
    { const char* const er = getenv("MX_EQ_ENV_ROWS"); eq_env_rows_ = !(er && atoi(er) == 0); }   // (A/B, read per graph: tests build both kinds in one process)
    { const char* const el = getenv("MX_EQ_LEAN"); eq_lean_ = !(el && atoi(el) == 0); }           // (likewise)
}

void Graph::upload_eq_tables() {
    // host-side coefficients: same libm as the reference on this host (eq_three.rs:113-115)
    lo_f_ = 2.0 * std::sin(3.14159265358979323846264338327950288 * 420.0 / sample_rate_);
    hi_f_ = 2.0 * std::sin(3.14159265358979323846264338327950288 * 2700.0 / sample_rate_);
    std::vector<EqScanTab> tabs(4);
    const long double fs[2] = {(long double)lo_f_, (long double)hi_f_};
    for (int v = 0; v < 4; ++v) {
        const uint64_t L = 4ull << v;
        for (int f = 0; f < 2; ++f) {
            for (int j = 0; j <= 64; ++j) toeplitz_pow(fs[f], L * (uint64_t)j, tabs[v].pw[f][j]);
            for (int k = 0; k < 6; ++k) toeplitz_pow(fs[f], L << k, tabs[v].p2[f][k]);
            // phase-A tables: s' = A s + b x + c with b = (f, f^2, f^3, f^4), c = VSA (1, f, f^2, f^3) (eq_three.rs:117-124)
            const long double ff = fs[f], vsa = 1.0L / 4294967295.0L;
            const long double b[4] = {ff, ff * ff, ff * ff * ff, ff * ff * ff * ff};
            const long double c[4] = {vsa, vsa * ff, vsa * ff * ff, vsa * ff * ff * ff};
            long double sum[4] = {0, 0, 0, 0};
            for (uint64_t m = 0; m < 32; ++m) {
                long double am[4], hb[4];
                toeplitz_pow_ld(ff, m, am);
                toeplitz_apply_ld(am, b, hb);
                for (int q = 0; q < 4; ++q) tabs[v].h[f][m][q] = (double)hb[q];
                if (m < L) for (int q = 0; q < 4; ++q) sum[q] += am[q];
            }
            long double cz[4];
            toeplitz_apply_ld(sum, c, cz);
            for (int q = 0; q < 4; ++q) tabs[v].cz[f][q] = (double)cz[q];
        }
    }
    eq_tabs_.alloc(tabs.size() * sizeof(EqScanTab));
    hip_check(hipMemcpy(eq_tabs_.p, tabs.data(), tabs.size() * sizeof(EqScanTab), hipMemcpyHostToDevice), "hipMemcpy(eq tabs)");
}

// The plan names the overlap-tail candidate (mx_plan.cpp tail_candidate); one the library chose itself is taken only while its second buffers stay below
// MX_OVERLAP_AUTO_MAX_GB (default 32) and a quarter of the free device memory (an upper bound: every port as interleaved stereo).
bool Graph::accept_tail() {
    if (plan_.tail_first < 0) return false;
    if (plan_.tail_auto) {
        const char* const ge = getenv("MX_OVERLAP_AUTO_MAX_GB");
        const double max_gb = ge ? atof(ge) : 32.0;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = 0;
        const double extra = (double)plan_.tail_ports.size() * (double)cap_frames_ * 8.0;
        if (extra > max_gb * 1073741824.0 || extra > (double)free_b / 4.0) return false;
    }
    tail_auto_ = plan_.tail_auto;
    hip_check(hipStreamCreateWithFlags(&tail_stream_, hipStreamNonBlocking), "hipStreamCreate(tail)");
    hip_check(hipEventCreateWithFlags(&ev_head_done_, hipEventDisableTiming), "hipEventCreate");
    for (auto& e : ev_tail_done_) hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    return true;
}

OutputDeviceState::OutputDeviceState(uint32_t frames_per_tick, size_t ticks) : frames(frames_per_tick) {
    const OutState st0{-1, -1, 0u, 0u};
    state.alloc(sizeof(OutState));
    hip_check(hipMemcpy(state.p, &st0, sizeof st0, hipMemcpyHostToDevice), "hipMemcpy(output device state)");
    rec.alloc(ticks * sizeof(OutTick));
}

// A channel count above any seen before: the scratch grows (its samples kept, the new part zero: Vec::resize, output_device.rs:185) and the
// per-run buffers are sized for a whole submission of it.  The stream is quiescent (construction, or behind sync()).
void OutputDeviceState::grow(uint32_t ch, size_t ticks, hipStream_t stream) {
    if (ch <= cmax) return;
    const size_t F = frames;
    DevBuf sc; sc.alloc(F * ch * sizeof(float));
    hip_check(hipMemsetAsync(sc.p, 0, F * ch * sizeof(float), stream), "hipMemsetAsync(output device scratch)");
    if (cmax) hip_check(hipMemcpyAsync(sc.p, scratch.p, F * cmax * sizeof(float), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync(output device scratch)");
    hip_check(hipStreamSynchronize(stream), "hipStreamSynchronize");
    scratch = std::move(sc);
    out.alloc(ticks * F * ch * sizeof(float));
    part.alloc(ticks * out_route_blocks(F, ch) * sizeof(uint32_t));
    cmax = ch;
}

// OutputDevice::update (output_device.rs:152-169); `device` has already been resolved by the adapter into `channels`
void OutputDeviceState::update(const void* params, size_t ticks, hipStream_t stream) {
    mx_output_device_params p; std::memcpy(&p, params, sizeof p);
    channels = p.channels;
    if (!p.channels) return;   // no stream: the stored left / right stay, nothing is zeroed
    grow(p.channels, ticks, stream);
    // the STORED (filtered) assignment against the requested one: a repeated request for a channel the stream lacks zeroes again every time
    if (left != p.left || right != p.right)
        hip_check(hipMemsetAsync(scratch.p, 0, (size_t)frames * cmax * sizeof(float), stream), "hipMemsetAsync(output device scratch)");
    left = p.left >= 0 && (uint32_t)p.left < p.channels ? p.left : -1;
    right = p.right >= 0 && (uint32_t)p.right < p.channels ? p.right : -1;
}

size_t OutputDeviceState::offset(uint32_t tick) const {
    size_t off = 0;
    for (const Span& sp : spans)
        if (tick > sp.first) off += (size_t)std::min(tick - sp.first, sp.n) * frames * sp.channels;
    return off;
}

// the module persists across a topology edit: its stored assignment, scratch, clip / lag times and statuses, a pending lag note
void OutputDeviceState::adopt(OutputDeviceState& old, size_t ticks, hipStream_t stream) {
    grow(old.cmax, ticks, stream);
    if (old.cmax) {
        const size_t bytes = (size_t)std::min(frames * cmax, old.frames * old.cmax) * sizeof(float);
        hip_check(hipMemcpyAsync(scratch.p, old.scratch.p, bytes, hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync(output device scratch)");
    }
    hip_check(hipMemcpyAsync(state.p, old.state.p, sizeof(OutState), hipMemcpyDeviceToDevice, stream), "hipMemcpyAsync(output device state)");
    channels = old.channels; left = old.left; right = old.right;
    if (old.lag.exchange(false)) lag.store(true);
}

// The span's OutputDevice launches.  One that reads an output of the tail (MX_FLAG_OVERLAP_TAIL / automatic mode) is held back with it and goes
// behind it on the tail stream, where the events that join the tail cover it; any other runs on stream_ after the span's groups.
void Graph::launch_outputs(uint64_t t0, uint32_t call_off, uint32_t n_calls, ProfSpan* prof) {
    bool here = false;
    for (uint32_t id : plan_.od_nodes) {
        Node& n = nodes_[id];
        const PortRef src = n.in_src[0];
        int32_t o = src.node;
        while (o >= 0 && nodes_[o].elided && nodes_[o].owner >= 0) o = nodes_[o].owner;
        const bool on_tail = overlap_this_run_ && o >= 0 && nodes_[o].group >= tail_gi_;
        OutputDeviceState& od = *n.od;
        const uint32_t C = od.channels;
        const size_t base = od.offset(call_off);
        od.spans.push_back(OutputDeviceState::Span{call_off, n_calls, C});
        OutRun r{};
        r.in = in_ptr(n, 0, false, parity_); r.dup = src.node >= 0 && nodes_[src.node].out_dup[src.port] ? 1u : 0u;
        r.frames = od.frames; r.channels = C; r.left = od.left; r.right = od.right; r.n_ticks = n_calls;
        r.scratch = (float*)od.scratch.p; r.out = (float*)od.out.p + base; r.partial = (uint32_t*)od.part.p;
        r.state = (OutState*)od.state.p; r.rec = (OutTick*)od.rec.p + call_off;
        r.t0 = t0; r.spt = (uint32_t)spt_; r.rate = (uint32_t)sample_rate_; r.lag = call_off == 0 && od.lag_run ? 1u : 0u;
        if (on_tail) deferred_.outs.push_back(r);
        else { launch_output_device(r, stream_); here = true; }
    }
    if (!prof) return;
    if (here) { hip_check(hipEventRecord(prof->od_end, stream_), "hipEventRecord"); prof->od = true; }
    prof->od_tail = !deferred_.outs.empty();
}

void Graph::flush_deferred_tail(bool gated) {
    if (!deferred_.pending) return;
    deferred_.pending = false;
    ProfSpan* const prof = deferred_.prof;
    deferred_.prof = nullptr;
    hip_check(hipStreamWaitEvent(tail_stream_, ev_head_done_, 0), "hipStreamWaitEvent");
    if (gated && gate_armed_) { launch_tail_gate((const uint32_t*)gate_flag_.p, gate_seq_, 300u, tail_stream_); ++n_gated_; } else ++n_at_once_;
    if (prof) hip_check(hipEventRecord(prof->tail_begin, tail_stream_), "hipEventRecord");
    for (const TailLaunch& t : deferred_.items) {
        launch_mixer((const MixDesc*)t.desc, t.n, t.max_ch, t.frames, t.dup_mode, tail_stream_);
        if (t.prof_ev) hip_check(hipEventRecord(t.prof_ev, tail_stream_), "hipEventRecord");
    }
    deferred_.items.clear();
    for (const OutRun& r : deferred_.outs) launch_output_device(r, tail_stream_);   // OutputDevices that read the tail's outputs
    if (prof && !deferred_.outs.empty()) hip_check(hipEventRecord(prof->od_tail_end, tail_stream_), "hipEventRecord");
    deferred_.outs.clear();
    for (const AudioTapSet* t : deferred_.taps) t->launch(t->n_head, t->size() - t->n_head, deferred_.parity, tail_stream_);   // the audio tap sets' taps on the tail's outputs, in the sets' order
    if (prof && !deferred_.taps.empty()) hip_check(hipEventRecord(prof->meters_tail_end, tail_stream_), "hipEventRecord");
    deferred_.taps.clear();
    if (tail_hook_) { auto hook = std::move(tail_hook_); tail_hook_ = nullptr; hook(tail_stream_); }   // (mx_exchange: pack + exchange of that run's buses, behind the bank)
    // recorded AFTER the hook: whoever waits for this tail (wait_tail) is then also ordered behind the hook's reads of the buses on the tail stream -- a later run's Mixer on
    // stream_ must not overwrite them under a pack that is still copying
    hip_check(hipEventRecord(ev_tail_done_[deferred_.parity], tail_stream_), "hipEventRecord");
    tail_pending_[deferred_.parity] = true;
}

void Graph::wait_tail(int parity_or_all) {
    if (deferred_.pending && (parity_or_all < 0 || parity_or_all == (int)deferred_.parity)) flush_deferred_tail(false);
    for (int p = 0; p < 2; ++p)
        if ((parity_or_all < 0 || parity_or_all == p) && tail_pending_[p]) {
            hip_check(hipStreamWaitEvent(stream_, ev_tail_done_[p], 0), "hipStreamWaitEvent");
            tail_pending_[p] = false;
        }
}

// The automatic second-stream mode ends, for good.  Everything outstanding completes; the double-buffered ports go back to their FIRST buffer (the last run's data moves
// there when it sits in the second), the second set of descriptors is dropped and the first rebuilt -- from here on the graph is a one-stream graph in every respect
// (update_params, cut runs and ensure_capacity touch the only descriptors there are).
void Graph::end_auto_tail() {
    if (tail_gi_ < 0) return;
    sync();
    for (Node& n : nodes_)
        for (size_t k = 0; k < n.out_type.size(); ++k) {
            if (n.out_off2[k] == SIZE_MAX) continue;
            if (parity_ && n.out_off[k] != SIZE_MAX) {
                hip_check(hipMemcpyAsync((float*)slab_.p + n.out_off[k], (const float*)slab_.p + n.out_off2[k], port_floats(n, k, cap_frames_) * sizeof(float), hipMemcpyDeviceToDevice, stream_), "hipMemcpyAsync(D2D)");
            }
            n.out_off2[k] = SIZE_MAX;
        }
    hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    tail_gi_ = -1;
    parity_ = 0;
    overlap_this_run_ = false;
    for (Group& g : groups_) { g.desc_alt.free_(); g.extra_alt.free_(); }
    build_descriptors();
    reupload_taps(tap_fpc_);   // every tap on stream_, the first buffers only
}

Graph::~Graph() {
    flush_scales(stream_);
    try { flush_deferred_tail(false); } catch (...) {}
    if (tail_stream_) (void)hipStreamSynchronize(tail_stream_);
    if (stream_) (void)hipStreamSynchronize(stream_);
    if (tail_stream_) { (void)hipStreamDestroy(tail_stream_); (void)hipEventDestroy(ev_head_done_); for (auto& e : ev_tail_done_) (void)hipEventDestroy(e); }
    for (Node& n : nodes_) { n.vmixer.reset(); n.vout.clear(); n.vsrc.reset(); n.rgba.reset(); n.mon.reset(); }   // every frame the video nodes hold, while the stream is there
    multiview_.clear();
    prof_runs_.clear(); prof_pool_.clear();
    for (Stage& st : stage_) { if (st.done) (void)hipEventDestroy(st.done); if (st.host) (void)hipHostFree(st.host); }
    // the descriptor ring launch_video_batch keeps per stream goes with a stream this graph OWNS; a caller's stream may be shared with other
    // graphs / scalers that are launching on it right now (their ring must not be freed under them): its ring lives as long as the process
    if (stream_) deck_stream_retired(stream_);   // (a caller's stream too: the caller may destroy it once the graph is gone)
    if (own_stream_ && stream_) { video_stream_retired(stream_); multiview_stream_retired(stream_); (void)hipStreamDestroy(stream_); }
}

// where mx::layout_slab puts the ports for cap_frames_ (second buffers while the tail mode is on), and the slab itself
void Graph::layout_slab() {
    SlabLayout L = mx::layout_slab(plan_, cap_frames_, tail_gi_ >= 0);
    for (size_t i = 0; i < nodes_.size(); ++i) { nodes_[i].out_off = std::move(L.out_off[i]); nodes_[i].out_off2 = std::move(L.out_off2[i]); }
    zero_off_ = L.zero_off;
    slab_floats_ = L.floats;
    slab_.alloc(L.floats * sizeof(float));
    hip_check(hipMemsetAsync(slab_.p, 0, L.floats * sizeof(float), stream_), "hipMemsetAsync(slab)");
    hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
}

float* Graph::out_ptr(const Node& n, uint32_t port, uint32_t parity) const {
    // run_off_frames_: a run that is cut at scheduled parameter updates launches span by span; a span's buffers start that many
    // (base-rate) frames into the port
    const size_t fpf = n.out_dup[port] ? 1 : floats_per_frame(n.out_type[port]);
    const size_t off = fpf * (run_off_frames_ * n.dom_num / n.dom_den);
    if (n.bound && port == 0) return const_cast<float*>(n.bound) + off;
    const bool alt = parity && n.out_off2[port] != SIZE_MAX;
    return (float*)slab_.p + (alt ? n.out_off2[port] : n.out_off[port]) + off;
}
const float* Graph::in_ptr(const Node& n, uint32_t port, bool null_if_disconnected, uint32_t parity) const {
    const PortRef pr = n.in_src[port];
    if (pr.node < 0) return null_if_disconnected ? nullptr : (const float*)slab_.p + zero_off_;
    return out_ptr(nodes_[pr.node], pr.port, parity);
}

static double db_to_linear(double db) { return std::pow(10.0, db / 20.0); }   // protocol/src/lib.rs:469-471

void Graph::upload_group_one(Group& g, uint32_t parity) {
    const size_t n = g.nodes.size();
    auto up = [&](DevBuf& b, const void* src, size_t bytes) {
        if (b.bytes < bytes || !b.p) b.alloc(bytes);
        if (bytes) hip_check(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice), "hipMemcpy(desc)");
    };
    DevBuf& desc = parity ? g.desc_alt : g.desc;
    switch (g.kind) {
    case MX_KIND_AMPLIFIER: {
        std::vector<AmpDesc> d(n);
        for (size_t i = 0; i < n; ++i) {
            const Node& nd = nodes_[g.nodes[i]];
            mx_amplifier_params p; std::memcpy(&p, nd.params.data(), sizeof p);
            d[i] = AmpDesc{in_ptr(nd, 0, false, parity), in_ptr(nd, 1, true, parity), out_ptr(nd, 0, parity), p.amplitude, p.mod_depth};
        }
        up(desc, d.data(), n * sizeof(AmpDesc));
        break;
    }
    case MX_KIND_ENVELOPE: {
        std::vector<EnvDesc> d(n);
        for (size_t i = 0; i < n; ++i) {
            const Node& nd = nodes_[g.nodes[i]];
            mx_envelope_params p; std::memcpy(&p, nd.params.data(), sizeof p);
            float gate_const = 0.f; uint32_t use_const = 0;
            if (nd.fuse_trigger >= 0) {   // Trigger folded in: its per-tick constant (trigger.rs:38-41) replaces the gate buffer (GateBits row i)
                mx_trigger_params tp; std::memcpy(&tp, nodes_[nd.fuse_trigger].params.data(), sizeof tp);
                gate_const = tp.gate_open ? 1.0f : 0.0f; use_const = 2; g.has_gates = true;
            }
            d[i] = EnvDesc{use_const ? nullptr : in_ptr(nd, 0, false, parity), out_ptr(nd, 0, parity), gate_const, use_const,
                           EnvParams{p.attack_ms, 1.0 / p.attack_ms, 1.0 / p.decay_ms,
                                     p.sustain_amplitude, 1.0 - p.sustain_amplitude, 1.0 / p.release_ms}};
        }
        up(desc, d.data(), n * sizeof(EnvDesc));
        if (!g.state.p) { g.state.alloc(n * sizeof(EnvState)); hip_check(hipMemset(g.state.p, 0, n * sizeof(EnvState)), "hipMemset"); }
        break;
    }
    case MX_KIND_EQ_THREE: {
        std::vector<EqDesc> d(n);
        std::vector<EnvTickDesc> td(n);
        bool any_env = false;
        for (size_t i = 0; i < n; ++i) {
            const Node& nd = nodes_[g.nodes[i]];
            mx_eq_three_params p; std::memcpy(&p, nd.params.data(), sizeof p);
            EqDesc e{};
            e.in = in_ptr(nd, 0, false, parity);
            e.gain_lo = db_to_linear(p.gain_lo_db); e.gain_mid = db_to_linear(p.gain_mid_db); e.gain_hi = db_to_linear(p.gain_hi_db);
            if (nd.fuse_amp >= 0) {          // EqThree -> StereoPanner(L = R) -> Amplifier in one kernel
                const Node& amp = nodes_[nd.fuse_amp];
                if (amp.out_dup[0]) e.flags |= MX_EQF_MONO_DUP;
                mx_amplifier_params ap; std::memcpy(&ap, amp.params.data(), sizeof ap);
                e.out = out_ptr(amp, 0, parity); e.ctl = in_ptr(amp, 1, true, parity);
                e.amp_one_minus = 1.0 - ap.mod_depth; e.amp_mod_depth = ap.mod_depth; e.amp_amplitude = ap.amplitude; e.epi = 2;
            } else if (nd.fuse_pan >= 0) {   // EqThree -> StereoPanner(L = R)
                e.out = out_ptr(nodes_[nd.fuse_pan], 0, parity); e.epi = 1;
                if (nodes_[nd.fuse_pan].out_dup[0]) e.flags |= MX_EQF_MONO_DUP;
            } else {
                e.out = out_ptr(nd, 0, parity); e.epi = 0;
            }
            if (nd.fuse_env >= 0) {          // Envelope (constant gate) evaluated inline as the control
                const Node& env = nodes_[nd.fuse_env];
                mx_envelope_params ep; std::memcpy(&ep, env.params.data(), sizeof ep);
                e.flags |= MX_EQF_ENV; e.ctl = nullptr;
                e.env = EnvParams{ep.attack_ms, 1.0 / ep.attack_ms, 1.0 / ep.decay_ms, ep.sustain_amplitude, 1.0 - ep.sustain_amplitude, 1.0 / ep.release_ms};
                if (!g.state2.p) { g.state2.alloc(n * sizeof(EnvState)); hip_check(hipMemset(g.state2.p, 0, n * sizeof(EnvState)), "hipMemset"); }
                // its per-tick states are laid out by k_env_ticks before the EQ kernel runs (gate = the folded Trigger, GateBits row i)
                td[i] = EnvTickDesc{e.env, e.amp_one_minus, e.amp_mod_depth, (EnvState*)g.state2.p + i};
                any_env = true; g.has_gates = true;
            }
            d[i] = e;
            const int em = eq_epilogue_mode(e.epi, e.flags, e.ctl != nullptr);
            g.eq_mode = i == 0 ? em : (g.eq_mode == em ? em : -1);
            // the groups were cut by the plan's idea of this mode (sub_key, from the fusion plan: mx_plan.cpp cut_groups); the descriptor's is the one the kernels see.  If they ever disagree a group
            // silently falls to the general direct-load kernel (29 ms against 5): refuse loudly instead
            if (nd.sub_key != 0 && nd.sub_key != 1 + em && !eq_mode_warned_) {   // (results are right either way: say it, once per graph, and go on)
                eq_mode_warned_ = true;
                fprintf(stderr, "mixlab_gpu: EqThree node %u was grouped for epilogue mode %d but its descriptor says %d: the group runs the general (slower) kernel\n",
                        (unsigned)g.nodes[i], nd.sub_key - 1, em);
            }
        }
        up(desc, d.data(), n * sizeof(EqDesc));
        if (any_env) up(g.tick_desc, td.data(), n * sizeof(EnvTickDesc));
        if (!g.state.p) { g.state.alloc(n * sizeof(EqState)); hip_check(hipMemset(g.state.p, 0, n * sizeof(EqState)), "hipMemset"); }
        break;
    }
    case MX_KIND_FM_SINE: {
        std::vector<FmDesc> d(n);
        for (size_t i = 0; i < n; ++i) {
            const Node& nd = nodes_[g.nodes[i]];
            mx_fm_sine_params p; std::memcpy(&p, nd.params.data(), sizeof p);
            const double freq_amp = (p.freq_hi - p.freq_lo) / 2.0;    // fm_sine.rs:42
            const double freq_mid = p.freq_lo + freq_amp;            // fm_sine.rs:43
            d[i] = FmDesc{in_ptr(nd, 0, false, parity), out_ptr(nd, 0, parity), freq_mid, freq_amp};
        }
        up(desc, d.data(), n * sizeof(FmDesc));
        break;
    }
    case MX_KIND_MIXER: {
        size_t total = 0;
        for (uint32_t id : g.nodes) total += nodes_[id].in_type.size();
        std::vector<MixChan> ch(total ? total : 1);
        DevBuf& xb = parity ? g.extra_alt : g.extra;
        if (xb.bytes < ch.size() * sizeof(MixChan) || !xb.p) xb.alloc(ch.size() * sizeof(MixChan));
        std::vector<MixDesc> d(n);
        size_t o = 0, n_dup = 0;
        for (size_t i = 0; i < n; ++i) {
            const Node& nd = nodes_[g.nodes[i]];
            const size_t nch = nd.in_type.size();
            const mx_mixer_channel_params* p = (const mx_mixer_channel_params*)nd.params.data();
            for (size_t c = 0; c < nch; ++c) {
                mx_mixer_channel_params cp; std::memcpy(&cp, p + c, sizeof cp);
                const PortRef src = nd.in_src[c];
                const uint32_t dup = (src.node >= 0 && nodes_[src.node].out_dup[src.port]) ? 1u : 0u;
                n_dup += dup;
                ch[o + c] = MixChan{in_ptr(nd, (uint32_t)c, false, parity), cp.fader * db_to_linear(cp.gain_db), cp.cue ? 1u : 0u, dup};  // mixer.rs:59
            }
            d[i] = MixDesc{(const MixChan*)xb.p + o, (uint32_t)nch, 0u, out_ptr(nd, 0, parity), out_ptr(nd, 1, parity)};
            o += nch;
        }
        g.dup_mode = n_dup == 0 ? 0 : (n_dup == total ? 1 : 2);
        g.max_taps = 0;
        for (uint32_t id : g.nodes) g.max_taps = std::max<uint32_t>(g.max_taps, (uint32_t)nodes_[id].in_type.size());   // Mixer: most channels
        hip_check(hipMemcpy(xb.p, ch.data(), ch.size() * sizeof(MixChan), hipMemcpyHostToDevice), "hipMemcpy(mixchan)");
        up(desc, d.data(), n * sizeof(MixDesc));
        break;
    }
    case MX_KIND_OSCILLATOR: {
        std::vector<OscDesc> d(n);
        for (size_t i = 0; i < n; ++i) {
            const Node& nd = nodes_[g.nodes[i]];
            mx_oscillator_params p; std::memcpy(&p, nd.params.data(), sizeof p);
            d[i] = OscDesc{out_ptr(nd, 0, parity), out_ptr(nd, 1, parity), p.freq, p.waveform, 0u};
        }
        up(desc, d.data(), n * sizeof(OscDesc));
        break;
    }
    case MX_KIND_STEREO_PANNER: {
        std::vector<PanDesc> d(n);
        for (size_t i = 0; i < n; ++i) { const Node& nd = nodes_[g.nodes[i]]; d[i] = PanDesc{in_ptr(nd, 0, false, parity), in_ptr(nd, 1, false, parity), out_ptr(nd, 0, parity)}; }
        up(desc, d.data(), n * sizeof(PanDesc));
        break;
    }
    case MX_KIND_STEREO_SPLITTER: {
        std::vector<SplitDesc> d(n);
        for (size_t i = 0; i < n; ++i) { const Node& nd = nodes_[g.nodes[i]]; d[i] = SplitDesc{in_ptr(nd, 0, false, parity), out_ptr(nd, 0, parity), out_ptr(nd, 1, parity)}; }
        up(desc, d.data(), n * sizeof(SplitDesc));
        break;
    }
    case MX_KIND_TRIGGER: {
        std::vector<TrigDesc> d(n);
        for (size_t i = 0; i < n; ++i) {
            const Node& nd = nodes_[g.nodes[i]];
            mx_trigger_params p; std::memcpy(&p, nd.params.data(), sizeof p);
            d[i] = TrigDesc{out_ptr(nd, 0, parity), p.gate_open ? 1.0f : 0.0f, 0u};   // trigger.rs:38-41
        }
        g.has_gates = true;
        up(desc, d.data(), n * sizeof(TrigDesc));
        break;
    }
    case MX_KIND_FIR: {
        size_t tt = 0, th = 0; g.max_taps = 0;
        for (uint32_t id : g.nodes) { const uint32_t h = history_frames(nodes_[id]); tt += h; th += h; g.max_taps = std::max(g.max_taps, h); }
        std::vector<double> taps(tt);
        if (g.extra.bytes < tt * sizeof(double) || !g.extra.p) g.extra.alloc(tt * sizeof(double));
        if (!g.state.p) { g.state.alloc(th * sizeof(float2)); hip_check(hipMemset(g.state.p, 0, th * sizeof(float2)), "hipMemset"); }
        std::vector<FirDesc> d(n);
        size_t o = 0;
        for (size_t i = 0; i < n; ++i) {
            const Node& nd = nodes_[g.nodes[i]];
            const uint32_t n_taps = history_frames(nd);
            std::memcpy(&taps[o], nd.params.data() + sizeof(mx_fir_params), (size_t)n_taps * sizeof(double));
            d[i] = FirDesc{in_ptr(nd, 0, false, parity), out_ptr(nd, 0, parity), (const double*)g.extra.p + o, (float2*)g.state.p + o, n_taps, 0u};
            o += n_taps;
        }
        hip_check(hipMemcpy(g.extra.p, taps.data(), tt * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(fir taps)");
        up(desc, d.data(), n * sizeof(FirDesc));
        break;
    }
    case MX_KIND_RESAMPLE: {
        size_t tt = 0, th = 0; g.max_taps = 0;
        g.rs_tab_doubles = 0; g.rs_win_frames = 0; g.rs_common_up = 0; g.rs_common_taps = 0; g.rs_common_down = 0; bool rs_first = true;
        for (uint32_t id : g.nodes) {
            mx_resample_params h; std::memcpy(&h, nodes_[id].params.data(), sizeof h);   // the ratio; the taps per phase are the plan's history length
            const uint32_t tpp = history_frames(nodes_[id]);
            tt += (size_t)h.up * tpp; th += tpp; g.max_taps = std::max(g.max_taps, tpp);
            g.rs_tab_doubles = (uint32_t)std::min<uint64_t>(0xffffffffu, std::max<uint64_t>(g.rs_tab_doubles, (uint64_t)h.up * tpp));
            g.rs_win_frames = (uint32_t)std::min<uint64_t>(0xffffffffu, std::max<uint64_t>(g.rs_win_frames, (uint64_t)255 * h.down / h.up + 2 + tpp));
            if (rs_first) { g.rs_common_up = h.up; g.rs_common_taps = tpp; g.rs_common_down = h.down; rs_first = false; }   // every node's ratio and taps per phase, where they agree
            else { if (g.rs_common_up != h.up) g.rs_common_up = 0; if (g.rs_common_taps != tpp) g.rs_common_taps = 0; if (g.rs_common_down != h.down) g.rs_common_down = 0; }
        }
        std::vector<double> taps(tt);
        if (g.extra.bytes < tt * sizeof(double) || !g.extra.p) g.extra.alloc(tt * sizeof(double));
        if (!g.state.p) { g.state.alloc(th * sizeof(float2)); hip_check(hipMemset(g.state.p, 0, th * sizeof(float2)), "hipMemset"); }
        std::vector<ResampleDesc> d(n);
        size_t o = 0, oh = 0;
        for (size_t i = 0; i < n; ++i) {
            const Node& nd = nodes_[g.nodes[i]];
            mx_resample_params h; std::memcpy(&h, nd.params.data(), sizeof h);
            const uint32_t tpp = history_frames(nd);
            const size_t cnt = (size_t)h.up * tpp;
            std::memcpy(&taps[o], nd.params.data() + sizeof h, cnt * sizeof(double));
            d[i] = ResampleDesc{in_ptr(nd, 0, false, parity), out_ptr(nd, 0, parity), (const double*)g.extra.p + o, (float2*)g.state.p + oh, h.up, h.down, tpp, 0u};
            o += cnt; oh += tpp;
        }
        hip_check(hipMemcpy(g.extra.p, taps.data(), tt * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy(resample taps)");
        up(desc, d.data(), n * sizeof(ResampleDesc));
        break;
    }
    default: break;  // PLOTTER (jobs built per run), SOURCE_* (no launch)
    }
}

void Graph::upload_group(Group& g) {
    upload_group_one(g, 0);
    if (tail_gi_ >= 0) upload_group_one(g, 1);   // the same descriptors with the double-buffered ports at their second buffer
}

void Graph::build_descriptors() {
    for (Group& g : groups_) upload_group(g);
}

void Graph::update_params(uint32_t node, const void* params, size_t len) {
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    if (len != nodes_[node].params.size()) throw Error(MX_ERR_INVALID, "params_len differs from the node's params (terminal count is frozen with the topology)");
    if (len && !params) throw Error(MX_ERR_INVALID, "params is NULL");
    if (nodes_[node].kind == MX_KIND_OUTPUT_DEVICE) check_output_device_params(params);
    // a Trigger's params live in the GateBits rows the next run uploads: nothing on the device reads them, nothing has to be waited for (and a Mixer bank that is being
    // held back for the next run stays held)
    if (nodes_[node].kind != MX_KIND_TRIGGER) sync();
    apply_params(node, params, len);
}

// ModuleT::update (src/module/mod.rs:16) on a quiescent stream: new params into the node, descriptors of every launch that
// reads them re-uploaded.  A Trigger only lives in the GateBits rows, which the next run refreshes.
void Graph::apply_params(uint32_t node, const void* params, size_t len) {
    Node& n = nodes_[node];
    if (len) std::memcpy(n.params.data(), params, len);
    if (n.kind == MX_KIND_TRIGGER) { ++gates_version_; return; }
    if (n.kind == MX_KIND_OUTPUT_DEVICE) { n.od->update(n.params.data(), od_ticks(), stream_); return; }
    if (n.kind == MX_KIND_VIDEO_MIXER && n.vmixer) {
        mx_video_mixer_params p; std::memcpy(&p, n.params.data(), sizeof p);
        n.vmixer->update(p);
    }
    if (n.group >= 0) upload_group(groups_[n.group]);
    int32_t o = (int32_t)node;
    while (nodes_[o].elided && nodes_[o].owner >= 0) o = nodes_[o].owner;   // Envelope -> EqThree chains
    if (o != (int32_t)node && nodes_[o].group >= 0) upload_group(groups_[nodes_[o].group]);
}

void Graph::check_schedule(uint32_t node, const void* params, size_t len) const {
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    const Node& n = nodes_[node];
    if (len != n.params.size()) throw Error(MX_ERR_INVALID, "params_len differs from the node's params (terminal count is frozen with the topology)");
    if (len && !params) throw Error(MX_ERR_INVALID, "params is NULL");
    if (n.kind == MX_KIND_OUTPUT_DEVICE) check_output_device_params(params);
}

void Graph::drop_schedules() {
    for (uint32_t id : sched_nodes_) { nodes_[id].sched.clear(); nodes_[id].gate_sched.clear(); }
    if (!sched_nodes_.empty()) ++gates_version_;
    sched_nodes_.clear();
}

void Graph::schedule_params(uint32_t node, uint32_t tick, const void* params, size_t len) {
    check_schedule(node, params, len);
    Node& n = nodes_[node];
    if (n.sched.empty() && n.gate_sched.empty()) sched_nodes_.push_back(node);
    if (n.kind == MX_KIND_TRIGGER) {
        mx_trigger_params tp; std::memcpy(&tp, params, sizeof tp);
        n.gate_sched.emplace_back(tick, tp.gate_open ? 1u : 0u);
        ++gates_version_;
        return;
    }
    Node::SchedEv ev; ev.tick = tick;
    ev.params.assign((const uint8_t*)params, (const uint8_t*)params + len);
    n.sched.push_back(std::move(ev));
}

// H2D copy on the graph's stream out of page-locked staging: the caller's buffer is free on return, nothing waits for the device
void Graph::stage_upload(void* dst, const void* src, size_t bytes) {
    if (!bytes) return;
    Stage& st = stage_[stage_next_];
    stage_next_ = (stage_next_ + 1) % 4;
    if (st.pending) { hip_check(hipEventSynchronize(st.done), "hipEventSynchronize"); st.pending = false; }
    if (st.cap < bytes) {
        if (st.host) (void)hipHostFree(st.host);
        st.host = nullptr; st.cap = 0;
        hip_check(hipHostMalloc(&st.host, bytes, hipHostMallocDefault), "hipHostMalloc(staging)");
        st.cap = bytes;
    }
    if (!st.done) hip_check(hipEventCreateWithFlags(&st.done, hipEventDisableTiming), "hipEventCreate");
    std::memcpy(st.host, src, bytes);
    // a graph with a second stream: by a kernel, not an SDMA copy -- a copy queued behind a cross-stream wait makes the HOST wait for that event (k_upload); everybody else
    // keeps the copy engine (a tick at a time it is the shorter path: 74 against 84 us per tick of 1024 strips)
    if (tail_gi_ >= 0) launch_upload(dst, st.host, bytes, stream_);
    else hip_check(hipMemcpyAsync(dst, st.host, bytes, hipMemcpyHostToDevice, stream_), "hipMemcpyAsync(H2D staged)");
    hip_check(hipEventRecord(st.done, stream_), "hipEventRecord");
    st.pending = true;
}

uint32_t Graph::trigger_of_row(const Group& g, uint32_t row) const {
    const Node& nd = nodes_[g.nodes[row]];
    if (g.kind == MX_KIND_TRIGGER) return g.nodes[row];
    if (g.kind == MX_KIND_ENVELOPE) return nd.fuse_trigger >= 0 ? (uint32_t)nd.fuse_trigger : ~0u;
    if (g.kind == MX_KIND_EQ_THREE) return nd.fuse_env >= 0 && nodes_[nd.fuse_env].fuse_trigger >= 0 ? (uint32_t)nodes_[nd.fuse_env].fuse_trigger : ~0u;
    return ~0u;
}

// GateBits rows of a group for the coming run: bit c of row i = gate_open of row i's Trigger during tick c -- its current params,
// then every scheduled update from its tick on (the reference applies client_update between two ticks, src/engine.rs:192-214)
void Graph::refresh_gates(Group& g, uint32_t run_calls) {
    if (!g.has_gates) return;
    if (g.gates.p && g.gates_version == gates_version_ && g.gates_calls == run_calls) return;
    const uint32_t words = (run_calls + 31) / 32;
    const size_t n = g.nodes.size();
    std::vector<uint32_t> bits(n * words, 0u);
    for (size_t i = 0; i < n; ++i) {
        const uint32_t tr = trigger_of_row(g, (uint32_t)i);
        if (tr == ~0u) continue;
        const Node& T = nodes_[tr];
        mx_trigger_params tp; std::memcpy(&tp, T.params.data(), sizeof tp);
        bool open = tp.gate_open != 0;
        uint32_t c = 0;
        uint32_t* row = bits.data() + i * words;
        auto fill_to = [&](uint32_t end) {   // bits [c, end) = open, a word at a time
            if (open && end > c) {
                uint32_t a = c, b = end;
                while (a < b) {
                    const uint32_t w = a >> 5, lo = a & 31, hi = std::min<uint32_t>(32, lo + (b - a));
                    const uint32_t mask = (hi == 32 ? 0xffffffffu : ((1u << hi) - 1u)) & ~((1u << lo) - 1u);
                    row[w] |= mask;
                    a += hi - lo;
                }
            }
            c = end;
        };
        for (const auto& ev : T.gate_sched) {               // stable by tick: submission order decides among updates for one tick
            const uint32_t at = ev.first < run_calls ? ev.first : run_calls;
            if (at > c) fill_to(at);
            open = ev.second != 0;
        }
        fill_to(run_calls);
    }
    if (g.gates.bytes < bits.size() * sizeof(uint32_t) || !g.gates.p) { sync(); g.gates.alloc(std::max<size_t>(bits.size() * sizeof(uint32_t), 256)); }
    stage_upload(g.gates.p, bits.data(), bits.size() * sizeof(uint32_t));
    g.gate_words = words; g.gates_version = gates_version_; g.gates_calls = run_calls;
}

void Graph::eq_spec_stats(uint64_t out[8]) {
    for (int k = 0; k < 8; ++k) out[k] = 0;
    if (!eq_stats_.p) return;
    sync();
    hip_check(hipMemcpy(out, eq_stats_.p, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost), "hipMemcpy(eq stats)");
}

void Graph::write_source(uint32_t node, const float* host, size_t frames) {
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    Node& n = nodes_[node];
    if (n.kind != MX_KIND_SOURCE_MONO && n.kind != MX_KIND_SOURCE_STEREO) throw Error(MX_ERR_INVALID, "node is not a SOURCE_*");
    if (n.bound) throw Error(MX_ERR_INVALID, "source is bound to a caller device buffer");
    if (frames > cap_frames_) throw Error(MX_ERR_INVALID, "more ticks than max_ticks_per_run");
    if (frames && !host) throw Error(MX_ERR_INVALID, "host_samples is NULL");
    const size_t fl = floats_per_frame(n.out_type[0]) * frames;
    hip_check(hipMemcpyAsync(out_ptr(n, 0, parity_), host, fl * sizeof(float), hipMemcpyHostToDevice, stream_), "hipMemcpyAsync(H2D source)");
    hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");  // host buffer is the caller's again on return
}

float* Graph::source_feed_ptr(uint32_t node, size_t frames) {
    check_source_write(node, frames);
    if (nodes_[node].kind != MX_KIND_SOURCE_STEREO) throw Error(MX_ERR_INVALID, "node is not a SOURCE_STEREO");
    return out_ptr(nodes_[node], 0, parity_);
}

void Graph::bind_source(uint32_t node, const void* dev) {
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    Node& n = nodes_[node];
    if (n.kind != MX_KIND_SOURCE_MONO && n.kind != MX_KIND_SOURCE_STEREO) throw Error(MX_ERR_INVALID, "node is not a SOURCE_*");
    if (dev && ((uintptr_t)dev & 15)) throw Error(MX_ERR_INVALID, "bound device buffer must be 16-byte aligned");
    sync();
    n.bound = (const float*)dev;
    build_descriptors();
    reupload_taps(tap_fpc_);
}

void Graph::set_input_enabled(uint32_t node, uint32_t port, bool enabled) {
    if (node >= nodes_.size() || port >= nodes_[node].in_src.size()) throw Error(MX_ERR_INVALID, "input terminal out of range");
    Node& n = nodes_[node];
    if (n.pos < 0) return;  // node is outside the run order
    const PortRef want = enabled ? plan_.nodes[node].in_src[port] : PortRef{};   // the plan keeps what was connected
    if (want.node == n.in_src[port].node && want.port == n.in_src[port].port) return;
    sync();
    n.in_src[port] = want;
    if (n.group >= 0) upload_group(groups_[n.group]);
}

void Graph::sync() {
    hip_check(hipSetDevice(device_), "hipSetDevice");   // the current device is per thread: a graph may be driven from another thread than its creator's
    flush_scales(stream_);
    flush_deferred_tail(false);
    hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
    if (tail_stream_) { hip_check(hipStreamSynchronize(tail_stream_), "hipStreamSynchronize"); tail_pending_[0] = tail_pending_[1] = false; }
}

void Graph::ensure_capacity(size_t frames) {
    if (frames <= cap_frames_) return;
    sync();
    cap_frames_ = frames;
    layout_slab();
    build_descriptors();
    reupload_taps(tap_fpc_);   // the ports moved; room for more ticks
}

static bool group_launches(const Group& g);

void Graph::run(uint64_t t0, size_t fpc, uint32_t n_calls, float* ms_by_kind, float* ms_total) {
    const size_t frames = fpc * (size_t)n_calls;
    auto drop_schedules = [&] { for (uint32_t id : sched_nodes_) { nodes_[id].sched.clear(); nodes_[id].gate_sched.clear(); } sched_nodes_.clear(); };
    if (frames > cap_frames_) { drop_schedules(); throw Error(MX_ERR_INVALID, "n_ticks exceeds max_ticks_per_run"); }
    if (n_calls == 0 || fpc == 0) { drop_schedules(); last_calls_ = n_calls; last_frames_per_call_ = fpc; for (AudioTapSet* s : taps_) s->empty_run(); scopes_.empty_run(); multiview_.empty_run(); return; }
    // graded / keyed / matted / placed video sources: a frame the transform cannot take fails the run HERE, before anything of it is launched or any node's state has moved
    for (uint32_t id : plan_.video_order) {
        const VideoSourceState* vs = nodes_[id].vsrc.get();
        if (!vs || !vs->transform.active()) continue;
        const uint64_t tick0 = t0 / spt_;
        const char* why = nullptr;
        vs->each_deliverable(tick0, tick0 + n_calls - 1, [&](const DFrame* f) { if (!why) why = vs->transform.input_error(f); });
        if (why) { drop_schedules(); throw Error(MX_ERR_INVALID, "node " + std::to_string(id) + " (SOURCE_VIDEO): " + why); }
    }
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (fpc != tap_fpc_) {   // (the module compat path's call length): frames per tick and record room
        if (std::any_of(taps_.begin(), taps_.end(), [](const AudioTapSet* s) { return !s->empty(); })) { sync(); reupload_taps(fpc); }
    }

    // ---- scheduled parameter updates (Engine::client_update between two ticks, src/engine.rs:192-214,277-398) ----
    // Trigger updates travel as one gate bit per tick and cost nothing.  Any other module's update cuts the run into spans:
    // the update is applied (ModuleT::update) between the span that ends before its tick and the span that starts with it.
    std::vector<uint32_t> cuts;   // span starts > 0
    bool any_sched = false;
    const char* beyond = "a scheduled parameter update lies beyond the run (tick_in_run >= n_ticks)";
    for (uint32_t sid : sched_nodes_) {
        Node& n = nodes_[sid];
        if (!n.gate_sched.empty()) {
            any_sched = true;
            bool sorted = true;
            for (size_t i = 1; i < n.gate_sched.size(); ++i) sorted = sorted && n.gate_sched[i - 1].first <= n.gate_sched[i].first;
            if (!sorted) std::stable_sort(n.gate_sched.begin(), n.gate_sched.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
            if (n.gate_sched.back().first >= n_calls) { drop_schedules(); throw Error(MX_ERR_INVALID, beyond); }
        }
        if (n.sched.empty()) continue;
        any_sched = true;
        std::stable_sort(n.sched.begin(), n.sched.end(), [](const Node::SchedEv& x, const Node::SchedEv& y) { return x.tick < y.tick; });
        if (n.sched.back().tick >= n_calls) { drop_schedules(); throw Error(MX_ERR_INVALID, beyond); }
        for (const Node::SchedEv& ev : n.sched) if (ev.tick) cuts.push_back(ev.tick);
    }
    std::sort(cuts.begin(), cuts.end());
    cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
    auto apply_at = [&](uint32_t tick) {   // every non-Trigger update scheduled for `tick`, in submission order
        bool any = false;
        for (uint32_t id : sched_nodes_) {
            Node& n = nodes_[id];
            if (n.kind == MX_KIND_TRIGGER) continue;
            for (const Node::SchedEv& ev : n.sched) if (ev.tick == tick) { if (!any) { sync(); any = true; } apply_params(id, ev.params.data(), ev.params.size()); }
        }
    };
    if (any_sched) apply_at(0);
    for (uint32_t id : plan_.od_nodes) {   // the lag flag is swapped by the run's first tick (output_device.rs:219); the spans of this run replace the last run's
        Node& n = nodes_[id];
        n.od->lag_run = n.od->lag.exchange(false);
        n.od->spans.clear();
        // a scheduled update to more channels than any before: the buffers grow now, not between two spans (the hand-off holds every span's ticks)
        uint32_t cmax = 0;
        for (const Node::SchedEv& ev : n.sched) { mx_output_device_params q; std::memcpy(&q, ev.params.data(), sizeof q); cmax = std::max(cmax, q.channels); }
        if (cmax > n.od->cmax) { sync(); n.od->grow(cmax, od_ticks(), stream_); }
    }
    for (uint32_t id : plan_.video_order) if (nodes_[id].mon) nodes_[id].mon->ticks.clear();
    scopes_.begin_run(n_calls);      // the records this run will count into are cleared now, on stream_ ahead of every launch of the run
    multiview_.begin_run(n_calls);   // the multiviewer renders the run's LAST recorded tick only

    // Plotter bookkeeping is host logic (plotter.rs:37-40): count += 1 per call, fire on every 6th
    size_t total_fired = 0;
    for (uint32_t pid : plan_.plotter_nodes) {
        Node& n = nodes_[pid];
        n.plot_fired.assign(n_calls, 0);
        n.plot_slot.assign(n_calls, -1);
        const bool connected = n.in_src[0].node >= 0;
        for (uint32_t c = 0; c < n_calls; ++c) {
            n.plot_count += 1;
            if (n.plot_count % 6 == 0 && connected) { n.plot_fired[c] = 1; n.plot_slot[c] = (int32_t)total_fired++; }
        }
    }
    if (total_fired) {
        const size_t need = total_fired * 2 * fpc * sizeof(float);
        if (plot_stage_.bytes < need) { sync(); plot_stage_.alloc(need); }
        if (plot_jobs_.bytes < total_fired * sizeof(PlotJob)) { sync(); plot_jobs_.alloc(total_fired * sizeof(PlotJob)); }
    }
    plot_job_off_ = 0;
    for (Group& g : groups_) refresh_gates(g, n_calls);

    const bool prof = ms_by_kind != nullptr || prof_on_;
    prof_this_run_ = prof;
    // MX_FLAG_OVERLAP_TAIL: an uncut run alternates the double-buffered ports and leaves its tail on the second stream; before its
    // earlier groups overwrite a buffer, the tail that last read THAT buffer (two runs ago) must be done -- not the previous run's
    // (automatic mode: a run of a tick or a few on a graph built for long submissions stays on one stream -- two cross-stream events cost 13 us of an 75 us tick)
    for (hipEvent_t e : head_waits_) hip_check(hipStreamWaitEvent(stream_, e, 0), "hipStreamWaitEvent");
    head_waits_.clear();
    overlap_this_run_ = tail_gi_ >= 0 && cuts.empty() && (!tail_auto_ || n_calls >= 16);
    if (overlap_this_run_) { parity_ ^= 1u; wait_tail((int)parity_); }
    else if (tail_gi_ >= 0) wait_tail(-1);
    if (cuts.empty()) {
        run_span(t0, fpc, 0, n_calls, n_calls);
    } else {
        cuts.push_back(n_calls);
        uint32_t from = 0;
        for (uint32_t to : cuts) {
            if (from) {
                apply_at(from);
                sync();
                run_off_frames_ = (size_t)from * fpc;
                build_descriptors();                       // every port pointer moves to the span's first tick
            }
            run_span(t0 + (uint64_t)from * fpc, fpc, from, to - from, n_calls);
            from = to;
        }
        sync();
        run_off_frames_ = 0;
        build_descriptors();
    }
    // the modules keep the last scheduled params (a Trigger's are read by the next run's GateBits)
    if (any_sched) {
        for (uint32_t sid : sched_nodes_) {
            Node& n = nodes_[sid];
            if (!n.gate_sched.empty()) {
                mx_trigger_params tp{}; tp.gate_open = n.gate_sched.back().second;
                std::memcpy(n.params.data(), &tp, sizeof tp);
                ++gates_version_;
                n.gate_sched.clear();
            }
            n.sched.clear();
        }
        sched_nodes_.clear();
    }
    hip_check(hipGetLastError(), "kernel launch");
    last_calls_ = n_calls;
    last_frames_per_call_ = fpc;
    for (AudioTapSet* s : taps_) s->run_ticks = s->empty() ? 0u : n_calls;
    if (prof) ++prof_runs_count_;
    if (ms_by_kind) (void)profile_collect(ms_by_kind, ms_total);
}

// ticks [call_off, call_off + n_calls) of the current run: one launch per (level, kind, domain) group, then the video section
void Graph::run_span(uint64_t t0, size_t fpc, uint32_t call_off, uint32_t n_calls, uint32_t run_calls) {
    const size_t frames = fpc * (size_t)n_calls;
    ProfSpan* prof = nullptr;   // the pool's last record, moved to prof_runs_ once the span is queued (deferred_.prof may point at it before)
    if (prof_this_run_) {
        if (prof_pool_.empty()) prof_pool_.push_back(std::make_unique<ProfSpan>(groups_.size()));
        prof = prof_pool_.back().get();
        prof->tail_held = prof->od = prof->od_tail = prof->meters = prof->meters_tail = false;
        hip_check(hipEventRecord(prof->begin, stream_), "hipEventRecord");
    }
    std::vector<PlotJob> jobs;
    size_t gi = 0;
    bool first_eq = true;
    for (Group& g : groups_) {
        const uint32_t n = (uint32_t)g.nodes.size();
        const size_t gf = frames * g.dom_num / g.dom_den;   // frames of this group's sample-rate domain
        const size_t gfpc = fpc * g.dom_num / g.dom_den;    // ... per tick
        const GateBits gates{(const uint32_t*)g.gates.p, g.gate_words, call_off};
        switch (g.kind) {
        case MX_KIND_AMPLIFIER: launch_amplifier((const AmpDesc*)desc_of(g), n, gf, stream_, fp_contract()); break;
        case MX_KIND_ENVELOPE: {
            const size_t need = envelope_scratch_bytes(n, gf);       // long streams: marker bitmaps and per-segment states (mx_k_envelope.hip)
            if (need && (g.spec.bytes < need || !g.spec.p)) { sync(); g.spec.alloc(need); }
            launch_envelope((const EnvDesc*)desc_of(g), (EnvState*)g.state.p, n, gf, gfpc, gates, t0, sample_rate_, stream_, fp_contract(), need ? g.spec.p : nullptr, need ? g.spec.bytes : 0);
            break;
        }
        case MX_KIND_EQ_THREE: {
            EqRun r{gf, gfpc, n_calls, fp_contract() ? 1u : 0u, t0, sample_rate_, 1.0 / sample_rate_, lo_f_, hi_f_, nullptr};
            uint32_t launch[5] = {MX_EQ_LAUNCH_SEQUENTIAL, 0u, 1u, (uint32_t)gf, 0u};   // what ran (mx_graph_debug_eq_launch)
            if (g.state2.p) {   // Envelopes folded into the epilogue: their state entering every tick of this span
                const size_t need = (size_t)n * n_calls * sizeof(EnvTick);
                if (g.env_ticks.bytes < need || !g.env_ticks.p) { sync(); g.env_ticks.alloc(need); }
                launch_env_ticks((const EnvTickDesc*)g.tick_desc.p, n, gates, n_calls, gfpc, t0, sample_rate_, (EnvTick*)g.env_ticks.p, stream_, fp_contract());
                r.ticks = (const EnvTick*)g.env_ticks.p;
            }
            if (eq_exact()) {
                EqSpecPlan plan;
                if (eq_plan_spec(n, gf, gfpc, lo_f_, hi_f_, plan, g.eq_mode == 6 || g.eq_mode == 7, g.eq_mode == 4 || g.eq_mode == 5)) {   // long streams: speculative time-parallel form, verified bit-exact
                    const size_t need = eq_spec_scratch_bytes(n, plan);
                    if (g.spec.bytes < need || !g.spec.p) { sync(); g.spec.alloc(need); }
                    if (!eq_stats_.p) { eq_stats_.alloc(8 * sizeof(uint64_t)); hip_check(hipMemset(eq_stats_.p, 0, 8 * sizeof(uint64_t)), "hipMemset"); }
                    gate_armed_ = false;
                    if (deferred_.pending) {
                        if (!gate_flag_.p) { gate_flag_.alloc(64); hip_check(hipMemset(gate_flag_.p, 0, 64), "hipMemset"); }
                        r.started = (uint32_t*)gate_flag_.p; r.started_seq = ++gate_seq_; gate_armed_ = true;
                    }
                    if (first_eq) {   // (mx_graph_debug_eq_env_rows: the launch's number, stored by the waves that take the row form)
                        if (!eq_rows_flag_.p) { eq_rows_flag_.alloc(64); hip_check(hipMemset(eq_rows_flag_.p, 0, 64), "hipMemset"); }
                        r.env_rows = (uint32_t*)eq_rows_flag_.p; r.env_rows_seq = ++eq_rows_seq_;
                    }
                    r.lean = eq_lean_ ? 1u : 0u;
                    const bool opens_gate = launch_eq_three_spec((const EqDesc*)desc_of(g), (EqState*)g.state.p, n, r, plan, g.eq_mode, g.spec.p, (uint64_t*)eq_stats_.p, stream_, launch, eq_env_rows_);
                    if (!opens_gate && !gate_test_) gate_armed_ = false;   // the direct form never stores the flag: a gate would spin to its time limit before the bank starts (MX_TAIL_GATE_TEST: tests of that bounded spin)
                    if (deferred_.pending) flush_deferred_tail(true);     // run k's Mixer bank: behind the gate this launch opens
                } else {
                    void* scratch = nullptr;
                    if (eq_use_poles_split(n, gf)) {     // short streams, few instances: two lanes per instance + a sample-parallel epilogue kernel
                        const size_t need = eq_poles_scratch_bytes(n, gf);
                        if (g.spec.bytes < need || !g.spec.p) { sync(); g.spec.alloc(need); }
                        scratch = g.spec.p;
                    }
                    launch_eq_three_exact((const EqDesc*)desc_of(g), (EqState*)g.state.p, n, r, scratch, stream_);
                    launch[1] = scratch ? 2u : 1u;   // lanes per instance: the split cascade, or one lane
                }
            } else {
                EqSplit sp{1u, 5u, 0u, 0u, gf, gf, nullptr, nullptr, nullptr};
                EqSpanPow pp{};
                eq_plan_split(n, gf, lo_f_, hi_f_, sp);
                if (sp.n_split > 1) {   // few instances, long streams: cut each stream into spans for different workgroups
                    const size_t need = (size_t)n * sp.n_split * 8 * sizeof(double) + (size_t)n * 12 * sizeof(double);
                    if (g.extra.bytes < need || !g.extra.p) { sync(); g.extra.alloc(need); }
                    sp.zbuf = (double*)g.extra.p;                         // [n][n_split][8] zero-state span end states
                    sp.bound = sp.zbuf + (size_t)n * sp.n_split * 8;      // [n][12] snapshot of the carried EqState
                    toeplitz_pow((long double)lo_f_, sp.span, pp.lo);
                    toeplitz_pow((long double)hi_f_, sp.span, pp.hi);
                }
                launch_eq_three_scan((const EqDesc*)desc_of(g), (EqState*)g.state.p, n, r, (const EqScanTab*)eq_tabs_.p, sp, pp, stream_);
                launch[0] = MX_EQ_LAUNCH_SCAN; launch[2] = sp.n_split; launch[3] = (uint32_t)sp.span; launch[4] = (uint32_t)sp.warm;
            }
            if (first_eq) {
                std::copy(launch, launch + 5, eq_launch_); first_eq = false;
                if (!r.env_rows) ++eq_rows_seq_;   // a launch of another form: the flag keeps an older launch's number
            }
            break;
        }
        case MX_KIND_FM_SINE: launch_fm_sine((const FmDesc*)desc_of(g), n, gf, t0, sample_rate_, stream_, sin_mode_); break;
        case MX_KIND_MIXER:
            if (overlap_this_run_ && (int)gi >= tail_gi_) {   // held back for the next run's EqThree launch, then beside its earlier groups (HBM-bound beside VALU-bound)
                if ((int)gi == tail_gi_) {
                    if (deferred_.pending) flush_deferred_tail(false);   // (a run whose earlier groups had no speculative EqThree launch: nothing opened a gate)
                    hip_check(hipEventRecord(ev_head_done_, stream_), "hipEventRecord");
                    deferred_.items.clear(); deferred_.outs.clear(); deferred_.taps.clear(); deferred_.parity = parity_; deferred_.prof = prof;
                    if (prof) prof->tail_held = true;
                }
                deferred_.items.push_back(TailLaunch{desc_of(g), n, g.max_taps, gf, g.dup_mode, prof ? prof->group_end[gi] : nullptr});
                if (gi + 1 == groups_.size()) deferred_.pending = true;
                ++gi;
                continue;
            }
            launch_mixer((const MixDesc*)desc_of(g), n, g.max_taps /* = most channels */, gf, g.dup_mode, stream_);
            break;
        case MX_KIND_OSCILLATOR: launch_oscillator((const OscDesc*)desc_of(g), n, gf, t0, sample_rate_, stream_, sin_mode_); break;
        case MX_KIND_STEREO_PANNER: launch_panner((const PanDesc*)desc_of(g), n, gf, stream_); break;
        case MX_KIND_STEREO_SPLITTER: launch_splitter((const SplitDesc*)desc_of(g), n, gf, stream_); break;
        case MX_KIND_TRIGGER: launch_trigger((const TrigDesc*)desc_of(g), n, gf, gfpc, &gates, stream_); break;
        case MX_KIND_FIR: launch_fir((const FirDesc*)desc_of(g), n, g.max_taps, gf, stream_, fp_contract()); break;
        case MX_KIND_RESAMPLE:
            launch_resample((const ResampleDesc*)desc_of(g), n, g.max_taps, g.rs_tab_doubles, g.rs_win_frames, frames * g.in_dom_num / g.in_dom_den, gf,
                            t0 * g.in_dom_num / g.in_dom_den, t0 * g.dom_num / g.dom_den, stream_, g.rs_common_up, fp_contract(), g.rs_common_taps, g.rs_common_down);
            break;
        case MX_KIND_PLOTTER: {
            jobs.clear();
            for (uint32_t id : g.nodes) {
                const Node& nd = nodes_[id];
                for (uint32_t c = 0; c < n_calls; ++c) {
                    if (!nd.plot_fired[call_off + c]) continue;
                    float* stage = (float*)plot_stage_.p + (size_t)nd.plot_slot[call_off + c] * 2 * fpc;
                    jobs.push_back(PlotJob{in_ptr(nd, 0, false, parity_) + (size_t)c * 2 * fpc, stage, stage + fpc});
                }
            }
            if (!jobs.empty()) {
                PlotJob* dst = (PlotJob*)plot_jobs_.p + plot_job_off_;
                stage_upload(dst, jobs.data(), jobs.size() * sizeof(PlotJob));
                launch_plotter(dst, (uint32_t)jobs.size(), fpc, stream_);
                plot_job_off_ += jobs.size();
            }
            break;
        }
        default: break;
        }
        // an event costs ~5 us of stream time: none for groups that launch nothing (sources, video kinds)
        if (prof && group_launches(g)) hip_check(hipEventRecord(prof->group_end[gi], stream_), "hipEventRecord");
        ++gi;
    }
    // video sub-graph: tick by tick (frames arrive per tick; nothing to batch over time)
    if (plan_.has_video) {
        for (uint32_t c = 0; c < n_calls; ++c) run_video_tick(t0 + (uint64_t)c * fpc, call_off + c);
        flush_scales(stream_);
        for (uint32_t id : plan_.video_order) if (nodes_[id].rgba) nodes_[id].rgba->end_run(stream_);   // the last ticks' sinks
    }
    if (prof && plan_.has_video) hip_check(hipEventRecord(prof->video_end, stream_), "hipEventRecord");
    // after everything else of the span on stream_ (the video section included): its profile interval starts at the latest event recorded there
    launch_outputs(t0, call_off, n_calls, prof);
    // the port buffers hold every tick of the run: the audio tap sets go once, after its last span, in this order on either stream
    if (call_off + n_calls == run_calls) for (AudioTapSet* s : taps_) launch_tap_set(*s, run_calls, prof);
    if (prof) { prof_runs_.push_back(std::move(prof_pool_.back())); prof_pool_.pop_back(); }
}

static bool group_launches(const Group& g) {
    switch (g.kind) {
    case MX_KIND_SOURCE_MONO: case MX_KIND_SOURCE_STEREO: case MX_KIND_SOURCE_VIDEO:
    case MX_KIND_VIDEO_MIXER: case MX_KIND_VIDEO_TO_RGBA: case MX_KIND_MONITOR: return false;   // bound buffers / the per-tick video section
    default: return true;
    }
}

void Graph::profile_enable(bool on) { prof_on_ = on; }

Graph::ProfSpan::ProfSpan(size_t n_groups) : group_end(n_groups) {
    for (hipEvent_t* e : {&begin, &video_end, &tail_begin, &od_end, &od_tail_end, &meters_end, &meters_tail_end}) hip_check(hipEventCreate(e), "hipEventCreate");
    for (hipEvent_t& e : group_end) hip_check(hipEventCreate(&e), "hipEventCreate");
}

Graph::ProfSpan::~ProfSpan() {
    for (hipEvent_t e : {begin, video_end, tail_begin, od_end, od_tail_end, meters_end, meters_tail_end}) (void)hipEventDestroy(e);
    for (hipEvent_t e : group_end) (void)hipEventDestroy(e);
}

uint32_t Graph::profile_collect(float* ms_by_kind, float* ms_total) {
    sync();
    if (ms_by_kind) for (int k = 0; k < MX_PROFILE_KINDS; ++k) ms_by_kind[k] = 0.f;
    if (ms_total) *ms_total = 0.f;
    const uint32_t n = prof_runs_count_;   // run() calls; a run cut into spans recorded one record per span
    prof_runs_count_ = 0;
    auto elapsed = [](hipEvent_t from, hipEvent_t to) { float ms = 0.f; hip_check(hipEventElapsedTime(&ms, from, to), "hipEventElapsedTime"); return ms; };
    for (auto& rec : prof_runs_) {
        const ProfSpan& p = *rec;
        perf_group_ms_.assign(groups_.size() + 1, 0.f);
        hipEvent_t last = p.begin;   // the latest event recorded on stream_
        for (size_t i = 0; i < groups_.size(); ++i) {
            if (!group_launches(groups_[i])) continue;
            float ms;
            if (p.tail_held && (int)i >= tail_gi_) {
                // a tail launch that was held back ran on its own stream, inside the NEXT run's window: its own begin (the tail's, or the tail group's before it) and end;
                // the run's total ends where its stream's work did
                ms = elapsed((int)i == tail_gi_ ? p.tail_begin : p.group_end[i - 1], p.group_end[i]);
            } else {
                ms = elapsed(last, p.group_end[i]);
                last = p.group_end[i];
            }
            if (ms_by_kind) ms_by_kind[groups_[i].kind] += ms;
            perf_group_ms_[i] = ms;
        }
        if (plan_.has_video) {
            const float ms = elapsed(last, p.video_end);
            if (ms_by_kind) ms_by_kind[MX_KIND_VIDEO_MIXER] += ms;
            perf_group_ms_[groups_.size()] = ms;
            last = p.video_end;
        }
        // OutputDevice launches: on stream_ after the span's groups and video section (`last` is the latest event before them there; their end
        // is the run's), or behind the tail on its stream (from the last tail group's event)
        perf_od_ms_ = 0.f;
        hipEvent_t end = last;
        if (p.od) { perf_od_ms_ += elapsed(last, p.od_end); end = p.od_end; }
        if (p.od_tail) perf_od_ms_ += elapsed(p.group_end.back(), p.od_tail_end);
        // meter, spectrum, loudness, stereo field and limiter launches: no kind of their own, counted in the total (and so in engine_us): on stream_ last of all, or on the tail stream
        // behind the tail (and its OutputDevices)
        if (p.meters) end = p.meters_end;
        perf_total_ms_ = elapsed(p.begin, end);
        if (ms_total) *ms_total += perf_total_ms_;
        if (p.meters_tail) {
            const float ms = elapsed(p.od_tail ? p.od_tail_end : p.group_end.back(), p.meters_tail_end);
            if (ms_total) *ms_total += ms;
            perf_total_ms_ += ms;
        }
        perf_calls_ = last_calls_;
        if (perf_calls_ && perf_total_ms_ * 1000.0 / perf_calls_ > 1e6 / (double)tps_)   // timing.rs:37-40: the tick ran over its budget
            perf_last_lag_s_ = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
        prof_pool_.push_back(std::move(rec));
    }
    prof_runs_.clear();
    return n;
}

// -------------------------------------------------------------------------------------------------
// state that a module carries from tick to tick, as device regions in a canonical order per kind
// -------------------------------------------------------------------------------------------------
std::vector<Graph::StateLoc> Graph::state_locs(uint32_t id) const {
    std::vector<StateLoc> out;
    const Node& n = nodes_[id];
    switch (n.kind) {
    case MX_KIND_EQ_THREE:
        if (n.group >= 0 && groups_[n.group].state.p) out.push_back({(EqState*)groups_[n.group].state.p + n.slot, sizeof(EqState)});
        break;
    case MX_KIND_ENVELOPE:
        if (n.elided && n.owner >= 0 && nodes_[n.owner].kind == MX_KIND_EQ_THREE) {   // evaluated inline by the EqThree kernel
            const Node& e = nodes_[n.owner];
            if (e.group >= 0 && groups_[e.group].state2.p) out.push_back({(EnvState*)groups_[e.group].state2.p + e.slot, sizeof(EnvState)});
        } else if (n.group >= 0 && groups_[n.group].state.p) {
            out.push_back({(EnvState*)groups_[n.group].state.p + n.slot, sizeof(EnvState)});
        }
        break;
    case MX_KIND_FIR: case MX_KIND_RESAMPLE:
        if (n.group >= 0 && groups_[n.group].state.p) {
            size_t off = 0, mine = 0;
            for (uint32_t other : groups_[n.group].nodes) {
                const size_t h = history_frames(nodes_[other]);
                if (other == id) { mine = h; break; }
                off += h;
            }
            out.push_back({(float2*)groups_[n.group].state.p + off, mine * sizeof(float2)});
        }
        break;
    default: break;
    }
    return out;
}

size_t Graph::state_bytes(uint32_t id) const {
    const Node& n = nodes_[id];
    switch (n.kind) {
    case MX_KIND_EQ_THREE: return sizeof(EqState);
    case MX_KIND_ENVELOPE: return sizeof(EnvState);
    case MX_KIND_FIR: case MX_KIND_RESAMPLE: return (size_t)history_frames(n) * sizeof(float2);
    default: return 0;
    }
}

void Graph::adopt_state(Graph& old, const int32_t* old_of_new, size_t n) {
    if (n != nodes_.size()) throw Error(MX_ERR_INVALID, "old_node_of_new must have one entry per node of the new graph");
    if (n && !old_of_new) throw Error(MX_ERR_INVALID, "old_node_of_new is NULL");
    for (size_t i = 0; i < n; ++i) {
        const int32_t j = old_of_new[i];
        if (j < 0) continue;
        if ((size_t)j >= old.nodes_.size()) throw Error(MX_ERR_INVALID, "old node out of range");
        if (old.nodes_[j].kind != nodes_[i].kind) throw Error(MX_ERR_TYPE, "a module cannot change kind across a topology edit");
    }
    old.sync(); sync();
    lineage_ = old.lineage_;   // to a key-locked deck this graph is the old one: its grain clock goes on (mx_deck_feed)
    hip_check(hipSetDevice(device_), "hipSetDevice");
    std::vector<CopyJob> jobs;   // thousands of small states (a 1024-strip graph: 2048 of 24 - 136 bytes): one launch, not one copy each
    for (size_t i = 0; i < n; ++i) {
        const int32_t j = old_of_new[i];
        if (j < 0) continue;
        const auto a = state_locs((uint32_t)i), b = old.state_locs((uint32_t)j);
        for (size_t k = 0; k < a.size() && k < b.size(); ++k)
            if (a[k].bytes == b[k].bytes && a[k].bytes)   // a filter whose length changed starts from silence
                jobs.push_back(CopyJob{a[k].p, b[k].p, a[k].bytes});
        // A module outside the run order (a cycle that feeds no terminal module) is served by no launch and has no state on the device, but
        // it persists like any other: what it carried waits on the host until an edit brings it back into the order.
        Node& nn = nodes_[i]; const Node& on = old.nodes_[j];
        if (a.empty() && state_bytes((uint32_t)i)) {
            if (!b.empty()) {
                nn.parked.resize(b[0].bytes);
                hip_check(hipMemcpy(nn.parked.data(), b[0].p, b[0].bytes, hipMemcpyDeviceToHost), "hipMemcpy(parked state)");
            } else {
                nn.parked = on.parked;
            }
            if (nn.parked.size() != state_bytes((uint32_t)i)) nn.parked.clear();   // a filter whose length changed starts from silence
        } else if (!a.empty() && b.empty() && on.parked.size() == a[0].bytes && a[0].bytes) {
            hip_check(hipMemcpy(a[0].p, on.parked.data(), a[0].bytes, hipMemcpyHostToDevice), "hipMemcpy(parked state)");
        }
    }
    DevBuf job_buf;
    if (!jobs.empty()) {
        job_buf.alloc(jobs.size() * sizeof(CopyJob));
        hip_check(hipMemcpyAsync(job_buf.p, jobs.data(), jobs.size() * sizeof(CopyJob), hipMemcpyHostToDevice, stream_), "hipMemcpyAsync(adopt jobs)");
        launch_copy_jobs((const CopyJob*)job_buf.p, (uint32_t)jobs.size(), stream_);
        sync();                   // `jobs` and job_buf go out of scope
    }
    for (size_t i = 0; i < n; ++i) {
        const int32_t j = old_of_new[i];
        if (j < 0) continue;
        Node& nn = nodes_[i]; Node& on = old.nodes_[j];
        if (nn.kind == MX_KIND_PLOTTER) nn.plot_count = on.plot_count;          // plotter.rs:37-40
        if (nn.mon) { nn.mon->has_epoch = on.mon->has_epoch; nn.mon->epoch = on.mon->epoch; nn.mon->queued = on.mon->queued; }   // Monitor.epoch (monitor.rs:122)
        if (nn.kind == MX_KIND_VIDEO_MIXER && on.vmixer) {                       // stored frames, scalers, expiry times
            mx_video_mixer_params p; std::memcpy(&p, nn.params.data(), sizeof p);
            nn.vmixer = std::move(on.vmixer);
            nn.vmixer->rebind(stream_, nn.vlazy, tps_);   // the old graph's stream may be gone after this call; this graph's fusion plan and tick rate apply
            nn.vmixer->update(p);
        }
        if (nn.kind == MX_KIND_OUTPUT_DEVICE) {   // the module persists: its stored assignment, scratch, clip / lag times and statuses, a pending lag note
            nn.od->adopt(*on.od, od_ticks(), stream_);
            nn.params = on.params;   // (mixlab_gpu.h: the new build's params are not applied)
        }
        if (nn.vsrc) nn.vsrc->adopt(*on.vsrc);
    }
    hip_check(hipStreamSynchronize(stream_), "hipStreamSynchronize");
}

Graph::Perf Graph::performance_info(uint64_t* module_us, size_t cap) {
    if (cap < nodes_.size() && module_us) throw Error(MX_ERR_INVALID, "module_us is shorter than the node count");
    Perf pf{};
    pf.tick_rate = tps_;
    pf.tick_budget_us = 1000000ull / tps_;                                          // timing.rs:9
    const double calls = perf_calls_ ? (double)perf_calls_ : 1.0;
    const double tick_us = perf_total_ms_ * 1000.0 / calls;
    pf.realtime = perf_calls_ != 0 && tick_us < (double)pf.tick_budget_us;         // timing.rs:33
    if (perf_last_lag_s_ >= 0.0) {                                                  // util.rs:47-60
        const double since = std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() - perf_last_lag_s_;
        pf.lag = since < 0.1 ? 2 : (since < 5.0 ? 1 : 0);
    }
    if (module_us) for (size_t i = 0; i < nodes_.size(); ++i) module_us[i] = 0;
    double accounted = 0.0;
    for (size_t gi = 0; gi < groups_.size() && gi < perf_group_ms_.size(); ++gi) {
        // one launch serves every module of the group and the modules folded into them: the launch's time per tick is
        // split evenly over all of those (PerformanceAccount::Module, timing.rs:86-94)
        std::vector<uint32_t> members;
        for (uint32_t id : groups_[gi].nodes) {
            members.push_back(id);
            const Node& nd = nodes_[id];
            for (int32_t f : {nd.fuse_pan, nd.fuse_amp, nd.fuse_env, nd.fuse_trigger}) if (f >= 0) members.push_back((uint32_t)f);
            if (nd.fuse_env >= 0 && nodes_[nd.fuse_env].fuse_trigger >= 0) members.push_back((uint32_t)nodes_[nd.fuse_env].fuse_trigger);
        }
        if (members.empty()) continue;
        const double us = perf_group_ms_[gi] * 1000.0 / calls;
        accounted += us;
        if (module_us) for (uint32_t id : members) module_us[id] += (uint64_t)(us / (double)members.size() + 0.5);
    }
    if (plan_.has_video && perf_group_ms_.size() > groups_.size()) {   // the per-tick video section
        std::vector<uint32_t> members;
        for (size_t i = 0; i < nodes_.size(); ++i) if (nodes_[i].kind == MX_KIND_VIDEO_MIXER || nodes_[i].kind == MX_KIND_VIDEO_TO_RGBA || nodes_[i].kind == MX_KIND_MONITOR) members.push_back((uint32_t)i);
        const double us = perf_group_ms_[groups_.size()] * 1000.0 / calls;
        accounted += us;
        if (module_us) for (uint32_t id : members) module_us[id] += (uint64_t)(us / (double)members.size() + 0.5);
    }
    if (!plan_.od_nodes.empty()) {   // OutputDevice launches, split evenly over the nodes
        const double us = perf_od_ms_ * 1000.0 / calls;
        accounted += us;
        if (module_us) for (uint32_t id : plan_.od_nodes) module_us[id] += (uint64_t)(us / (double)plan_.od_nodes.size() + 0.5);
    }
    pf.engine_us = (uint64_t)std::max(0.0, tick_us - accounted + 0.5);             // PerformanceAccount::Engine = tick - modules (timing.rs:43)
    return pf;
}

void Graph::read_output(uint32_t node, uint32_t port, float* host, size_t frames, size_t first_frame) {
    hip_check(hipSetDevice(device_), "hipSetDevice");
    wait_tail(-1);
    if (node >= nodes_.size() || port >= nodes_[node].out_type.size()) throw Error(MX_ERR_INVALID, "output terminal out of range");
    if (first_frame > cap_frames_ || frames > cap_frames_ - first_frame) throw Error(MX_ERR_INVALID, "more ticks than max_ticks_per_run");
    if (frames && !host) throw Error(MX_ERR_INVALID, "host_samples is NULL");
    const Node& n = nodes_[node];
    if (n.out_elided[port]) throw Error(MX_ERR_INVALID, "port is not materialised: it only feeds a fused consumer (build with MX_FLAG_NO_FUSE to observe it)");
    // the port's own sample-rate domain; a window starts and ends where whole ticks do
    const size_t f0 = first_frame * n.dom_num / n.dom_den;
    frames = (first_frame + frames) * n.dom_num / n.dom_den - f0;
    if (n.out_dup[port]) {   // stored as one float per frame (L == R): expand for the caller
        hip_check(hipMemcpyAsync(host, out_ptr(n, port, parity_) + f0, frames * sizeof(float), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H)");
        sync();
        for (size_t i = frames; i-- > 0;) { const float v = host[i]; host[2 * i] = v; host[2 * i + 1] = v; }
        return;
    }
    const size_t fpf = floats_per_frame(n.out_type[port]);
    hip_check(hipMemcpyAsync(host, out_ptr(n, port, parity_) + fpf * f0, fpf * frames * sizeof(float), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H)");
    sync();
}

void Graph::read_audio_out(uint32_t node, uint32_t first, uint32_t n, float* samples, size_t samples_cap, OutTick* ticks, size_t* n_samples) {
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (node >= nodes_.size() || nodes_[node].kind != MX_KIND_OUTPUT_DEVICE) throw Error(MX_ERR_INVALID, "node is not an OUTPUT_DEVICE");
    if ((uint64_t)first + n > last_calls_) throw Error(MX_ERR_INVALID, "the window lies beyond the last run");
    const Node& nd = nodes_[node];
    const size_t a = nd.od->offset(first), b = nd.od->offset(first + n);
    if (n_samples) *n_samples = b - a;
    if (!samples && !ticks) return;
    if (samples && samples_cap < b - a) throw Error(MX_ERR_INVALID, "samples_cap is smaller than the window's samples");
    wait_tail(-1);
    if (samples && b > a) hip_check(hipMemcpyAsync(samples, (const float*)nd.od->out.p + a, (b - a) * sizeof(float), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H)");
    if (ticks && n) hip_check(hipMemcpyAsync(ticks, (const OutTick*)nd.od->rec.p + first, (size_t)n * sizeof(OutTick), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H)");
    sync();
}

void Graph::audio_out_lag(uint32_t node) {
    if (node >= nodes_.size() || nodes_[node].kind != MX_KIND_OUTPUT_DEVICE) throw Error(MX_ERR_INVALID, "node is not an OUTPUT_DEVICE");
    nodes_[node].od->lag.store(true);   // AtomicBool::store (output_device.rs:126); nothing else of the graph is touched
}

// ---- the audio tap sets (mx_taps.hpp): what the engine keeps of them is the port a set sees, the list in launch order (taps_) and where a run's launches go ----

bool Graph::tap_port(mx_port_ref r, TapPort& t) const {
    if (r.node >= nodes_.size() || r.port >= nodes_[r.node].out_type.size()) return false;
    const Node& nd = nodes_[r.node];
    int32_t o = (int32_t)r.node;
    while (nodes_[o].elided && nodes_[o].owner >= 0) o = nodes_[o].owner;   // the node whose launch writes the port
    t.type = nd.out_type[r.port]; t.dup = nd.out_dup[r.port]; t.elided = nd.out_elided[r.port];
    t.on_tail = tail_gi_ >= 0 && nodes_[o].group >= tail_gi_; t.dom_num = nd.dom_num; t.dom_den = nd.dom_den;
    for (uint32_t par = 0; par < 2 && !t.elided; ++par)   // the port at tick 0 of the run (out_ptr without a span's offset)
        t.p[par] = nd.bound && r.port == 0 ? nd.bound : (const float*)slab_.p + (par && nd.out_off2[r.port] != SIZE_MAX ? nd.out_off2[r.port] : nd.out_off[r.port]);
    return true;
}

// (known wart: an upload that throws leaves the sets before it built for the new call length and tap_fpc_ at the old one)
void Graph::reupload_taps(size_t fpc) {
    for (AudioTapSet* s : taps_) if (!s->empty()) s->upload(fpc);
    tap_fpc_ = fpc;
}

// The run's launches of one tap set, after its last span and behind the sets before it: the set fixes the run struct of the whole set
// (begin_run), the engine says which taps go where.  Why no buffer a tap reads is overwritten before it has read it:
//  - a tap read on stream_ (every tap when the run is on one stream: a cut run, a short one in the automatic mode, a graph without the mode)
//    is queued there behind the run's producers and ahead of the next run's launches, which are the only ones that write that port again.  Its
//    descriptor points at THIS run's buffer parity: the tail-read ports alternate per run, run k + 1 writes the other buffer, and run k + 2 --
//    the next writer of this one -- comes after the tap on the same stream;
//  - a tap on an output of the tail (the Mixer bank and the buses above it) is held back with it (deferred_.taps) and goes on the tail
//    stream behind the tail's last launch.  Those outputs are single buffers written only by the tail, whose next launch (run k + 1's) is
//    queued behind this one on that same stream.  ev_tail_done_ is recorded after it, so every join -- a read-back of the records,
//    read_output, a run that reuses this parity -- covers the tap too.
// The sets only read the ports and write disjoint records, so none disturbs another.  Within a set, the records and the carried state of the
// two groups of taps are disjoint (slots), and a group's launches of consecutive runs follow each other on that group's stream (a run that
// changes the stream of the tail's taps has joined the tail first: run()'s wait_tail) -- so state that one run hands to the next, updated
// in place or through a pair of buffers that flips once per run for both groups, is read after it was written.
void Graph::launch_tap_set(AudioTapSet& s, uint32_t n_calls, ProfSpan* prof) {
    if (s.empty()) return;
    s.begin_run(n_calls);
    const uint32_t n = s.size(), n_head = overlap_this_run_ ? s.n_head : n;
    if (n_head < n) deferred_.taps.push_back(&s);   // (the rest of the set's run, from its run struct: flush_deferred_tail)
    if (n_head) s.launch(0, n_head, parity_, stream_);
    if (!prof) return;
    if (n_head) { hip_check(hipEventRecord(prof->meters_end, stream_), "hipEventRecord"); prof->meters = true; }   // (again, when an earlier set recorded it: the later record holds)
    prof->meters_tail = !deferred_.taps.empty();
}

void Graph::read_output_i16(uint32_t node, uint32_t port, int16_t* host, size_t frames) {
    hip_check(hipSetDevice(device_), "hipSetDevice");
    wait_tail(-1);
    if (node >= nodes_.size() || port >= nodes_[node].out_type.size()) throw Error(MX_ERR_INVALID, "output terminal out of range");
    if (frames > cap_frames_) throw Error(MX_ERR_INVALID, "more ticks than max_ticks_per_run");
    if (frames && !host) throw Error(MX_ERR_INVALID, "host_samples is NULL");
    const Node& n = nodes_[node];
    if (n.out_elided[port]) throw Error(MX_ERR_INVALID, "port is not materialised: it only feeds a fused consumer (build with MX_FLAG_NO_FUSE to observe it)");
    const size_t cnt = floats_per_frame(n.out_type[port]) * (frames * n.dom_num / n.dom_den);
    if (!cnt) return;
    if (conv_stage_.bytes < cnt * sizeof(int16_t)) { sync(); conv_stage_.alloc(cnt * sizeof(int16_t)); }
    launch_f32_to_i16(out_ptr(n, port, parity_), (int16_t*)conv_stage_.p, cnt, n.out_dup[port] ? 1 : 0, stream_);
    hip_check(hipMemcpyAsync(host, conv_stage_.p, cnt * sizeof(int16_t), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H i16)");
    sync();
}

void Graph::write_source_i16(uint32_t node, const int16_t* host, size_t frames) {
    hip_check(hipSetDevice(device_), "hipSetDevice");
    if (node >= nodes_.size()) throw Error(MX_ERR_INVALID, "node out of range");
    Node& n = nodes_[node];
    if (n.kind != MX_KIND_SOURCE_MONO && n.kind != MX_KIND_SOURCE_STEREO) throw Error(MX_ERR_INVALID, "node is not a SOURCE_*");
    if (n.bound) throw Error(MX_ERR_INVALID, "source is bound to a caller device buffer");
    if (frames > cap_frames_) throw Error(MX_ERR_INVALID, "more ticks than max_ticks_per_run");
    if (frames && !host) throw Error(MX_ERR_INVALID, "host_samples is NULL");
    const size_t cnt = floats_per_frame(n.out_type[0]) * frames;
    if (!cnt) return;
    if (conv_stage_.bytes < cnt * sizeof(int16_t)) { sync(); conv_stage_.alloc(cnt * sizeof(int16_t)); }
    hip_check(hipMemcpyAsync(conv_stage_.p, host, cnt * sizeof(int16_t), hipMemcpyHostToDevice, stream_), "hipMemcpyAsync(H2D i16)");
    launch_i16_to_f32((const int16_t*)conv_stage_.p, out_ptr(n, 0, parity_), cnt, stream_);
    sync();   // host buffer is the caller's again on return
}

void* Graph::debug_eq_records(size_t* bytes) const {
    for (const Group& g : groups_)
        if (g.kind == MX_KIND_EQ_THREE && g.spec.p) { if (bytes) *bytes = g.spec.bytes; return g.spec.p; }
    if (bytes) *bytes = 0;
    return nullptr;
}

bool Graph::eq_env_rows() {
    if (!eq_rows_flag_.p || !eq_rows_seq_) return false;
    sync();
    uint32_t v = 0;
    hip_check(hipMemcpy(&v, eq_rows_flag_.p, sizeof v, hipMemcpyDeviceToHost), "hipMemcpy(eq env rows)");
    return v == eq_rows_seq_;
}

uint32_t Graph::eq_lean() {
    if (!eq_rows_flag_.p || !eq_rows_seq_) return 0u;
    sync();
    uint32_t v[3] = {0u, 0u, 0u};
    hip_check(hipMemcpy(v, eq_rows_flag_.p, sizeof v, hipMemcpyDeviceToHost), "hipMemcpy(eq lean)");
    return (v[1] == eq_rows_seq_ ? 1u : 0u) | (v[2] == eq_rows_seq_ ? 2u : 0u);
}

float* Graph::output_ptr(uint32_t node, uint32_t port, size_t* fpf, bool stream_ordered_consumer) {
    if (node >= nodes_.size() || port >= nodes_[node].out_type.size()) throw Error(MX_ERR_INVALID, "output terminal out of range");
    if (nodes_[node].out_elided[port]) throw Error(MX_ERR_INVALID, "port is not materialised: it only feeds a fused consumer (build with MX_FLAG_NO_FUSE to observe it)");
    if (nodes_[node].out_dup[port]) throw Error(MX_ERR_INVALID, "port is stored as one float per frame (L == R fused result): use mx_graph_read_output, or build with MX_FLAG_NO_FUSE");
    if (fpf) *fpf = floats_per_frame(nodes_[node].out_type[port]) * (spt_ * nodes_[node].dom_num / nodes_[node].dom_den);   // floats per TICK in the port's own rate domain
    // A consumer that takes the raw pointer of a bus reads it in stream order on stream(): a Mixer bank the library moved to the second stream ON ITS OWN (short submissions,
    // MX_OVERLAP_AUTO) would not be ordered before it -- so the automatism ends here, for good.  (A host that asked for MX_FLAG_OVERLAP_TAIL knows about mx_graph_tail_stream.)
    // The same holds for a port the tail READS: it is double-buffered while the mode is on, and a raw pointer would see fresh data only every other run.
    if (stream_ordered_consumer && tail_gi_ >= 0 && tail_auto_ && (nodes_[node].group >= tail_gi_ || nodes_[node].out_off2[port] != SIZE_MAX)) end_auto_tail();
    return out_ptr(nodes_[node], port, parity_);
}

int Graph::read_plotter(uint32_t node, uint32_t call, float* left, float* right) {
    if (node >= nodes_.size() || nodes_[node].kind != MX_KIND_PLOTTER) throw Error(MX_ERR_INVALID, "node is not a Plotter");
    const Node& n = nodes_[node];
    if (call >= n.plot_fired.size()) throw Error(MX_ERR_INVALID, "tick_in_run is outside the last run");
    if (!n.plot_fired[call]) return 0;
    const size_t fpc = last_frames_per_call_;
    const float* stage = (const float*)plot_stage_.p + (size_t)n.plot_slot[call] * 2 * fpc;
    hip_check(hipMemcpyAsync(left, stage, fpc * sizeof(float), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H)");
    hip_check(hipMemcpyAsync(right, stage + fpc, fpc * sizeof(float), hipMemcpyDeviceToHost, stream_), "hipMemcpyAsync(D2H)");
    sync();
    return 1;
}

}  // namespace mx
