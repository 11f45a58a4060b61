// mx_plan.cpp -- the graph compiler.  See mx_plan.hpp.  Host arithmetic only: nothing here opens a device.
#include "mx_plan.hpp"
#include "mx_kernels.hpp"   // eq_epilogue_mode, MX_EQF_*

#include <algorithm>
#include <cstring>
#include <string>

namespace mx {

// ModuleT::inputs()/outputs() of each kind (reference file:line in include/mixlab_gpu.h)
static void kind_ports(uint32_t kind, size_t params_len, std::vector<uint8_t>& in, std::vector<uint8_t>& out) {
    auto need = [&](size_t sz, const char* name) {
        if (params_len != sz) throw Error(MX_ERR_INVALID, std::string("params_len does not match ") + name);
    };
    switch (kind) {
    case MX_KIND_AMPLIFIER: need(sizeof(mx_amplifier_params), "mx_amplifier_params"); in = {MX_STEREO, MX_MONO}; out = {MX_STEREO}; break;
    case MX_KIND_ENVELOPE: need(sizeof(mx_envelope_params), "mx_envelope_params"); in = {MX_MONO}; out = {MX_MONO}; break;
    case MX_KIND_EQ_THREE: need(sizeof(mx_eq_three_params), "mx_eq_three_params"); in = {MX_MONO}; out = {MX_MONO}; break;
    case MX_KIND_FM_SINE: need(sizeof(mx_fm_sine_params), "mx_fm_sine_params"); in = {MX_MONO}; out = {MX_STEREO}; break;
    case MX_KIND_MIXER: {
        if (params_len % sizeof(mx_mixer_channel_params)) throw Error(MX_ERR_INVALID, "mixer params_len is not a multiple of mx_mixer_channel_params");
        in.assign(params_len / sizeof(mx_mixer_channel_params), MX_STEREO); out = {MX_STEREO, MX_STEREO}; break;
    }
    case MX_KIND_OSCILLATOR: need(sizeof(mx_oscillator_params), "mx_oscillator_params"); in = {}; out = {MX_MONO, MX_STEREO}; break;
    case MX_KIND_PLOTTER: need(0, "() (Plotter has no params)"); in = {MX_STEREO}; out = {}; break;
    case MX_KIND_STEREO_PANNER: need(0, "()"); in = {MX_MONO, MX_MONO}; out = {MX_STEREO}; break;
    case MX_KIND_STEREO_SPLITTER: need(0, "()"); in = {MX_STEREO}; out = {MX_MONO, MX_MONO}; break;
    case MX_KIND_TRIGGER: need(sizeof(mx_trigger_params), "mx_trigger_params"); in = {}; out = {MX_MONO}; break;
    case MX_KIND_SOURCE_MONO: in = {}; out = {MX_MONO}; break;
    case MX_KIND_SOURCE_STEREO: in = {}; out = {MX_STEREO}; break;
    case MX_KIND_VIDEO_MIXER: need(sizeof(mx_video_mixer_params), "mx_video_mixer_params"); in.assign(4, MX_VIDEO); out.assign(3, MX_VIDEO); break;  // video_mixer.rs:42-49
    case MX_KIND_SOURCE_VIDEO: in = {}; out = {MX_VIDEO}; break;
    case MX_KIND_FIR: in = {MX_STEREO}; out = {MX_STEREO}; break;        // blob checked by check_blobs
    case MX_KIND_RESAMPLE: in = {MX_STEREO}; out = {MX_STEREO}; break;
    case MX_KIND_VIDEO_TO_RGBA: need(sizeof(mx_video_to_rgba_params), "mx_video_to_rgba_params"); in = {MX_VIDEO}; out = {}; break;
    case MX_KIND_MONITOR:   // monitor.rs:99-102
        if (params_len != sizeof(mx_monitor_params_ex)) need(sizeof(mx_monitor_params), "mx_monitor_params (or mx_monitor_params_ex)");
        in = {MX_VIDEO, MX_STEREO}; out = {}; break;
    case MX_KIND_OUTPUT_DEVICE: need(sizeof(mx_output_device_params), "mx_output_device_params"); in = {MX_STEREO}; out = {}; break;   // output_device.rs:80-81
    default: throw Error(MX_ERR_INVALID, "unknown module kind");
    }
}

void check_output_device_params(const void* params) {
    mx_output_device_params p; std::memcpy(&p, params, sizeof p);
    if (p.channels > 256 || p.left < -1 || p.right < -1) throw Error(MX_ERR_INVALID, "mx_output_device_params: channels <= 256, left / right >= -1 (-1 = None)");
}

static inline size_t floats_per_frame(uint8_t lt) { return lt == MX_MONO ? 1 : (lt == MX_STEREO ? 2 : 0); }
static inline bool is_video_kind(uint32_t k) { return k == MX_KIND_VIDEO_MIXER || k == MX_KIND_SOURCE_VIDEO || k == MX_KIND_VIDEO_TO_RGBA || k == MX_KIND_MONITOR; }

// Run order: DFS through inputs from terminal modules (src/engine.rs:408-457).  The reference
// iterates a HashSet (unspecified order); ascending id is one of its valid orders.
static void run_order(Plan& P, const mx_edge* edges, size_t n_edges) {
    const size_t n_nodes = P.nodes.size();
    std::vector<uint8_t> feeds(n_nodes, 0), seen(n_nodes, 0);
    for (size_t e = 0; e < n_edges; ++e) feeds[edges[e].src_node] = 1;
    // iterative DFS (graphs with 1e5 nodes must not blow the stack)
    struct Frame { uint32_t id; uint32_t next; };
    std::vector<Frame> stack;
    for (uint32_t root = 0; root < n_nodes; ++root) {
        if (feeds[root] || seen[root]) continue;
        seen[root] = 1; stack.push_back({root, 0});
        while (!stack.empty()) {
            Frame& f = stack.back();
            const PlanNode& n = P.nodes[f.id];
            if (f.next < n.in_src.size()) {
                const PortRef pr = n.in_src[f.next++];
                if (pr.node >= 0 && !seen[pr.node]) { seen[pr.node] = 1; stack.push_back({(uint32_t)pr.node, 0}); }
            } else {
                P.order.push_back(f.id);
                stack.pop_back();
            }
        }
    }
    // A cycle with no terminal module is never reached from a terminal, so the reference never runs
    // it (engine.rs:428-430); we mirror that: such nodes stay out of the order.
    for (size_t i = 0; i < P.order.size(); ++i) P.nodes[P.order[i]].pos = (int)i;
    // dependency levels; an input whose producer runs later this tick is a back-edge and reads
    // Disconnected (engine.rs:479-482: buffers.get(output_id) is None)
    for (uint32_t id : P.order) {
        PlanNode& n = P.nodes[id];
        int lvl = 0;
        for (PortRef& pr : n.in_src) {
            if (pr.node < 0) continue;
            if (P.nodes[pr.node].pos < 0 || P.nodes[pr.node].pos >= n.pos) { pr.node = -1; continue; }  // back-edge => Disconnected
            lvl = std::max(lvl, P.nodes[pr.node].level + 1);
        }
        n.level = lvl;
    }
}

// variable-length blobs of the build-specified modules; what they say about the node's carried history
static void check_blobs(Plan& P, const mx_node* nodes) {
    for (size_t i = 0; i < P.nodes.size(); ++i) {
        PlanNode& n = P.nodes[i];
        const size_t len = nodes[i].params_len;
        if (n.kind == MX_KIND_FIR) {
            mx_fir_params h{}; if (len >= sizeof h) std::memcpy(&h, nodes[i].params, sizeof h);
            if (len < sizeof h || h.n_taps == 0 || h.n_taps > 16384 || len != sizeof h + (size_t)h.n_taps * sizeof(double))
                throw Error(MX_ERR_INVALID, "mx_fir_params: params_len must be 8 + 8 * n_taps (1 <= n_taps <= 16384)");
            n.history = h.n_taps;
        } else if (n.kind == MX_KIND_RESAMPLE) {
            mx_resample_params h{}; if (len >= sizeof h) std::memcpy(&h, nodes[i].params, sizeof h);
            if (len < sizeof h || !h.up || !h.down || !h.taps_per_phase || h.taps_per_phase > 4096 ||
                len != sizeof h + (size_t)h.up * h.taps_per_phase * sizeof(double))
                throw Error(MX_ERR_INVALID, "mx_resample_params: params_len must be 16 + 8 * up * taps_per_phase");
            n.history = h.taps_per_phase;
        }
    }
}

// sample-rate domains: every input of a node must live in one domain; Resample multiplies it by up / down
static void rate_domains(Plan& P, const mx_node* nodes) {
    auto gcd_u = [](uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a ? a : 1; };
    for (uint32_t id : P.order) {
        PlanNode& n = P.nodes[id];
        bool have = false; uint32_t dn = 1, dd = 1;
        for (const PortRef& pr : n.in_src) {
            if (pr.node < 0 || n.in_type[&pr - n.in_src.data()] == MX_VIDEO) continue;
            const PlanNode& sn = P.nodes[pr.node];
            if (have && (sn.dom_num != dn || sn.dom_den != dd)) throw Error(MX_ERR_TYPE, "inputs of a module live in different sample-rate domains");
            dn = sn.dom_num; dd = sn.dom_den; have = true;
        }
        n.in_dom_num = dn; n.in_dom_den = dd; n.dom_num = dn; n.dom_den = dd;
        if (n.kind == MX_KIND_RESAMPLE) {
            mx_resample_params h; std::memcpy(&h, nodes[id].params, sizeof h);
            const uint64_t a = (uint64_t)dn * h.up, b = (uint64_t)dd * h.down, g = gcd_u(a, b);
            n.dom_num = (uint32_t)(a / g); n.dom_den = (uint32_t)(b / g);
        }
        if ((P.spt * n.dom_num) % n.dom_den) throw Error(MX_ERR_INVALID, "resampling ratio does not give a whole number of samples per tick");
        const bool rate_dependent = n.kind == MX_KIND_EQ_THREE || n.kind == MX_KIND_ENVELOPE || n.kind == MX_KIND_OSCILLATOR || n.kind == MX_KIND_FM_SINE;
        if (n.kind == MX_KIND_PLOTTER && (n.in_dom_num != 1 || n.in_dom_den != 1))
            throw Error(MX_ERR_INVALID, "Plotter is only accepted in the base sample-rate domain");
        if (rate_dependent && (n.dom_num != 1 || n.dom_den != 1))
            throw Error(MX_ERR_INVALID, "EqThree / Envelope / Oscillator / FmSine depend on the sample rate and are only accepted in the base domain");
    }
}

// Graph-compiler fusion.  A port buffer is a per-tick temporary of Engine::run_tick
// (src/engine.rs:461,504-506), observable only through connections, so a port whose only consumers
// are folded into its producer's kernel need not exist.  Two patterns, both bit-identical to the
// separate modules because the folded arithmetic is applied to the very f32 the producer stores:
//   F1  EqThree -> StereoPanner(L = R = that EQ) [-> Amplifier input]   => epilogue of the EQ kernel
//   F2  Trigger (single consumer) -> Envelope gate                       => constant gate, no buffer
static void plan_fusion(Plan& P) {
    std::vector<PlanNode>& nodes_ = P.nodes;
    const size_t N = nodes_.size();
    std::vector<std::vector<std::vector<std::pair<uint32_t, uint32_t>>>> cons(N);
    for (size_t i = 0; i < N; ++i) cons[i].resize(nodes_[i].out_type.size());
    for (uint32_t id : P.order)
        for (uint32_t k = 0; k < nodes_[id].in_src.size(); ++k) {
            const PortRef pr = nodes_[id].in_src[k];
            if (pr.node >= 0) cons[pr.node][pr.port].push_back({id, k});
        }
    // does `from` (transitively, through its inputs) depend on `target`?  bounded search, conservative
    auto depends_on = [&](int32_t from, uint32_t target) {
        std::vector<int32_t> st{from};
        size_t visited = 0;
        while (!st.empty()) {
            const int32_t x = st.back(); st.pop_back();
            if ((uint32_t)x == target) return true;
            if (++visited > 256) return true;
            for (const PortRef& pr : nodes_[x].in_src) if (pr.node >= 0) st.push_back(pr.node);
        }
        return false;
    };
    for (uint32_t e : P.order) {
        PlanNode& E = nodes_[e];
        if (E.kind != MX_KIND_EQ_THREE) continue;
        const auto& c = cons[e][0];
        if (c.size() != 2 || c[0].first != c[1].first || c[0].second == c[1].second) continue;
        const uint32_t p = c[0].first;
        PlanNode& Pn = nodes_[p];
        if (Pn.kind != MX_KIND_STEREO_PANNER || Pn.elided) continue;
        E.fuse_pan = (int32_t)p; E.out_elided[0] = 1;
        Pn.elided = true; Pn.owner = (int32_t)e;
        const auto& pc = cons[p][0];
        if (pc.size() == 1 && nodes_[pc[0].first].kind == MX_KIND_AMPLIFIER && pc[0].second == 0) {
            const uint32_t a = pc[0].first;
            PlanNode& A = nodes_[a];
            const PortRef ctl = A.in_src[1];
            if (ctl.node < 0 || !depends_on(ctl.node, e)) {
                E.fuse_amp = (int32_t)a; Pn.out_elided[0] = 1;
                A.elided = true; A.owner = (int32_t)e;
                if (ctl.node >= 0) E.level = std::max(E.level, nodes_[ctl.node].level + 1);   // the fused kernel reads the control port
            }
        }
    }
    for (uint32_t v : P.order) {
        PlanNode& V = nodes_[v];
        if (V.kind != MX_KIND_ENVELOPE) continue;
        const PortRef g = V.in_src[0];
        if (g.node < 0 || nodes_[g.node].kind != MX_KIND_TRIGGER || cons[g.node][0].size() != 1) continue;
        PlanNode& G = nodes_[g.node];
        V.fuse_trigger = g.node;
        G.elided = true; G.owner = (int32_t)v; G.out_elided[0] = 1;
    }
    for (uint32_t e : P.order) {
        PlanNode& E = nodes_[e];
        if (E.kind != MX_KIND_EQ_THREE || E.fuse_pan < 0) continue;
        // F3: the fused Amplifier's control is a constant-gate Envelope that feeds nothing else: its closed form
        // (envelope.rs:34-58) is evaluated in the epilogue; for a constant gate only the run's first sample can
        // change the Envelope's state, so no per-sample state machine is needed
        if (E.fuse_amp >= 0) {
            const PortRef ctl = nodes_[E.fuse_amp].in_src[1];
            if (ctl.node >= 0 && nodes_[ctl.node].kind == MX_KIND_ENVELOPE && nodes_[ctl.node].fuse_trigger >= 0 &&
                cons[ctl.node][0].size() == 1) {
                PlanNode& V = nodes_[ctl.node];
                E.fuse_env = ctl.node;
                V.elided = true; V.owner = (int32_t)e; V.out_elided[0] = 1;
            }
        }
        // F4: the fused result is stereo with L == R by construction; if only Mixers read it, store one float per frame
        const uint32_t x = (uint32_t)(E.fuse_amp >= 0 ? E.fuse_amp : E.fuse_pan);
        const auto& xc = cons[x][0];
        bool only_mixers = !xc.empty();
        for (const auto& c : xc) only_mixers = only_mixers && (nodes_[c.first].kind == MX_KIND_MIXER || nodes_[c.first].kind == MX_KIND_OUTPUT_DEVICE);   // (an OutputDevice expands it)
        if (only_mixers) nodes_[x].out_dup[0] = 1;
    }
}

// groups: (level, kind); nodes folded into another node's kernel are never launched.  EqThree nodes also by the epilogue the compiler gave them (plain, -> Panner,
// -> Amplifier with a constant / a buffer / an inline Envelope as control; stereo or one float per frame): a launch group of ONE mode takes the kernel
// specialised for it -- sixteen strips of another mode among a thousand put the whole group on the general direct-load form (29 ms against 5, tools/ctl_probe.py)
static void cut_groups(Plan& P) {
    std::vector<PlanNode>& nodes_ = P.nodes;
    auto eq_key = [&](const PlanNode& nd) -> int {
        if (nd.kind != MX_KIND_EQ_THREE) return 0;
        const uint32_t epi = nd.fuse_amp >= 0 ? 2u : (nd.fuse_pan >= 0 ? 1u : 0u);
        uint32_t fl = 0;
        if (nd.fuse_amp >= 0 ? nodes_[nd.fuse_amp].out_dup[0] : (nd.fuse_pan >= 0 && nodes_[nd.fuse_pan].out_dup[0])) fl |= MX_EQF_MONO_DUP;
        if (nd.fuse_env >= 0) fl |= MX_EQF_ENV;
        const bool has_ctl = nd.fuse_amp >= 0 && nd.fuse_env < 0 && nodes_[nd.fuse_amp].in_src[1].node >= 0;
        return 1 + eq_epilogue_mode(epi, fl, has_ctl);
    };
    for (PlanNode& n : nodes_) n.sub_key = eq_key(n);
    std::vector<uint32_t> sorted;
    for (uint32_t id : P.order) if (!nodes_[id].elided && nodes_[id].kind != MX_KIND_OUTPUT_DEVICE) sorted.push_back(id);
    for (uint32_t id : P.order) if (nodes_[id].kind == MX_KIND_OUTPUT_DEVICE) P.od_nodes.push_back(id);
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) {
        if (nodes_[a].level != nodes_[b].level) return nodes_[a].level < nodes_[b].level;
        if (nodes_[a].kind != nodes_[b].kind) return nodes_[a].kind < nodes_[b].kind;
        if (nodes_[a].sub_key != nodes_[b].sub_key) return nodes_[a].sub_key < nodes_[b].sub_key;
        const uint64_t da = ((uint64_t)nodes_[a].dom_num << 32) | nodes_[a].dom_den, db = ((uint64_t)nodes_[b].dom_num << 32) | nodes_[b].dom_den;
        return da < db;
    });
    for (uint32_t id : sorted) {
        PlanNode& n = nodes_[id];
        if (P.groups.empty() || P.groups.back().level != n.level || P.groups.back().kind != n.kind || P.groups.back().sub_key != n.sub_key ||
            P.groups.back().dom_num != n.dom_num || P.groups.back().dom_den != n.dom_den ||
            P.groups.back().in_dom_num != n.in_dom_num || P.groups.back().in_dom_den != n.in_dom_den) {
            PlanGroup g; g.level = n.level; g.kind = n.kind; g.sub_key = n.sub_key;
            g.dom_num = n.dom_num; g.dom_den = n.dom_den; g.in_dom_num = n.in_dom_num; g.in_dom_den = n.in_dom_den;
            P.groups.push_back(std::move(g));
        }
        n.group = (int)P.groups.size() - 1;
        n.slot = (uint32_t)P.groups.back().nodes.size();
        P.groups.back().nodes.push_back(id);
    }
    for (uint32_t id = 0; id < nodes_.size(); ++id) if (nodes_[id].kind == MX_KIND_PLOTTER && nodes_[id].group >= 0) P.plotter_nodes.push_back(id);
}

// the video nodes: which there are, what a Monitor may ask for, and which VideoMixers hand their program over lazily
static void plan_video(Plan& P, const mx_node* nodes, const mx_graph_opts& o) {
    std::vector<PlanNode>& nodes_ = P.nodes;
    for (uint32_t id : P.order) if (is_video_kind(nodes_[id].kind)) P.video_order.push_back(id);
    for (size_t i = 0; i < nodes_.size(); ++i) {
        const PlanNode& n = nodes_[i];
        if (n.kind == MX_KIND_MONITOR) {
            mx_monitor_params p; std::memcpy(&p, nodes[i].params, sizeof p);
            if (p.width == 0 || p.height == 0 || (p.width & 1) || (p.height & 1) || p.width > 16384 || p.height > 16384)
                throw Error(MX_ERR_INVALID, "monitor picture must be non-zero, even and at most 16384 a side");
            uint32_t depth = 0;
            if (nodes[i].params_len == sizeof(mx_monitor_params_ex)) { mx_monitor_params_ex px; std::memcpy(&px, nodes[i].params, sizeof px); depth = px.queue_depth; }
            // without a queue depth every tick of a submission keeps its scaled picture on the device until the next run
            const uint64_t kept = (uint64_t)(depth ? depth : std::max<uint32_t>(1u, o.max_ticks_per_run)) * (((uint64_t)p.width + 63) & ~63ull) * p.height * 3 / 2;
            if (kept > (64ull << 30)) throw Error(MX_ERR_NOMEM, "a Monitor that keeps every tick of a submission would hold more than 64 GiB of pictures: give it a queue depth (mx_monitor_params_ex) or fewer ticks per run");
        }
        if (is_video_kind(n.kind)) P.has_video = true;
    }
    // a VideoMixer whose program output feeds exactly one video node of this graph hands it over as an
    // unevaluated cross-fade chain: a cascade of mixers becomes one fused pass (mx_k_video.hip k_fade_chain*)
    if (!(P.flags & MX_FLAG_NO_FUSE)) {
        std::vector<uint32_t> n_cons(nodes_.size(), 0); std::vector<uint8_t> ok(nodes_.size(), 1);
        for (const PlanNode& n : nodes_)
            for (const PortRef& pr : n.in_src)
                if (pr.node >= 0 && nodes_[pr.node].kind == MX_KIND_VIDEO_MIXER && pr.port == 0) {
                    n_cons[pr.node]++;
                    if (n.kind != MX_KIND_VIDEO_MIXER && n.kind != MX_KIND_VIDEO_TO_RGBA) ok[pr.node] = 0;
                }
        for (size_t i = 0; i < nodes_.size(); ++i)
            if (nodes_[i].kind == MX_KIND_VIDEO_MIXER) nodes_[i].vlazy = n_cons[i] == 1 && ok[i];
    }
}

// MX_FLAG_OVERLAP_TAIL: the last launch group, if it is a Mixer bank alone on the highest level of an audio-only graph, may run beside
// the next run's earlier groups; every port it reads gets a second buffer (the next run must not overwrite what it is still reading)
// AUTOMATIC for graphs with at least 64 EqThree instances and submissions of at least 16 ticks, while the second buffers stay affordable (the executor's
// test): the bank's launch is held back until the next run's EqThree launch has been placed and then shares the SIMDs with it -- 1024 strips x 2048 ticks
// 5.42 -> 4.84 ms, x 256 ticks 0.915 -> 0.860, 128 strips x 2048 ticks 0.934 -> 0.875 (profiles/r05/short_submission_regime.md).  Launched at once instead
// the same mode LOST from 256 ticks up: the next run's k_env_ticks ran beside the bank (140 us instead of 9) with the EqThree launch waiting behind it.
// MX_OVERLAP_AUTO=0 turns the automatism off; results are bit-identical either way.
static void tail_candidate(Plan& P, bool auto_on) {
    const std::vector<PlanNode>& nodes_ = P.nodes;
    const std::vector<PlanGroup>& groups_ = P.groups;
    const bool eq_exact = (P.flags & MX_FLAG_EQ_EXACT) || !(P.flags & MX_FLAG_EQ_FAST);
    const size_t max_ticks = P.spt ? P.cap_frames / P.spt : 0;
    size_t n_eq = 0;
    for (const PlanGroup& g : groups_) if (g.kind == MX_KIND_EQ_THREE) n_eq = std::max(n_eq, g.nodes.size());
    const bool overlap_auto = auto_on && eq_exact && n_eq >= 64 && max_ticks >= 16;
    // The tail is every Mixer group at the END of the launch order: a bank, or a bank and the buses above it (group buses -> master).  What its groups read from the
    // groups before them is double-buffered; what they read from each other is not (they run in order on the one tail stream).
    size_t t_first = groups_.size();
    while (t_first > 0 && groups_[t_first - 1].kind == MX_KIND_MIXER) --t_first;
    if (!(((P.flags & MX_FLAG_OVERLAP_TAIL) || overlap_auto) && !P.has_video && groups_.size() >= 2 && t_first >= 1 && t_first < groups_.size() &&
          groups_[t_first - 1].level < groups_[t_first].level && P.plotter_nodes.empty()))
        return;
    std::vector<std::pair<uint32_t, uint32_t>> ports;
    for (size_t tg = t_first; tg < groups_.size(); ++tg)
        for (uint32_t id : groups_[tg].nodes)
            for (const PortRef& pr : nodes_[id].in_src) {
                if (pr.node < 0) continue;
                const PlanNode& sn = nodes_[pr.node];
                if (sn.group >= (int)t_first && sn.group < (int)tg) continue;   // another tail group's output: same stream, in order
                if (sn.kind == MX_KIND_SOURCE_MONO || sn.kind == MX_KIND_SOURCE_STEREO || sn.group >= (int)tg) return;   // a source is rewritten by the caller while the tail may still read it
                if (std::find(ports.begin(), ports.end(), std::make_pair((uint32_t)pr.node, (uint32_t)pr.port)) == ports.end()) ports.push_back({(uint32_t)pr.node, pr.port});
            }
    P.tail_first = (int)t_first;
    P.tail_auto = !(P.flags & MX_FLAG_OVERLAP_TAIL);
    P.tail_ports = std::move(ports);
}

Plan compile_plan(const mx_node* nodes, size_t n_nodes, const mx_edge* edges, size_t n_edges, const mx_graph_opts& o, const PlanEnv& env) {
    if (n_nodes && !nodes) throw Error(MX_ERR_INVALID, "nodes is NULL");
    if (n_edges && !edges) throw Error(MX_ERR_INVALID, "edges is NULL");
    Plan P;
    P.sample_rate = o.sample_rate ? o.sample_rate : 44100u;   // src/engine.rs:53
    P.tps = o.ticks_per_second ? o.ticks_per_second : 60u;    // src/engine.rs:54
    if (P.sample_rate % P.tps) throw Error(MX_ERR_INVALID, "sample_rate must be a multiple of ticks_per_second");
    P.spt = P.sample_rate / P.tps;                            // src/engine.rs:55
    const uint32_t max_ticks = o.max_ticks_per_run ? o.max_ticks_per_run : 1u;
    P.cap_frames = env.cap_frames ? env.cap_frames : P.spt * (size_t)max_ticks;
    P.flags = o.flags;
    if ((P.flags & MX_FLAG_FP_CONTRACT) && (P.flags & MX_FLAG_EQ_FAST) && !(P.flags & MX_FLAG_EQ_EXACT))
        throw Error(MX_ERR_INVALID, "MX_FLAG_FP_CONTRACT is a mode of the exact-order kernels: not with MX_FLAG_EQ_FAST");

    P.nodes.resize(n_nodes);
    for (size_t i = 0; i < n_nodes; ++i) {
        PlanNode& n = P.nodes[i];
        n.kind = nodes[i].kind;
        if (nodes[i].params_len && !nodes[i].params) throw Error(MX_ERR_INVALID, "node params is NULL");
        kind_ports(n.kind, nodes[i].params_len, n.in_type, n.out_type);
        n.in_src.assign(n.in_type.size(), PortRef{});
        n.out_elided.assign(n.out_type.size(), 0); n.out_dup.assign(n.out_type.size(), 0);
        if (n.kind == MX_KIND_OUTPUT_DEVICE) check_output_device_params(nodes[i].params);
    }
    for (size_t e = 0; e < n_edges; ++e) {
        const mx_edge& ed = edges[e];
        if (ed.src_node >= n_nodes || ed.dst_node >= n_nodes) throw Error(MX_ERR_INVALID, "edge references a node out of range");
        const PlanNode& s = P.nodes[ed.src_node];
        PlanNode& d = P.nodes[ed.dst_node];
        if (ed.src_port >= s.out_type.size() || ed.dst_port >= d.in_type.size()) throw Error(MX_ERR_INVALID, "edge references a terminal out of range");
        if (s.out_type[ed.src_port] != d.in_type[ed.dst_port])   // Workspace::connect, workspace.rs:97-114
            throw Error(MX_ERR_TYPE, "line type mismatch on connection");
        d.in_src[ed.dst_port] = PortRef{(int32_t)ed.src_node, ed.src_port};
    }
    run_order(P, edges, n_edges);
    check_blobs(P, nodes);
    rate_domains(P, nodes);
    if (!(P.flags & MX_FLAG_NO_FUSE)) plan_fusion(P);
    cut_groups(P);
    plan_video(P, nodes, o);
    tail_candidate(P, env.overlap_auto);
    return P;
}

size_t port_floats(const PlanNode& n, size_t port, size_t cap_frames) {
    return (n.out_dup[port] ? 1 : floats_per_frame(n.out_type[port])) * (cap_frames * n.dom_num / n.dom_den + 1);
}

SlabLayout layout_slab(const Plan& P, size_t cap_frames, bool tail_on) {
    SlabLayout L;
    size_t off = 0;
    auto bump = [&](size_t floats) { size_t o = off; off += (floats + 63) & ~(size_t)63; return o; };  // 256-byte aligned
    // Disconnected inputs read this region (io.rs:8-9); a node behind a Resample runs cap_frames * up / down frames per
    // launch, so the region is sized for the largest sample-rate domain of the graph
    size_t zero_frames = cap_frames;
    for (const PlanNode& n : P.nodes) {
        zero_frames = std::max(zero_frames, cap_frames * n.dom_num / n.dom_den + 1);
        zero_frames = std::max(zero_frames, cap_frames * n.in_dom_num / n.in_dom_den + 1);
    }
    L.zero_floats = 2 * zero_frames;
    L.zero_off = bump(L.zero_floats);
    L.out_off.resize(P.nodes.size()); L.out_off2.resize(P.nodes.size());
    for (size_t i = 0; i < P.nodes.size(); ++i) L.out_off2[i].assign(P.nodes[i].out_type.size(), SIZE_MAX);
    if (tail_on) for (const auto& pp : P.tail_ports) L.out_off2[pp.first][pp.second] = 0;   // marked; placed below, next to the first buffer
    for (size_t i = 0; i < P.nodes.size(); ++i) {
        const PlanNode& n = P.nodes[i];
        L.out_off[i].assign(n.out_type.size(), SIZE_MAX);
        for (size_t k = 0; k < n.out_type.size(); ++k) {
            if (n.out_elided[k]) { L.out_off2[i][k] = SIZE_MAX; continue; }
            const size_t fl = port_floats(n, k, cap_frames);
            L.out_off[i][k] = bump(fl);
            if (L.out_off2[i][k] != SIZE_MAX) L.out_off2[i][k] = bump(fl);
        }
    }
    L.floats = off;
    return L;
}

}  // namespace mx
