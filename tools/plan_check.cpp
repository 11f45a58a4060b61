// plan_check.cpp -- the graph compiler (mixlab_amd/csrc/mx_plan.cpp) as a plain host executable, for a sanitizer build:
//   clang++ -std=c++17 -g -fsanitize=address,undefined -D__HIP_PLATFORM_AMD__ -I<rocm>/include tools/plan_check.cpp mixlab_amd/csrc/mx_plan.cpp -o plan_check
//   plan_check [graph.bin ...]
// Compiles and lays out the 1024-strip bench graph, then every graph file given (tools/plan_check.py writes three random seeds):
//   u32 sample_rate, tps, max_ticks, flags, n_nodes, n_edges; per node u32 kind, u32 params_len, params; per edge 4 x u32.
// tools/plan_check.py builds and runs it.  No device, no Python in the process.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>

#include "../mixlab_amd/csrc/mx_plan.hpp"
#include "../mixlab_amd/csrc/mx_kernels.hpp"

namespace mx {
// the one function of the library mx_plan.cpp links against (mx_k_eq_exact.hip), restated for the stand-alone build
int eq_epilogue_mode(uint32_t epi, uint32_t flags, bool has_ctl) {
    const int mode = epi != 2u ? 0 : ((flags & MX_EQF_ENV) ? 3 : (has_ctl ? 2 : 1));
    const int stereo = !(epi == 0u || (flags & MX_EQF_MONO_DUP));
    return mode * 2 + stereo;
}
}  // namespace mx

struct GraphDesc {
    mx_graph_opts opts{};
    std::vector<std::vector<uint8_t>> blobs;
    std::vector<mx_node> nodes;
    std::vector<mx_edge> edges;
    uint32_t add(uint32_t kind, const void* p, size_t len) {
        blobs.emplace_back((const uint8_t*)p, (const uint8_t*)p + len);
        nodes.push_back(mx_node{kind, (uint32_t)len, nullptr});
        return (uint32_t)nodes.size() - 1;
    }
    void connect(uint32_t s, uint32_t sp, uint32_t d, uint32_t dp) { edges.push_back(mx_edge{s, sp, d, dp}); }
    void fix() { for (size_t i = 0; i < nodes.size(); ++i) nodes[i].params = blobs[i].empty() ? nullptr : blobs[i].data(); }
};

static GraphDesc bench_graph(uint32_t strips) {
    GraphDesc g;
    g.opts.sample_rate = 48000; g.opts.ticks_per_second = 60; g.opts.max_ticks_per_run = 2048; g.opts.device = -1;
    std::vector<mx_mixer_channel_params> ch(strips);
    for (auto& c : ch) { std::memset(&c, 0, sizeof c); c.fader = 1.0; }
    const uint32_t mix = g.add(MX_KIND_MIXER, ch.data(), ch.size() * sizeof ch[0]);
    for (uint32_t k = 0; k < strips; ++k) {
        mx_trigger_params tp{}; tp.gate_open = k & 1;
        mx_envelope_params ep{25.0, 500.0, 0.8, 200.0};
        mx_eq_three_params qp{-3.0, 1.0, 2.0};
        mx_amplifier_params ap{1.0, 0.5};
        const uint32_t trig = g.add(MX_KIND_TRIGGER, &tp, sizeof tp), env = g.add(MX_KIND_ENVELOPE, &ep, sizeof ep), src = g.add(MX_KIND_SOURCE_MONO, nullptr, 0);
        const uint32_t eq = g.add(MX_KIND_EQ_THREE, &qp, sizeof qp), pan = g.add(MX_KIND_STEREO_PANNER, nullptr, 0), amp = g.add(MX_KIND_AMPLIFIER, &ap, sizeof ap);
        g.connect(trig, 0, env, 0); g.connect(src, 0, eq, 0); g.connect(eq, 0, pan, 0); g.connect(eq, 0, pan, 1);
        g.connect(pan, 0, amp, 0); g.connect(env, 0, amp, 1); g.connect(amp, 0, mix, k);
    }
    g.fix();
    return g;
}

static GraphDesc read_graph(const char* path) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error(std::string("cannot open ") + path);
    const std::vector<uint8_t> b((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t at = 0;
    auto u32 = [&] { if (at + 4 > b.size()) throw std::runtime_error("short graph file"); uint32_t v; std::memcpy(&v, &b[at], 4); at += 4; return v; };
    GraphDesc g;
    g.opts.sample_rate = u32(); g.opts.ticks_per_second = u32(); g.opts.max_ticks_per_run = u32(); g.opts.flags = u32(); g.opts.device = -1;
    const uint32_t n_nodes = u32(), n_edges = u32();
    for (uint32_t i = 0; i < n_nodes; ++i) {
        const uint32_t kind = u32(), len = u32();
        if (at + len > b.size()) throw std::runtime_error("short graph file");
        g.add(kind, b.data() + at, len); at += len;
    }
    for (uint32_t e = 0; e < n_edges; ++e) { const uint32_t s = u32(), sp = u32(), d = u32(), dp = u32(); g.connect(s, sp, d, dp); }
    g.fix();
    return g;
}

static void check(const char* what, const GraphDesc& g) {
    for (uint32_t flags : {g.opts.flags, g.opts.flags | (uint32_t)MX_FLAG_NO_FUSE, g.opts.flags | (uint32_t)MX_FLAG_OVERLAP_TAIL}) {
        mx_graph_opts o = g.opts; o.flags = flags;
        const mx::Plan P = mx::compile_plan(g.nodes.data(), g.nodes.size(), g.edges.data(), g.edges.size(), o, mx::PlanEnv{});
        size_t floats = 0;
        for (size_t cap : {P.cap_frames, 2 * P.cap_frames})
            for (bool tail : {false, P.tail_first >= 0}) floats = mx::layout_slab(P, cap, tail).floats;
        std::printf("%s flags %u: %zu nodes, %zu ordered, %zu groups, tail %d (%zu ports), %zu floats\n", what, flags, P.nodes.size(), P.order.size(), P.groups.size(),
                    P.tail_first, P.tail_ports.size(), floats);
    }
}

int main(int argc, char** argv) {
    try {
        check("bench graph, 1024 strips", bench_graph(1024));
        for (int i = 1; i < argc; ++i) check(argv[i], read_graph(argv[i]));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "plan_check: %s\n", e.what());
        return 1;
    }
    return 0;
}
