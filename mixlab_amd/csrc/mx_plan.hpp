// mx_plan.hpp -- the graph compiler as a value: everything Graph decides about a topology before it touches a device.
//
// compile_plan() checks nodes and edges, cuts back-edges, orders and levels the nodes, assigns sample-rate domains, plans the
// fusion, cuts the launch groups and names the overlap-tail candidate; layout_slab() places every materialised port in the slab.
// Both are host arithmetic only: mx_graph_build and mx_graph_debug_plan go through the very same two functions.
#pragma once
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "mx_common.hpp"

namespace mx {

struct PortRef { int32_t node = -1; uint32_t port = 0; };

// What the compiler says about one node.  Graph's Node starts as a copy of it and rewrites nothing of it but in_src (set_input_enabled).
struct PlanNode {
    uint32_t kind = 0;
    std::vector<uint8_t> in_type, out_type;   // mx_line per terminal (ModuleT::inputs()/outputs())
    std::vector<PortRef> in_src;              // workspace.connections (back-edges already cut)
    int pos = -1;                             // position in the run order; -1: outside it (a cycle that feeds no terminal module)
    int level = 0;
    uint32_t dom_num = 1, dom_den = 1;        // sample-rate domain of the OUTPUT ports relative to the graph's rate (Resample changes it)
    uint32_t in_dom_num = 1, in_dom_den = 1;  // ... of the input ports
    uint32_t slot = 0;                        // index inside its launch group
    int group = -1;
    int sub_key = 0;                          // EQ_THREE: 1 + the epilogue mode the compiler gave the node (launch groups are of one mode); 0 otherwise
    uint32_t history = 0;                     // FIR: taps; RESAMPLE: taps per phase -- the stereo frames of input the node carries from run to run
    // fusion (plan_fusion)
    bool elided = false;                      // never launched: its work is folded into `owner`'s kernel
    int32_t owner = -1;                       // node whose descriptors carry this node's params
    int32_t fuse_pan = -1, fuse_amp = -1;     // EQ_THREE: StereoPanner / Amplifier folded into the epilogue
    int32_t fuse_trigger = -1;                // ENVELOPE: Trigger folded in as a constant gate
    int32_t fuse_env = -1;                    // EQ_THREE: constant-gate Envelope evaluated inline as the fused Amplifier's control
    std::vector<uint8_t> out_elided;          // per output port: buffer not materialised
    std::vector<uint8_t> out_dup;             // per output port: stereo with L == R stored as ONE float per frame
    bool vlazy = false;                       // VIDEO_MIXER: program output handed over as an unevaluated cross-fade chain
};

inline uint32_t history_frames(const PlanNode& n) { return n.history; }

struct PlanGroup {
    int level = 0;
    uint32_t kind = 0;
    int sub_key = 0;
    uint32_t dom_num = 1, dom_den = 1, in_dom_num = 1, in_dom_den = 1;   // every node of a group shares one rate domain
    std::vector<uint32_t> nodes;
};

// what the compiler would otherwise read from the environment, and the capacity the caller wants
struct PlanEnv {
    bool overlap_auto = true;   // MX_OVERLAP_AUTO (0 turns the automatic second-stream mode off)
    size_t cap_frames = 0;      // frames per run the slab is sized for; 0: samples per tick * opts.max_ticks_per_run
};

struct Plan {
    std::vector<PlanNode> nodes;
    std::vector<uint32_t> order;
    std::vector<PlanGroup> groups;          // sorted by (level, kind, sub_key, domain)
    std::vector<uint32_t> od_nodes;         // OutputDevice nodes of the order (never in a launch group)
    std::vector<uint32_t> plotter_nodes;    // launched Plotter nodes
    std::vector<uint32_t> video_order;      // the video nodes of the order, in run order
    bool has_video = false;
    uint32_t flags = 0, sample_rate = 44100, tps = 60;
    size_t spt = 735, cap_frames = 735;
    // The overlap-tail CANDIDATE: every Mixer group from tail_first on would run on a second stream, the ports they read from earlier groups double-buffered.
    // Whether the second buffers are affordable is for the executor to say (an automatic candidate only).
    int tail_first = -1;                    // -1: none
    bool tail_auto = false;                 // from the automatic rule, not from MX_FLAG_OVERLAP_TAIL
    std::vector<std::pair<uint32_t, uint32_t>> tail_ports;   // (node, output port)
};

Plan compile_plan(const mx_node* nodes, size_t n_nodes, const mx_edge* edges, size_t n_edges, const mx_graph_opts& opts, const PlanEnv& env);

struct SlabLayout {
    size_t zero_off = 0, zero_floats = 0;   // the region Disconnected inputs read
    size_t floats = 0;                      // the whole slab
    std::vector<std::vector<size_t>> out_off, out_off2;   // per node, per output port, in floats; SIZE_MAX: none
};
size_t port_floats(const PlanNode& n, size_t port, size_t cap_frames);   // length of one buffer of an output port
SlabLayout layout_slab(const Plan& plan, size_t cap_frames, bool tail_on);

void check_output_device_params(const void* params);   // the OutputDevice parameter rule (build and every update)

}  // namespace mx
