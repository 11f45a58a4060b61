"""The graph compiler on its own (mx_graph_debug_plan: the compile_plan / layout_slab a build goes through, no device) against the
restatements the GPU tests rely on -- the oracle's run order, engine_domains, predict_fusion -- and against the structure and layout
rules the executor takes for granted.  The graphs are the random families' own draws: the full random graphs, every workspace of the
edit sessions, the random video scenarios."""
import ctypes as C
import struct
from fractions import Fraction
from types import SimpleNamespace

import pytest

import oracle
import random_video as rv
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from random_edits import EDIT_SEEDS, MAX_RUN
from random_taps import predict_fusion
from test_cpu_random_edits import session
from test_cpu_random_video import SEEDS as VIDEO_SEEDS
from test_gpu_random_graphs import FULL_SEEDS, engine_domains, n_inputs, port_types, random_graph
from test_gpu_random_video import workspace as video_workspace
from tick_shapes import by_id

NONE = abi.PLAN_NONE
FIELDS = [f for f, _t in abi.PlanNode._fields_]
IDS = [f"{s}-{n}" for s, n in FULL_SEEDS]
EDIT_IDS = [f"{s}-{n}" for s, n in EDIT_SEEDS]


def plan(ws, max_ticks=MAX_RUN, flags=0, overlap_auto=1, cap_frames=0):
    """-> ([a mutable record per node], info, cap_frames)"""
    recs, info = abi.debug_plan(ws.nodes, ws.edges, ws.sample_rate, ws.ticks_per_second, max_ticks, flags, overlap_auto, cap_frames)
    out = []
    for r in recs:
        d = {f: getattr(r, f) for f in FIELDS}
        for f in ("out_elided", "out_dup", "out_off", "out_off2"):
            d[f] = list(d[f])
        out.append(SimpleNamespace(**d))
    return out, SimpleNamespace(**{f: getattr(info, f) for f, _t in abi.PlanInfo._fields_}), cap_frames or ws.spt * max_ticks


def full_ws(shape_id, seed):
    shape = by_id(shape_id)
    return random_graph(seed, shape.sample_rate, shape.ticks_per_second, full=True)[0]


def session_workspaces(shape_id, seed):
    """every workspace an edit session passes through: the drawn one, then the one each edit left"""
    shape = by_id(shape_id)
    out = [full_ws(shape_id, seed)]
    for run in session(shape_id, seed)[1]:
        ed = run.get("edited")
        if ed:
            ws = Workspace(shape.sample_rate, shape.ticks_per_second)
            ws.nodes = [(k, p or None) for k, p in ed["nodes"]]
            ws._conn = {(d, dp): (s, sp) for (s, sp, d, dp) in ed["edges"]}
            out.append(ws)
    return out


# ---- the checks: each raises an AssertionError that names the graph (`what`) and the node ----
def check_order(what, recs, info, order):
    got = sorted((r.pos, n) for n, r in enumerate(recs) if r.pos >= 0)
    assert [n for _p, n in got] == list(order) and [p for p, _n in got] == list(range(len(order))), f"{what}: the run order differs: {got} != {order}"
    assert info.n_order == len(order), f"{what}: n_order"
    for n, r in enumerate(recs):
        assert (r.pos >= 0) == (n in set(order)), f"{what}: node {n}: position {r.pos} outside the run order"


def check_domains(what, recs, dom):
    for n, d in dom.items():
        assert Fraction(recs[n].dom_num, recs[n].dom_den) == d, f"{what}: node {n}: domain {recs[n].dom_num}/{recs[n].dom_den} != {d}"


def check_fusion(what, recs, folded, stored_dup):
    for n, r in enumerate(recs):
        for p in range(r.n_out):
            assert bool(r.out_elided[p]) == ((n, p) in folded), f"{what}: node {n}: port {p} elided = {r.out_elided[p]}, predicted {(n, p) in folded}"
            assert bool(r.out_dup[p]) == ((n, p) in stored_dup), f"{what}: node {n}: port {p} dup = {r.out_dup[p]}, predicted {(n, p) in stored_dup}"


def forward_inputs(ws, recs, n):
    kind, params = ws.nodes[n]
    n_in = {abi.KIND_VIDEO_MIXER: 4, abi.KIND_VIDEO_TO_RGBA: 1, abi.KIND_MONITOR: 2}.get(kind, n_inputs(kind, params))
    srcs = [ws._conn.get((n, k)) for k in range(n_in)]
    return [(k, s) for k, s in enumerate(srcs) if s is not None and 0 <= recs[s[0]].pos < recs[n].pos]


def root_of(what, recs, n):
    seen = 0
    while recs[n].elided:
        assert recs[n].owner >= 0 and seen <= len(recs), f"{what}: node {n}: the owner chain of an elided node does not end at a launched one"
        n = recs[n].owner; seen += 1
    return n


def check_structure(what, ws, recs, info):
    key = lambda r: (r.level, ws_kind[r.node], r.sub_key, r.dom_num, r.dom_den)
    ws_kind = [k for k, _p in ws.nodes]
    groups = {}
    for n, r in enumerate(recs):
        if r.pos < 0 or r.elided:
            continue
        for k, s in forward_inputs(ws, recs, n):
            root = root_of(what, recs, s[0])   # (a folded producer is computed by its owner's kernel; where that is this node, nothing is waited for)
            assert root == n or r.level > recs[root].level, f"{what}: node {n}: level {r.level} does not exceed its input {k}'s producer's"
        if ws_kind[n] == abi.KIND_EQ_THREE and r.fuse_amp >= 0:
            for k, s in forward_inputs(ws, recs, r.fuse_amp):
                if k == 1 and r.fuse_env < 0:
                    assert r.level > recs[root_of(what, recs, s[0])].level, f"{what}: node {n}: level {r.level} is not above the folded Amplifier's control"
    for n, r in enumerate(recs):
        r.node = n
        launched = r.pos >= 0 and not r.elided and ws_kind[n] != abi.KIND_OUTPUT_DEVICE
        assert (r.group >= 0) == launched, f"{what}: node {n}: group {r.group} but launched = {launched}"
        if launched:
            groups.setdefault(r.group, []).append(r)
        if r.elided:
            root_of(what, recs, n)
    assert sorted(groups) == list(range(info.n_groups)), f"{what}: groups {sorted(groups)} of {info.n_groups}"
    for g, rs in groups.items():
        assert sorted(r.slot for r in rs) == list(range(len(rs))), f"{what}: node {rs[0].node}: the slots of group {g} are not 0 .. n - 1"
        for r in rs:
            full = lambda x: key(x) + (x.in_dom_num, x.in_dom_den)
            assert full(r) == full(rs[0]), f"{what}: node {r.node}: group {g} is not uniform: {full(r)} != {full(rs[0])}"
    keys = [key(groups[g][0])[:3] + ((groups[g][0].dom_num << 32) | groups[g][0].dom_den,) for g in range(info.n_groups)]
    assert keys == sorted(keys), f"{what}: the groups are not sorted by (level, kind, sub_key, domain)"


def check_layout(what, ws, recs, info, cap):
    spans = lambda r: [cap * r.dom_num // r.dom_den + 1, cap * r.in_dom_num // r.in_dom_den + 1]
    zero = 2 * max([cap] + [x for r in recs for x in spans(r)])
    assert (info.zero_off, info.zero_floats) == (0, zero), f"{what}: the zero region is ({info.zero_off}, {info.zero_floats}), not (0, {zero})"
    line = {abi.KIND_VIDEO_MIXER: [0] * 3, abi.KIND_SOURCE_VIDEO: [0]}
    types = [line.get(k) for k, _p in ws.nodes]
    audio = port_types(ws) if all(t is None for t in types) else None
    regions = [(0, zero, "zero", -1)]
    for n, r in enumerate(recs):
        ty = types[n] if types[n] is not None else (audio[n] if audio is not None else [])
        assert r.n_out == len(ty), f"{what}: node {n}: {r.n_out} output ports"
        for p in range(r.n_out):
            if r.out_elided[p]:
                assert r.out_off[p] == NONE and r.out_off2[p] == NONE, f"{what}: node {n}: elided port {p} has an offset"
                continue
            fl = (1 if r.out_dup[p] else ty[p]) * (cap * r.dom_num // r.dom_den + 1)
            for off in (r.out_off[p], r.out_off2[p]):
                if off == NONE:
                    assert off is not r.out_off[p], f"{what}: node {n}: materialised port {p} has no offset"
                    continue
                assert off % 64 == 0, f"{what}: node {n}: port {p} offset {off} is not a multiple of 64 floats"
                regions.append((off, fl, p, n))
    regions.sort()
    for (a, la, pa, na), (b, _lb, pb, nb) in zip(regions, regions[1:]):
        assert a + la <= b, f"{what}: node {nb}: port {pb} at {b} overlaps node {na} port {pa} at {a} + {la}"
    assert regions[-1][0] + regions[-1][1] <= info.slab_floats, f"{what}: node {regions[-1][3]}: beyond the slab"


def check_all(what, ws, order=None, video=False):
    recs, info, cap = plan(ws)
    if not video:
        e_order, dom, bad = engine_domains(ws)
        assert bad is None
        check_order(what, recs, info, e_order if order is None else order)
        check_domains(what, recs, dom)
        check_fusion(what, recs, *predict_fusion(ws, e_order, n_inputs))
        unfused, _i, _c = plan(ws, flags=abi.FLAG_NO_FUSE)
        assert not any(r.elided or any(r.out_elided) or any(r.out_dup) for r in unfused), f"{what}: MX_FLAG_NO_FUSE folds something"
    check_structure(what, ws, recs, info)
    check_layout(what, ws, recs, info, cap)
    recs2, info2, cap2 = plan(ws, cap_frames=2 * cap)
    check_structure(what, ws, recs2, info2)
    check_layout(what + " (twice the capacity)", ws, recs2, info2, cap2)
    return recs, info


@pytest.mark.parametrize("shape_id,seed", FULL_SEEDS, ids=IDS)
def test_full_random_graph_plan(shape_id, seed):
    ws = full_ws(shape_id, seed)
    check_all(f"seed {seed}", ws, order=oracle.OracleGraph(ws).run_order())


@pytest.mark.parametrize("shape_id,seed", EDIT_SEEDS, ids=EDIT_IDS)
def test_every_workspace_of_an_edit_session_plan(shape_id, seed):
    stages = session_workspaces(shape_id, seed)
    assert len(stages) >= 3   # two edits at least
    for i, ws in enumerate(stages):
        check_all(f"seed {seed} after {i} edits", ws)   # (the session has held each stage's engine_domains order against the oracle's)


@pytest.mark.parametrize("seed", VIDEO_SEEDS)
def test_random_video_graph_plan(seed):
    ws = video_workspace(rv.scenario(seed))
    recs, info = check_all(f"video seed {seed}", ws, video=True)
    assert info.has_video == 1 and info.tail_first_group == -1
    for n, r in enumerate(recs):
        for _k, s in forward_inputs(ws, recs, n):
            assert recs[s[0]].pos < r.pos


# ---- the overlap-tail candidate ----
def bench_graph(strips=64, plotter=False, direct_source=False):
    """`strips` of Oscillator -> EqThree -> Panner -> Amplifier into one Mixer"""
    ws = Workspace(44100, 60)
    amps = []
    for i in range(strips):
        o = ws.oscillator(110.0 + i, 0); e = ws.eq_three(0.0, -3.0, 1.0); p = ws.stereo_panner(); a = ws.amplifier(1.0, 0.0)
        ws.connect(o, 0, e, 0); ws.connect(e, 0, p, 0); ws.connect(e, 0, p, 1); ws.connect(p, 0, a, 0)
        amps.append(a)
    extra = [ws.source_stereo()] if direct_source else []
    m = ws.mixer([(0.0, 1.0, False)] * (strips + len(extra)))
    for c, a in enumerate(amps + extra):
        ws.connect(a, 0, m, c)
    if plotter:
        ws.connect(m, 0, ws.plotter(), 0)
    return ws, amps, m


def tail(ws, ticks=16, flags=0, overlap_auto=1):
    recs, info, _cap = plan(ws, max_ticks=ticks, flags=flags, overlap_auto=overlap_auto)
    return recs, info, sorted((n, p) for n, r in enumerate(recs) for p in range(r.n_out) if r.out_off2[p] != NONE)


def test_tail_candidate_of_a_bench_shaped_graph():
    ws, amps, m = bench_graph()
    recs, info, ports = tail(ws)
    assert info.tail_first_group == info.n_groups - 1 == recs[m].group and info.tail_auto == 1
    assert ports == [(a, 0) for a in amps] and info.tail_ports == 64
    check_layout("bench graph", ws, recs, info, 16 * ws.spt)
    assert tail(ws, overlap_auto=0)[1].tail_first_group == -1
    assert tail(bench_graph(plotter=True)[0])[1].tail_first_group == -1
    assert tail(bench_graph(plotter=True)[0], flags=abi.FLAG_OVERLAP_TAIL)[1].tail_first_group == -1
    assert tail(bench_graph(direct_source=True)[0])[1].tail_first_group == -1
    assert tail(bench_graph(direct_source=True)[0], flags=abi.FLAG_OVERLAP_TAIL)[1].tail_first_group == -1
    for ws2, ticks in ((bench_graph(63)[0], 16), (ws, 15)):
        recs2, info2, ports2 = tail(ws2, ticks)
        assert info2.tail_first_group == -1 and ports2 == [] and info2.tail_ports == 0
        recs2, info2, ports2 = tail(ws2, ticks, flags=abi.FLAG_OVERLAP_TAIL)
        assert info2.tail_first_group == info2.n_groups - 1 and info2.tail_auto == 0 and len(ports2) == info2.tail_ports == len(ws2.nodes) // 4


# ---- every Error of the plan, with its code and message ----
INVALID, TYPE = abi.MX_ERR_INVALID, abi.MX_ERR_TYPE
FIR1 = struct.pack("<II", 1, 0) + struct.pack("<d", 1.0)


def rs(up, down):
    return struct.pack("<IIII", up, down, 1, 0) + struct.pack(f"<{up}d", *([1.0] * up))


SRC_S, SRC_M, OSC = (abi.KIND_SOURCE_STEREO, None), (abi.KIND_SOURCE_MONO, None), (abi.KIND_OSCILLATOR, abi.OscillatorParams(440.0, 0, 0))
ERRORS = {
    "edge node": ([SRC_S], [(0, 0, 1, 0)], INVALID, "edge references a node out of range", {}),
    "edge terminal": ([SRC_S, (abi.KIND_FIR, FIR1)], [(0, 1, 1, 0)], INVALID, "edge references a terminal out of range", {}),
    "line type": ([SRC_M, (abi.KIND_FIR, FIR1)], [(0, 0, 1, 0)], TYPE, "line type mismatch on connection", {}),
    "params_len": ([(abi.KIND_EQ_THREE, b"\0" * 8)], [], INVALID, "params_len does not match mx_eq_three_params", {}),
    "params_len plotter": ([(abi.KIND_PLOTTER, b"\0" * 4)], [], INVALID, "params_len does not match () (Plotter has no params)", {}),
    "params_len panner": ([(abi.KIND_STEREO_PANNER, b"\0" * 4)], [], INVALID, "params_len does not match ()", {}),
    "params_len mixer": ([(abi.KIND_MIXER, b"\0" * 25)], [], INVALID, "mixer params_len is not a multiple of mx_mixer_channel_params", {}),
    "params_len monitor": ([(abi.KIND_MONITOR, b"\0" * 12)], [], INVALID, "params_len does not match mx_monitor_params (or mx_monitor_params_ex)", {}),
    "unknown kind": ([(9999, None)], [], INVALID, "unknown module kind", {}),
    "fir blob": ([(abi.KIND_FIR, FIR1 + b"\0" * 8)], [], INVALID, "mx_fir_params: params_len must be 8 + 8 * n_taps (1 <= n_taps <= 16384)", {}),
    "resample blob": ([(abi.KIND_RESAMPLE, rs(2, 1)[:-8])], [], INVALID, "mx_resample_params: params_len must be 16 + 8 * up * taps_per_phase", {}),
    "mixed domains": ([SRC_S, (abi.KIND_RESAMPLE, rs(2, 1)), (abi.KIND_MIXER, [abi.MixerChannelParams(0.0, 1.0, 0)] * 2)],
                      [(0, 0, 1, 0), (0, 0, 2, 0), (1, 0, 2, 1)], TYPE, "inputs of a module live in different sample-rate domains", {}),
    "ratio": ([SRC_S, (abi.KIND_RESAMPLE, rs(1, 4))], [(0, 0, 1, 0)], INVALID, "resampling ratio does not give a whole number of samples per tick", {}),
    "plotter domain": ([SRC_S, (abi.KIND_RESAMPLE, rs(2, 1)), (abi.KIND_PLOTTER, None)], [(0, 0, 1, 0), (1, 0, 2, 0)], INVALID,
                       "Plotter is only accepted in the base sample-rate domain", {}),
    "rate-bound domain": ([SRC_S, (abi.KIND_RESAMPLE, rs(2, 1)), (abi.KIND_STEREO_SPLITTER, None), (abi.KIND_EQ_THREE, abi.EqThreeParams(0.0, 0.0, 0.0))],
                          [(0, 0, 1, 0), (1, 0, 2, 0), (2, 0, 3, 0)], INVALID,
                          "EqThree / Envelope / Oscillator / FmSine depend on the sample rate and are only accepted in the base domain", {}),
    "rate": ([OSC], [], INVALID, "sample_rate must be a multiple of ticks_per_second", {"sample_rate": 44100, "ticks_per_second": 8}),
    "contract": ([OSC], [], INVALID, "MX_FLAG_FP_CONTRACT is a mode of the exact-order kernels: not with MX_FLAG_EQ_FAST", {"flags": abi.FLAG_FP_CONTRACT | abi.FLAG_EQ_FAST}),
    "output device": ([(abi.KIND_OUTPUT_DEVICE, abi.OutputDeviceParams(257, -1, -1, 0))], [], INVALID,
                      "mx_output_device_params: channels <= 256, left / right >= -1 (-1 = None)", {}),
    "monitor size": ([(abi.KIND_MONITOR, struct.pack("<II", 81, 46))], [], INVALID, "monitor picture must be non-zero, even and at most 16384 a side", {}),
}


@pytest.mark.parametrize("name", list(ERRORS))
def test_plan_errors_keep_their_code_and_message(name):
    nodes, edges, code, message, opts = ERRORS[name]
    with pytest.raises(abi.MxError) as e:
        abi.debug_plan(nodes, edges, **opts)
    assert (e.value.code, str(e.value)) == (code, f"mixlab_gpu error {code}: {message}")


def test_engine_domains_refusals_come_back_with_the_same_message():
    why = {"mixed": "mixed domains", "ratio": "ratio", "rate": "rate-bound domain"}
    for reason, name in why.items():
        nodes, edges, code, message, _opts = ERRORS[name]
        ws = Workspace(44100, 60)
        ws.nodes = list(nodes)
        ws._conn = {(d, dp): (s, sp) for (s, sp, d, dp) in edges}
        assert engine_domains(ws)[2][1] == reason
    ws.nodes[-1] = (abi.KIND_PLOTTER, None); ws._conn[(3, 0)] = (1, 0)
    assert engine_domains(ws)[2] == (3, "rate")
    with pytest.raises(abi.MxError, match="Plotter is only accepted in the base sample-rate domain"):
        plan(ws)


# ---- the checks can fail ----
FAULT_SEEDS = [FULL_SEEDS[0], FULL_SEEDS[25], FULL_SEEDS[50]]


@pytest.mark.parametrize("shape_id,seed", FAULT_SEEDS, ids=[f"{s}-{n}" for s, n in FAULT_SEEDS])
def test_a_flipped_field_is_named_with_its_seed_and_node(shape_id, seed):
    ws = full_ws(shape_id, seed)
    order, _dom, _bad = engine_domains(ws)
    what = f"seed {seed}"
    folded, dup = predict_fusion(ws, order, n_inputs)
    # an elided bit
    recs, info, cap = plan(ws)
    n = next(n for n in order if recs[n].n_out)
    recs[n].out_elided[0] ^= 1
    with pytest.raises(AssertionError, match=rf"{what}: node {n}: port 0 elided"):
        check_fusion(what, recs, folded, dup)
    # a level
    recs, info, cap = plan(ws)
    n = next(n for n in order if not recs[n].elided and any(root_of(what, recs, s[0]) != n for _k, s in forward_inputs(ws, recs, n)))
    recs[n].level = 0
    with pytest.raises(AssertionError, match=rf"{what}: node {n}: "):
        check_structure(what, ws, recs, info)
    # an offset
    recs, info, cap = plan(ws)
    a, b = [n for n in order if recs[n].n_out and recs[n].out_off[0] != NONE][:2]
    recs[b].out_off[0] = recs[a].out_off[0]
    with pytest.raises(AssertionError, match=rf"{what}: node ({a}|{b}): port 0 at"):
        check_layout(what, ws, recs, info, cap)
    recs[b].out_off[0] += 32
    with pytest.raises(AssertionError, match=rf"{what}: node {b}: port 0 offset"):
        check_layout(what, ws, recs, info, cap)
    # a position
    recs, info, cap = plan(ws)
    recs[order[0]].pos = -1
    with pytest.raises(AssertionError, match=rf"{what}: "):
        check_order(what, recs, info, order)


def test_the_records_are_the_header_s_size():
    assert C.sizeof(abi.PlanNode) == 136 and C.sizeof(abi.PlanInfo) == 56
