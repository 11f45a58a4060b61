"""Random topology edits for the full random graphs (tests/test_gpu_random_graphs.py random_graph(full=True)), shared by the GPU test
(tests/test_gpu_random_edits.py) and its CPU proof (tests/test_cpu_random_edits.py): what an edit draws, how a session of runs and edits
goes, and what every build must give after mx_graph_adopt_state -- the oracle's graph runner with OracleGraph.adopt_state, the meter and
OutputDevice models fed the ORACLE's samples.

The rules the expected side follows are the header's (include/mixlab_gpu.h): a surviving module keeps its state -- EqThree poles and delay
line, Envelope state, Fir / Resample history, Plotter count, and of an OutputDevice everything the module holds, its params included --
a Fir / Resample whose length changed starts from silence, a new module starts fresh, taps are not carried.  `fault` makes the expected
side wrong in exactly one of those ways (FAULTS): the CPU test shows that each of them changes the values the GPU test compares.

Everything here is drawn from a stream of its own (default_rng(7100 + seed)); the graph generator's draws are its own as ever.  Nothing here
needs a GPU but what `builds` names."""
from __future__ import annotations

import copy
import hashlib
import struct
from fractions import Fraction

import numpy as np

import oracle
import synth
from meter_model import METER_TICK, MeterModel, records_equal
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from output_device_model import OutputDeviceModel
from random_taps import predict_fusion
from test_gpu_random_graphs import (FULL_KINDS, FULL_SEEDS, MAX_RUN, MONO, OUT_TYPES, PARAM_KINDS, STEREO, FullDraw, bits, drop_refused_edges, engine_domains, n_inputs,
                                    od_args, port_types, random_graph, random_od, random_params)
from tick_shapes import by_id

FAULTS = ("no_eq", "no_env", "no_fir", "no_resample", "no_plot", "no_od", "fresh_carried", "new_of_old", "off_by_one", "relen_carried",
          "creation_params", "od_new_params")
STATEFUL = {abi.KIND_EQ_THREE: "eq", abi.KIND_ENVELOPE: "env", abi.KIND_FIR: "fir", abi.KIND_RESAMPLE: "resample", abi.KIND_PLOTTER: "plot",
            abi.KIND_OUTPUT_DEVICE: "od"}
IN_TYPES = {abi.KIND_AMPLIFIER: [STEREO, MONO], abi.KIND_ENVELOPE: [MONO], abi.KIND_EQ_THREE: [MONO], abi.KIND_FM_SINE: [MONO], abi.KIND_PLOTTER: [STEREO],
            abi.KIND_STEREO_PANNER: [MONO, MONO], abi.KIND_STEREO_SPLITTER: [STEREO], abi.KIND_FIR: [STEREO], abi.KIND_RESAMPLE: [STEREO],
            abi.KIND_OUTPUT_DEVICE: [STEREO]}
BASE = Fraction(1)


def input_types(kind, params):
    return [STEREO] * len(params) if kind == abi.KIND_MIXER else IN_TYPES.get(kind, [])


def fir_taps(params):
    return struct.unpack_from("<I", params)[0]


# ---------------------------------------------------------------------------------------------------------------------------
# the draw of one edit
# ---------------------------------------------------------------------------------------------------------------------------
def edit(rng, ws, current_params, intended, graveyard=None, mode=None, info=None):
    """-> (ws', mapping): the workspace after one topology edit and, per node of ws', the index in `ws` of the module it is (-1: a new one).

    A random 10-30 % of the modules go; about as many new ones come, drawn by the generator's own per-kind rules (FullDraw) -- or, some of
    them, taken back from `graveyard` (the (kind, params) of modules removed by earlier edits; this edit's go into it): a module that
    returns is a new module.  A random share of the survivors' inputs is drawn again, the inputs that lost their producer among them;
    half the time a surviving EqThree and a surviving Envelope are wired into a strip like the benchmark's (new Panner, Amplifier and
    Trigger around them), so that the fused build evaluates that Envelope inline from then on.  Then the node order is permuted and
    drop_refused_edges makes the graph one the engine builds.  Survivors are built with `current_params[node]`, with two exceptions on
    purpose: now and then a surviving Fir gets another tap count (it must start from silence), and a surviving OutputDevice other params
    than it holds (they are not applied: info["current"] keeps the held ones).

    mode "all": every module survives as it is, only the order changes.  mode "none": nothing survives.
    info (a dict) receives "intended" and "current" of ws' and the lists "fir_relen", "od_reparam", "returned" (nodes of ws') and "strip"."""
    N = len(ws.nodes)
    graveyard = graveyard if graveyard is not None else []
    if mode == "all":
        gone = set()
    elif mode == "none":
        gone = set(range(N))
    else:
        gone = {int(n) for n in rng.choice(N, size=min(N - 1, max(1, int(round(N * rng.uniform(0.1, 0.3))))), replace=False)}
    survivors = [n for n in range(N) if n not in gone]
    _order, dom, _bad = engine_domains(ws)
    tmp = Workspace(ws.sample_rate, ws.ticks_per_second)
    dr = FullDraw(rng, tmp)
    t_of, held, relen, reparam, returned = {}, {}, [], [], []
    for n in survivors:
        kind, params = ws.nodes[n][0], current_params[n]
        built = params
        t = len(tmp.nodes)
        if kind == abi.KIND_FIR and mode is None and rng.random() < 0.15:
            other = int(rng.integers(1, 70))
            other += other >= fir_taps(params)
            built = params = struct.pack("<II", other, 0) + rng.uniform(-0.5, 0.5, other).tobytes()
            relen.append(t)
        elif kind == abi.KIND_OUTPUT_DEVICE and mode is None and rng.random() < 0.3:
            c, left, right = random_od(rng)
            built = abi.OutputDeviceParams(c, -1 if left is None else left, -1 if right is None else right, 0)
            reparam.append(t)
        assert tmp.add(kind, built) == t
        t_of[n] = t
        held[t] = params
        d = dom.get(n, intended.get(n, BASE))
        dr.intended[t] = intended.get(n, BASE)
        if d not in dr.domains:
            dr.domains.append(d)
        for p, ty in enumerate(OUT_TYPES[kind]):
            dr.out(t, p, ty, d)
    for (d_n, d_p), (s_n, s_p) in ws._conn.items():
        if d_n in t_of and s_n in t_of:
            tmp._conn[(t_of[d_n], d_p)] = (t_of[s_n], s_p)
    graveyard += [(ws.nodes[n][0], current_params[n]) for n in sorted(gone)] if mode is None else []
    old_pool = len(graveyard) - len(gone) if mode is None else len(graveyard)   # only modules of EARLIER edits return
    if mode != "all":
        # survivors' inputs: the ones that lost their producer half the time, the others a random share
        share = rng.uniform(0.1, 0.4)
        for n in survivors:
            kind, params = ws.nodes[n]
            for k, ty in enumerate(input_types(kind, params)):
                lost = (n, k) in ws._conn and ws._conn[(n, k)][0] in gone
                if rng.random() < (0.5 if lost else share):
                    tmp._conn.pop((t_of[n], k), None)
                    dr.ins.append((t_of[n], k, ty, dr.intended[t_of[n]]))
        n_new = int(rng.integers(10, 30)) if mode == "none" else max(1, int(round(N * rng.uniform(0.1, 0.3)))) if N < 44 else 1
        for _ in range(n_new):
            u = rng.random()
            if u < 0.3 and old_pool > 0:
                kind, params = graveyard.pop(int(rng.integers(0, old_pool)))
                old_pool -= 1
                t = tmp.add(kind, params)
                returned.append(t)
                d = nd = dr.pick_domain(kind)
                if kind == abi.KIND_RESAMPLE:      # (its ratio gives whole ticks in the base domain: it was drawn so)
                    ratio = Fraction(*struct.unpack_from("<II", params))
                    d = d if (tmp.spt * d * ratio).denominator == 1 else BASE
                    nd = d * ratio
                dr.intended[t] = d
                if nd not in dr.domains:
                    dr.domains.append(nd)
                for p, ty in enumerate(OUT_TYPES[kind]):
                    dr.out(t, p, ty, nd)
                dr.ins += [(t, k, ty, d) for k, ty in enumerate(input_types(kind, params))]
            elif u < 0.36:
                dr.sink()
            else:
                dr.module(rng.choice(FULL_KINDS))
        for (n, port, ty, d) in dr.ins:
            dr.connect_input(n, port, ty, d)
    strip = None
    eqs = [t for t in t_of.values() if tmp.nodes[t][0] == abi.KIND_EQ_THREE]
    envs = [t for t in t_of.values() if tmp.nodes[t][0] == abi.KIND_ENVELOPE]
    if mode is None and eqs and envs and rng.random() < 0.5:
        e, v = eqs[int(rng.integers(0, len(eqs)))], envs[int(rng.integers(0, len(envs)))]
        for key in [key for key, src in tmp._conn.items() if src in ((e, 0), (v, 0))]:
            del tmp._conn[key]
        p = tmp.stereo_panner(); a = tmp.amplifier(1.0, 0.5); g = tmp.trigger(bool(rng.integers(0, 2)))
        tmp.connect(e, 0, p, 0); tmp.connect(e, 0, p, 1); tmp.connect(p, 0, a, 0); tmp.connect(g, 0, v, 0); tmp.connect(v, 0, a, 1)
        if rng.random() < 0.5:          # read by a Mixer: the Amplifier's port is stored one float per frame
            bus = tmp.mixer([(float(rng.uniform(-12, 0)), 0.8, False)])
            tmp.connect(a, 0, bus, 0)
        strip = (e, v)
    M = len(tmp.nodes)
    perm = [int(x) for x in rng.permutation(M)]          # node t of tmp is node perm[t] of ws'
    if M > 1 and perm == list(range(M)):
        perm = perm[1:] + perm[:1]
    ws2 = Workspace(ws.sample_rate, ws.ticks_per_second)
    inv = [0] * M
    for t, i in enumerate(perm):
        inv[i] = t
    ws2.nodes = [tmp.nodes[inv[i]] for i in range(M)]
    for (d_n, d_p), (s_n, s_p) in tmp._conn.items():
        ws2._conn[(perm[d_n], d_p)] = (perm[s_n], s_p)
    old_of_t = {t: n for n, t in t_of.items()}
    mapping = [old_of_t.get(inv[i], -1) for i in range(M)]
    intended2 = {perm[t]: d for t, d in dr.intended.items()}
    drop_refused_edges(ws2, intended2)
    if info is not None:
        info.update(intended=intended2, current=[held.get(inv[i], tmp.nodes[inv[i]][1]) for i in range(M)], fir_relen=sorted(perm[t] for t in relen),
                    od_reparam=sorted(perm[t] for t in reparam), returned=sorted(perm[t] for t in returned),
                    strip=None if strip is None else (perm[strip[0]], perm[strip[1]]))
    return ws2, mapping


# ---------------------------------------------------------------------------------------------------------------------------
# what a workspace is to the engine: run order, ports, the fusion plan and the launch layout
# ---------------------------------------------------------------------------------------------------------------------------
def predict_slots(ws, order, dom):
    """{node: ((level, kind, domain), slot)} as Graph::Graph lays out an MX_FLAG_NO_FUSE build: launch groups by (level, kind, domain) in
    run order, a node's slot its rank in its group.  (The fused build moves EqThree groups by their epilogue; Fir, Resample and standalone
    Envelope groups are laid out like this in both.)  An OutputDevice is in no group."""
    pos = {n: i for i, n in enumerate(order)}
    level, count, slots = {}, {}, {}
    for n in order:
        kind, params = ws.nodes[n]
        srcs = [ws._conn.get((n, k)) for k in range(n_inputs(kind, params))]
        fwd = [s[0] for s in srcs if s is not None and s[0] in pos and pos[s[0]] < pos[n]]
        level[n] = max([level[s] + 1 for s in fwd], default=0)
        in_dom = dom[fwd[0]] if fwd else BASE
        if kind != abi.KIND_OUTPUT_DEVICE:
            key = (level[n], kind, dom[n], in_dom)
            slots[n] = (key, count.get(key, 0))
            count[key] = count.get(key, 0) + 1
    return slots


class Stage:
    """one workspace of a session with what the comparison needs of it"""

    def __init__(self, ws, uid, current):
        self.ws, self.uid, self.current = ws, list(uid), list(current)
        self.order, self.dom, bad = engine_domains(ws)
        assert bad is None
        self.pos = {n: i for i, n in enumerate(self.order)}
        self.types = port_types(ws)
        self.sources = [(n, MONO if ws.nodes[n][0] == abi.KIND_SOURCE_MONO else STEREO) for n in range(len(ws.nodes))
                        if ws.nodes[n][0] in (abi.KIND_SOURCE_MONO, abi.KIND_SOURCE_STEREO)]
        self.frames = {(n, p): int(ws.spt * self.dom[n]) for n in self.order for p in range(len(self.types[n]))}
        self.ods = [n for n in self.order if ws.nodes[n][0] == abi.KIND_OUTPUT_DEVICE]
        self.plotters = [n for n in self.order if ws.nodes[n][0] == abi.KIND_PLOTTER]
        self.od_in = {od: self.read_src(od, 0) for od in self.ods}
        self.folded, self.stored_dup = predict_fusion(ws, self.order, n_inputs)
        self.common = [pt for pt in self.frames if pt not in self.folded]
        self.updatable = [n for n in self.order if ws.nodes[n][0] in PARAM_KINDS and ws.nodes[n][1]]
        self.slots = predict_slots(ws, self.order, self.dom)
        self._cone = {}

    def read_src(self, n, k):
        """the port input k of node n reads, None where it reads Disconnected (unconnected, a back-edge, a producer that never runs)"""
        src = self.ws._conn.get((n, k))
        return src if src is not None and src[0] in self.pos and self.pos[src[0]] < self.pos[n] else None

    def inline_env(self, n):
        return (n, 0) in self.folded          # the fused build evaluates this Envelope in its EqThree's kernel (state2)

    def cone(self, n):
        """a digest of everything node n's output depends on: its module (by uid), kind and params, and the same of every producer it reads"""
        if n not in self._cone:
            kind, _p = self.ws.nodes[n]
            ins = []
            for k in range(n_inputs(kind, self.ws.nodes[n][1])):
                src = self.read_src(n, k) if n in self.pos else None
                ins.append(None if src is None else (self.cone(src[0]), src[1]))
            what = repr((self.uid[n], kind, n in self.pos, abi.params_bytes(self.current[n]), ins))
            self._cone[n] = hashlib.sha256(what.encode()).hexdigest()
        return self._cone[n]


def oracle_workspace(st, born=None, mapping=None):
    """the workspace the oracle is built from: the stage's with every module's CURRENT params (fault: survivors get their creation params)"""
    ws = Workspace(st.ws.sample_rate, st.ws.ticks_per_second)
    ws.nodes = [(kind, st.current[n]) for n, (kind, _p) in enumerate(st.ws.nodes)]
    if born is not None:             # (a Fir may have changed its length since: it keeps what it was built with)
        ws.nodes = [(kind, born[st.uid[n]] if mapping[n] >= 0 and kind != abi.KIND_FIR else p) for n, (kind, p) in enumerate(ws.nodes)]
    ws._conn = dict(st.ws._conn)
    return ws


def adopt(og_new, og_old, mapping, st_new, st_old, od_old, rate, fault=None):
    """The expected side of mx_graph_adopt_state: the oracle's adopt_state for the graph, and for every OutputDevice of the new stage the model
    that goes on (the survivor's own: the module persists, the new build's params are not applied) or a new one.  -> {od: model}.
    `fault` (FAULTS) makes it wrong in one way; the draws do not depend on it."""
    kinds_new = [k for k, _p in st_new.ws.nodes]
    kinds_old = [k for k, _p in st_old.ws.nodes]
    eff = list(mapping)
    if fault == "new_of_old":            # the list read as "old node j is new node list[j]"
        eff = [-1] * len(mapping)
        for j, i in enumerate(mapping):
            if 0 <= j < len(kinds_old) and 0 <= i < len(eff):
                eff[i] = j
    elif fault == "off_by_one":
        eff = [j + 1 if j >= 0 else -1 for j in mapping]
    elif fault == "fresh_carried":       # a new module takes the state of the first old module of its kind
        for i, j in enumerate(mapping):
            if j < 0 and kinds_new[i] in STATEFUL:
                eff[i] = next((o for o, k in enumerate(kinds_old) if k == kinds_new[i]), -1)
    eff = [j if 0 <= j < len(kinds_old) and kinds_old[j] == kinds_new[i] else -1 for i, j in enumerate(eff)]   # (a device refuses the rest; here: nothing carried)
    skip = {"no_eq": abi.KIND_EQ_THREE, "no_env": abi.KIND_ENVELOPE, "no_fir": abi.KIND_FIR, "no_resample": abi.KIND_RESAMPLE,
            "no_plot": abi.KIND_PLOTTER, "no_od": abi.KIND_OUTPUT_DEVICE}.get(fault)
    eff = [-1 if kinds_new[i] == skip else j for i, j in enumerate(eff)]
    og_new.adopt_state(og_old, eff)
    if fault == "relen_carried":         # as much of the history as fits, whatever the lengths
        for i, j in enumerate(eff):
            if j >= 0 and kinds_new[i] in (abi.KIND_FIR, abi.KIND_RESAMPLE):
                a, b = og_new.hist(i), og_old.hist(j)
                if a is not None and b is not None and a.size != b.size:
                    a[:min(a.size, b.size)] = b[:min(a.size, b.size)]
    ods = {}
    for od in st_new.ods:
        j = eff[od]
        if j >= 0 and j in od_old:
            ods[od] = od_old[j]
            if fault == "od_new_params":
                ods[od].update(*od_args(st_new.ws.nodes[od][1]))
        else:
            ods[od] = OutputDeviceModel(rate, *od_args(st_new.ws.nodes[od][1]))
    return ods


# ---------------------------------------------------------------------------------------------------------------------------
# a session: runs of 1-6 ticks with edits at run boundaries
# ---------------------------------------------------------------------------------------------------------------------------
# sixteen of the full graphs: eight at 44.1 kHz, five at 48 kHz, one each of the 100, 1000 and 8000 ticks-per-second shapes.  The first
# session's first edit keeps every module and only permutes them; the second's keeps none.
EDIT_SEEDS = FULL_SEEDS[:8] + FULL_SEEDS[24:29] + [FULL_SEEDS[48], FULL_SEEDS[51], FULL_SEEDS[53]]
SPECIAL = {EDIT_SEEDS[0]: "all", EDIT_SEEDS[1]: "none"}
BUILD_FLAGS = {"fused": 0, "unfused": abi.FLAG_NO_FUSE, "ticked": 0, "overlap": abi.FLAG_OVERLAP_TAIL, "mixed": 0}


def build_flags(name, n_edits):
    """"mixed" alternates between the fused layout and MX_FLAG_NO_FUSE from edit to edit: every state crosses between the two layouts, both ways"""
    return abi.FLAG_NO_FUSE if name == "mixed" and n_edits % 2 else BUILD_FLAGS[name]


def run_edit_session(shape_id, seed, builds, flags, first_tick=0, special=None, fault=None, collect=None, shadow=False):
    """random_graph(full=True) through 4-7 runs of 1-6 ticks from `first_tick`, with a topology edit (edit()) before about half of the runs
    after the first, two at least: every build in `builds` builds the edited graph with its own flags, adopts the old one's state, closes the
    old one and sets its meters again; the oracle does OracleGraph.adopt_state (adopt()).  Scheduled updates, updates between runs and lag
    notes go on as in run_full_graph.  Compared bit for bit per run: every materialised port of every build, the meter records, the
    OutputDevice hand-offs and records, and every Plotter's indication of every tick.

    special = "all" / "none": the session's first edit keeps every module (only the order changes) / keeps none.
    builds may be empty: the oracle and the models alone; every run's expected values are appended to `collect` (a list), `fault` is adopt()'s.
    shadow: the oracle graph of before each edit is kept running beside the edited one, fed the same samples and updates module by module;
    every survivor whose whole input cone the edit left alone must give the same output in both -- the adopt shown right without trusting
    it.  -> the coverage the session reached: a list of (what, run, node)."""
    shape = by_id(shape_id)
    ws, _sources = random_graph(seed, shape.sample_rate, shape.ticks_per_second, full=True)
    spt = ws.spt
    rate = shape.sample_rate
    rng = np.random.default_rng(7100 + seed)
    n_uid = len(ws.nodes)
    st = Stage(ws, range(n_uid), [p for _k, p in ws.nodes])
    born = {u: p for u, (_k, p) in enumerate(ws.nodes)}
    intended = {n: st.dom.get(n, BASE) for n in range(len(ws.nodes))}
    og = oracle.OracleGraph(oracle_workspace(st))
    assert og.run_order() == st.order
    n_edits = 0
    graphs = {name: ws.build(max_ticks_per_run=1 if name == "ticked" else MAX_RUN, flags=flags | build_flags(name, 0)) for name in builds}
    od_models = {od: OutputDeviceModel(rate, *od_args(ws.nodes[od][1])) for od in st.ods}
    n_runs = int(rng.integers(4, 8))
    edits_at = {r for r in range(1, n_runs) if rng.random() < 0.5}
    while len(edits_at) < 2:
        edits_at.add(int(rng.integers(1, n_runs)))
    graveyard, cover = [], []
    taps, tap_params, models = [], {}, {}
    prev = None                          # shadow: (the stage before the last edit, its oracle graph, its OutputDevice models, {new node: old node} with untouched cones)

    def ports_of(name, g, stage):
        fused_layout = not (flags | build_flags(name, n_edits)) & abi.FLAG_NO_FUSE
        got = []
        for pt in stage.frames:
            try:
                g.read_output(*pt, 1, stage.types[pt[0]][pt[1]] == STEREO, rate=(stage.frames[pt], spt))
                got.append(pt)
            except abi.MxError as e:
                assert fused_layout and "MX_FLAG_NO_FUSE" in str(e)   # folded away by the graph compiler
        assert set(got) == set(stage.frames) - (stage.folded if fused_layout else set()), f"seed {seed}: {name}: the fusion plan is not the predicted one"
        return got

    def set_taps(stage):
        """taps are not carried: a random third of the ports and every OutputDevice's input, every meter from 0"""
        new = {pt for pt in stage.common if rng.random() < 1 / 3} | {src for src in stage.od_in.values() if src is not None}
        new = sorted(new)
        tap_params.clear(); models.clear()
        for pt in new:
            tap_params[pt] = abi.MeterParams(int(rng.integers(0, 9)), float(rng.uniform(0.5, 1.0)))
            models[pt] = MeterModel(stage.types[pt[0]][pt[1]], tap_params[pt].hold_ticks, tap_params[pt].release)
        for g in graphs.values():
            g.set_meters(new, [tap_params[pt] for pt in new])
        return new

    ports = {name: ports_of(name, g, st) for name, g in graphs.items()}
    taps = set_taps(st)
    tick = first_tick
    for run in range(n_runs):
        edited = None
        if run in edits_at:
            mode = special if n_edits == 0 else None
            info = {}
            ws2, mapping = edit(rng, st.ws, st.current, intended, graveyard, mode, info)
            uid2 = [st.uid[j] if j >= 0 else n_uid + sum(1 for x in mapping[:i] if x < 0) for i, j in enumerate(mapping)]
            n_uid += sum(1 for j in mapping if j < 0)
            st2 = Stage(ws2, uid2, info["current"])
            for i, j in enumerate(mapping):
                if j < 0:
                    born[uid2[i]] = ws2.nodes[i][1]
            og2 = oracle.OracleGraph(oracle_workspace(st2, born if fault == "creation_params" else None, mapping))
            assert og2.run_order() == st2.order
            fresh = oracle.OracleGraph(oracle_workspace(st2))
            if shadow:
                shadow_ods = {od: copy.deepcopy(m) for od, m in od_models.items()}
            od_models = adopt(og2, og, mapping, st2, st, od_models, rate, fault)
            cover += coverage(run, mode, mapping, info, st, st2, og, og2, fresh, od_models)
            if shadow:
                same = {i: j for i, j in enumerate(mapping) if j >= 0 and i in st2.pos and j in st.pos and st2.cone(i) == st.cone(j)}
                prev = (st, og, shadow_ods, same, n_edits == 0)
            n_edits += 1
            for name in list(graphs):
                g2 = ws2.build(max_ticks_per_run=1 if name == "ticked" else MAX_RUN, flags=flags | build_flags(name, n_edits))
                assert g2.run_order() == st2.order
                g2.adopt_state(graphs[name], mapping)
                graphs[name].close()
                graphs[name] = g2
            edited = {"mapping": list(mapping), "nodes": [(k, abi.params_bytes(p)) for k, p in ws2.nodes], "edges": sorted(ws2.edges),
                      "held": [abi.params_bytes(p) for p in st2.current], "mode": mode}
            st, og, intended = st2, og2, info["intended"]
            ports = {name: ports_of(name, g, st) for name, g in graphs.items()}
            taps = set_taps(st)
        L = int(rng.integers(1, MAX_RUN + 1))
        ws = st.ws
        shadow_node = {}
        if prev is not None:
            old_of_uid = {u: j for j, u in enumerate(prev[0].uid)}
            shadow_node = {n: old_of_uid[u] for n, u in enumerate(st.uid) if u in old_of_uid}

        def update(n, p, scheduled_for=None):
            """ModuleT::update on the expected side, and on the builds unless it is scheduled into the run"""
            st.current[n] = p
            og.update_params(n, p)
            if n in od_models:
                od_models[n].update(*od_args(p))
            j = shadow_node.get(n)
            if j is not None and len(abi.params_bytes(p)) == len(abi.params_bytes(prev[0].current[j])):
                prev[1].update_params(j, p)
                if j in prev[2]:
                    prev[2][j].update(*od_args(p))
            if scheduled_for is None:
                for g in graphs.values():
                    g.update_params(n, p)

        if run and rng.random() < 0.5 and st.updatable:   # updates between runs
            for n in rng.choice(st.updatable, size=min(len(st.updatable), 3), replace=False):
                update(int(n), random_params(rng, ws, int(n)))
        for od in st.ods:
            if rng.random() < 0.3:       # the cpal callback ran short
                od_models[od].note_lag()
                if shadow_node.get(od) in (prev[2] if prev else {}):
                    prev[2][shadow_node[od]].note_lag()
                for g in graphs.values():
                    g.audio_out_lag(od)
        events = {}                      # tick in run -> [(node, params)], one event per node and tick
        for n in st.updatable:
            if rng.random() < 0.3:
                for k in sorted(set(rng.integers(0, L, size=int(rng.integers(1, 3))).tolist())):
                    events.setdefault(k, []).append((n, random_params(rng, ws, n)))

        def samples(u, ty):              # a source's samples belong to the module, whatever its index
            return (synth.noise(9000 + 97 * seed + 13 * run + u, L * spt * ty) * np.float32(1.5)).astype(np.float32)

        data = {n: samples(st.uid[n], ty) for (n, ty) in st.sources}
        want, want_meters, want_od, want_plot = {}, [], {od: ([], []) for od in st.ods}, {n: [] for n in st.plotters}
        for k in range(L):
            for (n, p) in events.get(k, []):
                update(n, p, scheduled_for=k)
            for (n, ty) in st.sources:
                og.set_source(n, data[n][k * spt * ty:(k + 1) * spt * ty])
            og.run_tick(tick + k)
            for pt in st.frames:
                want.setdefault(pt, []).append(og.output(*pt))
            want_meters.append([models[pt].tick(og.output(*pt)) for pt in taps])
            for od in st.ods:
                x = og.output(*st.od_in[od]) if st.od_in[od] is not None else np.zeros(2 * spt, np.float32)
                pushed, rec = od_models[od].run_tick((tick + k) * spt, x)
                want_od[od][0].append(pushed); want_od[od][1].append(rec)
            for n in st.plotters:
                want_plot[n].append(og.plotter(n))
            if prev is not None:
                cover += shadow_tick(prev, st, og, run, tick + k, k, spt, L, samples, want_od, what=f"{shape_id} seed {seed} run {run} tick {k}")
        want_meters = np.array(want_meters, dtype=METER_TICK).reshape(L, len(taps))
        if collect is not None:
            collect.append({"run": run, "ticks": L, "tick0": tick, "edited": edited, "taps": list(taps),
                            "ports": {pt: b"".join(x.tobytes() for x in want[pt]) for pt in st.frames}, "meters": want_meters.tobytes(),
                            "od": {od: (b"".join(x.tobytes() for x in want_od[od][0]), list(want_od[od][1])) for od in st.ods},
                            "plot": {n: [None if v is None else v[0].tobytes() + v[1].tobytes() for v in want_plot[n]] for n in st.plotters},
                            "stage": st, "kinds": [k for k, _p in st.ws.nodes]})
        for name, g in graphs.items():
            step = 1 if name == "ticked" else L
            got, got_meters, got_od = {}, [], {od: [[], []] for od in st.ods}
            what = f"{shape_id} seed {seed} run {run} ({L} ticks from {tick}, {n_edits} edits): {name} graph"
            for k0 in range(0, L, step):
                for (n, ty) in st.sources:
                    g.write_source(n, data[n][k0 * spt * ty:(k0 + step) * spt * ty], step)
                for k in range(k0, k0 + step):
                    for (n, p) in events.get(k, []):
                        g.schedule_params(n, k - k0, p)
                g.run_ticks(tick + k0, step)
                for pt in ports[name]:
                    got.setdefault(pt, []).append(g.read_output(*pt, step, st.types[pt[0]][pt[1]] == STEREO, rate=(st.frames[pt], spt)))
                got_meters.append(g.read_meters(0, step))
                for od in st.ods:
                    s, r = g.read_audio_out(od, 0, step)
                    got_od[od][0].append(s); got_od[od][1] += [tuple(int(v) for v in q) for q in r.tolist()]
                for n in st.plotters:
                    for k in range(k0, k0 + step):
                        a, b = g.read_plotter(n, k - k0), want_plot[n][k]
                        assert (a is None) == (b is None), f"{what}: Plotter {n} tick {k}: fired {a is not None}, the oracle's {b is not None}"
                        assert a is None or all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b)), f"{what}: Plotter {n} tick {k}: left / right differ"
            for pt, chunks in got.items():
                a, b = np.concatenate(chunks), np.concatenate(want[pt])
                assert np.array_equal(bits(a), bits(b)), f"{what}: node {pt[0]} (kind {ws.nodes[pt[0]][0]}) port {pt[1]} differs from the oracle"
            ok = records_equal(np.concatenate(got_meters), want_meters)
            if not ok.all():
                k, i = (int(v[0]) for v in np.nonzero(~ok))
                raise AssertionError(f"{what}: meter on {taps[i]} tick {k}: got {np.concatenate(got_meters)[k, i]}, want {want_meters[k, i]}")
            for od in st.ods:
                a, b = np.concatenate(got_od[od][0]), np.concatenate(want_od[od][0])
                assert a.size == b.size and np.array_equal(bits(a), bits(b)), f"{what}: OutputDevice {od} hand-off differs"
                assert got_od[od][1] == want_od[od][1], f"{what}: OutputDevice {od} records {got_od[od][1]} != {want_od[od][1]}"
        tick += L
    for g in graphs.values():
        g.close()
    if collect is not None:
        collect.append({"rng": rng.bit_generator.state["state"]})
    return cover


def shadow_tick(prev, st, og, run, tick, k, spt, L, samples, want_od, what):
    """one tick of the graph of before the last edit, and the comparison of every survivor with an untouched cone"""
    st0, og0, ods0, same, first = prev
    for (j, ty) in st0.sources:
        og0.set_source(j, samples(st0.uid[j], ty)[k * spt * ty:(k + 1) * spt * ty])
    og0.run_tick(tick)
    seen = []
    for i, j in same.items():
        kind = st.ws.nodes[i][0]
        for p in range(len(st.types[i])):
            assert np.array_equal(bits(og.output(i, p)), bits(og0.output(j, p))), f"{what}: node {i} (kind {kind}) port {p} is not what it is without the edit"
        if kind == abi.KIND_PLOTTER:
            a, b = og.plotter(i), og0.plotter(j)
            assert (a is None) == (b is None) and (a is None or all(np.array_equal(bits(x), bits(y)) for x, y in zip(a, b))), f"{what}: Plotter {i}"
        if kind == abi.KIND_OUTPUT_DEVICE:
            x = og0.output(*st0.od_in[j]) if st0.od_in[j] is not None else np.zeros(2 * spt, np.float32)
            pushed, rec = ods0[j].run_tick(tick * spt, x)
            assert np.array_equal(bits(pushed), bits(want_od[i][0][-1])) and rec == want_od[i][1][-1], f"{what}: OutputDevice {i} is not what it is without the edit"
        if kind in STATEFUL and k == 0:
            seen.append(("cone_" + STATEFUL[kind], run, i))
            if first:                    # the graph beside it was never edited
                seen.append(("cone0_" + STATEFUL[kind], run, i))
    return seen


def coverage(run, mode, mapping, info, st, st2, og, og2, fresh, od_models):
    """what this edit puts to the test: (what, run, node of the new graph) for every survivor whose state, at this moment, is not a fresh module's"""
    out = []
    if mode is not None:
        out.append(("edit_" + mode, run, -1))
    out += [("returned", run, i) for i in info["returned"]]
    for i, j in enumerate(mapping):
        kind = st2.ws.nodes[i][0]
        if j < 0 or kind not in STATEFUL:
            continue
        if i not in st2.pos or j not in st.pos:      # outside the run order on one side: no launch serves the module there, its state waits
            if kind != abi.KIND_OUTPUT_DEVICE and og2.node_state(i) != fresh.node_state(i):
                out.append(("parked_" + ("in" if i not in st2.pos else "out") + ("" if j in st.pos or i in st2.pos else "_parked"), run, i))
            continue
        if kind == abi.KIND_OUTPUT_DEVICE:
            m = od_models[i]
            lively = m.last_clip is not None or m.last_lag is not None or m.lag_flag
            if lively and i in info["od_reparam"]:
                out.append(("od_reparam", run, i))
        elif kind == abi.KIND_FIR and i in info["fir_relen"]:
            if np.any(og.hist(j)):
                out.append(("fir_relen", run, i))
            continue
        else:
            lively = og2.node_state(i) != fresh.node_state(i)
        if not lively:
            continue
        name = STATEFUL[kind]
        out.append((name, run, i))
        if kind == abi.KIND_ENVELOPE:
            out.append((f"env_{'inline' if st.inline_env(j) else 'standalone'}_to_{'inline' if st2.inline_env(i) else 'standalone'}", run, i))
        if kind == abi.KIND_FIR and st2.slots[i][1] > 0:
            out.append(("fir_offset", run, i))
        if kind == abi.KIND_RESAMPLE and st2.slots[i][1] > 0:
            out.append(("resample_offset", run, i))
        if kind != abi.KIND_OUTPUT_DEVICE and st.slots[j] != st2.slots[i]:
            out.append(("slot_changed", run, i))
        if kind != abi.KIND_OUTPUT_DEVICE and st.slots[j][0] != st2.slots[i][0]:
            out.append(("group_changed", run, i))
    return out
