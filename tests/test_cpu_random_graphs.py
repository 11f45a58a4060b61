"""The full random-graph generator (tests/test_gpu_random_graphs.py, random_graph(full=True)) and the oracle's graph runner without a GPU:
what the generator draws, that every graph it draws builds and runs in the oracle, and the oracle's sample-rate domain pass, which
follows Graph::Graph (mx_engine.cpp): back-edges carry no domain, and a module whose inputs live in two domains is refused."""
import hashlib

import numpy as np
import pytest

import oracle
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from random_taps import CLASS_OF, EMITTING, FAULTS, RESETTING, SETS, difference
from test_gpu_random_graphs import ALL_SETS_RUNS, ALL_SETS_SEEDS, FULL_SEEDS, engine_domains, port_types, random_graph, run_full_graph
from tick_shapes import by_id

AUDIO_KINDS = {abi.KIND_AMPLIFIER, abi.KIND_ENVELOPE, abi.KIND_EQ_THREE, abi.KIND_FM_SINE, abi.KIND_MIXER, abi.KIND_OSCILLATOR, abi.KIND_PLOTTER,
               abi.KIND_STEREO_PANNER, abi.KIND_STEREO_SPLITTER, abi.KIND_TRIGGER, abi.KIND_SOURCE_MONO, abi.KIND_SOURCE_STEREO, abi.KIND_FIR,
               abi.KIND_RESAMPLE, abi.KIND_OUTPUT_DEVICE}


def test_full_graphs_draw_every_kind_waveform_and_resampled_domains():
    kinds, waves, fed, cross, inside = set(), set(), 0, 0, 0
    for seed in range(64):
        ws, _sources = random_graph(seed, full=True)
        og = oracle.OracleGraph(ws)
        order = og.run_order()
        types = port_types(ws)
        kinds |= {ws.nodes[n][0] for n in order}
        waves |= {ws.nodes[n][1].waveform for n in order if ws.nodes[n][0] == abi.KIND_OSCILLATOR}
        # a resampled domain (read from the oracle's port lengths) that feeds a module other than a Resample
        resampled = {n for n in order for p, ty in enumerate(types[n]) if og.output(n, p).size != ty * ws.spt}
        pos = {n: i for i, n in enumerate(order)}
        edges = [(s, d) for (s, _sp, d, _dp) in ws.edges if s in pos and d in pos]
        fed += any(s in resampled and pos[s] < pos[d] and ws.nodes[d][0] != abi.KIND_RESAMPLE for (s, d) in edges)
        # back-edges out of a resampled port: into the same domain, and into a base-domain module
        _order, dom, _bad = engine_domains(ws)
        cross += any(s in resampled and pos[s] >= pos[d] and dom[d] == 1 for (s, d) in edges)
        inside += any(s in resampled and pos[s] >= pos[d] and dom[d] == dom[s] for (s, d) in edges)
    assert kinds == AUDIO_KINDS
    assert waves == {abi.WAVE_ON, abi.WAVE_OFF, abi.WAVE_SINE, abi.WAVE_SQUARE, abi.WAVE_TRIANGLE, abi.WAVE_SAW}
    assert fed >= 16
    assert cross >= 1 and inside >= 1


def test_round_one_graphs_are_unchanged():
    """full=False draws what it always drew: the 64 seeds of the first GPU test and the tick-shape tests keep their graphs (the digest
    of every node's kind and params, every edge and the source list, as the generator drew them before full=True existed)"""
    h = hashlib.sha256()
    for seed in range(64):
        ws, sources = random_graph(seed)
        for kind, params in ws.nodes:
            h.update(bytes([kind])); h.update(abi.params_bytes(params))
        h.update(repr(sorted(ws.edges)).encode()); h.update(repr(sources).encode())
    assert h.hexdigest() == "ed5c93852e1f4dc787cc8146f87fa7782a35c035bb30c35216b1df6f80c8d33b"


@pytest.mark.parametrize("shape_id,seed", [("44k1", s) for s in range(64)] + FULL_SEEDS)
def test_every_full_graph_builds_and_runs_in_the_oracle(shape_id, seed):
    shape = by_id(shape_id)
    ws, sources = random_graph(seed, shape.sample_rate, shape.ticks_per_second, full=True)
    order, dom, refusal = engine_domains(ws)
    assert refusal is None
    og = oracle.OracleGraph(ws)
    assert og.run_order() == order
    assert any(ws.nodes[n][0] == abi.KIND_MIXER for n in order)
    types = port_types(ws)
    for t in range(3):
        for (n, ty) in sources:
            og.set_source(n, np.full(ws.spt * ty, 0.25 * (t + 1), np.float32))
        og.run_tick(t)
        for n in order:
            for p, ty in enumerate(types[n]):
                assert og.output(n, p).size == ty * ws.spt * dom[n]


def back_edge_graph(splitter_reads_mixer):
    """source -> Resample(160 / 147) -> Mixer input 0; Amplifier -> Mixer input 1; Mixer -> Amplifier; a Splitter reads the Amplifier
    (the Mixer runs first, the Amplifier's edge into it is the back-edge) or the Mixer (the Amplifier runs first: its input is the back-edge)"""
    ws = Workspace(44100, 60)
    s = ws.source_stereo()
    r = ws.resample(160, 147, np.full((160, 4), 0.25))
    y = ws.mixer([(0.0, 1.0, False), (-6.0, 0.5, True)])
    m = ws.amplifier(0.5, 0.0)
    sp = ws.stereo_splitter()
    ws.connect(s, 0, r, 0); ws.connect(r, 0, y, 0); ws.connect(m, 0, y, 1); ws.connect(y, 0, m, 0)
    ws.connect(y if splitter_reads_mixer else m, 0, sp, 0)
    return ws, s, r, y, m, sp


def test_oracle_domain_pass_ignores_back_edges():
    ws, s, r, y, m, sp = back_edge_graph(False)
    og = oracle.OracleGraph(ws)
    assert og.run_order() == [s, r, y, m, sp]
    x = np.linspace(-1, 1, 2 * 735).astype(np.float32)
    og.set_source(s, x)
    og.run_tick(0)
    rs = og.output(r, 0)
    assert rs.size == 2 * 800
    for port in (og.output(y, 0), og.output(y, 1), og.output(m, 0)):
        assert port.size == 2 * 800   # the Mixer and the Amplifier live in the Resample's domain: the back-edge gave them none
    assert og.output(sp, 0).size == 800
    # the Mixer's input 1 reads Disconnected: its outputs are input 0's alone
    master, cue = oracle.mixer_run([(0.0, 1.0, False), (-6.0, 0.5, True)], [rs, None], rs.size)
    assert np.array_equal(og.output(y, 0).view(np.uint32), master.view(np.uint32))
    assert np.array_equal(og.output(y, 1).view(np.uint32), cue.view(np.uint32))
    order, dom, refusal = engine_domains(ws)
    assert refusal is None and dom[y] == dom[m] == dom[r] != 1


def test_oracle_refuses_a_module_whose_inputs_live_in_two_domains():
    ws, s, r, y, m, sp = back_edge_graph(True)
    with pytest.raises(RuntimeError):
        oracle.OracleGraph(ws)   # the Amplifier runs first in the base domain; the Mixer mixes it with the Resample's output
    order, dom, refusal = engine_domains(ws)
    assert order == [s, r, m, y, sp] and refusal == (y, "mixed")


def test_oracle_runs_an_output_device_as_a_sink_in_the_engine_run_order():
    ws = Workspace(48000, 60)
    src = ws.source_stereo()
    od_a = ws.output_device(2, 0, 1)
    amp = ws.amplifier(1.5, 0.0)
    od_b = ws.output_device(6, 9, None)
    ws.connect(src, 0, amp, 0); ws.connect(amp, 0, od_b, 0)
    og = oracle.OracleGraph(ws)
    assert og.run_order() == engine_domains(ws)[0] == [od_a, src, amp, od_b]
    og.set_source(src, np.ones(1600, np.float32))
    og.run_tick(0)
    og.update_params(od_a, abi.OutputDeviceParams(8, 7, 7, 0))
    og.run_tick(1)
    assert np.all(og.output(amp, 0) == np.float32(1.5))


# ---------------------------------------------------------------------------------------------------------------------------
# the random taps of all seven sets (tests/random_taps.py) on the oracle and the models alone: the draws of
# test_full_random_graph_every_tap_set, what they cover, that there is something to see, and that each way the tap host could be
# wrong changes the records that test compares
# ---------------------------------------------------------------------------------------------------------------------------
def test_full_graphs_and_the_meter_draws_are_unchanged():
    """random_graph(full=True) and run_full_graph's own stream (default_rng(7000 + seed): meter taps and their params, run lengths,
    updates, events, lag notes) draw for every existing test id what they drew before the other tap sets got a stream of their own
    (default_rng(8000 + seed)): the digests were taken before tests/random_taps.py existed.  The second one needs the ports the fused
    build folds away (the meters are drawn among the others); tests/test_gpu_random_graphs.py asserts that prediction on the device."""
    h = hashlib.sha256()
    for shape_id, seed in [("44k1", s) for s in range(64)] + FULL_SEEDS:
        shape = by_id(shape_id)
        ws, sources = random_graph(seed, shape.sample_rate, shape.ticks_per_second, full=True)
        for kind, params in ws.nodes:
            h.update(bytes([kind])); h.update(abi.params_bytes(params))
        h.update(repr(sorted(ws.edges)).encode()); h.update(repr(sources).encode())
    assert h.hexdigest() == "7847646b1e38d2e0bae8cd1d4e045bb068cf35a7970771bf3341f5f304f0538a"
    h = hashlib.sha256()
    for shape_id, seed in FULL_SEEDS:
        drawn = []
        run_full_graph(shape_id, seed, (), abi.FLAG_EQ_EXACT, collect=drawn)
        h.update(repr(drawn).encode())
    assert h.hexdigest() == "3f5021bb53f2c52297929eafd1a5d4e2171a7ddf7869e9fcf42085a75a98a260"


_expected = {}


def expected(shape_id, seed, fault=None):
    """(the RandomTaps, [{"run", "ticks", "want": {set: records}}]) of one seed: the oracle and the models alone"""
    if (seed, fault) not in _expected:
        runs = []
        ts = run_full_graph(shape_id, seed, (), abi.FLAG_EQ_EXACT, tap_sets=SETS, n_runs=ALL_SETS_RUNS, fault=fault, collect=runs)
        if fault is not None:
            return ts, runs
        _expected[(seed, fault)] = (ts, runs)
    return _expected[(seed, fault)]


def test_every_set_is_set_again_on_its_own_and_after_a_one_tick_run():
    empties = 0
    for shape_id, seed in ALL_SETS_SEEDS:
        ts, runs = expected(shape_id, seed)
        assert ALL_SETS_RUNS[0] <= len(runs) < ALL_SETS_RUNS[1] and runs[ts.one_tick_run]["ticks"] == 1 and ts.one_tick_run + 1 < len(runs)
        assert any(ts.one_tick_run + 1 in ts.plan[name] for name in SETS)
        assert len({tuple(sorted(ts.plan[name])) for name in SETS}) > 1          # not all at the same runs
        for name in SETS:
            assert ts.plan[name] and min(ts.plan[name]) >= 1
            n_empty = sum(1 for what in ts.plan[name].values() if what == "empty")
            empties += n_empty
            if shape_id != "8k_8000":
                assert sum(1 for ports in ts.orders[name] if not ports) == n_empty, f"{shape_id} {seed}: {name} was left without a tap"
            assert all(len(set(ports)) == len(ports) <= ts.cap for ports in ts.orders[name])
    assert empties >= len(SETS)


def test_the_taps_cover_every_kind_of_port():
    """Summed over the seeds, every set taps a Source, an Oscillator or FmSine, an EqThree, an Amplifier, a Mixer, a Fir or Resample, a
    control line (Trigger or Envelope), a mono and a stereo port, a dup-stored port and a port whose tick is not spt frames -- the stereo
    field set the stereo ones among them (an EqThree, a Trigger and an Envelope have mono outputs only) -- and no set is given sorted lists only.
    Most sets also tap an Oscillator's stereo twin, and some the one Mixer without channels these graphs have."""
    seen = {name: set() for name in SETS}
    for shape_id, seed in ALL_SETS_SEEDS:
        ts, _runs = expected(shape_id, seed)
        for name in SETS:
            for pt in ts.tapped[name]:
                seen[name] |= {CLASS_OF[ts.ws.nodes[pt[0]][0]], "mono" if ts.types[pt[0]][pt[1]] == 1 else "stereo"}
                seen[name] |= {"own_tick"} if ts.frames[pt] != ts.spt else set()
                seen[name] |= {"dup"} if pt in ts.dup else set()
                if ts.ws.nodes[pt[0]][0] == abi.KIND_MIXER and not ts.ws.nodes[pt[0]][1]:
                    seen[name].add("empty_mixer")
                if ts.ws.nodes[pt[0]][0] == abi.KIND_OSCILLATOR and pt[1] == 1:
                    seen[name].add("stereo_twin")
            if any(ports != sorted(ports) for ports in ts.orders[name]):
                seen[name].add("unsorted")
    stereo_only = {"source", "oscillator", "amplifier", "mixer", "fir_resample", "stereo", "own_tick", "dup", "unsorted"}
    for name in SETS:
        want = stereo_only if name == "stereo" else stereo_only | {"eq", "control", "mono"}
        assert want <= seen[name], f"{name}: no tap on {sorted(want - seen[name])}"
    assert sum("empty_mixer" in s for s in seen.values()) >= 2 and sum("stereo_twin" in s for s in seen.values()) >= 5   # (of the seven sets)


def something_to_see(name, rec):
    if rec["ticks"] is None and rec["emitted"] is None:
        return False
    if name == "meters":
        return bool((rec["ticks"]["hold"] > 0).any())
    if name == "spectra":
        return bool((rec["ticks"] > 0).any())
    if name == "loudness":
        return bool((rec["ticks"]["true_peak"] > 0).any())
    if name == "stereo":
        return rec["emitted"] is not None and any(r["gon"].any() for _t, row in rec["emitted"] for r in row)
    if name == "limiters":
        return bool((rec["ticks"]["min_gain"] < 1).any()) and any(not np.array_equal(y.view(np.uint32), x.view(np.uint32))
                                                                   for y, x in zip(rec["limited"], rec["delayed"]))
    at = 28                                   # a record without its tick_in_run: 28 more bytes of header, then the table
    if name == "tempo":
        return any(np.frombuffer(b, "<u8", 1, at)[0] > 0 for _t, row in rec["emitted"] for b in row)
    return any(int.from_bytes(b[:4], "little") > 0 and np.frombuffer(b, "<u8", -1, at).any() for _t, row in rec["emitted"] for b in row)


def test_every_set_has_something_to_see():
    """not trivially empty records: a band above 0, a true peak above 0, a goniometer emission with cells, a gain below 1 and a limited copy
    that is not the delayed input, a tempo record with R[0] > 0, a tonality record with hops and a non-zero bin -- each on at least three
    seeds of 44k1 and three of 48k"""
    lively = {(name, shape_id): 0 for name in SETS for shape_id in ("44k1", "48k")}
    for shape_id, seed in ALL_SETS_SEEDS:
        if shape_id in ("44k1", "48k"):
            _ts, runs = expected(shape_id, seed)
            for name in SETS:
                lively[(name, shape_id)] += any(something_to_see(name, r["want"][name]) for r in runs)
    print(lively)
    assert min(lively.values()) >= 3, lively


# the seeds the faults are tried on (a 48 kHz desk, 441-frame ticks, and the short ticks: a spectrum's history is longer than a tick there only)
FAULT_SEEDS = [ALL_SETS_SEEDS[i] for i in (9, 16, 19, 20, 21, 22)]
APPLIES = {"no_reset": RESETTING, "meters_reset": ("meters",), "reset_per_run": SETS, "c_per_run": EMITTING, "base_frames": SETS,
           "left_only": SETS, "sorted_order": SETS, "one_tick_late": SETS}


@pytest.mark.parametrize("fault", FAULTS)
def test_a_wrong_tap_host_changes_the_expected_records(fault):
    """Each fault is one way the device could be wrong that test_full_random_graph_every_tap_set exists to notice (random_taps.FAULTS): with
    it switched into the EXPECTED side, the records of every set it applies to must differ from the right ones on one of FAULT_SEEDS --
    by the very comparison the GPU test uses.  The draws are the same with and without the fault."""
    assert FAULT_SEEDS[0][0] == "48k" and {s for s, _ in FAULT_SEEDS[1:]} == {"44k1_100", "16k_1000", "8k_8000"}
    caught = {name: [] for name in APPLIES[fault]}
    for shape_id, seed in FAULT_SEEDS:
        ts, right = expected(shape_id, seed)
        ts_f, wrong = expected(shape_id, seed, fault)
        assert ts_f.orders == ts.orders and [r["ticks"] for r in wrong] == [r["ticks"] for r in right]
        for name in SETS:
            if any(difference(name, a["want"][name], b["want"][name]) for a, b in zip(wrong, right)):
                assert name in caught, f"{fault} changed the {name} records of seed {seed}: it should not touch that set"
                caught[name].append(seed)
    print(f"{fault}: caught by " + ", ".join(f"{name} {seeds}" for name, seeds in caught.items()))
    assert all(caught.values()), f"{fault}: no seed catches it for {[name for name, seeds in caught.items() if not seeds]}"
