"""The random edit sessions (tests/random_edits.py, tests/test_gpu_random_edits.py) on the oracle and the models alone: that the expected
side's adopt is right without trusting it, what the draws are (pinned), what they cover, and that each way a device's
mx_graph_adopt_state could be wrong changes the values the GPU test compares."""
import hashlib

import numpy as np
import pytest

import oracle
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from random_edits import EDIT_SEEDS, FAULTS, SPECIAL, STATEFUL, run_edit_session

IDS = [f"{s}-{n}" for s, n in EDIT_SEEDS]
_sessions = {}


def session(shape_id, seed, fault=None):
    """(coverage, [the expected values of every run]) of one seed; without a fault the graph of before each edit runs on beside the edited
    one (shadow=True: run_edit_session asserts that every survivor with an untouched input cone gives the same in both)"""
    if (seed, fault) not in _sessions:
        runs = []
        cover = run_edit_session(shape_id, seed, (), abi.FLAG_EQ_EXACT, special=SPECIAL.get((shape_id, seed)), fault=fault, collect=runs, shadow=fault is None)
        if fault is not None:
            return cover, runs
        _sessions[(seed, fault)] = (cover, runs)
    return _sessions[(seed, fault)]


def chain(n_fir, n_rs=5):
    """source -> EqThree; gate -> Envelope; stereo source -> Fir(n_fir) -> Resample(2 / 1, n_rs per phase) -> Plotter"""
    ws = Workspace(44100, 60)
    s = ws.source_mono(); e = ws.eq_three(3.0, -6.0, 4.5); g = ws.source_mono(); v = ws.envelope()
    ss = ws.source_stereo(); f = ws.fir(np.linspace(-0.4, 0.4, n_fir)); r = ws.resample(2, 1, np.linspace(-0.3, 0.3, 2 * n_rs).reshape(2, n_rs))
    sp = ws.source_stereo(); p = ws.plotter()
    ws.connect(s, 0, e, 0); ws.connect(g, 0, v, 0); ws.connect(ss, 0, f, 0); ws.connect(f, 0, r, 0); ws.connect(sp, 0, p, 0)
    return ws, (s, e, g, v, ss, f, r, sp, p)


def test_oracle_adopt_state_carries_each_state_and_only_at_equal_length():
    """the fixed rules of OracleGraph.adopt_state, read from include/mixlab_gpu.h: eq, env, plot and hist of every mapped node; a history only
    where the carried length is the same; kinds must match; params are not state"""
    rng = np.random.default_rng(1)
    ws, ids = chain(9)
    s, e, g, v, ss, f, r, sp, p = ids
    a = oracle.OracleGraph(ws)
    for t in range(4):
        a.set_source(s, rng.uniform(-1, 1, 735)); a.set_source(g, np.ones(735, np.float32)); a.set_source(ss, rng.uniform(-1, 1, 1470)); a.set_source(sp, rng.uniform(-1, 1, 1470))
        a.run_tick(t)
    fresh = oracle.OracleGraph(ws)
    assert all(a.node_state(n) != fresh.node_state(n) for n in (e, v, f, r, p))
    b = oracle.OracleGraph(ws)
    b.adopt_state(a, list(range(len(ws.nodes))))
    assert all(b.node_state(n) == a.node_state(n) for n in range(len(ws.nodes)))
    c = oracle.OracleGraph(ws)
    c.adopt_state(a, [-1 if n in (e, f) else n for n in range(len(ws.nodes))])
    assert c.node_state(e) == fresh.node_state(e) and c.node_state(f) == fresh.node_state(f) and c.node_state(v) == a.node_state(v)
    ws2, _ids = chain(10, 4)             # both filters changed their length: from silence; the others carried
    d = oracle.OracleGraph(ws2)
    d.adopt_state(a, list(range(len(ws.nodes))))
    assert not d.hist(f).any() and not d.hist(r).any() and d.hist(f).size == 20 and d.hist(r).size == 8
    assert d.node_state(e) == a.node_state(e) and d.node_state(v) == a.node_state(v) and d.node_state(p) == a.node_state(p)
    with pytest.raises(TypeError):
        b.adopt_state(a, [e, s] + list(range(2, len(ws.nodes))))
    with pytest.raises(AssertionError):
        b.adopt_state(a, [0])
    with pytest.raises(AssertionError):
        b.adopt_state(a, [99] + list(range(1, len(ws.nodes))))
    # the next tick of the adopted graph is the next tick of the old one
    for graph in (a, b):
        graph.set_source(s, np.full(735, 0.5, np.float32)); graph.set_source(g, np.zeros(735, np.float32))
        graph.set_source(ss, np.full(1470, 0.25, np.float32)); graph.set_source(sp, np.full(1470, 0.1, np.float32))
        graph.run_tick(4)
    for n, port in ((e, 0), (v, 0), (f, 0), (r, 0)):
        assert np.array_equal(a.output(n, port).view(np.uint32), b.output(n, port).view(np.uint32))
    assert (a.plotter(p) is None) == (b.plotter(p) is None)


@pytest.mark.parametrize("shape_id,seed", EDIT_SEEDS, ids=IDS)
def test_a_survivor_with_an_untouched_cone_does_not_notice_the_edit(shape_id, seed):
    """The oracle's adopt shown right without trusting it: the graph of before each edit is kept running beside the edited one, fed the same
    samples and updates module by module, and every survivor whose whole input cone -- the modules, params, sources and connections it
    depends on -- the edit left alone gives the same output in both, tick by tick (the assertions are run_edit_session's, shadow=True).
    Before a session's first edit that graph was never edited."""
    session(shape_id, seed)


def test_every_stateful_kind_has_such_a_survivor():
    seen = {what for s in EDIT_SEEDS for what, _run, _node in session(*s)[0]}
    for name in STATEFUL.values():
        assert "cone0_" + name in seen, f"no {name} with an untouched cone survives a first edit"


DIGESTS = {200: "c1f99e77776fb7a6", 201: "e2e439c6093341cd", 202: "7def620754a93444", 203: "d61a02dce2d524a5", 204: "7f484247641f1a2a", 205: "b11aa04d86fd459d",
           206: "b63589596768b1db", 207: "08ab8a8e0ffe299d", 300: "0b9afd781137f728", 301: "039c3b69d7df5299", 302: "55e1b34187bc56f6", 303: "4baeb03a7d3f675e",
           304: "66d7c55e4dabbdd5", 400: "961497d7ed1db879", 500: "d4e74f0e4269d21c", 600: "4caf3401abf67560"}


def digest(runs):
    h = hashlib.sha256()
    for r in runs[:-1]:
        h.update(repr((r["run"], r["ticks"], r["tick0"], r["taps"], r["edited"])).encode())
    h.update(repr(runs[-1]).encode())
    return h.hexdigest()[:16]


@pytest.mark.parametrize("shape_id,seed", EDIT_SEEDS, ids=IDS)
def test_the_draws_are_pinned(shape_id, seed):
    """workspaces (kinds, built params, edges), mappings, held params, meter taps, run lengths and the state of the session's stream at its end"""
    _cover, runs = session(shape_id, seed)
    assert 4 <= len(runs) - 1 <= 7 and sum(1 for r in runs[:-1] if r["edited"]) >= 2 and runs[0]["edited"] is None
    assert all(1 <= r["ticks"] <= 6 for r in runs[:-1])
    assert digest(runs) == DIGESTS[seed]


def test_the_edits_cover_every_way_a_state_crosses():
    """Each of these survives at least one edit with a state that is not a fresh module's at that moment (the oracle's state bytes of the
    adopted node against those of the same graph built fresh; an OutputDevice: a recorded clip or lag time, or a pending lag note).
    Layouts are predicted: an Envelope is inline where the fusion planner folds its port into the EqThree kernel (random_taps.predict_fusion,
    which the GPU tests hold to the built graph); groups and slots are the MX_FLAG_NO_FUSE layout's (random_edits.predict_slots)."""
    seen = {}
    for s in EDIT_SEEDS:
        for what, run, node in session(*s)[0]:
            seen.setdefault(what, []).append((s[1], run, node))
    print({k: len(v) for k, v in sorted(seen.items())})
    for what in ("eq", "env_standalone_to_inline", "env_inline_to_standalone", "env_standalone_to_standalone", "fir_offset", "fir_relen", "resample",
                 "plot", "od", "od_reparam", "slot_changed", "group_changed", "returned", "edit_none", "edit_all", "parked_in", "parked_out"):
        assert seen.get(what), f"no edit of the seed set has: {what}"
    assert len(seen["edit_none"]) == len(seen["edit_all"]) == 1


# fault -> where the expected values change: (shape, seed, run, what) with what ("port", node, port) | ("plot", node) | ("od", node)
FAULT_AT = {
    "no_eq": ("44k1", 200, 1, ("port", 0, 0)),
    "no_env": ("44k1", 203, 2, ("port", 21, 0)),
    "no_fir": ("44k1", 204, 1, ("port", 21, 0)),
    "no_resample": ("44k1", 204, 1, ("port", 37, 0)),
    "no_plot": ("44k1", 204, 1, ("plot", 9)),
    "no_od": ("44k1", 200, 4, ("od", 12)),
    "fresh_carried": ("44k1", 201, 3, ("port", 0, 0)),
    "new_of_old": ("44k1", 200, 1, ("port", 0, 0)),
    "off_by_one": ("44k1", 200, 1, ("port", 0, 0)),
    "relen_carried": ("48k", 304, 2, ("port", 25, 0)),
    "creation_params": ("44k1", 200, 1, ("port", 0, 0)),
    "od_new_params": ("44k1", 200, 4, ("od", 12)),
}


def differences(right, wrong):
    """[(run, what)] where the expected values of two sessions of the same draws differ"""
    out = []
    for a, b in zip(right[:-1], wrong[:-1]):
        out += [(a["run"], ("port",) + pt) for pt in a["ports"] if a["ports"][pt] != b["ports"][pt]]
        out += [(a["run"], ("plot", n)) for n in a["plot"] if a["plot"][n] != b["plot"][n]]
        out += [(a["run"], ("od", n)) for n in a["od"] if a["od"][n] != b["od"][n]]
    return out


@pytest.mark.parametrize("fault", FAULTS)
def test_a_wrong_adopt_changes_the_expected_values(fault):
    """Each fault is one way a device's mx_graph_adopt_state could be wrong (random_edits.FAULTS).  With it switched into the EXPECTED side, the
    values of the named seed, run and port (or Plotter, or OutputDevice) differ from the right ones -- the values the GPU test compares bit
    for bit, so a device with that fault fails there.  The draws are the same with and without the fault."""
    shape_id, seed, run, what = FAULT_AT[fault]
    _cover, right = session(shape_id, seed)
    _cover, wrong = session(shape_id, seed, fault)
    assert digest(wrong) == digest(right)
    diff = differences(right, wrong)
    print(f"{fault}: {len(diff)} values differ, first {diff[:3]}")
    assert (run, what) in diff
    only = {"no_eq": abi.KIND_EQ_THREE, "no_env": abi.KIND_ENVELOPE, "no_fir": abi.KIND_FIR, "no_resample": abi.KIND_RESAMPLE, "no_plot": abi.KIND_PLOTTER,
            "no_od": abi.KIND_OUTPUT_DEVICE, "od_new_params": abi.KIND_OUTPUT_DEVICE, "relen_carried": abi.KIND_FIR}.get(fault)
    if only is not None:                 # the named value is the faulted module's own output
        assert right[run]["kinds"][what[1]] == only
