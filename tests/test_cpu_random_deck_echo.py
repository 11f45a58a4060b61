"""The random deck sessions with the echo (tests/random_decks.py session(echo=True)) on the oracle and the models alone, in the manner of
tests/test_cpu_random_decks.py: what the seeds of tests/test_gpu_random_deck_echo.py draw, that with echo=False not a draw moves, that the seeds cover the
paths the GPU test is there for (COVERAGE), that the echo is heard, and that each way the device could get such a session wrong (random_decks.ECHO_FAULTS)
changes an item that test compares."""
import hashlib

import numpy as np
import pytest

import deck_echo_model as em
import random_decks as rd
from deck_model import T_PLAY
from mixlab_amd import abi
from random_taps import SETS, predict_fusion
from test_cpu_random_decks import run_difference
from test_cpu_random_decks import session as plain_session
from test_gpu_random_deck_echo import SEEDS, TAP_SEEDS
from test_gpu_random_graphs import ALL_SETS_RUNS, engine_domains, n_inputs, run_full_graph

SESSIONS = [("meters", s, n) for s, n in SEEDS] + [("all", s, n) for s, n in TAP_SEEDS]
# the two tiny tick lengths are exempt: a session there is 12 to 30 ticks of 16 frames or of one, so few frames or none lie past the shortest delay of 256 and a
# share of ticks that differ from dry means nothing; tests/deck_echo_cases.py has their sound
AUDIBLE_SHAPES = ("44k1", "48k", "44k1_100")
_sessions = {}

COVERAGE = {"two echo decks and one without in a feed", "a walking echo deck before a one-block one in feed order", "echo on a key-locked deck",
            "echo heard by Fir or Resample", "echo heard by an OutputDevice",
            "left out while ringing and fed again", "load on a ringing deck", "set_keylock set on a ringing deck", "set_keylock change on a ringing deck",
            "set_keylock clear on a ringing deck", "off -> on inside a feed", "delay lowered under a running block", "freeze", "ping-pong",
            "block across a tick boundary", "one-block and walking forms", "echo schedule in the one-tick run of an all-taps session",
            "echo on at 16k_1000", "echo on at 8k_8000", "set_echo set", "set_echo repeat", "set_echo clear", "schedule_echo OFF", "on again after OFF",
            "longest delay", "wet 0", "negative feedback", "damp 0", "damp 0.3", "damp 1", "echo-out"}


def session(mode, shape_id, seed, fault=None):
    """(the DeckSession, [{"run", "ticks", "ports", "decks", "taps"}]) of one seed: the oracle and the models alone"""
    key = (mode, seed, fault)
    if key not in _sessions:
        runs = []
        kw = {} if mode == "meters" else {"tap_sets": SETS, "n_runs": ALL_SETS_RUNS}
        ds = run_full_graph(shape_id, seed, (), abi.FLAG_EQ_EXACT, collect=runs, decks=rd.session(fault, echo=True), **kw)
        runs = [r for r in runs if "decks" in r]
        if fault is not None:
            return ds, runs
        _sessions[key] = (ds, runs)
    return _sessions[key]


def echo_ticks(ds, r):
    """(deck, tick, dry, port, whether PLAY is set in the tick) of every fed tick with the echo on"""
    for n in r["fed"]:
        e = r["info"][n]["echo"]
        dry, port = (np.asarray(e[k]).reshape(r["ticks"], -1) for k in ("dry", "port"))
        for k, st in enumerate(e["sets"]):
            if st is not None:
                yield n, k, dry[k], port[k], bool(r["info"][n]["recs"][k].flags & T_PLAY)


def test_the_seed_lists_are_the_issues():
    by_shape = {s: sum(1 for x, _n in SEEDS if x == s) for s, _n in SEEDS}
    assert by_shape == {"44k1": 4, "48k": 4, "44k1_100": 1, "16k_1000": 1, "8k_8000": 1}
    assert 2 <= len(TAP_SEEDS) <= 3 and set(TAP_SEEDS) <= set(SEEDS)


def test_the_draws_are_pinned():
    """everything the plain sessions pin, and every echo call"""
    h = hashlib.sha256()
    for mode, shape_id, seed in SESSIONS:
        ds, _runs = session(mode, shape_id, seed)
        h.update(repr((mode, shape_id, seed, ds.drawn)).encode())
    assert h.hexdigest() == "07fc72df46cd9d514cbe9ef63f1a8bd427185ca974291b2999b3e728ed19181f"


def test_without_the_echo_not_a_draw_moves_and_with_it_the_other_streams_draw_what_they_drew():
    for mode, shape_id, seed in SESSIONS[:3] + SESSIONS[-1:]:
        ds, _runs = session(mode, shape_id, seed)
        plain, plain_runs = plain_session(mode, shape_id, seed)
        assert [x for x in ds.drawn if not x[0].startswith("echo")] == plain.drawn
        assert ds.rng.bit_generator.state == plain.rng.bit_generator.state and plain.erng is None
        assert all("echo" not in r["info"][n] for r in plain.runs for n in r["fed"]) and all("echo_counts" not in r["decks"] for r in plain_runs)


def test_the_pools_are_the_issues():
    for spt, short in ((735, [256, 257, 734, 735, 736, 737, 1473]), (800, [256, 257, 799, 800, 801, 802, 1603]), (441, [256, 257, 440, 441, 442, 443, 885]),
                       (16, [256, 257]), (1, [256, 257])):
        assert rd.echo_delay_pool(spt) == (short, [5000, 262144])
    assert abs(sum(rd.ECHO_GAIN_WEIGHTS) - 1) < 1e-12 and len(rd.ECHO_GAIN_WEIGHTS) == len(rd.ECHO_GAINS)
    assert all(em.check(em.Echo(256, *g, 0)) is None for g in rd.ECHO_GAINS)
    for mode, shape_id, seed in SESSIONS:
        ds, _runs = session(mode, shape_id, seed)
        assert sum(1 for d in ds.decks.values() if not d.has_echo) == max(1, round(len(ds.decks) / 3)) and len(ds.decks) >= 2
        assert all(n in r["fed"] for r in ds.runs for n in list(r["echo_set"]) + list(r["echo_sched"]))       # a left-out deck gets no echo call
        assert all(len(s) <= 3 for r in ds.runs for s in r["echo_sched"].values())
        assert all(not r["info"][n]["echo"]["sched"] for r in ds.runs for n in r["fed"] if not ds.decks[n].has_echo)
        order, _dom, refusal = engine_domains(ds.ws)      # (what the plain sessions ask of their graphs, on seeds that are not all theirs)
        assert refusal is None and predict_fusion(ds.ws, order, n_inputs)[1], f"{shape_id} {seed}: the graft left no port stored one float per frame"
        if mode == "all":
            assert ds.runs[ds.taps.one_tick_run]["ticks"] == 1 and all(ds.taps.tapped[name] & set(ds.taps.dup) for name in SETS)
    share = [d.has_echo for _m, s, n in SESSIONS for d in session(_m, s, n)[0].decks.values()]
    assert 0.25 < 1 - sum(share) / len(share) < 0.42, f"{len(share) - sum(share)} of {len(share)} decks never have an echo"


def covered():
    """{item of COVERAGE: the first (mode, shape, seed, run, deck) that shows it}"""
    seen = {}

    def note(item, *where):
        seen.setdefault(item, where)

    for mode, shape_id, seed in SESSIONS:
        ds, _runs = session(mode, shape_id, seed)
        spt = ds.spt
        left = {}                              # deck -> it sat out the last run(s) with its echo on, the clock past 0 and a line that is not silent
        for r in ds.runs:
            at = (mode, shape_id, seed, r["run"])
            for n, what in r["keylock"].items():
                if r["ringing"].get(n) and what[0] != "repeat":
                    note(f"set_keylock {what[0]} on a ringing deck", *at, n)
            for n in r["load"]:
                if r["ringing"].get(n):
                    note("load on a ringing deck", *at, n)
            for n in ds.decks:
                if n not in r["fed"]:
                    left[n] = left.get(n) or bool(r["ringing"].get(n))
            echoing = [n for n in r["fed"] if any(r["info"][n]["echo"]["delays"])]
            if len(echoing) >= 2 and len(echoing) < len(r["fed"]):
                note("two echo decks and one without in a feed", *at)
            forms = [len(r["info"][n]["echo"]["blocks"]) == 1 for n in echoing]
            if any(not a and any(forms[i + 1:]) for i, a in enumerate(forms)):
                note("a walking echo deck before a one-block one in feed order", *at)
            if True in forms and False in forms:
                note("one-block and walking forms", *at)
            for n in r["fed"]:
                i, e = r["info"][n], r["info"][n]["echo"]
                if left.pop(n, False) and e["ringing"] and e["t0"] > 0 and e["delays"][0]:
                    note("left out while ringing and fed again", *at, n)
                if n in r["echo_set"]:
                    note(f"set_echo {r['echo_set'][n][0]}", *at, n)
                if not any(e["delays"]):
                    continue
                if i["kl"] is not None:
                    note("echo on a key-locked deck", *at, n)
                listeners = {rd.SLOT_CLASS.get(ds.ws.nodes[d][0]) for (d, _dp), src in ds.ws._conn.items() if src == (n, 0)}
                if "fir_resample" in listeners:
                    note("echo heard by Fir or Resample", *at, n)
                if "output_device" in listeners:
                    note("echo heard by an OutputDevice", *at, n)
                d = e["delays"]
                if any(not a and b for a, b in zip(d, d[1:])):
                    note("off -> on inside a feed", *at, n)
                    if any(a and not b for a, b in zip(d, d[1:])) and d.index(0) > 0:
                        note("on again after OFF", *at, n)
                if any(x is em.OFF for x in e["sched"].values()):
                    note("schedule_echo OFF", *at, n)
                for first, frames in e["blocks"]:
                    if first // spt != (first + frames - 1) // spt:
                        note("block across a tick boundary", *at, n)
                    for k in range(first // spt + 1, len(d)):      # tick k lowers the delay under a block that began before it and would have gone on
                        if first < k * spt <= first + frames and 0 < d[k] < d[k - 1] and first + d[k - 1] - 1 > k * spt and first + frames < first + d[k - 1] - 1:
                            note("delay lowered under a running block", *at, n)
                if mode == "all" and r["run"] == ds.taps.one_tick_run and e["sched"]:
                    note("echo schedule in the one-tick run of an all-taps session", *at, n)
                if shape_id in ("16k_1000", "8k_8000"):
                    note(f"echo on at {shape_id}", *at, n)
                for k, st in enumerate(e["sets"]):
                    if st is None:
                        continue
                    gains = (st.send, st.feedback, st.wet, st.damp)
                    for item, yes in (("freeze", gains == rd.FREEZE and (e["ringing"] or (k > 0 and d[k - 1]))), ("ping-pong", st.flags & em.PINGPONG),
                                      ("longest delay", st.delay == em.MAX_DELAY), ("wet 0", st.wet == 0), ("negative feedback", st.feedback < 0), ("damp 0", st.damp == 0),
                                      ("damp 0.3", st.damp == 0.3), ("damp 1", st.damp == 1)):
                        if yes:
                            note(item, *at, n)
                playing = [bool(t.flags & T_PLAY) for t in i["recs"]]
                dry, port = (np.asarray(e[k]).reshape(r["ticks"], -1) for k in ("dry", "port"))
                if any(d[k] and not playing[k] and not dry[k].any() and port[k].any() for k in range(len(d))):
                    note("echo-out", *at, n)
    return seen


def test_the_seeds_cover_what_the_gpu_test_is_there_for():
    seen = covered()
    for item in sorted(seen):
        print(f"{item}: {seen[item]}")
    assert set(seen) == COVERAGE, f"missing: {sorted(COVERAGE - set(seen))}; unlisted: {sorted(set(seen) - COVERAGE)}"


def test_the_echo_is_heard_and_rings_out_over_a_silent_deck():
    """conditions on the draws, checked on the model, per seed at the three real tick lengths: at least a quarter of the fed (deck, tick) pairs with the echo on
    differ in some bit from the deck's dry samples, and at least one tick of an echo-out -- the deck's PLAY flag cleared, its dry samples silent -- sounds.  (A
    deck that is silent because it ran past its track or stands before it, PLAY still set, is no echo-out.)"""
    for mode, shape_id, seed in SESSIONS:
        if shape_id not in AUDIBLE_SHAPES:
            continue
        ds, _runs = session(mode, shape_id, seed)
        pairs = [(bool(np.any(dry.view(np.uint32) != port.view(np.uint32))), bool(port.any() and not dry.any() and not playing))
                 for r in ds.runs for _n, _k, dry, port, playing in echo_ticks(ds, r)]
        heard, out = sum(a for a, _b in pairs), sum(b for _a, b in pairs)
        print(f"{mode} {shape_id} {seed}: {heard} of {len(pairs)} echo ticks differ from dry, {out} ticks of an echo-out sound")
        assert 4 * heard >= len(pairs) > 0, f"{mode} {shape_id} {seed}: the echo changes {heard} of {len(pairs)} ticks"
        assert out, f"{mode} {shape_id} {seed}: no tick of an echo-out sounds"


# the session seed that catches the fault (others may too), by the GPU test's own comparison.  Every misreading of the echo model is caught by a session draw:
# none is left to the directed cases alone
CAUGHT_BY = {"r_from_y": ("44k1", 200), "ramp_n_plus_1": ("44k1", 204), "ramp_f32": ("44k1", 213), "delay_from_tick_start": ("48k", 302),
             "pingpong_crosses_x": ("16k_1000", 501), "seek_restarts": ("48k", 306), "line_kept_off_on": ("48k", 301), "block_plus_one": ("44k1_100", 400),
             "echo_partition_identity": ("44k1", 210), "echo_clock_runs_when_left_out": ("8k_8000", 601), "echo_restart_per_feed": ("48k", 306),
             "echo_cleared_by_load": ("44k1", 200), "echo_restart_on_set_keylock": ("44k1", 210), "echo_on_host_written": ("48k", 302),
             "echo_events_late": ("48k", 309), "echo_ramp_over_feed": ("48k", 309), "echo_walk_as_one_block": ("44k1", 204)}


@pytest.mark.parametrize("fault", rd.ECHO_FAULTS)
def test_a_wrong_echo_changes_what_the_gpu_test_compares(fault):
    """Each fault is one way the device could get an echo session wrong (random_decks.ECHO_FAULTS: the echo model's misreadings and the feed's): switched into the
    EXPECTED side, it must change a port, a record, a debug count, a deck's state or its echo state on the seed named -- by the very comparison the GPU test uses,
    the draws the same."""
    shape_id, seed = CAUGHT_BY[fault]
    assert (shape_id, seed) in SEEDS
    ds, right = session("meters", shape_id, seed)
    ds_f, wrong = session("meters", shape_id, seed, fault)
    assert ds_f.drawn == ds.drawn and len(wrong) == len(right)
    d = next((d for d in (run_difference(a, b) for a, b in zip(wrong, right)) if d), None)
    print(f"{fault}: caught by {shape_id}-{seed} ({d[0] if d else None}): {d[1] if d else ''}")
    assert d, f"{fault}: {shape_id}-{seed} does not catch it"
