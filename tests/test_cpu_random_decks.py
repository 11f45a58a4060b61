"""The random deck sessions (tests/random_decks.py) on the oracle, the deck models and the restated launch plan alone: what the seeds of
tests/test_gpu_random_decks.py draw, that they cover the paths the GPU test is there for, that the decks are not trivially silent, and that each
way the device could get a session wrong (random_decks.FAULTS) changes an item that test compares."""
import hashlib

import numpy as np
import pytest

import deck_cases as dc
import deck_keylock_cases as kc
import random_decks as rd
from deck_model import ONE, T_PLAY
from mixlab_amd import abi
from random_taps import SETS, predict_fusion
from test_gpu_random_decks import SEEDS, TAP_SEEDS
from test_gpu_random_graphs import ALL_SETS_RUNS, engine_domains, n_inputs, run_full_graph

SESSIONS = [("meters", s, n) for s, n in SEEDS] + [("all", s, n) for s, n in TAP_SEEDS]
_sessions = {}


def session(mode, shape_id, seed, fault=None):
    """(the DeckSession, [{"run", "ticks", "ports", "decks", "taps"}]) of one seed: the oracle and the models alone"""
    key = (mode, seed, fault)
    if key not in _sessions:
        runs = []
        kw = {} if mode == "meters" else {"tap_sets": SETS, "n_runs": ALL_SETS_RUNS}
        ds = run_full_graph(shape_id, seed, (), abi.FLAG_EQ_EXACT, collect=runs, decks=rd.session(fault), **kw)
        runs = [r for r in runs if "decks" in r]
        if fault is not None:
            return ds, runs
        _sessions[key] = (ds, runs)
    return _sessions[key]


def feeds():
    """every run of every session that feeds a deck: (session id, the DeckSession, its record of the run)"""
    for mode, shape_id, seed in SESSIONS:
        ds, _runs = session(mode, shape_id, seed)
        for r in ds.runs:
            if r["fed"]:
                yield (mode, shape_id, seed), ds, r


def plain(r):
    return [n for n in r["fed"] if r["info"][n]["kl"] is None]


def locked(r):
    return [n for n in r["fed"] if r["info"][n]["kl"] is not None]


def test_the_seed_lists_are_the_issues():
    by_shape = {s: sum(1 for x, _n in SEEDS if x == s) for s, _n in SEEDS}
    assert by_shape["44k1"] == 6 and by_shape["48k"] == 6 and all(by_shape.get(s, 0) >= 1 for s in ("44k1_100", "16k_1000", "8k_8000"))
    assert 14 <= len(SEEDS) <= 18 and 5 <= len(TAP_SEEDS) <= 7 and set(TAP_SEEDS) <= set(SEEDS)
    assert sum(1 for s, _n in TAP_SEEDS if s in ("16k_1000", "8k_8000")) == 2


def test_the_draws_are_pinned():
    """graft, tracks, events, settings, loads and feed orders of every session"""
    h = hashlib.sha256()
    for mode, shape_id, seed in SESSIONS:
        ds, _runs = session(mode, shape_id, seed)
        h.update(repr((mode, shape_id, seed, ds.drawn)).encode())
        for d in ds.decks.values():
            h.update(d.track0.tobytes())
    assert h.hexdigest() == "2ef5300e6d44e36e2834d09db515d010238a2eabfe0fff83a51d55b416dace8f"


def test_every_run_has_the_shape_the_issue_gives_it():
    for mode, shape_id, seed in SESSIONS:
        ds, runs = session(mode, shape_id, seed)
        assert 2 <= len(ds.wires) <= 5 and all(len(w) <= 3 for w in ds.wires.values())
        assert sum(1 for d in ds.decks.values() if d.n_frames < 700) <= 1 and all(d.n_frames in rd.LENGTHS for d in ds.decks.values())
        assert all(1 <= r["ticks"] <= 6 for r in ds.runs) and any(not r["fed"] for r in ds.runs)
        assert set(ds.decks) == {n for n, (kind, _p) in enumerate(ds.ws.nodes) if kind == abi.KIND_SOURCE_STEREO}
        if mode == "all":
            assert ds.runs[ds.taps.one_tick_run]["ticks"] == 1
        order, _dom, refusal = engine_domains(ds.ws)
        assert refusal is None and predict_fusion(ds.ws, order, n_inputs)[1], f"{shape_id} {seed}: the graft left no port stored one float per frame"


def test_the_feeds_cover_mixed_blocks_and_the_kernel_choice():
    forms, shapes, phases = set(), set(), set()
    for _sid, ds, r in feeds():
        p, k = plain(r), locked(r)
        shapes |= {"two and two"} if len(p) >= 2 and len(k) >= 2 else set()
        shapes |= {"key-locked only"} if k and not p else set()
        shapes |= {"one deck"} if len(r["fed"]) == 1 else set()
        shapes |= {"shuffled"} if r["fed"] != sorted(r["fed"]) else set()
        whole, varying = set(), set()       # the plain decks with a playing tick whose phase stands / varies (mx_deck.hpp deck_phase_varies)
        for n in p:
            for t in r["info"][n]["recs"]:
                tick_forms = [dc.chunk_form(t, n0, min(dc.CHUNK, ds.spt - n0)) for n0 in range(0, ds.spt, dc.CHUNK)]
                if len(p) >= 3:
                    forms |= set(tick_forms)
                if tick_forms[0] != "zero":
                    (varying if t.dstep or t.step % ONE else whole).add(n)
        if any(a != b for a in whole for b in varying):
            phases.add("both")
        if whole and not varying:
            phases.add("whole only")
    assert forms == {"zero", "stream", "gather"}, forms
    assert shapes == {"two and two", "key-locked only", "one deck", "shuffled"}, shapes
    assert phases == {"both", "whole only"}, phases


def test_decks_come_and_go_between_the_runs():
    seen = set()
    for mode, shape_id, seed in SESSIONS:
        ds, _runs = session(mode, shape_id, seed)
        fed = [set(r["fed"]) for r in ds.runs]
        seen |= {"no decks after decks"} if any(a and not b for a, b in zip(fed, fed[1:])) else set()
        for n in ds.decks:
            f = [n in x for x in fed]
            seen |= {"fed, host-written, fed"} if any(a and not b and c for a, b, c in zip(f, f[1:], f[2:])) else set()
            loads = [r["run"] for r in ds.runs if n in r["load"]]
            seen |= {"load between feeds"} if any(any(f[:at]) and any(f[at:]) for at in loads) else set()
        for r in ds.runs:
            seen |= {what for what, _kl in r["keylock"].values()}
    assert seen == {"no decks after decks", "fed, host-written, fed", "load between feeds", "set", "change", "repeat", "clear"}, seen


def test_the_key_locked_decks_cover_clock_carry_search_and_record_growth():
    seen = set()
    for mode, shape_id, seed in SESSIONS:
        ds, _runs = session(mode, shape_id, seed)
        for n in ds.decks:
            left, most, cap = None, None, 0   # the clock a key-locked deck left a feed with; its largest feed in grains; kl_rec_'s room (mx_deck.cpp)
            for r in ds.runs:
                if n in r["keylock"]:
                    left = None
                if n not in r["fed"]:
                    left = (left[0], True) if left else None
                    continue
                i = r["info"][n]
                kl = i["kl"]
                if kl is None:
                    left = None
                    continue
                playing = bool(i["recs"][0].flags & T_PLAY)
                for g in i["grains"]:
                    seen.add("unsearched" if g.flags & 1 or kl.radius == 0 else "searched")
                if i["clock"] >= kl.hop and 0 < i["clock"] % kl.hop < kl.overlap and playing:
                    seen.add("fade across a run boundary")
                if left and left[1] and left[0] == i["clock"] and i["clock"] % kl.hop and playing:
                    seen.add("sat out mid-grain and returned")
                if mode == "all" and r["run"] == ds.taps.one_tick_run and i["grains"]:
                    seen.add("grain in the one-tick run")
                g = len(i["grains"])
                if most is not None and g > 2 * most and most > 0 and 2 + g > cap:
                    seen.add("record buffer grows")
                if 2 + g > cap:
                    cap = 2 * (2 + g)
                most = max(most or 0, g)
                left = (kc.count_feed(dict.fromkeys(kc.COUNT_KEYS, 0), kl, i["clock"], i["recs"], i["grains"], ds.spt), False)
    assert seen == {"searched", "unsearched", "fade across a run boundary", "sat out mid-grain and returned", "grain in the one-tick run",
                    "record buffer grows"}, seen


def test_every_tap_set_reads_a_deck_fed_source_port():
    seen = set()
    for shape_id, seed in TAP_SEEDS:
        ds, runs = session("all", shape_id, seed)
        assert all(ds.taps.tapped[name] & set(ds.taps.dup) for name in SETS)   # (what run_full_graph asks of the fused build at its end)
        for r, rec in zip(runs, ds.runs):
            seen |= {name for name, ports in r["taps"].items() if any(p == 0 and n in rec["fed"] for (n, p) in ports)}
    assert seen == set(SETS), f"no deck-fed source port under {sorted(set(SETS) - seen)}"


def test_deck_fed_sources_feed_every_class_of_listener():
    seen, grafted = set(), set()
    for mode, shape_id, seed in SESSIONS:
        ds, _runs = session(mode, shape_id, seed)
        fed = {n for r in ds.runs for n in r["fed"]}
        for n in fed:
            listeners = [ds.ws.nodes[d][0] for (d, _dp), src in ds.ws._conn.items() if src == (n, 0)]
            seen |= {rd.SLOT_CLASS.get(k, "other") for k in listeners} | ({"nobody"} if not listeners else set())
        for n, wires in ds.wires.items():
            if n in fed:
                grafted |= {rd.SLOT_CLASS[ds.ws.nodes[d][0]] for d, _dp in wires} | ({"nobody"} if not wires else set())
    want = {"mixer", "amp_split", "fir_resample", "output_device", "nobody"}
    assert want <= seen and want <= grafted, (seen, grafted)


def test_the_decks_are_not_trivially_silent():
    """conditions on the draws, checked on the model: per seed at least half of the fed (deck, tick) pairs hold a non-zero sample, and per seed
    with a key-locked deck at 44.1 / 48 kHz a searched grain was moved"""
    for mode, shape_id, seed in SESSIONS:
        ds, _runs = session(mode, shape_id, seed)
        pairs = [bool(np.any(x)) for r in ds.runs for n in r["fed"] for x in np.asarray(r["samples"][n]).reshape(r["ticks"], -1)]
        assert 2 * sum(pairs) >= len(pairs) > 0, f"{mode} {shape_id} {seed}: {sum(pairs)} of {len(pairs)} fed ticks are not silent"
        if shape_id in ("44k1", "48k") and any(locked(r) for r in ds.runs):
            moved = [g for r in ds.runs for n in locked(r) for g in r["info"][n]["grains"] if not g.flags & 1 and r["info"][n]["kl"].radius and g.delta]
            assert moved, f"{mode} {shape_id} {seed}: no searched grain with a delta"


def run_difference(a, b):
    """what the GPU test compares per run and build, between two expected sides: None or (item, line)"""
    for pt in b["ports"]:
        if a["ports"][pt] != b["ports"][pt]:
            return "port", f"port {pt} differs"
    return rd.difference(a["decks"], b["decks"])


@pytest.mark.parametrize("fault", rd.FAULTS)
def test_a_wrong_deck_feed_changes_what_the_gpu_test_compares(fault):
    """Each fault is one way the device could get a session wrong (random_decks.FAULTS): switched into the EXPECTED side, it must change a port,
    a tick or grain record, a debug count or a deck's state on one of the seeds -- by the very comparison the GPU test uses, the draws the same."""
    caught = []
    for shape_id, seed in SEEDS:
        ds, right = session("meters", shape_id, seed)
        ds_f, wrong = session("meters", shape_id, seed, fault)
        assert ds_f.drawn == ds.drawn and len(wrong) == len(right)
        d = next((d for d in (run_difference(a, b) for a, b in zip(wrong, right)) if d), None)
        if d:
            caught.append((shape_id, seed, d[0]))
    print(f"{fault}: caught by " + ", ".join(f"{s}-{n} ({item})" for s, n, item in caught))
    assert caught, f"{fault}: no seed catches it"
