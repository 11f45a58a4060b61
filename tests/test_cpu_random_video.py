"""The random video graphs without a device (tests/random_video.py): what is drawn is pinned, what the seed set covers is asserted, every run has something to
see, every FAULT switched into the model changes a compared item on named seeds, and the model agrees with itself under both groupings of the ticks."""
import functools

import pytest

import random_video as rv

# the seeds of both suites.  Chosen for the something-to-see condition below (seeds whose graphs mostly show None were replaced, not excused)
SEEDS = (1, 2, 3, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 17, 19, 20)
DIGEST = "1dfe530c552858f58cfa728cb180d871abb55b5ff4ce75db36d8bb0eeb594610"


@functools.lru_cache(maxsize=None)
def scenario_of(seed):
    return rv.scenario(seed)


@functools.lru_cache(maxsize=None)
def expected(seed, kind, fault=None):
    sc = scenario_of(seed)
    return rv.expect(sc, rv.groupings(sc, kind), fault)


def coverage(seed):
    """the coverage items scenario `seed` has, by name"""
    sc, runs = scenario_of(seed), expected(seed, "batched")
    n_src = sc["n_sources"]
    have = set()
    for s, d in enumerate(sc["sources"]):
        have.add("feeder " + d["feeder"])
        have.add("transform " + d["transform"])
        have.add("nv12 source" if d["nv12"] else "planar source")
        if d.get("two_sizes") and any(e["op"] == "place" and e["src"] == s and e["params"] and e["params"]["crop_w"] == 0 for evs in sc["events"].values() for e in evs):
            have.add("whole-frame place on a ring of two sizes")
        if any(r["n"] >= 2 and r["ports"][(s, 0)] is not None for r in runs):
            have.add("multi-tick run of a " + d["feeder"])
    uses = {}
    for m in sc["mixers"]:
        for ref in m["inputs"]:
            if ref is not None:
                uses[tuple(ref)] = uses.get(tuple(ref), 0) + 1
                have.add("input from " + ("a source" if ref[0] < n_src else ("a program", "an A port", "a B port")[ref[1]]))
        have.add("a mixer with an unconnected input" if None in m["inputs"] else "a mixer with four inputs")
    for s in sc["sinks"] + ([sc["monitor"]] if sc["monitor"] else []):
        uses[(s["mixer"] + n_src, 0)] = uses.get((s["mixer"] + n_src, 0), 0) + 1
    if max(uses.values()) >= 2:
        have.add("fan-out")
    faders = [m["params"]["fader"] for m in sc["mixers"]] + [u["params"]["fader"] for us in sc["mixer_updates"].values() for u in us]
    have |= {f"fader {f}" for f in faders if f in (0.0, 1.0)}
    if sc["events"][sc["one_tick_run"] + 1] and (sc["one_tick_run"], 1) in [(r["start"], r["n"]) for r in runs]:
        have.add("re-set after a one-tick run")
    if sc["first_tick"]:
        have.add("ticks past 2^33 samples")
    for r in runs:
        i = r["info"]
        have |= {name for name, n in (("scope on a symbolic program", i["scope_symbolic"]), ("multiview of a symbolic program", i["mv_symbolic"]), ("scope on None", i["scope_none"]),
                                      ("scope on nv12", i["scope_nv12"]), ("multiview of nv12", i["mv_nv12"]), ("size change on a sink's input inside a run", i["sink_size_change"])) if n}
        if (r["scopes"] is not None and not r["scopes"]["records"]) or (r["mv"] is not None and not r["mv"]["n_recorded"]):
            have.add("a run that records no tick")
        if r["mv"] is not None and r["mv"]["n_recorded"] >= 2:
            have.add("a run with two recorded multiview ticks")
    return have


WANTED = (["feeder " + f for f in rv.FEEDERS] + ["transform " + t for t in rv.TRANSFORMS] + ["multi-tick run of a " + f for f in ("ring", "repeat", "queue")] +
          ["input from a source", "input from a program", "input from an A port", "input from a B port", "a mixer with an unconnected input", "fan-out", "fader 0.0", "fader 1.0",
           "nv12 source", "whole-frame place on a ring of two sizes", "re-set after a one-tick run", "ticks past 2^33 samples", "scope on a symbolic program",
           "multiview of a symbolic program", "scope on None", "scope on nv12", "multiview of nv12", "size change on a sink's input inside a run", "a run that records no tick",
           "a run with two recorded multiview ticks"])


def test_the_scenarios_are_the_pinned_ones():
    assert len(SEEDS) >= 16
    got = rv.digest([rv.scenario(s) for s in SEEDS])
    print(got)
    assert got == DIGEST
    assert rv.digest([rv.scenario(s) for s in SEEDS]) == got, "a scenario depends on more than its seed"


def test_the_seed_set_covers_what_the_issue_lists():
    where = {}
    for seed in SEEDS:
        for item in coverage(seed):
            where.setdefault(item, []).append(seed)
    for item in WANTED:
        print(f"{item}: seeds {where.get(item, [])}")
    assert not [item for item in WANTED if item not in where]


@pytest.mark.parametrize("seed", SEEDS)
def test_every_seed_has_something_to_see(seed):
    """at least half of the compared ports at run ends hold a picture; a scope set yields a counted record; a multiview set yields a canvas that shows something"""
    runs = expected(seed, "batched")
    ports = [v for r in runs for v in r["ports"].values()]
    held = sum(v is not None for v in ports)
    print(f"seed {seed}: {held} of {len(ports)} ports hold a picture")
    assert 2 * held >= len(ports)
    if any(r["scopes"] is not None for r in runs):
        assert any(rec["counted"] == 1 for r in runs if r["scopes"] for row in r["scopes"]["records"] for rec in row)
    if any(r["mv"] is not None for r in runs):
        assert any(r["mv"]["status"][3] for r in runs if r["mv"])


# fault -> the seeds that catch it (each changes a compared item there; found by trying every seed of SEEDS, kept as the named ones)
CAUGHT_ON = {"scope_c_per_run": (2, 3, 5), "mv_uses_scope_counter": (3, 5, 6), "set_does_not_reset_c": (5, 6, 8), "mv_first_recorded_tick": (1, 3, 7),
             "place_before_key": (1, 2, 3), "stale_after_reset": (1, 2, 3), "removed_transform_stays": (1, 2, 3), "tap_sees_raw_source": (1, 3, 6),
             "ab_ignore_update": (1, 3, 5), "ring_restarts_per_run": (1, 2, 3), "ring_beats_queue": (1, 5, 6), "no_expiry": (1, 5, 8, 14),
             "mv_honours_coverage": (1, 2, 3), "sink_shows_previous_tick": (3, 5, 7)}


@pytest.mark.parametrize("fault", rv.FAULTS)
def test_a_wrong_video_host_changes_what_is_compared(fault):
    """Each fault is one way the engine could be wrong that the GPU suite exists to notice: switched into the EXPECTED side, at least one compared item must
    differ from the right expectations on every named seed -- by the very items the GPU test compares.  The draws are the same with and without it."""
    assert len(CAUGHT_ON[fault]) >= 2 and set(CAUGHT_ON[fault]) <= set(SEEDS)
    for seed in CAUGHT_ON[fault]:
        kind = "batched"
        diff = rv.differences(expected(seed, kind, fault), expected(seed, kind))
        print(f"{fault}: seed {seed}: {len(diff)} items differ, first {diff[:3]}")
        assert diff, f"{fault} changes nothing that is compared on seed {seed}"


@pytest.mark.parametrize("seed", SEEDS)
def test_single_and_batched_groupings_agree_where_both_observe(seed):
    """The scenario is defined per absolute tick: at every run end the two groupings share, the ports and the sinks are the same, and the scope records of the
    whole scenario, in tick order, are the same (a record's tick_in_run is its run's; the absolute tick is compared)."""
    single, batched = expected(seed, "single"), expected(seed, "batched")
    by_end = {r["start"] + r["n"]: r for r in single}
    for r in batched:
        s = by_end[r["start"] + r["n"]]
        assert [p for p in r["ports"] if not rv.same_pic(r["ports"][p], s["ports"][p])] == [], f"run ending at tick {r['start'] + r['n']}"
        assert all(rv.same_planes(None if r["sinks"][k] is None else [r["sinks"][k]], None if s["sinks"][k] is None else [s["sinks"][k]]) for k in r["sinks"])

    def stream(runs):
        out = []
        for r in runs:
            for row in (r["scopes"]["records"] if r["scopes"] else []):
                out.append((r["start"] + row[0]["tick_in_run"], [dict(rec, tick_in_run=0) for rec in row]))
        return out
    a, b = stream(single), stream(batched)
    assert [t for t, _ in a] == [t for t, _ in b]
    assert all(len(x) == len(y) and all(rv.sm.same(p, q) for p, q in zip(x, y)) for (_, x), (_, y) in zip(a, b))
    # and the Monitor's ticks, all of them
    if single[0]["monitor"] is not None:
        ma, mb = [t for r in single for t in r["monitor"]], [t for r in batched for t in r["monitor"]]
        assert len(ma) == len(mb) and all(rv.same_monitor_tick(x, y) for x, y in zip(ma, mb))
