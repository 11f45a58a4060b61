"""The chain family of the random video graphs without a device (random_video.scenario(seed, chain=True)): sources whose transform is a drawn subset of GRADE, KEY,
MATTE, PLACE, set in a drawn call order and set again, removed and put back at run boundaries, over rings that mix yuv420p and yuva420p frames.  What is drawn is
pinned, what the seed set covers is asserted by name, every seed has something to see (and a chain that is not the identity), every drawn setting is one the library
accepts, every fault of random_video.CHAIN_FAULTS -- and the four older ones that meet the new ops -- changes a compared item on named seeds, and the model agrees
with itself under both groupings of the ticks."""
import functools

import numpy as np
import pytest

import random_video as rv
import video_grade_model as gm
import video_matte_model as mt
from mixlab_amd import video

# the seeds of both chain suites.  Chosen for the coverage list and the something-to-see conditions below (seeds that failed either were replaced, not excused)
CHAIN_SEEDS = (1, 3, 4, 7, 8, 15, 17, 21, 23, 26, 31, 36, 41, 46)
CHAIN_DIGEST = "3efe49e2659ad0a3a2f344beaa6f4aae15fbf2aaf8b6486ffb99def6dee586a9"
STAGE_OPS = set(rv.STAGES)


@functools.lru_cache(maxsize=None)
def scenario_of(seed):
    return rv.scenario(seed, chain=True)


@functools.lru_cache(maxsize=None)
def expected(seed, kind, fault=None):
    sc = scenario_of(seed)
    return rv.expect(sc, rv.groupings(sc, kind), fault)


def chain_sources(sc):
    return [s for s, d in enumerate(sc["sources"]) if d.get("stages")]


def grade_abi(par):
    """the library's parameters of a drawn grade setting (the lattice goes separately: random_video.grade_p(par).nodes)"""
    return video.GradeParams(par["flags"], gm.gamma_curve(*par["curve"]), par["m"], par["off"])


def matte_abi(par):
    """the library's parameters of a drawn matte setting; a wipe goes through the library's own helper, so that it and the model's wipe() meet"""
    if "wipe" in par:
        return video.matte_wipe(*par["wipe"])
    return video.MatteParams(clean=par["clean"], choke=par["choke"], soften=par["soften"], mask=par["mask"], invert=bool(par["invert"]), feather_q4=par["feather"],
                             shape=par["shape"])


def stage_events(sc, s):
    """[(boundary, op, params, what, the stage's params before, the stages on after)] of source s's stage setters in the order they are applied; what: "set" (the
    stage was off), "re-set" or "remove"; the stages on are in the chain's order"""
    on, out = {}, []
    for b, evs in sc["events"].items():
        for e in evs:
            if e.get("src") == s and e["op"] in STAGE_OPS:
                prev = on.get(e["op"])
                what = "remove" if e["params"] is None else ("re-set" if prev is not None else "set")
                on[e["op"]] = e["params"]
                out.append((b, e["op"], e["params"], what, prev, [op for op in rv.STAGES if on.get(op) is not None]))
    return out


def coverage(seed):
    """the coverage items chain scenario `seed` has, by name"""
    sc, runs = scenario_of(seed), expected(seed, "batched")
    have = set()
    for s in chain_sources(sc):
        d = sc["sources"][s]
        if d["order"] != d["stages"]:
            have.add("a setter call order other than the chain's")
        rings = [e for evs in sc["events"].values() for e in evs if e["op"] == "ring" and e["src"] == s]
        if "grade" in d["stages"] and any(len({sc["frames"][f]["alpha"] for f in e["frames"]}) == 2 for e in rings):
            have.add("a ring that mixes frames with and without coverage on a graded source")
        if d["two_sizes"] and ("grade" in d["stages"] or "matte" in d["stages"]) and any(len({sc["frames"][f]["w"] for f in e["frames"]}) == 2 for e in rings):
            have.add("a ring of two sizes under grade or matte")
        if any(r["n"] >= 2 and r["ports"][(s, 0)] is not None for r in runs) and d["feeder"] in ("ring", "repeat", "queue"):
            have.add("multi-tick run of a " + d["feeder"] + " on a chain source")
        removed = set()
        for b, op, par, what, prev, after in stage_events(sc, s):
            later_on = [o for o in after if rv.STAGES.index(o) > rv.STAGES.index(op)]
            earlier_on = [o for o in after if rv.STAGES.index(o) < rv.STAGES.index(op)]
            if what == "re-set" and later_on:
                have.add("a re-set of a stage that is not the last while a later one is on")
            if what == "remove":
                removed.add(op)
                if later_on and earlier_on:
                    have.add("removal of a middle stage")
            if what == "set" and op in removed:
                have.add("a stage put back")
            if b == sc["one_tick_run"] + 1 and what == "re-set":
                have.add("the re-set after the one-tick run on a chain stage")
                if later_on:
                    have.add("the re-set after the one-tick run on a stage that is not the last")
            if op == "grade" and par is not None and par["flags"] & gm.LUT:
                have.add(f"lattice {(1 << par['k']) + 1}")
                if what == "re-set" and prev["flags"] & gm.LUT and (prev["k"], prev["lattice"]) != (par["k"], par["lattice"]):
                    have.add("a LUT re-set")
            if op == "matte" and par is not None:
                p = rv.matte_p(par)
                if "wipe" in par:
                    have.add("a wipe")
                elif p.mask is not None:
                    have.add("a circle mask" if p.shape == mt.CIRCLE else "a rectangle mask")
                if p.choke:
                    have.add("choke that shrinks" if p.choke > 0 else "choke that grows")
                if p.soften >= 1:
                    have.add("soften")
    if sc["first_tick"]:
        have.add("ticks past 2^33 samples")
    for r in runs:
        i = r["info"]
        for sub in i["subsets"]:
            have.add("stages " + sub)
        have |= {name for name, n in (("matte without key on a yuva420p frame", i["matte_no_key_on_coverage"]), ("a scope tap on a chain source's port", i["scope_chain"]),
                                      ("a multiview view of a chain source's port", i["mv_chain"]), ("a chain source feeding a symbolic program", i["chain_into_program"])) if n}
    return have


ALONE = ["stages " + op for op in rv.STAGES]
WANTED = (ALONE + ["stages grade+key+matte+place", "stages grade+place", "stages key+matte", "matte without key on a yuva420p frame",
                   "a setter call order other than the chain's", "a re-set of a stage that is not the last while a later one is on", "removal of a middle stage",
                   "a stage put back", "the re-set after the one-tick run on a chain stage", "the re-set after the one-tick run on a stage that is not the last",
                   "a ring that mixes frames with and without coverage on a graded source", "a ring of two sizes under grade or matte", "lattice 17", "lattice 33",
                   "a LUT re-set", "a rectangle mask", "a circle mask", "choke that shrinks", "choke that grows", "soften", "a wipe", "a scope tap on a chain source's port",
                   "a multiview view of a chain source's port", "a chain source feeding a symbolic program", "ticks past 2^33 samples"] +
          [f"multi-tick run of a {f} on a chain source" for f in ("ring", "repeat", "queue")])


def test_the_chain_scenarios_are_the_pinned_ones():
    assert len(CHAIN_SEEDS) >= 12
    got = rv.digest([rv.scenario(s, chain=True) for s in CHAIN_SEEDS])
    print(got)
    assert got == CHAIN_DIGEST
    assert rv.digest([rv.scenario(s, chain=True) for s in CHAIN_SEEDS]) == got, "a scenario depends on more than its seed"
    assert all(rv.scenario(s, chain=True) != rv.scenario(s) for s in CHAIN_SEEDS), "the chain family draws from an RNG base of its own"


def test_the_chain_seed_set_covers_what_the_issue_lists():
    where = {}
    for seed in CHAIN_SEEDS:
        for item in coverage(seed):
            where.setdefault(item, []).append(seed)
    for item in WANTED:
        print(f"{item}: seeds {where.get(item, [])}")
    assert not [item for item in WANTED if item not in where]
    subsets = sorted(item for item in where if item.startswith("stages "))
    print(f"{len(subsets)} of the 15 subsets: {subsets}")
    assert len(subsets) >= 8
    for seed in CHAIN_SEEDS:        # what the generator promises of every chain scenario
        sc = scenario_of(seed)
        for s, d in enumerate(sc["sources"]):
            banded = any(e["op"] == "band" and e["src"] == s for evs in sc["events"].values() for e in evs)
            assert not (banded and d.get("stages")), "a grade or a matte is never drawn together with a row band"
            if d.get("stages"):
                assert sorted(d["order"]) == sorted(d["stages"]) and [e["op"] for e in sc["events"][0] if e.get("src") == s and e["op"] in STAGE_OPS] == d["order"]
                mine = [e for evs in sc["events"].values() for e in evs if e.get("src") == s and e["op"] in ("ring", "repeat", "shot", "queue")]
                ids = [f for e in mine for f in ([e["frame"]] if "frame" in e else list(e.get("frames", ())) + [q["frame"] for q in e.get("entries", ())])]
                assert {sc["frames"][f]["fmt"] for f in ids} == {0}, "a chain source's frames are yuv420p or yuva420p"
                if "grade" in d["stages"] or "matte" in d["stages"]:
                    assert all({sc["frames"][f]["alpha"] for f in e["frames"]} == {True, False} for e in mine if e["op"] == "ring"), "every ring mixes both formats"


@pytest.mark.parametrize("seed", CHAIN_SEEDS)
def test_every_chain_seed_has_something_to_see(seed):
    """At least half of the compared ports at run ends hold a picture; a scope set yields a counted record; a multiview set yields a canvas that shows something;
    and at least half of the run-end pictures on chain sources' ports differ from the raw frame that was delivered: a chain of identities tests nothing."""
    sc, runs = scenario_of(seed), expected(seed, "batched")
    ports = [v for r in runs for v in r["ports"].values()]
    held = sum(v is not None for v in ports)
    print(f"seed {seed}: {held} of {len(ports)} ports hold a picture")
    assert 2 * held >= len(ports)
    if any(r["scopes"] is not None for r in runs):
        assert any(rec["counted"] == 1 for r in runs if r["scopes"] for row in r["scopes"]["records"] for rec in row)
    if any(r["mv"] is not None for r in runs):
        assert any(r["mv"]["status"][3] for r in runs if r["mv"])
    assert chain_sources(sc), "no source with a chain"
    pairs = [(r["ports"][(s, 0)], r["raw"][(s, 0)]) for r in runs for s in chain_sources(sc) if r["ports"][(s, 0)] is not None]
    changed = sum(not got.same(raw) for got, raw in pairs)
    pixels = sum(not got.same(raw) and not ((got.w, got.h) == (raw.w, raw.h) and all(np.array_equal(x, y) for x, y in zip(got.planes, raw.planes))
                                            and (got.a is None or bool((got.a == (255 if raw.a is None else raw.a)).all()))) for got, raw in pairs)
    print(f"seed {seed}: {changed} of {len(pairs)} pictures on chain sources' ports differ from the raw frame ({pixels} in more than the presence of a coverage plane)")
    assert pairs and 2 * changed >= len(pairs) and 2 * pixels >= len(pairs)


@pytest.mark.parametrize("seed", CHAIN_SEEDS)
def test_every_drawn_setting_is_one_the_library_takes(seed):
    """every matte setting passes mx_video_matte_check (a wipe: the library's helper gives the fields the model's wipe() gives); the library exports no check of a
    grade setting, so the header's ranges are asserted: flag bits of the three, |m| <= 32767, |off| <= 255 * 4096, a lattice of 17 or 33 nodes with values <= 4096
    exactly where the LUT bit is set"""
    sc = scenario_of(seed)
    n = 0
    for evs in sc["events"].values():
        for e in evs:
            par = e.get("params")
            if e["op"] == "matte" and par is not None:
                c = matte_abi(par)
                video.matte_check(c)
                p = rv.matte_p(par)
                assert c.flags == p.flags and (c.clean_black, c.clean_white) == (p.clean or (0, 0)) and (c.choke, c.soften) == (p.choke, p.soften)
                assert p.mask is None or ((c.mask_x0, c.mask_y0, c.mask_x1, c.mask_y1) == tuple(p.mask) and (c.mask_shape, c.mask_invert, c.mask_feather_q4) == (p.shape, p.invert, p.feather))
                assert -6 <= p.choke <= 6 and 0 <= p.soften <= 6
                n += 1
            elif e["op"] == "grade" and par is not None:
                assert 1 <= par["flags"] <= 7 and all(abs(x) <= 32767 for x in par["m"]) and all(abs(x) <= 255 * 4096 for x in par["off"])
                assert 0 < par["curve"][0] and par["curve"][1] < par["curve"][2]
                p = rv.grade_p(par)
                assert (p.nodes is not None) == bool(par["flags"] & gm.LUT)
                if p.nodes is not None:
                    assert par["k"] in (4, 5) and p.nodes.shape == ((1 << par["k"]) + 1,) * 3 + (3,) and p.nodes.dtype == np.uint16 and int(p.nodes.max()) <= 4096
                c = grade_abi(par)
                assert c.flags == par["flags"] and bytes(c.curve_y) == gm.gamma_curve(*par["curve"]).tobytes()
                n += 1
    assert n


# fault -> the seeds that catch it (each changes a compared item there; found by trying every seed of CHAIN_SEEDS, kept as the named ones)
CAUGHT_ON = {"matte_before_key": (3, 4, 7), "grade_after_key": (1, 3, 4), "grade_drops_coverage": (1, 3, 4), "matte_ignores_coverage": (3, 8, 15),
             "old_lattice_after_reset": (1, 8, 21), "stale_after_reset": (1, 3, 4), "removed_transform_stays": (1, 3, 4), "place_before_key": (1, 3, 4),
             "tap_sees_raw_source": (1, 3, 4)}
# the seeds of CAUGHT_ON["stale_after_reset"] on which the picture that stays is one a LATER stage's list would hold: the stage set again is not the last one on
STALE_BEHIND_A_LATER_STAGE = (1, 3, 4)
FAULTS = rv.CHAIN_FAULTS + ("stale_after_reset", "removed_transform_stays", "place_before_key", "tap_sees_raw_source")


def stale_runs_behind_a_later_stage(seed):
    """indices of the runs of the batched grouping in which a chain source shows a stage that was set again while a later stage was on (until the source's next
    setter), with the source"""
    sc, runs = scenario_of(seed), expected(seed, "batched")
    out = []
    for s in chain_sources(sc):
        evs = stage_events(sc, s)
        for k, (b, op, par, what, _prev, after) in enumerate(evs):
            if what == "re-set" and any(rv.STAGES.index(o) > rv.STAGES.index(op) for o in after):
                end = min([x[0] for x in evs[k + 1:] if x[0] > b] + [sc["n_ticks"]])
                out += [(i, s) for i, r in enumerate(runs) if b <= r["start"] < end]
    return out


@pytest.mark.parametrize("fault", FAULTS)
def test_a_wrong_source_transform_changes_what_is_compared(fault):
    """Each fault is one way the engine's SourceTransform could be wrong that the GPU suite exists to notice: switched into the EXPECTED side, at least one compared
    item must differ from the right expectations on every named seed -- by the very items the GPU test compares.  The draws are the same with and without it."""
    assert len(CAUGHT_ON[fault]) >= 2 and set(CAUGHT_ON[fault]) <= set(CHAIN_SEEDS)
    for seed in CAUGHT_ON[fault]:
        diff = rv.differences(expected(seed, "batched", fault), expected(seed, "batched"))
        print(f"{fault}: seed {seed}: {len(diff)} items differ, first {diff[:3]}")
        assert diff, f"{fault} changes nothing that is compared on seed {seed}"
    if fault == "stale_after_reset":
        assert STALE_BEHIND_A_LATER_STAGE and set(STALE_BEHIND_A_LATER_STAGE) <= set(CAUGHT_ON[fault])
        for seed in STALE_BEHIND_A_LATER_STAGE:
            diff = rv.differences(expected(seed, "batched", fault), expected(seed, "batched"))
            hit = [(i, s) for i, s in stale_runs_behind_a_later_stage(seed) if (i, f"port ({s}, 0)") in diff]
            print(f"{fault}: seed {seed}: the source's port differs in runs {hit} that follow a re-set of a stage that is not the last")
            assert hit


@pytest.mark.parametrize("seed", CHAIN_SEEDS)
def test_single_and_batched_groupings_agree_where_both_observe(seed):
    """as in test_cpu_random_video: the ports and the sinks at every run end the two groupings share, the scope records in tick order, the Monitor's ticks"""
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
    if single[0]["monitor"] is not None:
        ma, mb = [t for r in single for t in r["monitor"]], [t for r in batched for t in r["monitor"]]
        assert len(ma) == len(mb) and all(rv.same_monitor_tick(x, y) for x, y in zip(ma, mb))
