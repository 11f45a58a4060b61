"""Random deck sessions on the full random graphs (tests/test_gpu_random_graphs.py run_full_graph(decks=...)), shared by the GPU test
(tests/test_gpu_random_decks.py) and its CPU proof (tests/test_cpu_random_decks.py): further SOURCE_STEREO nodes grafted into the graph, a deck
(DESIGN.md section 0.15), plain or key-locked (0.16), on every stereo source, and a session of feeds, events, set_keylock calls and loads
over run_full_graph's runs.  The expected side is one KeylockModel per deck (tests/deck_keylock_model.py: the plain model while key-lock is
off) whose samples go into the oracle's source; everything downstream is what run_full_graph compares anyway.

Everything here is drawn from a stream of its own (default_rng(9000 + seed)): the graph generator's stream, run_full_graph's (7000 + seed) and
random_taps' (8000 + seed) draw what they always drew.  Nothing here needs a GPU but the device side of DeckSession, which takes built graphs.

`fault` makes the EXPECTED side wrong in one way the device could be (FAULTS); the CPU test shows that each changes an item the GPU test
compares.  The draws are the same with and without a fault: what is drawn never looks at a model."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import deck_cases as dc
import deck_keylock_cases as kc
import deck_keylock_model as km
import deck_model as dm
from deck_keylock_model import Keylock
from deck_model import ONE
from mixlab_amd import abi, deck
from test_gpu_random_graphs import drop_refused_edges, engine_domains, resample_ratio

STEREO = 2
FAULTS = ("other_parity", "sorted_nodes", "plain_first", "stale_source", "advances_when_left_out", "restart_per_feed", "no_restart_after_pause",
          "clock_lost_when_left_out", "ticked_events_late")
LENGTHS = (1, 31, 33, 700, 4097, 6000)
KINDS = ("noise", "music", "period 16")
# hop 256 / 512 / 1024, overlap 16 .. 256, radius 0 / 5 / 300, pitch at unity, at 44.1 in 48 and just above the first bank edge
SETTINGS = (Keylock(ONE, 256, 64, 5), Keylock(kc.STEP_441, 512, 16, 300), Keylock(ONE, 1024, 256, 300), Keylock(dc.EDGE1 + 1, 256, 32, 5),
            Keylock(ONE, 512, 128, 0), Keylock(kc.STEP_441, 256, 128, 300))
SLOT_CLASS = {abi.KIND_MIXER: "mixer", abi.KIND_AMPLIFIER: "amp_split", abi.KIND_STEREO_SPLITTER: "amp_split", abi.KIND_FIR: "fir_resample",
              abi.KIND_RESAMPLE: "fir_resample", abi.KIND_OUTPUT_DEVICE: "output_device", abi.KIND_PLOTTER: "plotter"}
FEED_KEYS = ("ticks_zero", "ticks_stream", "ticks_gather", "chunks_zero", "chunks_stream", "chunks_gather")

_tables = []


def tables():
    if not _tables:
        _tables.append(np.stack([deck.deck_tables(b) for b in range(4)]))
    return _tables[0]


def session(fault=None):
    """what run_full_graph(decks=...) takes"""
    return functools.partial(DeckSession, fault=fault)


def c_params(p):
    return deck.params(p.step, p.slew, p.loop_in, p.loop_out, p.flags)


def tick_tuple(t):
    return (t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank)


def head_tuple(h):
    """an abi.DeckHead"""
    p = h.params
    return (h.pos_q32, h.step_q32, p.step_q32, p.slew_q32, p.loop_in, p.loop_out, p.flags, h.last_loop_in, h.last_loop_out, h.last_looping)


def model_head_tuple(h):
    p = h.params
    return (h.pos, h.step, p.step, p.slew, p.loop_in, p.loop_out, p.flags, h.last_loop_in, h.last_loop_out, 1 if h.last_looping else 0)


def graft(rng, ws):
    """2-5 further SOURCE_STEREO nodes, each wired into 0-3 STEREO inputs of modules whose input lives in the base domain: a class of module is
    drawn first (Mixer; Amplifier or Splitter; Fir or Resample; OutputDevice; Plotter), then an unconnected input of it, else a connected one
    is rewired -- never one fed by a Panner or an Amplifier (the first strip stays whole: its Amplifier's port is the one the fused build stores
    one float per frame) or by a source.
    Where a rewired edge changes the run order so that the engine would refuse the graph, edges are dropped as _full_graph drops them.
    -> {new source: [(module, input)] it feeds}"""
    order, dom, bad = engine_domains(ws)
    assert bad is None
    slots = {}
    for n in order:
        kind, params = ws.nodes[n]
        cls = SLOT_CLASS.get(kind)
        if cls is None or (dom[n] / resample_ratio(params) if kind == abi.KIND_RESAMPLE else dom[n]) != 1:
            continue
        for p in (range(len(params)) if kind == abi.KIND_MIXER else (0,)):
            slots.setdefault(cls, []).append((n, p))
    fixed = (abi.KIND_AMPLIFIER, abi.KIND_STEREO_PANNER, abi.KIND_SOURCE_STEREO, abi.KIND_SOURCE_MONO)
    new = [ws.source_stereo() for _ in range(int(rng.integers(2, 6)))]
    for s in new:
        for _ in range(int(rng.integers(0, 4))):
            names = sorted(c for c in slots if slots[c])
            if not names:
                break
            pool = slots[names[int(rng.integers(0, len(names)))]]
            cand = [x for x in pool if x not in ws._conn] or [x for x in pool if ws.nodes[ws._conn[x][0]][0] not in fixed]
            if cand:
                d = cand[int(rng.integers(0, len(cand)))]
                ws.connect(s, 0, *d)
                pool.remove(d)
    drop_refused_edges(ws, dict(dom))
    return {s: sorted(d for d, src in ws._conn.items() if src == (s, 0)) for s in new}


def difference(got, want):
    """None where one run's deck records equal `want`, else (item, a line on the first difference).  got / want: {"decks": {node: {"ticks", "grains",
    "state"}}, "feed_counts", "keylock_counts"}; a deck that was not fed has ticks and grains None"""
    for node, w in want["decks"].items():
        g = got["decks"][node]
        for item in ("ticks", "grains", "state"):
            if g[item] != w[item]:
                k = next((i for i, (a, b) in enumerate(zip(g[item], w[item])) if a != b), None) if g[item] is not None and w[item] is not None else None
                where = f" first at {k}: got {g[item][k]}, want {w[item][k]}" if k is not None else f" got {g[item]}, want {w[item]}"
                return item, f"deck on node {node}: {item} differ:{where}"
    for item in ("feed_counts", "keylock_counts"):
        if got[item] != want[item]:
            return item, f"{item}: got {got[item]}, want {want[item]}"
    return None


class Deck:
    """one deck of a session: its node, track, model and what the draws need to know of it"""

    def __init__(self, node, track, kind, kl, fault):
        self.node, self.n_frames, self.kind = node, len(track), kind
        self.track0 = track
        mis = (fault,) if fault in km.MISREADINGS else ()
        self.model = km.KeylockModel(track.copy(), tables(), mis)
        self.kl = kl                      # the setting now in force (None: plain)
        self.clock = 0                    # the grain clock as the header walks it (kc.count_feed), for the debug counts
        self.loop, self.started = None, False
        self.head = dm.Head()             # the head as the draws see it: never a faulty one
        self.was_fed, self.sat_out = False, False
        self.last = None                  # the samples of its last feed
        self.late = None                  # ticked_events_late: the event pushed out of the last run
        if kl is not None:
            self.model.set_keylock(kl)


class DeckSession:
    def __init__(self, seed, ws, sources, shape, fault=None):
        assert fault is None or fault in FAULTS
        self.rng = rng = np.random.default_rng(9000 + seed)
        self.seed, self.ws, self.spt, self.fault = seed, ws, ws.spt, fault
        self.wires = graft(rng, ws)
        sources += [(s, STEREO) for s in self.wires]
        self.nodes = [n for (n, ty) in sources if ty == STEREO]
        self.decks, short = {}, False
        for n in self.nodes:
            n_frames = LENGTHS[int(rng.integers(0, len(LENGTHS)))]
            if n_frames < 700 and short:          # one short track a graph at the most
                n_frames = LENGTHS[int(rng.integers(3, len(LENGTHS)))]
            short |= n_frames < 700
            kind = KINDS[int(rng.integers(0, len(KINDS)))]
            kl = SETTINGS[int(rng.integers(0, len(SETTINGS)))] if rng.random() < 0.5 else None
            self.decks[n] = Deck(n, kc.track(kind, n_frames, f"random decks {seed} node {n}"), kind, kl, fault)
        self.drawn = [("graft", sorted(self.wires.items())), ("decks", [(n, d.n_frames, d.kind, d.kl) for n, d in self.decks.items()])]
        self.dev, self.got, self.runs = {}, {}, []
        self.plan = self.want = None

    # ---- the draws ------------------------------------------------------------------------------------------------------------------
    def start(self, n_runs, graphs):
        """one run (not the first) feeds no deck; every build gets Deck objects of its own"""
        self.no_deck_run = int(self.rng.integers(1, n_runs))
        self.drawn.append(("no_deck_run", self.no_deck_run))
        for name in graphs:
            self.dev[name] = {}
            for n, d in self.decks.items():
                h = self.dev[name][n] = deck.Deck(d.n_frames)
                h.load(d.track0)
                if d.kl is not None:
                    h.set_keylock(deck.keylock(*d.kl))

    def before_run(self, run, L):
        """draws the run: per deck a set_keylock call and a load between the runs, whether it is fed, its events tick by tick; the order of the
        feed call.  The calls go to the models and to every build's decks here."""
        rng, spt = self.rng, self.spt
        plan = {"run": run, "ticks": L, "fed": [], "events": {}, "keylock": {}, "load": {}}
        for n, d in self.decks.items():
            if run:
                u = rng.random()
                other = SETTINGS[int(rng.integers(0, len(SETTINGS)))]
                if u < 0.5:
                    pass
                elif u < 0.7 or d.kl is None and u < 0.85:
                    while other == d.kl:
                        other = SETTINGS[(SETTINGS.index(other) + 1) % len(SETTINGS)]
                    plan["keylock"][n] = ("set" if d.kl is None else "change", other)
                elif u < 0.85:
                    plan["keylock"][n] = ("repeat", d.kl)
                else:
                    plan["keylock"][n] = ("clear", None)
                if rng.random() < 0.15:
                    a = int(rng.integers(0, d.n_frames))
                    b = int(rng.integers(a + 1, min(d.n_frames, a + 1500) + 1))
                    plan["load"][n] = (a, dc.track(f"random decks {self.seed} node {n} load before run {run}", b - a))
            fed = rng.random() < 0.8 and run != self.no_deck_run
            if not fed:
                continue
            plan["fed"].append(n)
            events, h = {}, d.head
            for k in range(L):
                ev, d.loop = dc.draw_event(rng, d.n_frames, d.loop, not d.started)
                d.started = True
                if not 0 <= h.pos < d.n_frames * ONE and (ev is None or ev[1] is None):   # a deck that ran out is cued back into its track
                    ev = (ev[0] if ev else None, dc.frames(float(rng.uniform(0, d.n_frames))))
                if ev is not None:
                    events[k] = ev
                _t, h = dm.plan(h, *(events.get(k, (None, None))), spt, d.n_frames)
            d.head = h
            plan["events"][n] = events
        plan["fed"] = [plan["fed"][int(i)] for i in rng.permutation(len(plan["fed"]))]
        self.plan = plan
        self.drawn.append(("run", run, L, plan["fed"], sorted(plan["events"].items()), sorted(plan["keylock"].items()),
                           sorted((n, a, hashlib.sha256(t.tobytes()).hexdigest()) for n, (a, t) in plan["load"].items())))
        for n, (_what, kl) in plan["keylock"].items():
            d = self.decks[n]
            d.kl, d.clock = kl, 0
            d.model.set_keylock(kl)
            for decks in self.dev.values():
                decks[n].set_keylock(deck.keylock(*kl) if kl is not None else None)
        for n, (a, piece) in plan["load"].items():
            self.decks[n].model.load(a, piece)
            for decks in self.dev.values():
                decks[n].load(piece, a)
        self.got = {name: {"decks": {n: {"ticks": None, "grains": None, "state": None} for n in self.decks}, "feed_counts": dict.fromkeys(FEED_KEYS, 0),
                           "keylock_counts": dict.fromkeys(kc.COUNT_KEYS, 0)} for name in self.dev}
        for g in self.got.values():
            for n in plan["fed"]:
                g["decks"][n].update(ticks=[], grains=[])

    def fed(self, node):
        return node in self.plan["fed"]

    # ---- the expected side ----------------------------------------------------------------------------------------------------------
    def expect_run(self):
        """runs every fed deck's model over the run.  -> {source node: the samples the oracle's source takes} for the deck-fed sources (a fault: for
        others too); self.want is what the records of the run must be"""
        plan, spt, fault = self.plan, self.spt, self.fault
        L, fed = plan["ticks"], plan["fed"]
        want = {"decks": {}, "feed_counts": dict.fromkeys(FEED_KEYS, 0), "keylock_counts": dict.fromkeys(kc.COUNT_KEYS, 0)}
        samples, info = {}, {}
        for n in fed:
            d = self.decks[n]
            m = d.model
            events = dict(plan["events"][n])
            if fault == "ticked_events_late":      # every event a tick late; the one of the last tick waits for the deck's next feed
                events = {k + 1: ev for k, ev in events.items()}
                if d.late is not None:
                    events[0] = d.late
                d.late = events.pop(L, None)
            for k, (p, s) in events.items():
                m.schedule(k, p, s)
            if fault == "clock_lost_when_left_out" and d.sat_out:
                m.t = 0
            samples[n], recs, grains = m.feed(L, spt)
            info[n] = {"kl": d.kl, "recs": recs, "grains": grains, "clock": d.clock}
            want["decks"][n] = {"ticks": [tuple(t) for t in recs], "grains": [tuple(x) for x in grains]}
            if d.kl is None:
                for k, v in dc.launch_counts(recs, spt).items():
                    want["feed_counts"][k] += v
            else:
                d.clock = kc.count_feed(want["keylock_counts"], d.kl, d.clock, recs, grains, spt)
        data = {}
        for i, n in enumerate(fed):                # where the samples land
            to = n
            if fault == "sorted_nodes":
                to = sorted(fed)[i]
            elif fault == "plain_first":
                to = fed[([x for x in fed if self.decks[x].kl is None] + [x for x in fed if self.decks[x].kl is not None]).index(n)]
            data[to] = samples[n]
        for n, d in self.decks.items():
            if n in fed:
                if fault == "other_parity":        # this feed is heard in the next run, the last one now
                    data[n], d.last = (np.resize(d.last, 2 * L * spt) if d.last is not None else np.zeros(2 * L * spt, np.float32)), data[n]
                else:
                    d.last = data[n]
            else:
                if fault == "stale_source" and d.was_fed and d.last is not None:
                    data[n] = np.resize(d.last, 2 * L * spt)
                if fault == "advances_when_left_out":
                    d.model.feed(L, spt)
                want["decks"][n] = {"ticks": None, "grains": None}
            want["decks"][n]["state"] = model_head_tuple(d.model.deck.head)
            d.sat_out = n not in fed and (d.sat_out or d.was_fed)
            d.was_fed = n in fed
        self.want = want
        self.runs.append({"run": plan["run"], "ticks": L, "fed": list(fed), "info": info, "keylock": dict(plan["keylock"]), "load": sorted(plan["load"]),
                          "samples": {n: samples[n] for n in fed}})
        return {n: np.ascontiguousarray(x, dtype=np.float32) for n, x in data.items()}

    # ---- the device side ------------------------------------------------------------------------------------------------------------
    def feed(self, name, g, k0, step):
        """ticks [k0, k0 + step) of the run into graph `g` of build `name`: one mx_deck_feed, the decks in the run's drawn order"""
        fed = self.plan["fed"]
        if not fed:
            return
        decks = self.dev[name]
        for n in fed:
            for k, (p, s) in self.plan["events"][n].items():
                if k0 <= k < k0 + step:
                    decks[n].schedule(k - k0, c_params(p) if p is not None else None, s)
        deck.feed([decks[n] for n in fed], fed, g, step)
        got = self.got[name]
        for k, v in deck.debug_last_feed().items():
            got["feed_counts"][k] += v
        for k, v in deck.debug_last_keylock().items():
            got["keylock_counts"][k] += v

    def read(self, name, k0, step):
        got = self.got[name]["decks"]
        for n in self.plan["fed"]:
            d = self.dev[name][n]
            got[n]["ticks"] += [tick_tuple(t) for t in d.read_ticks(0, step)]
            grains = d.read_grains()
            assert len(grains) == d.grain_count()
            got[n]["grains"] += [(x.a_q32, x.g_q32, k0 + x.tick, x.frame, x.delta, x.dist, x.flags) for x in grains]

    def difference(self, name):
        """the build's records of the run against the models': None, or a line on the first difference"""
        got = self.got[name]
        for n, d in self.dev[name].items():
            got["decks"][n]["state"] = head_tuple(d.state())
        d = difference(got, self.want)
        return None if d is None else d[1]

    def close(self):
        for decks in self.dev.values():
            for d in decks.values():
                d.close()
        self.dev = {}
