"""Random deck sessions on the full random graphs (tests/test_gpu_random_graphs.py run_full_graph(decks=...)), shared by the GPU test
(tests/test_gpu_random_decks.py) and its CPU proof (tests/test_cpu_random_decks.py): further SOURCE_STEREO nodes grafted into the graph, a deck
(DESIGN.md section 0.15), plain or key-locked (0.16), on every stereo source, and a session of feeds, events, set_keylock calls and loads
over run_full_graph's runs.  The expected side is one KeylockModel per deck (tests/deck_keylock_model.py: the plain model while key-lock is
off) whose samples go into the oracle's source; everything downstream is what run_full_graph compares anyway.

Everything here is drawn from a stream of its own (default_rng(9000 + seed)): the graph generator's stream, run_full_graph's (7000 + seed) and
random_taps' (8000 + seed) draw what they always drew.  Nothing here needs a GPU but the device side of DeckSession, which takes built graphs.

`fault` makes the EXPECTED side wrong in one way the device could be (FAULTS); the CPU test shows that each changes an item the GPU test
compares.  The draws are the same with and without a fault: what is drawn never looks at a model.

session(echo=True) adds the deck echo (tests/test_gpu_random_deck_echo.py, tests/test_cpu_random_deck_echo.py): two decks in three
get set_echo calls between the runs and schedule_echo calls inside them, from one more stream of its own (default_rng(9500 + seed)) -- the deck,
graph and tap streams draw what they always drew, and with echo=False not a draw moves.  Each deck's EchoModel (tests/deck_echo_model.py) runs over
what its KeylockModel wrote before the samples go to the oracle's source; mx_deck_debug_last_echo and every deck's echo_state join the compared items,
and ECHO_FAULTS the ways of getting a session wrong."""
from __future__ import annotations

import functools
import hashlib

import numpy as np

import deck_cases as dc
import deck_echo_model as em
import deck_keylock_cases as kc
import deck_keylock_model as km
import deck_model as dm
import synth
from deck_echo_model import OFF, PINGPONG, Echo
from deck_keylock_model import Keylock
from deck_model import ONE
from mixlab_amd import abi, deck
from test_gpu_random_graphs import drop_refused_edges, engine_domains, resample_ratio

STEREO = 2
FAULTS = ("other_parity", "sorted_nodes", "plain_first", "stale_source", "advances_when_left_out", "restart_per_feed", "no_restart_after_pause",
          "clock_lost_when_left_out", "ticked_events_late")
# echo sessions only: every misreading of the echo model, and the ways a feed could get the echo of a session wrong (each described where it is switched in)
ECHO_FEED_FAULTS = {"echo_" + m: m for m in em.FEED_MISREADINGS}      # the two that live in the model's run over a feed
ECHO_FAULTS = em.MISREADINGS + ("echo_partition_identity", "echo_clock_runs_when_left_out", "echo_restart_per_feed", "echo_cleared_by_load", "echo_restart_on_set_keylock",
                                "echo_on_host_written", "echo_events_late", *ECHO_FEED_FAULTS)
LENGTHS = (1, 31, 33, 700, 4097, 6000)
KINDS = ("noise", "music", "period 16")
# hop 256 / 512 / 1024, overlap 16 .. 256, radius 0 / 5 / 300, pitch at unity, at 44.1 in 48 and just above the first bank edge
SETTINGS = (Keylock(ONE, 256, 64, 5), Keylock(kc.STEP_441, 512, 16, 300), Keylock(ONE, 1024, 256, 300), Keylock(dc.EDGE1 + 1, 256, 32, 5),
            Keylock(ONE, 512, 128, 0), Keylock(kc.STEP_441, 256, 128, 300))
SLOT_CLASS = {abi.KIND_MIXER: "mixer", abi.KIND_AMPLIFIER: "amp_split", abi.KIND_STEREO_SPLITTER: "amp_split", abi.KIND_FIR: "fir_resample",
              abi.KIND_RESAMPLE: "fir_resample", abi.KIND_OUTPUT_DEVICE: "output_device", abi.KIND_PLOTTER: "plotter"}
FEED_KEYS = ("ticks_zero", "ticks_stream", "ticks_gather", "chunks_zero", "chunks_stream", "chunks_gather")
ECHO_KEYS = ("decks_one_block", "decks_sequential", "blocks", "blocks_crossing")
# (send, feedback, wet, damp): the freeze, negative feedback, wet 0, damp 0 / 0.3 / 1; PINGPONG is drawn beside them
FREEZE = (0.0, 1.0, 1.0, 0.0)
ECHO_GAINS = (FREEZE, (1.0, -0.7, 1.0, 0.3), (1.0, 0.6, 0.0, 0.3), (1.0, 0.5, 1.0, 0.0), (1.0, 0.8, 2.0, 0.3), (0.5, 0.9, 1.0, 1.0), (1.0, 0.6, 1.0, 0.0), (0.7, -0.5, 1.5, 1.0))
ECHO_GAIN_WEIGHTS = (0.08, 0.14, 0.06, 0.16, 0.16, 0.12, 0.16, 0.12)

_tables = []


def tables():
    if not _tables:
        _tables.append(np.stack([deck.deck_tables(b) for b in range(4)]))
    return _tables[0]


def session(fault=None, echo=False):
    """what run_full_graph(decks=...) takes"""
    return functools.partial(DeckSession, fault=fault, echo=echo)


def echo_delay_pool(spt):
    """(the short delays, the long ones): both forms occur at this tick length -- the floor and one above it, the tick length from one under to two over (the
    one-block threshold is D > spt), two ticks and three frames, 5000, and the longest"""
    short = [256, 257] + [v for v in (spt - 1, spt, spt + 1, spt + 2, 2 * spt + 3) if v >= 256]
    return short, [5000, 262144]


def c_echo(e):
    return abi.DeckEcho(e.delay, e.flags, e.send, e.feedback, e.wet, e.damp) if e is not OFF and e is not None else None


def echo_state_tuple(d):
    """a deck.Deck"""
    t, on, e = d.echo_state()
    return t, on, (e.delay, e.flags, e.send, e.feedback, e.wet, e.damp)


def model_echo_state(m):
    t, on, e = m.state()
    return t, on, (e.delay, e.flags, *(float(np.float32(v)) for v in (e.send, e.feedback, e.wet, e.damp)))


def count_echo_feed(c, spt, delays):
    """adds one deck's feed to mx_deck_debug_last_echo's four counts, from the model's cutter"""
    blocks = em.cut(spt, delays)
    if len(blocks) == 1:
        c["decks_one_block"] += 1
    elif blocks:
        c["decks_sequential"] += 1
        c["blocks"] += len(blocks)
        c["blocks_crossing"] += sum(1 for first, n in blocks if first // spt != (first + n - 1) // spt)


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
    "state"}}, "feed_counts", "keylock_counts"}; a deck that was not fed has ticks and grains None.  An echo session has "echo_state" per deck and
    "echo_counts" beside them"""
    echo = "echo_counts" in want
    for node, w in want["decks"].items():
        g = got["decks"][node]
        for item in ("ticks", "grains", "state") + (("echo_state",) if echo else ()):
            if g[item] != w[item]:
                k = next((i for i, (a, b) in enumerate(zip(g[item], w[item])) if a != b), None) if g[item] is not None and w[item] is not None else None
                where = f" first at {k}: got {g[item][k]}, want {w[item][k]}" if k is not None else f" got {g[item]}, want {w[item]}"
                return item, f"deck on node {node}: {item} differ:{where}"
    for item in ("feed_counts", "keylock_counts") + (("echo_counts",) if echo else ()):
        if got[item] != want[item]:
            return item, f"{item}: got {got[item]}, want {want[item]}"
    return None


class Deck:
    """one deck of a session: its node, track, model and what the draws need to know of it"""

    def __init__(self, node, track, kind, kl, fault):
        self.node, self.n_frames, self.kind = node, len(track), kind
        self.has_echo = False             # an echo session: whether this deck ever gets an echo call
        self.echo = em.EchoModel((fault,) if fault in em.MISREADINGS else (ECHO_FEED_FAULTS[fault],) if fault in ECHO_FEED_FAULTS else ())
        self.echo_on, self.echo_set = False, None   # the echo as the draws see it
        self.echo_late = None             # echo_events_late: the schedule pushed out of the last run
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
    def __init__(self, seed, ws, sources, shape, fault=None, echo=False):
        assert fault is None or fault in FAULTS or (echo and fault in ECHO_FAULTS)
        self.rng = rng = np.random.default_rng(9000 + seed)
        self.erng = np.random.default_rng(9500 + seed) if echo else None
        self.seed, self.ws, self.spt, self.fault, self.echo = seed, ws, ws.spt, fault, echo
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
        if echo:                                      # a third of the decks, to the nearest and one at the least, never have one
            nodes, without = list(self.decks), max(1, round(len(self.decks) / 3)) if len(self.decks) > 1 else 0
            for i in self.erng.permutation(len(nodes))[without:]:
                self.decks[nodes[int(i)]].has_echo = True
            self.drawn.append(("echo decks", [n for n, d in self.decks.items() if d.has_echo]))
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
        if self.echo:
            self.draw_echo(plan, L)
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
            if self.echo:
                g["echo_counts"] = dict.fromkeys(ECHO_KEYS, 0)

    def draw_setting(self, like=None):
        """an Echo from the pools; like: keep this one's delay (a change of gains alone)"""
        e = self.erng
        short, long = echo_delay_pool(self.spt)
        u = e.random()
        delay = like.delay if like is not None else long[1] if u < 0.03 else long[0] if u < 0.13 else short[int(e.integers(0, len(short)))]
        g = ECHO_GAINS[int(e.choice(len(ECHO_GAINS), p=ECHO_GAIN_WEIGHTS))]
        return Echo(delay, *g, PINGPONG if e.random() < 0.5 else 0)

    def draw_echo(self, plan, L):
        """the echo calls of the run, for the fed decks that have an echo at all (a left-out deck gets none): between the runs nothing, set_echo with a
        setting, set_echo repeating the setting in force, or set_echo(None); inside the run schedule_echo at up to three ticks -- a setting (half of them
        keep the delay), OFF while it is on, on again while it is off"""
        e = self.erng
        plan["echo_set"], plan["echo_sched"] = {}, {}
        for n, d in self.decks.items():
            if not d.has_echo or n not in plan["fed"]:
                continue
            u = e.random()
            if not d.echo_on:
                if u >= 0.2:
                    plan["echo_set"][n] = ("set", self.draw_setting())
            elif u < 0.5:
                pass
            elif u < 0.75:
                plan["echo_set"][n] = ("set", self.draw_setting(d.echo_set if e.random() < 0.4 else None))
            elif u < 0.9:
                plan["echo_set"][n] = ("repeat", d.echo_set)
            else:
                plan["echo_set"][n] = ("clear", OFF)
            if n in plan["echo_set"]:
                new = plan["echo_set"][n][1]
                d.echo_on, d.echo_set = new is not OFF, (new if new is not OFF else d.echo_set)
            count = min(L, int(e.choice(4, p=(0.45, 0.25, 0.18, 0.12))))
            sched = {}
            for k in sorted(int(k) for k in e.choice(L, size=count, replace=False)):
                if d.echo_on and e.random() < 0.4:
                    sched[k] = OFF
                    d.echo_on = False
                else:
                    sched[k] = self.draw_setting(d.echo_set if d.echo_on and e.random() < 0.5 else None)
                    d.echo_on, d.echo_set = True, sched[k]
            if sched:
                plan["echo_sched"][n] = sched
        self.drawn.append(("echo", plan["run"], sorted((n, what, tuple(x) if x is not OFF else OFF) for n, (what, x) in plan["echo_set"].items()),
                           sorted((n, sorted((k, tuple(x) if x is not OFF else OFF) for k, x in s.items())) for n, s in plan["echo_sched"].items())))

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
        self.ringing = {}
        if self.echo:                              # the echo runs in place on what the deck wrote
            samples, host_written = self.expect_echo(samples, want, info)
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
            if self.echo:
                want["decks"][n]["echo_state"] = model_echo_state(d.echo)
                if n in host_written:
                    data[n] = host_written[n]
            d.sat_out = n not in fed and (d.sat_out or d.was_fed)
            d.was_fed = n in fed
        self.want = want
        self.runs.append({"run": plan["run"], "ticks": L, "fed": list(fed), "info": info, "keylock": dict(plan["keylock"]), "load": sorted(plan["load"]),
                          "samples": {n: samples[n] for n in fed}, "ringing": self.ringing, "echo_set": dict(plan.get("echo_set", {})),
                          "echo_sched": dict(plan.get("echo_sched", {}))})
        return {n: np.ascontiguousarray(x, dtype=np.float32) for n, x in data.items()}

    def expect_echo(self, dry, want, info):
        """every deck's EchoModel over the run.  -> ({fed deck: its port after the echo}, {left-out deck: its source} under one fault); want gains
        "echo_counts": the four counts of mx_deck_debug_last_echo summed over the run's feeds, under "feed" for a build that feeds the run in one call and
        under "ticked" for the build that feeds it tick by tick; info[n]["echo"] is what the coverage checks read"""
        plan, spt, fault = self.plan, self.spt, self.fault
        L, fed = plan["ticks"], plan["fed"]
        counts = {"feed": dict.fromkeys(ECHO_KEYS, 0), "ticked": dict.fromkeys(ECHO_KEYS, 0)}
        out, delays, seeks = dict(dry), {}, {}
        for n, d in self.decks.items():
            m = d.echo
            reach = m.hist[max(0, m.t - m.set.delay - 1):m.t]
            ringing = bool(m.on and m.t > 0 and reach.any())          # the echo is on and the line the next frames read is not silent
            self.ringing[n] = ringing                                 # (between the runs: where this run's load and set_keylock calls met it)
            if n in fed:
                info[n]["echo"] = {"ringing": ringing, "t0": m.t, "dry": dry[n]}
            if fault == "echo_cleared_by_load" and n in plan["load"]:
                m.hist[:] = 0
            if fault == "echo_restart_on_set_keylock" and n in plan["keylock"]:
                m.t = 0
            if fault == "echo_restart_per_feed" and n in fed:
                m.t = 0
        for n in fed:
            m = self.decks[n].echo
            sched = {0: plan["echo_set"][n][1]} if n in plan["echo_set"] else {}
            inside = dict(plan["echo_sched"].get(n, {}))
            if fault == "echo_events_late":        # every schedule_echo a tick late; the one of the last tick waits for the deck's next feed
                d = self.decks[n]
                inside = {k + 1: e for k, e in inside.items()}
                if d.echo_late is not None:
                    inside.setdefault(0, d.echo_late)
                d.echo_late = inside.pop(L, None)
            sched.update(inside)
            on, st, delays[n], sets = m.on, m.set, [], []
            for k in range(L):
                if k in sched:
                    on = sched[k] is not OFF
                    st = sched[k] if on else st
                delays[n].append(st.delay if on else 0)
                sets.append(st if on else None)
            for k, e in sched.items():
                m.schedule(k, e)
            seeks[n] = {k for k, (_p, s) in plan["events"][n].items() if s is not None}
            count_echo_feed(counts["feed"], spt, delays[n])
            for k in range(L):
                count_echo_feed(counts["ticked"], spt, delays[n][k:k + 1])
            info[n]["echo"].update(delays=delays[n], sets=sets, sched=sched, blocks=em.cut(spt, delays[n]))
        # the decks with an echo in some tick, in feed order, and as the feed partitions them: the one-block decks first, the walking ones behind
        echoing = [n for n in fed if any(delays[n])]
        parted = [n for n in echoing if len(em.cut(spt, delays[n])) == 1] + [n for n in echoing if len(em.cut(spt, delays[n])) > 1]
        for k, n in enumerate(echoing):
            src = parted[k] if fault == "echo_partition_identity" else n      # ... the k-th descriptor on the k-th echo deck's port
            out[n] = self.decks[src].echo.run(dry[n], spt, seeks=seeks[src])
        for n in fed:
            if n not in echoing:                   # (its schedule is used up and its state moves all the same)
                self.decks[n].echo.run(dry[n], spt)
            info[n]["echo"]["port"] = out[n]
        host_written = {}
        for n, d in self.decks.items():
            m = d.echo
            if n in fed or not m.on:
                continue
            if fault == "echo_clock_runs_when_left_out":
                grown = np.zeros((max(m.hist.shape[0], m.t + L * spt), 2), np.float32)
                grown[:m.hist.shape[0]] = m.hist
                m.hist, m.t = grown, m.t + L * spt
            if fault == "echo_on_host_written":    # what run_full_graph writes into the source of a deck that is not fed
                x = (synth.noise(9000 + 97 * self.seed + 13 * plan["run"] + n, L * spt * STEREO) * np.float32(1.5)).astype(np.float32)
                host_written[n] = m.run(x, spt)
        want["echo_counts"] = counts
        return out, host_written

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
            if self.echo:
                if k0 == 0 and n in self.plan["echo_set"]:
                    decks[n].set_echo(c_echo(self.plan["echo_set"][n][1]))
                for k, e in self.plan["echo_sched"].get(n, {}).items():
                    if k0 <= k < k0 + step:
                        decks[n].schedule_echo(k - k0, c_echo(e))
        deck.feed([decks[n] for n in fed], fed, g, step)
        got = self.got[name]
        for k, v in deck.debug_last_feed().items():
            got["feed_counts"][k] += v
        for k, v in deck.debug_last_keylock().items():
            got["keylock_counts"][k] += v
        if self.echo:
            for k, v in deck.debug_last_echo().items():
                got["echo_counts"][k] += v

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
            if self.echo:
                got["decks"][n]["echo_state"] = echo_state_tuple(d)
        want = dict(self.want, echo_counts=self.want["echo_counts"]["ticked" if name == "ticked" else "feed"]) if self.echo else self.want
        d = difference(got, want)
        return None if d is None else d[1]

    def close(self):
        for decks in self.dev.values():
            for d in decks.values():
                d.close()
        self.dev = {}
