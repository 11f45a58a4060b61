"""The sweep filter's shared cases (tests/test_cpu_deck_filter.py, tests/test_gpu_deck_filter.py): a deck script (tests/deck_cases.py's vocabulary), a filter script
and, for one case, an echo script, tick by tick.  The smallest shapes at which the kernel can still go wrong: the two real tick lengths 441 and 800 (neither a
multiple of the kernel's 64-frame super-block, so blocks straddle tick boundaries at every offset), ticks of 63, 64 and 65 frames (a block that ends on a tick
boundary, one short of it, one past it), 64 ticks of 16 frames (four ticks a block), 300 ticks of one frame (64 ticks a block, the ramp weight always 0), g and k at
both range ends, on / off / kind changes inside a feed, and a ring-out through the f32 subnormals.

A case is a tick length, a track length and a list of feeds; a feed is a number of ticks, the deck's events (tick, Params or None, seek or None), the filter's
(tick, Filt or OFF) and the echo's (tick, Echo or OFF)."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

import deck_cases as dc
from deck_echo_model import Echo, EchoModel
from deck_filter_model import BP, HP, LP, NOTCH, OFF, Filt, FilterModel
from deck_keylock_model import Keylock, KeylockModel
from deck_model import ONE, PLAY, DeckModel

Feed = namedtuple("Feed", "n_ticks deck filt echo", defaults=((),))
Case = namedtuple("Case", "name spt n_frames feeds keylock", defaults=(None,))

LONG_FEEDS = {16: 64, 1: 300}    # tick length -> the ticks of its case's one feed, more than the other cases' graphs hold


def g_of(hz: float, rate: float = 48000.0) -> float:
    return float(np.float32(math.tan(math.pi * hz / rate)))


def track(case: Case) -> np.ndarray:
    return dc.track("filter " + case.name, case.n_frames)


def simple(name, spt, events, n_ticks=12, n_frames=3001, loop=True):
    """the deck plays a short looped track of noise and clicks at unity from frame 0; events: the filter's"""
    return Case(name, spt, n_frames, [Feed(n_ticks, [(0, dc.play(ONE, loop=(0, n_frames) if loop else None), 0)], list(events))])


def sweep(kind, hz0, hz1, ticks, k, rate):
    return [(t, Filt(kind, g_of(hz0 * (hz1 / hz0) ** (t / (ticks - 1)), rate), k)) for t in range(ticks)]


def _cases():
    out = []
    # each kind at rest: one setting at tick 0 (a fade-in tick, then constant ticks), at the two real tick lengths
    for kind, name, spt, g, k in ((LP, "lp", 441, 0.05, 0.5), (HP, "hp", 800, 0.3, 1.0), (BP, "bp", 441, 0.12, 0.2), (NOTCH, "notch", 800, 1.0, 0.7)):
        out.append(simple(f"{name} at rest, {spt} frames a tick", spt, [(0, Filt(kind, g, k))]))
    # super-block edges: a change of setting at tick 5, of kind at tick 8
    for spt in (63, 64, 65):
        out.append(simple(f"{spt} frames a tick", spt, [(0, Filt(LP, 0.08, 0.3)), (5, Filt(LP, 0.4, 0.9, 0.8)), (8, Filt(HP, 0.4, 0.9, 0.8))]))
    out.append(simple("16 frames a tick", 16, [(0, Filt(BP, 0.1, 0.1))] + [(t, Filt(LP, 0.05 + 0.01 * t, 0.3)) for t in range(7, 40, 3)] + [(41, OFF), (44, Filt(HP, 0.2, 1.5))],
                      n_ticks=LONG_FEEDS[16]))
    out.append(simple("one frame a tick", 1, [(0, Filt(LP, 0.1, 0.2)), (150, Filt(BP, 0.5, 1.0, 0.5)), (200, OFF), (220, Filt(NOTCH, 0.3, 0.1))], n_ticks=LONG_FEEDS[1]))
    # the transition itself: a low-pass closing from 20 kHz to 80 Hz over 8 ticks at Q = 10, a high-pass opening
    out.append(simple("lp sweep 20 kHz to 80 Hz", 800, sweep(LP, 20000.0, 80.0, 8, 0.1, 48000.0)))
    out.append(simple("hp sweep 20 Hz to 8 kHz", 441, sweep(HP, 20.0, 8000.0, 8, 0.7, 26460.0)))
    # the range ends
    for name, g, k in (("g at the floor", 2.0 ** -12, 0.5), ("g at the ceiling", 16.0, 0.5), ("k at the floor", 0.3, 0.05), ("k at the ceiling", 0.3, 2.0)):
        out.append(simple(name, 441, [(0, Filt(LP, g, k)), (6, Filt(NOTCH, g, k))]))
    # the issue's schedule: on at 3, swept at 5, a kind change at 6, off at 8, on again at 10; the deck seeks at 7 (no business of the filter's)
    out.append(Case("schedules inside a feed", 800, 12000, [Feed(12, [(0, dc.play(ONE), 0), (7, None, dc.frames(100))],
                                                                [(3, Filt(LP, 0.3, 0.1)), (5, Filt(LP, 0.05, 0.1)), (6, Filt(BP, 0.05, 0.1)), (8, OFF), (10, Filt(HP, 0.1, 0.4))])]))
    out.append(simple("wet 0", 441, [(0, Filt(LP, 0.05, 0.1, 0.0))]))
    out.append(simple("wet ramped out before an off", 441, [(0, Filt(LP, 0.05, 0.1)), (5, Filt(LP, 0.05, 0.1, 0.0)), (6, OFF)]))
    # the ring-out: PLAY cleared at tick 4, the resonance of a band-pass at Q = 20 audible in the zero ticks that follow
    stop = dc.play(ONE, on=False)
    out.append(Case("ring-out", 441, 4097, [Feed(12, [(0, dc.play(ONE), dc.frames(500)), (4, stop, None)], [(0, Filt(BP, 0.02, 0.05))])]))
    out.append(Case("under key-lock", 800, 8000, [Feed(12, [(0, dc.play(dc.frames(1.08)), dc.frames(300))], [(0, Filt(LP, 0.2, 0.3)), (6, Filt(HP, 0.2, 0.3))])],
                    Keylock(ONE, 256, 128, 300)))
    out.append(Case("a loop of three frames", 441, 4097, [Feed(12, [(0, dc.play(dc.frames(0.37), loop=(1000, 1003)), dc.frames(1001.25))], [(0, Filt(NOTCH, 0.4, 0.2))])]))
    # a burst of two ticks, then silence: two real poles near z = 0.9 carry every sample through the f32 subnormals into zero (about 830 frames after the stop)
    out.append(Case("subnormal ring-out", 441, 4097, [Feed(12, [(0, dc.play(ONE), 0), (2, stop, None)], [(0, Filt(LP, 0.0526, 2.0))])]))
    # filter with echo: the echo-out under a closing low-pass -- PLAY cleared at tick 6, the low-pass closes over ticks 2 .. 7
    out.append(Case("echo-out under a closing low-pass", 800, 12000,
                    [Feed(12, [(0, dc.play(ONE), 0), (6, stop, None)], [(t + 2, f) for t, f in sweep(LP, 12000.0, 200.0, 6, 0.5, 48000.0)], [(0, Echo(900, 1.0, 0.6, 1.0, 0.3))])]))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the case each misreading of deck_filter_model.MISREADINGS (and `echo_first`, below) is shown by, and the grouping of its ticks into feeds
SHOWN_BY = {"ramp_n_plus_1": ("lp sweep 20 kHz to 80 Hz", None), "coef_frozen": ("lp sweep 20 kHz to 80 Hz", None), "gn_f32": ("lp sweep 20 kHz to 80 Hz", None),
            "a1_f32": ("lp at rest, 441 frames a tick", None), "v2_from_new_s1": ("lp at rest, 441 frames a tick", None), "shared_state": ("lp at rest, 441 frames a tick", None),
            "seek_clears": ("schedules inside a feed", None), "feed_clears": ("bp at rest, 441 frames a tick", [5, 7]), "kind_change_clears": ("schedules inside a feed", None),
            "state_kept_off_on": ("schedules inside a feed", None), "no_fade_in": ("hp at rest, 800 frames a tick", None), "kind_at_tick_end": ("schedules inside a feed", None),
            "only_playing_ticks": ("ring-out", None), "schedule_late": ("schedules inside a feed", None), "echo_first": ("echo-out under a closing low-pass", None)}


def flatten(case: Case):
    """(total ticks, {tick: (Params, seek)}, {tick: Filt or OFF}, {tick: Echo or OFF}) over the whole case"""
    deck_ev, filt_ev, echo_ev, t0 = {}, {}, {}, 0
    for f in case.feeds:
        for (t, p, s) in f.deck:
            deck_ev[t0 + t] = (p, s)
        for (t, e) in f.filt:
            filt_ev[t0 + t] = e
        for (t, e) in f.echo:
            echo_ev[t0 + t] = e
        t0 += f.n_ticks
    return t0, deck_ev, filt_ev, echo_ev


_samples = {}


def deck_samples(case: Case, tables) -> np.ndarray:
    """what the deck writes over the whole case, float32 (total ticks, spt * 2), from DeckModel / KeylockModel; computed once a case (the deck's samples do not
    depend on how its ticks are grouped into feeds: tests/test_cpu_deck.py) and never written to"""
    if case.name not in _samples:
        total, deck_ev, _f, _e = flatten(case)
        tr = track(case)
        m = KeylockModel(tr, tables) if case.keylock else DeckModel(tr, tables)
        if case.keylock:
            m.set_keylock(case.keylock)
        for t, (p, s) in deck_ev.items():
            m.schedule(t, p, s)
        x = m.feed(total, case.spt)[0].reshape(total, -1)
        x.setflags(write=False)
        _samples[case.name] = x
    return _samples[case.name]


def playing_ticks(case: Case) -> set:
    total, deck_ev, _f, _e = flatten(case)
    on, out = False, set()
    for t in range(total):
        if t in deck_ev and deck_ev[t][0] is not None:
            on = bool(deck_ev[t][0].flags & PLAY)
        if on:
            out.add(t)
    return out


def run_model(case: Case, tables, mis=(), split=None, echo_first=False):
    """([port per feed], [(on, Filt, state4, counts) after each feed], the FilterModel, the EchoModel) with the feeds as given or regrouped by split (feed lengths
    over the same ticks).  echo_first: the misreading that runs the echo ahead of the filter"""
    total, deck_ev, filt_ev, echo_ev = flatten(case)
    lengths = list(split) if split is not None else [f.n_ticks for f in case.feeds]
    assert sum(lengths) == total
    xs = deck_samples(case, tables)
    playing = playing_ticks(case)
    fm, em, ports, states, at = FilterModel(mis), EchoModel(), [], [], 0
    for n in lengths:
        for t in range(at, at + n):
            if t in filt_ev:
                fm.schedule(t - at, filt_ev[t])
            if t in echo_ev:
                em.schedule(t - at, echo_ev[t])
        x = xs[at:at + n].reshape(-1)
        seeks = {t - at for t in range(at, at + n) if t in deck_ev and deck_ev[t][1] is not None and t > 0}
        run_filter = lambda v: fm.run(v, case.spt, seeks=seeks, playing={t - at for t in playing if at <= t < at + n})   # noqa: E731
        y = run_filter(em.run(x, case.spt)) if echo_first else em.run(run_filter(x), case.spt)
        ports.append(y)
        states.append((fm.on, fm.set, fm.state4(), dict(fm.counts)))
        at += n
    return ports, states, fm, em


def settings_per_tick(case: Case) -> list:
    """the setting in force in every tick of the case (None: no filter), as mx_deck_filter_host takes them"""
    total, _d, filt_ev, _e = flatten(case)
    cur, out = None, []
    for t in range(total):
        if t in filt_ev:
            cur = None if filt_ev[t] is OFF else filt_ev[t]
        out.append(cur)
    return out
