"""The reverb's shared cases (tests/test_cpu_deck_reverb.py, tests/test_gpu_deck_reverb.py): a deck script (tests/deck_cases.py's vocabulary), a reverb script and,
for one case, a filter and an echo script, tick by tick.  The smallest shapes at which the kernel can still go wrong: ticks of 1, 16, 63, 64, 65, 441 and 800
frames against a reach of 64 (blocks that end on a tick boundary, one short of it, one past it, 4 and 64 ticks a block), every delay at its minimum and at its
maximum, blocks straddling tick boundaries, a setting that lowers the reach under a running block and one that raises it, off and on inside a feed, a feed of
17 600 frames that wraps both ring sizes, a ramp of all eleven ramped fields, and a ring-out through the f32 subnormals.

A case is a tick length, a track length and a list of feeds; a feed is a number of ticks, the deck's events (tick, Params or None, seek or None), the reverb's
(tick, Reverb or OFF), the filter's (tick, Filt or OFF) and the echo's (tick, Echo or OFF)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import deck_cases as dc
import deck_echo_model as em
import deck_filter_model as fm
import deck_reverb_model as rm
from deck_echo_model import Echo, EchoModel
from deck_filter_model import LP, Filt, FilterModel
from deck_keylock_model import Keylock, KeylockModel
from deck_model import ONE, PLAY, DeckModel
from deck_reverb_model import OFF, Reverb, ReverbModel

Feed = namedtuple("Feed", "n_ticks deck rev filt echo", defaults=((), ()))
Case = namedtuple("Case", "name spt n_frames feeds keylock", defaults=(None,))

LONG_FEEDS = {16: 64, 1: 300, 800: 22}    # tick length -> the most ticks one feed of its cases has, where that is more than the other cases' graphs hold

# the designed default at 48 kHz, size 1, two seconds, written down: what mx_deck_reverb_design(48000, 1, 2, 0.3, 0.5, 1, 1, 0.5) gives (tests/test_cpu_deck_reverb.py
# holds the library to the restatement these numbers come from)
DEFAULT = rm.design(48000.0, 1.0, 2.0, 0.3, 0.5, 1.0, 1.0, 0.5)
FLOOR = Reverb((128,) * 8, (64,) * 4, (0.8, -0.7, 0.75, 0.6, -0.65, 0.7, 0.5, -0.85), 1.0, 0.9, 0.6, 0.3, 0.6)                 # reach 64
STAGGER = Reverb((128, 129, 131, 137, 139, 149, 151, 157), (64, 67, 71, 73), (0.8,) * 8, 1.0, 1.0, 0.5, 0.2, 0.5)               # reach 64, every delay its own
CEILING = Reverb((12000,) * 8, (2000,) * 4, (0.9,) * 8, 1.0, 1.0, 1.0, 0.4, 0.75)                                               # reach 2000
MID = Reverb((601, 701, 809, 907, 1009, 1103, 1201, 1301), (500, 503, 509, 521), (0.85,) * 8, 0.8, 1.0, 0.7, 0.25, 0.5)         # reach 500
DELAYS4 = (200, 331, 467, 599, 733, 863, 997, 1129)


def track(case: Case) -> np.ndarray:
    return dc.track("reverb " + case.name, case.n_frames)


def simple(name, spt, events, n_ticks=12, n_frames=3001):
    """the deck plays a short looped track of noise and clicks at unity from frame 0; events: the reverb's"""
    return Case(name, spt, n_frames, [Feed(n_ticks, [(0, dc.play(ONE, loop=(0, n_frames)), 0)], list(events))])


def _cases():
    out = []
    out.append(simple("designed default, 800 frames a tick", 800, [(0, DEFAULT)]))
    out.append(simple("designed default, 441 frames a tick", 441, [(0, DEFAULT)]))
    # a reach of 64 against every tick length: a block that ends on a tick boundary, one short, one past; four ticks a block; 64 ticks a block
    for spt in (63, 64, 65):
        out.append(simple(f"{spt} frames a tick", spt, [(0, FLOOR), (5, STAGGER), (8, FLOOR._replace(wet=1.0))]))
    out.append(simple("16 frames a tick", 16, [(0, STAGGER), (20, FLOOR), (41, OFF), (44, STAGGER)], n_ticks=LONG_FEEDS[16]))
    out.append(simple("one frame a tick", 1, [(0, FLOOR), (150, STAGGER), (200, OFF), (220, FLOOR)], n_ticks=LONG_FEEDS[1]))
    out.append(simple("every delay at its minimum", 441, [(0, FLOOR)]))
    # every delay at its maximum, 17 600 frames: the tank rings (16384) and the diffuser rings (4096) both wrap, and the tank is heard from frame 12 000 on
    out.append(simple("every delay at its maximum, both rings wrap", 800, [(0, CEILING)], n_ticks=LONG_FEEDS[800]))
    # the reach lowered under a running block (500 -> 64 at tick 5: the block that began in tick 4 ends early) and raised (64 -> 500)
    out.append(simple("reach lowered mid-feed", 441, [(0, MID), (5, STAGGER)]))
    out.append(simple("reach raised mid-feed", 441, [(0, STAGGER), (5, MID)]))
    # on at 3, a change of delays on the running reverb at 5, off at 8, on again at 10; the deck seeks at 7 (no business of the reverb's)
    out.append(Case("schedules inside a feed", 800, 12000, [Feed(12, [(0, dc.play(ONE), 0), (7, None, dc.frames(100))],
                                                                [(3, MID), (5, MID._replace(delay=DELAYS4, diff=(300, 307, 311, 313))), (8, OFF), (10, STAGGER)])]))
    # all eleven ramped fields move at tick 4, the delays stay
    moved = MID._replace(gain=(0.5, -0.6, 0.7, -0.8, 0.9, 0.4, -0.3, 0.2), send=-0.5, dry=0.25, wet=2.0)
    out.append(simple("a ramp of every ramped field", 441, [(0, MID), (4, moved)]))
    # reverb-out: PLAY cleared at tick 4, the tail rings on; plain and under key-lock
    stop = dc.play(ONE, on=False)
    out.append(Case("reverb-out", 441, 4097, [Feed(12, [(0, dc.play(ONE), dc.frames(500)), (4, stop, None)], [(0, DEFAULT._replace(wet=1.0))])]))
    out.append(Case("under key-lock", 800, 8000, [Feed(12, [(0, dc.play(dc.frames(1.08)), dc.frames(300))], [(0, DEFAULT), (6, MID)])], Keylock(ONE, 256, 128, 300)))
    # behind a filter and an echo: the echo repeats are reverberated; PLAY cleared at tick 6
    out.append(Case("behind a filter and an echo", 800, 12000,
                    [Feed(12, [(0, dc.play(ONE), 0), (6, stop, None)], [(1, DEFAULT)], [(0, Filt(LP, 0.2, 0.3))], [(0, Echo(900, 1.0, 0.6, 1.0, 0.3))])]))
    out.append(simple("wet 0", 441, [(0, MID._replace(wet=0.0, dry=1.0))]))
    # the four-tap delay: no recirculation, no diffusion, no damping; send 0.5 so that the sent input is not the port's
    out.append(simple("gain 0 multi-tap", 441, [(0, Reverb(DELAYS4, (64, 71, 67, 73), (0.0,) * 8, 0.5, 1.0, 1.0, 0.0, 0.0))]))
    # a burst of one tick, then silence: every pass round the tank takes three bits (gain 1/8, the mixing orthogonal), 128 frames a pass -- through the f32
    # subnormals after 42 passes and into zero
    out.append(Case("subnormal ring-out", 800, 4097, [Feed(12, [(0, dc.play(ONE), 0), (1, stop, None)], [(0, Reverb((128,) * 8, (64,) * 4, (0.125,) * 8, 1.0, 1.0, 1.0, 0.0, 0.0))])]))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# the case each misreading of deck_reverb_model.MISREADINGS (and `reverb_first`, below) is shown by, and the grouping of its ticks into feeds
SHOWN_BY = {"ramp_n_plus_1": ("a ramp of every ramped field", None), "ramp_f64": ("a ramp of every ramped field", None), "v_for_w": ("every delay at its minimum", None),
            "diffusers_other_order": ("designed default, 441 frames a tick", None), "diffusers_lr_swapped": ("designed default, 441 frames a tick", None),
            "hadamard_in_place": ("every delay at its minimum", None), "c_f32": ("every delay at its minimum", None), "even_odd_swapped": ("every delay at its minimum", None),
            "output_after_gain": ("every delay at its minimum", None), "seek_clears": ("schedules inside a feed", None), "feed_clears": ("reach raised mid-feed", [5, 7]),
            "clock_stops": ("reverb-out", None), "delays_at_tick_end": ("schedules inside a feed", None), "no_fade_in": ("designed default, 441 frames a tick", None),
            "reverb_first": ("behind a filter and an echo", None)}


def flatten(case: Case):
    """(total ticks, {tick: (Params, seek)}, {tick: Reverb or OFF}, {tick: Filt or OFF}, {tick: Echo or OFF}) over the whole case"""
    deck_ev, rev_ev, filt_ev, echo_ev, t0 = {}, {}, {}, {}, 0
    for f in case.feeds:
        for (t, p, s) in f.deck:
            deck_ev[t0 + t] = (p, s)
        for (t, e) in f.rev:
            rev_ev[t0 + t] = e
        for (t, e) in f.filt:
            filt_ev[t0 + t] = e
        for (t, e) in f.echo:
            echo_ev[t0 + t] = e
        t0 += f.n_ticks
    return t0, deck_ev, rev_ev, filt_ev, echo_ev


_samples = {}


def deck_samples(case: Case, tables) -> np.ndarray:
    """what the deck writes over the whole case, float32 (total ticks, spt * 2), from DeckModel / KeylockModel; computed once a case (the deck's samples do not
    depend on how its ticks are grouped into feeds: tests/test_cpu_deck.py) and never written to"""
    if case.name not in _samples:
        total, deck_ev, *_ = flatten(case)
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
    total, deck_ev, *_ = flatten(case)
    on, out = False, set()
    for t in range(total):
        if t in deck_ev and deck_ev[t][0] is not None:
            on = bool(deck_ev[t][0].flags & PLAY)
        if on:
            out.add(t)
    return out


_runs = {}


def run_model(case: Case, tables, mis=(), split=None, reverb_first=False):
    """([port per feed], [(t, on, Reverb, counts) after each feed], [(lines, mask) after each feed], [reverb input per feed]) with the feeds as given or regrouped by
    split (feed lengths over the same ticks).  reverb_first: the misreading that runs the reverb ahead of the echo.  Computed once per argument set and shared."""
    key = (case.name, tuple(mis), tuple(split) if split is not None else None, reverb_first)
    if key in _runs:
        return _runs[key]
    total, deck_ev, rev_ev, filt_ev, echo_ev = flatten(case)
    lengths = list(split) if split is not None else [f.n_ticks for f in case.feeds]
    assert sum(lengths) == total
    xs = deck_samples(case, tables)
    playing = playing_ticks(case)
    r, f, e, ports, states, lines, inputs, at = ReverbModel(mis), FilterModel(), EchoModel(), [], [], [], [], 0
    for n in lengths:
        for t in range(at, at + n):
            if t in rev_ev:
                r.schedule(t - at, rev_ev[t])
            if t in filt_ev:
                f.schedule(t - at, filt_ev[t])
            if t in echo_ev:
                e.schedule(t - at, echo_ev[t])
        x = f.run(xs[at:at + n].reshape(-1), case.spt)
        seeks = {t - at for t in range(at, at + n) if t in deck_ev and deck_ev[t][1] is not None and t > 0}
        run_rev = lambda v: r.run(v, case.spt, seeks=seeks, playing={t - at for t in playing if at <= t < at + n})   # noqa: E731
        if reverb_first:
            y = e.run(run_rev(x), case.spt)
        else:
            x = e.run(x, case.spt)
            y = run_rev(x)
        for a in (x, y):
            a.setflags(write=False)
        inputs.append(x)
        ports.append(y)
        states.append((r.t, r.on, r.set, rm.counts_of(case.spt, r.last_reaches)))
        lines.append(r.lines())
        at += n
    _runs[key] = (ports, states, lines, inputs)
    return _runs[key]


def settings_per_tick(case: Case) -> list:
    """the setting in force in every tick of the case (None: no reverb), as mx_deck_reverb_host and mx_deck_reverb_plan take them"""
    total, _d, rev_ev, _f, _e = flatten(case)
    cur, out = None, []
    for t in range(total):
        if t in rev_ev:
            cur = None if rev_ev[t] is OFF else rev_ev[t]
        out.append(cur)
    return out
