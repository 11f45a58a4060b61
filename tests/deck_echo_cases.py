"""The echo's shared cases (tests/test_cpu_deck_echo.py, tests/test_gpu_deck_echo.py): a deck script (tests/deck_cases.py's vocabulary) and an echo script, tick by
tick, at the two real tick lengths and at the suite's two tiny ones (16 frames and one frame a tick).  The smallest shapes at which the kernel can still go wrong: delays at the floor and one above it (blocks of 255 and 256 frames,
the ring index wrapping), delays around the tick length on both sides of the one-block threshold D > spt, blocks that straddle tick boundaries, a tick that
lowers the delay under a running block, off and on inside a feed, and a tail that runs into f32 subnormals.

A case is a tick length, a track length and a list of feeds; a feed is a number of ticks, the deck's events (tick, Params or None, seek or None) and the echo's
(tick, Echo or OFF)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import deck_cases as dc
from deck_echo_model import OFF, PINGPONG, Echo, EchoModel
from deck_keylock_model import Keylock, KeylockModel
from deck_model import ONE, DeckModel

Feed = namedtuple("Feed", "n_ticks deck echo")
Case = namedtuple("Case", "name spt n_frames feeds keylock identity", defaults=(None, False))

LONG_SPT = 1 << 20       # MX_DECK_MAX_SPT: one tick carries the clock past the ring's 2^19 frames
LONG_FEEDS = {16: 64, 1: 600}    # tick length -> the ticks of its cases' one feed, more than the other cases' graphs hold


def track(case: Case) -> np.ndarray:
    return dc.track("echo " + case.name, case.n_frames)


def simple(name, spt, e: Echo, n_ticks=12, n_frames=4097):
    return Case(name, spt, n_frames, [Feed(n_ticks, [(0, dc.play(ONE), 0)], [(0, e)])])


def _cases():
    out = []
    # every delay of the issue's list, 12 ticks in one feed: the sequential form, blocks across tick boundaries; damp 0 / 0.3 / 1, ping-pong, negative feedback
    for D, spt, kw in ((256, 441, dict(feedback=0.5)), (257, 800, dict(damp=0.3, flags=PINGPONG)), (440, 441, dict(feedback=-0.6)), (441, 441, dict(damp=1.0)),
                       (442, 441, dict(damp=0.3, flags=PINGPONG)), (799, 800, dict(damp=0.3)), (800, 800, dict(feedback=-0.7, flags=PINGPONG)),
                       (801, 800, dict(damp=1.0, flags=PINGPONG, wet=0.7)), (802, 800, dict()), (5000, 800, dict(damp=0.3, feedback=0.8)), (5000, 441, dict(flags=PINGPONG))):
        out.append(simple(f"delay {D}, {spt} frames a tick", spt, Echo(D, **kw)))
    # the freeze: a running echo, then send 0 / feedback 1 / damp 0 -- after the ramp tick the line goes round bit for bit
    out.append(Case("freeze", 441, 4097, [Feed(14, [(0, dc.play(ONE), 0)], [(0, Echo(440, 1.0, 0.5, 1.0, 0.0)), (4, Echo(440, 0.0, 1.0, 1.0, 0.0))])]))
    # the issue's schedule: on at 3, gains at 5, 5000 -> 256 at 6, off at 8, on again at 10; the deck seeks at 7 (no business of the echo's)
    out.append(Case("schedules inside a feed", 800, 12000, [Feed(12, [(0, dc.play(ONE), 0), (7, None, dc.frames(100))],
                                                                [(3, Echo(5000, 1.0, 0.5, 1.0, 0.0)), (5, Echo(5000, 0.5, -0.8, 2.0, 0.0)), (6, Echo(256, 0.5, -0.8, 2.0, 0.3)),
                                                                 (8, OFF), (10, Echo(300, 1.0, 0.6, 1.0, 0.0, PINGPONG))])]))
    # echo-out: PLAY cleared at tick 4, the tail rings on; plain, under key-lock, under a loop of three frames
    stop = dc.play(ONE, on=False)
    out.append(Case("echo-out", 441, 4097, [Feed(12, [(0, dc.play(ONE), dc.frames(500)), (4, stop, None)], [(0, Echo(442, 1.0, 0.6, 1.0, 0.3))])]))
    out.append(Case("echo-out under key-lock", 800, 8000, [Feed(12, [(0, dc.play(dc.frames(1.08)), dc.frames(300)), (4, dc.play(dc.frames(1.08), on=False), None)],
                                                                 [(0, Echo(900, 1.0, 0.6, 1.0, 0.0, PINGPONG))])], Keylock(ONE, 256, 128, 300)))
    out.append(Case("echo-out under a loop of three frames", 441, 4097, [Feed(12, [(0, dc.play(dc.frames(0.37), loop=(1000, 1003)), dc.frames(1001.25)),
                                                                                    (4, dc.play(dc.frames(0.37), loop=(1000, 1003), on=False), None)], [(0, Echo(256, 1.0, 0.7, 1.0, 1.0))])]))
    # a burst, then feedback 0.5 at the floor delay until every sample has passed through the subnormals into zero (137 repeats)
    tail = [Feed(16, [(0, dc.play(ONE), 0)], [(0, Echo(256, 1.0, 0.5, 1.0, 0.0))]), Feed(16, [], []), Feed(12, [], [])]
    out.append(Case("subnormal tail", 800, 300, tail))
    # the longest delay, the clock past 2^19 inside one tick: two feeds of one tick of 2^20 frames, all but the first 4097 frames silence
    out.append(Case("delay 262144, ring wrap", LONG_SPT, 4097, [Feed(1, [(0, dc.play(ONE), 0)], [(0, Echo(262144, 1.0, 0.5, 1.0, 0.3, PINGPONG))]), Feed(1, [], [])], None, True))
    # the suite's tiny ticks: a block of D - 1 frames spans 16 or 17 ticks of 16 frames (echo_block_end across many tick boundaries, ending inside a tick or on its edge)
    for D, kw in ((256, dict(feedback=0.6, damp=0.3)), (257, dict(feedback=-0.6, flags=PINGPONG))):
        out.append(simple(f"delay {D}, 16 frames a tick", 16, Echo(D, **kw), n_ticks=LONG_FEEDS[16]))
    # ... and 255 ticks of one frame, where the ramp weight n / spt is always 0: tick 300 changes the three gains alone and sounds the old ones whole; 256 -> 300 at tick 400 (the
    # new delay reads the line the old one wrote), off at 500, on again at 520
    out.append(Case("one frame a tick", 1, 4097, [Feed(LONG_FEEDS[1], [(0, dc.play(ONE), 0)],
                                                       [(0, Echo(256, 1.0, 0.6, 1.0, 0.0)), (300, Echo(256, 0.5, -0.8, 2.0, 0.0)), (400, Echo(300, 0.5, -0.8, 2.0, 0.3)), (500, OFF),
                                                        (520, Echo(256, 1.0, 0.5, 1.0, 0.0, PINGPONG))])]))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
QUICK = [c for c in CASES if c.spt != LONG_SPT]     # what the CPU suite runs through every misreading


def flatten(case: Case):
    """(total ticks, {tick: (Params, seek)}, {tick: Echo or OFF}) over the whole case"""
    deck_ev, echo_ev, t0 = {}, {}, 0
    for f in case.feeds:
        for (t, p, s) in f.deck:
            deck_ev[t0 + t] = (p, s)
        for (t, e) in f.echo:
            echo_ev[t0 + t] = e
        t0 += f.n_ticks
    return t0, deck_ev, echo_ev


def deck_samples(case: Case, tables, lengths):
    """[x per feed]: what the deck writes, from DeckModel / KeylockModel -- or, for a case marked `identity` (unity from frame 0, where the deck's output IS the
    track: tests/test_gpu_deck.py proves it on the device), from the track itself: DeckModel walks a tick frame by frame in Python integers, 2^20 of them is minutes"""
    total, deck_ev, _ = flatten(case)
    tr = track(case)
    if case.identity:
        x = np.zeros((total * case.spt, 2), np.float32)
        x[:case.n_frames] = tr.astype(np.float32) / np.float32(32768.0)
        return [x[at * case.spt:(at + n) * case.spt].reshape(-1) for at, n in zip(np.cumsum([0] + lengths[:-1]), lengths)]
    m = KeylockModel(tr, tables) if case.keylock else DeckModel(tr, tables)
    if case.keylock:
        m.set_keylock(case.keylock)
    out, at = [], 0
    for n in lengths:
        for t in range(at, at + n):
            if t in deck_ev:
                m.schedule(t - at, *deck_ev[t])
        out.append(m.feed(n, case.spt)[0])
        at += n
    return out


def run_model(case: Case, tables, mis=(), split=None, xs=None):
    """([port per feed], [(t, on, Echo) after each feed]) with the feeds as given or regrouped by split (feed lengths over the same ticks)"""
    total, deck_ev, echo_ev = flatten(case)
    lengths = list(split) if split is not None else [f.n_ticks for f in case.feeds]
    assert sum(lengths) == total
    xs = xs if xs is not None else deck_samples(case, tables, lengths)
    m, ports, states, at = EchoModel(mis), [], [], 0
    for n, x in zip(lengths, xs):
        for t in range(at, at + n):
            if t in echo_ev:
                m.schedule(t - at, echo_ev[t])
        ports.append(m.run(x, case.spt, seeks={t - at for t in range(at, at + n) if t in deck_ev and deck_ev[t][1] is not None and t > 0}))
        states.append(m.state())
        at += n
    return ports, states


def delays_of(case: Case, lengths=None):
    """per feed the delay of every tick (0: no echo), as mx_deck_echo_plan takes them"""
    total, _d, echo_ev = flatten(case)
    lengths = lengths if lengths is not None else [f.n_ticks for f in case.feeds]
    cur, per_tick = 0, []
    for t in range(total):
        if t in echo_ev:
            cur = 0 if echo_ev[t] is OFF else echo_ev[t].delay
        per_tick.append(cur)
    out, at = [], 0
    for n in lengths:
        out.append(per_tick[at:at + n])
        at += n
    return out
