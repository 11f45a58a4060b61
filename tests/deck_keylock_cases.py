"""The key-locked deck's shared cases (tests/test_cpu_deck_keylock.py, tests/test_gpu_deck_keylock.py).

A case is a track, a tick length and a list of feeds; a feed is a number of ticks (8 at the most: the GPU suite's max_ticks_per_run), the events scheduled into it
-- (tick, Params or None, seek or None), as in deck_cases -- and what mx_deck_set_keylock is called with before it: KEEP (no call), None (off) or a Keylock.
The smallest shapes at which clock, search and render can still go wrong: tick lengths around the render chunk, hops of a chunk and of many ticks, grain starts on
the first and last frame of a tick, fades across tick and feed boundaries, more candidates than lanes, every bank, tracks shorter than the overlap."""
from __future__ import annotations

import zlib
from collections import namedtuple

import numpy as np

import deck_cases as dc
from deck_cases import frames, play
from deck_keylock_model import Keylock, KeylockModel
from deck_model import ONE

KEEP = "keep"
KFeed = namedtuple("KFeed", "n_ticks events keylock", defaults=((), KEEP))
KCase = namedtuple("KCase", "name spt n_frames feeds track", defaults=("noise",))

STEP_441 = 3946001203   # mx_deck_step(44100, 48000, 1.0)


def track(case_or_kind, n_frames: int | None = None, name: str = "") -> np.ndarray:
    """int16 (n_frames, 2).  noise: deck_cases' seeded noise with the extremes in it.  music: a few partials plus a little noise, different in L and R, so that the
    search has something to find.  silent.  period Q: s[f] depends on f mod Q only (Q even, L = R).  extreme: -32768 / +32767 alternating on both channels."""
    kind, n, name = (case_or_kind.track, case_or_kind.n_frames, case_or_kind.name) if isinstance(case_or_kind, KCase) else (case_or_kind, n_frames, name)
    f = np.arange(n)
    if kind == "noise":
        return dc.track("keylock " + name, n)
    if kind == "music":
        rng = np.random.default_rng(zlib.crc32(name.encode()))
        l = 9000 * np.sin(2 * np.pi * f / 109.1) + 5000 * np.sin(2 * np.pi * f / 37.3 + 1.0) + 2500 * np.sin(2 * np.pi * f / 11.7) + rng.normal(0, 300, n)
        r = 8000 * np.sin(2 * np.pi * f / 109.1 + 0.4) + 6000 * np.sin(2 * np.pi * f / 23.9) + rng.normal(0, 300, n)
        return np.stack([np.round(l), np.round(r)], axis=1).astype(np.int16)
    if kind == "silent":
        return np.zeros((n, 2), np.int16)
    if kind.startswith("period"):
        q = int(kind.split()[1])
        rng = np.random.default_rng(q)
        cell = rng.integers(-12000, 12000, size=q).astype(np.int16)
        return np.repeat(cell[f % q][:, None], 2, axis=1)
    if kind == "extreme":
        v = np.where(f % 2 == 0, -32768, 32767).astype(np.int16)
        return np.stack([v, v], axis=1)
    raise ValueError(kind)


def run(name, spt, n_frames, kl, step, seek, ticks, kind="noise", events=()):
    """one setting from the start; `ticks` is the list of feed lengths, `events` further (feed, tick, params, seek)"""
    feeds = []
    for fi, n in enumerate(ticks):
        ev = [(0, play(step), seek)] if fi == 0 else []
        ev += [(t, p, s) for (f, t, p, s) in events if f == fi]
        feeds.append(KFeed(n, tuple(ev), kl if fi == 0 else KEEP))
    return KCase(name, spt, n_frames, feeds, kind)


def _cases():
    out = []
    t108 = frames(1.08)
    # every tick length around the render chunk; hop of one chunk, so grains start often.  At 257 a grain starts on the LAST frame of tick 0 and its fade straddles the
    # tick boundary and -- the feeds being 1, 1, 2, ... ticks -- a feed boundary; at 256 every tick starts a grain on its FIRST frame; at 800 several start per tick.
    out.append(run("spt 1, hop 256", 1, 700, Keylock(ONE, 256, 16, 5), t108, frames(100.5), [8] * 35, "music"))
    out.append(run("spt 255, hop 256", 255, 4097, Keylock(ONE, 256, 64, 40), t108, frames(50.25), [1, 2, 8, 3], "music"))
    out.append(run("spt 256, hop 256", 256, 4097, Keylock(ONE, 256, 128, 1), frames(0.92), frames(10), [3, 1, 4], "music"))
    out.append(run("spt 257, hop 256", 257, 4097, Keylock(ONE, 256, 64, 5), t108, frames(77.75), [1, 1, 2, 1, 3], "music"))
    out.append(run("spt 800, hop 256, more candidates than lanes", 800, 4097, Keylock(STEP_441, 256, 128, 300), frames(1.5), frames(20.5), [2, 3], "music"))
    # hop of many ticks: ticks and whole feeds without a grain start; the longest overlap and the widest search
    out.append(run("spt 1, hop 4096", 1, 300, Keylock(ONE, 4096, 1024, 512), t108, 0, [8, 8], "music"))
    out.append(run("spt 255, hop 4096, overlap 1024, radius 1024", 255, 7000, Keylock(ONE, 4096, 1024, 1024), t108, frames(30.5), [8, 8, 8], "music"))
    out.append(run("hop 2048, overlap 1024, noise", 800, 6000, Keylock(STEP_441, 2048, 1024, 300), frames(0.92), frames(5.5), [4, 2]))
    out.append(run("recommended setting", 800, 6000, Keylock(ONE, 1024, 256, 512), t108, frames(12.25), [3, 3], "music"))
    # radius 0: plain overlap-add, no search
    out.append(run("radius 0", 800, 4097, Keylock(ONE, 512, 16, 0), t108, frames(12.25), [2, 2], "music"))
    # every bank: pitch at the least, at and above each bank edge, at the most
    for label, p in (("least", 1 << 30), ("edge1", dc.EDGE1), ("edge1+1", dc.EDGE1 + 1), ("2", 2 * ONE), ("2+1", 2 * ONE + 1), ("most", 4 * ONE)):
        out.append(run(f"pitch {label}", 257, 4097, Keylock(p, 256, 32, 5), ONE, frames(300.37), [2, 1]))
    # the constructed tracks: all D equal; D(-q) = D(+q) < D(0); the largest D there is
    out.append(run("silent track", 800, 4097, Keylock(ONE, 256, 64, 300), t108, frames(9.5), [2], "silent"))
    out.append(run("periodic track: a tie between -q and +q", 800, 4097, Keylock(ONE, 512, 64, 30), ONE + (ONE >> 6), frames(64), [3], "period 16"))
    out.append(run("extreme amplitudes, overlap 1024", 800, 6000, Keylock(ONE, 2048, 1024, 9), frames(1.0005), frames(3), [4, 2], "extreme"))
    # tracks and heads at the edges
    out.append(run("track shorter than the overlap", 257, 10, Keylock(ONE, 256, 16, 5), frames(0.01), frames(2.5), [2, 2]))
    out.append(run("track of one frame", 256, 1, Keylock(ONE, 256, 16, 1024), frames(0.001), frames(-0.5), [2]))
    out.append(run("head before the track", 257, 2000, Keylock(ONE, 256, 64, 40), t108, frames(-700.5), [3, 1]))
    out.append(run("head past the track", 257, 2000, Keylock(ONE, 256, 64, 40), t108, frames(1700.5), [3, 1]))
    out.append(run("far outside", 800, 2000, Keylock(ONE, 256, 64, 40), ONE, frames(2000 + 5000), [2]))
    # what moves the head: a seek mid-feed (the fade runs from the old place to the new), a loop of three frames, a slewed brake to 0 and back, backwards, a pause
    out.append(run("seek mid-feed", 257, 4097, Keylock(ONE, 256, 64, 40), t108, frames(100), [4, 4], "music", [(0, 2, None, frames(3000.5)), (1, 1, None, frames(50))]))
    out.append(run("loop of three frames", 800, 4097, Keylock(ONE, 256, 64, 40), t108, frames(1001.25), [2, 1], "music", [(0, 0, play(t108, loop=(1000, 1003)), None)]))
    out.append(run("long loop", 800, 4097, Keylock(ONE, 512, 64, 100), t108, frames(3000.125), [4, 2], "music", [(0, 0, play(t108, loop=(100, 3500)), None)]))
    out.append(run("brake to 0 and back", 257, 4097, Keylock(ONE, 256, 64, 40), ONE, frames(700), [8, 8], "music",
                   [(0, 1, play(0, slew=frames(1.0) // 900), None), (1, 2, play(ONE, slew=frames(1.0) // 900), None)]))
    out.append(run("negative step", 800, 4097, Keylock(ONE, 512, 128, 200), -t108, frames(3800.61), [3, 2], "music"))
    out.append(run("pause between playing ticks", 257, 4097, Keylock(ONE, 256, 64, 40), t108, frames(100), [5, 3], "music",
                   [(0, 2, play(t108, on=False), None), (0, 3, play(t108), None), (1, 0, play(t108, on=False), None), (1, 2, play(t108), None)]))
    # key-lock set, changed (the clock restarts), repeated, cleared (the plain deck plays on) and set again, between feeds
    a, b = Keylock(ONE, 256, 64, 40), Keylock(STEP_441, 512, 16, 300)
    out.append(KCase("set, changed, cleared", 257, 4097, [KFeed(2, ((0, play(t108), frames(40.5)),), KEEP), KFeed(3, (), a), KFeed(2, (), b), KFeed(2, (), b), KFeed(2, (), None),
                                                          KFeed(3, ((1, None, frames(900)),), a)], "music"))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def run_model(case: KCase, tables, mis=(), split=None):
    """[(samples float32, [Tick], [Grain])] per feed of the case -- its own feeds, or the same ticks regrouped into feeds of the lengths `split` (a set_keylock then goes
    before the feed that holds the tick it went before; a split must not cut a feed that calls it away from that tick)"""
    m = KeylockModel(track(case), tables, mis)
    events, calls, t0 = {}, {}, 0
    for f in case.feeds:
        for (t, p, s) in f.events:
            events[t0 + t] = (p, s)
        if f.keylock != KEEP:
            calls[t0] = f.keylock
        t0 += f.n_ticks
    lengths = split if split is not None else [f.n_ticks for f in case.feeds]
    assert sum(lengths) == t0
    out, at = [], 0
    for n in lengths:
        assert all(not at < t < at + n for t in calls), "the split cuts a set_keylock away from its tick"
        if at in calls:
            m.set_keylock(calls[at])
        for t in range(at, at + n):
            if t in events:
                m.schedule(t - at, *events[t])
        out.append(m.feed(n, case.spt))
        at += n
    return out


def fractional_pitch_phase_rows(case: KCase, results) -> set:
    """the phase rows p = (u >> 24) & 255 of every filter evaluation that reaches the track while the pitch has a fractional part (the render kernel then reads its
    rows from LDS): row 0 and row 255 are the ends of the staged bank"""
    rows, kl, t, cur, prev = set(), None, 0, None, None
    for f, (_s, recs, grains) in zip(case.feeds, results):
        if f.keylock != KEEP:
            kl, t = f.keylock, 0
        if kl is None or kl.pitch % ONE == 0:
            continue
        at = {(g.tick, g.frame): g for g in grains}
        for ti, r in enumerate(recs):
            if not r.flags & 1:
                t = 0
                continue
            for n in range(case.spt):
                m = (t + n) % kl.hop
                if m == 0:
                    prev, cur = (None if t + n == 0 else cur), at[(ti, n)].g
                us = [cur + m * kl.pitch] + ([prev + (kl.hop + m) * kl.pitch] if prev is not None and m < kl.overlap else [])
                rows |= {(u >> 24) & 255 for u in us if -16 <= u >> 32 < case.n_frames + 15}
            t += case.spt
    return rows


# ---- mx_deck_debug_last_keylock, restated from the header ----
CHUNK = dc.CHUNK


def keylock_counts(case: KCase, results) -> dict:
    """the four numbers summed over the feeds of a case: results = run_model(case, ...).  A chunk fades when a frame of it has m < overlap in a grain that has a
    previous one; it straddles when a grain starts after its first frame.  The clock is walked as the header says."""
    c = dict.fromkeys(COUNT_KEYS, 0)
    kl, t = None, 0
    for f, (_s, recs, grains) in zip(case.feeds, results):
        if f.keylock != KEEP:
            kl, t = f.keylock, 0
        if kl is None:
            continue
        t = count_feed(c, kl, t, recs, grains, case.spt)
    return c


COUNT_KEYS = ("grains_searched", "grains_unsearched", "chunks_fading", "chunks_straddling")


def count_feed(c: dict, kl: Keylock, t: int, recs, grains, spt: int) -> int:
    """adds one feed of a deck key-locked with kl to the four numbers; t is the deck's clock as the feed begins.  -> the clock after it"""
    for g in grains:
        c["grains_unsearched" if g.flags & 1 or kl.radius == 0 else "grains_searched"] += 1
    for r in recs:
        if not r.flags & 1:
            t = 0
            continue
        for n0 in range(0, spt, CHUNK):
            ts = np.arange(t + n0, t + min(n0 + CHUNK, spt))
            c["chunks_fading"] += bool(np.any((ts % kl.hop < kl.overlap) & (ts >= kl.hop)))
            c["chunks_straddling"] += bool(np.any(ts[1:] % kl.hop == 0))
        t += spt
    return t
