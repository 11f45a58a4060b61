"""The deck's shared cases (tests/test_cpu_deck.py, tests/test_gpu_deck.py): tracks, command scripts, a seeded random command stream, and a restatement of the
kernel's launch plan (mixlab_amd/csrc/mx_deck.hpp deck_chunk_plan) that says which form every chunk of a case takes.

A case is a track length, a tick length and a list of feeds; a feed is a number of ticks and the events scheduled into it: (tick, Params or None, seek or None).
The smallest shapes at which the kernel can still go wrong: tick lengths around the chunk, tracks shorter than the filter, heads outside the track, every bank edge,
loops of a frame."""
from __future__ import annotations

import zlib
from collections import namedtuple

import numpy as np

from deck_model import LOOP, ONE, PLAY, T_BEFORE, T_LOOPING, T_PAST, T_PLAY, Params

CHUNK = 256                                    # MX_DECK_CHUNK
WINDOW = 4 * CHUNK + 32
SPTS = (1, CHUNK - 1, CHUNK, CHUNK + 1, 735, 800)
RATE_OF = {735: (44100, 60), 800: (48000, 60)}   # the two real rates; the others are spt x 60 Hz (a graph wants rate = spt x ticks per second)

Feed = namedtuple("Feed", "n_ticks events")
Case = namedtuple("Case", "name spt n_frames feeds")

EDGE1 = 4 * ONE // 3                           # the largest m with 3 m <= 4 * 2^32


def rate_of(spt: int):
    return RATE_OF.get(spt, (spt * 60, 60))


def track(case_or_name, n_frames: int | None = None) -> np.ndarray:
    """int16 (n_frames, 2), seeded by the case's name; the extremes occur"""
    name, n = (case_or_name.name, case_or_name.n_frames) if isinstance(case_or_name, Case) else (case_or_name, n_frames)
    if name.startswith(CANCEL):
        return cancelling_track(n)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    t = rng.integers(-32768, 32768, size=(n, 2), dtype=np.int64).astype(np.int16)
    t[rng.integers(0, n, size=max(1, n // 64))] = (-32768, 32767)
    return t


CANCEL, CANCEL_POS = "cancelling taps", (100 << 32) | (3 << 24) | 0x5A5A5A
_cancel = {}


def cancelling_track(n_frames: int) -> np.ndarray:
    """A track whose 32 taps around CANCEL_POS (bank 0) cancel to about 2^-39 of full scale.  16-bit samples times f32 coefficients add up almost exactly in f64, so
    on ordinary audio the ORDER of the f64 operations never reaches the f32 result; here the sum is so small that the last bits of the f64 products are its leading
    bits, and a changed order or a fused multiply-add shows.  29 taps are random, three are searched: x14 over 128 values, x15 over all,
    x16 the nearest integer to what is left."""
    if n_frames not in _cancel:
        from mixlab_amd import deck
        T = deck.deck_tables(0).astype(np.float64)
        p, w = (CANCEL_POS >> 24) & 255, (CANCEL_POS & 0xFFFFFF) * 2.0 ** -24
        c = T[p] + w * (T[p + 1] - T[p])
        rng = np.random.default_rng(99)
        x = rng.integers(-20000, 20000, size=32).astype(np.float64)
        x[14:17] = 0
        r = float(np.sum(c * x))
        x14 = np.arange(-64, 64, dtype=np.float64)[:, None] * 100.0
        x15 = np.arange(-32768, 32768, dtype=np.float64)[None, :]
        t = r + c[14] * x14 + c[15] * x15
        x16 = np.clip(np.round(-t / c[16]), -32768, 32767)
        res = np.abs(t + c[16] * x16)
        i, j = np.unravel_index(np.argmin(res), res.shape)
        x[14], x[15], x[16] = x14[i, 0], x15[0, j], x16[i, j]
        tr = np.zeros((n_frames, 2), np.int16)
        idx = CANCEL_POS >> 32
        tr[idx - 15:idx + 17, 0] = x.astype(np.int16)
        tr[idx - 15:idx + 17, 1] = -x.astype(np.int16)
        _cancel[n_frames] = tr
    return _cancel[n_frames].copy()


def play(step, slew=0, loop=None, on=True):
    return Params(int(step), int(slew), loop[0] if loop else 0, loop[1] if loop else 0, (PLAY if on else 0) | (LOOP if loop else 0))


def frames(f: float) -> int:
    return int(round(f * ONE))


def one_shot(name, spt, n_frames, params, seek, n_ticks=3):
    return Case(name, spt, n_frames, [Feed(n_ticks, [(0, params, seek)])])


def _cases():
    out = []
    # every step of the list and its negative, two chunks per tick, from a fractional position inside a 4097-frame track
    steps = {"0": 0, "1": 1, "unity": ONE, "unity+1": ONE + 1, "unity-1": ONE - 1, "0.92": frames(0.92), "1.08": frames(1.08), "edge1": EDGE1, "edge1+1": EDGE1 + 1,
             "edge2": 2 * ONE, "edge2+1": 2 * ONE + 1, "max": 4 * ONE}
    for k, s in steps.items():
        out.append(one_shot(f"step {k}", CHUNK + 1, 4097, play(s), frames(300.37)))
        if s:
            out.append(one_shot(f"step -{k}", CHUNK + 1, 4097, play(-s), frames(3800.61)))
    # transparency, and the phase that reads row P: p = 255 with w = 0xFFFFFF
    out.append(one_shot("unity from frame 0", 800, 4097, play(ONE), 0, n_ticks=6))
    out.append(one_shot("last phase standing", CHUNK, 4097, play(0), (10 << 32) | 0xFFFFFFFF, n_ticks=1))
    out.append(one_shot("last phase moving", CHUNK + 1, 4097, play(ONE), (10 << 32) | 0xFFFFFFFF, n_ticks=2))
    out.append(one_shot(CANCEL, CHUNK, 4097, play(0), CANCEL_POS, n_ticks=1))
    out.append(one_shot(CANCEL + ", creeping", CHUNK, 4097, play(1), CANCEL_POS - 100, n_ticks=1))
    # short tracks, heads outside the track
    for n in (1, 31, 33, 4097):
        out.append(one_shot(f"{n} frames from 40 before", CHUNK + 1, n, play(frames(0.92)), frames(-40.25), n_ticks=2 if n < 4097 else 1))
        out.append(one_shot(f"{n} frames backwards over the end", CHUNK - 1, n, play(-frames(1.08)), frames(n + 30.5), n_ticks=2))
    out.append(one_shot("straddles the end", 735, 4097, play(frames(1.08)), frames(4097 - 500.75), n_ticks=2))
    out.append(one_shot("far past the end", CHUNK + 1, 4097, play(ONE), frames(4097 + 5000), n_ticks=2))
    out.append(one_shot("far before the start", CHUNK + 1, 4097, play(-ONE), frames(-5000), n_ticks=2))
    out.append(one_shot("beyond the clamp, coming back", 800, 33, play(-4 * ONE), frames(33 + (1 << 20) + 777.5), n_ticks=2))
    out.append(one_shot("below the clamp", 800, 33, play(4 * ONE), -frames((1 << 20) + 777.5), n_ticks=2))
    # slews: one unit per frame; the largest, accelerating through bank edges within a tick; a brake to a standstill; a back-spin that turns round inside a chunk
    out.append(Case("slew of one unit", CHUNK + 1, 4097, [Feed(4, [(0, play(ONE), frames(100)), (1, play(ONE + 1000, slew=1), None)])]))
    out.append(Case("largest slew through the bank edges", 800, 4097, [Feed(5, [(0, play(frames(0.9)), frames(50.5)), (1, play(frames(1.3), slew=1 << 24), None),
                                                                                   (3, play(4 * ONE, slew=1 << 24), None)])]))
    out.append(Case("brake", 735, 4097, [Feed(5, [(0, play(ONE), frames(700)), (1, play(0, slew=frames(1.0) // 1500), None)])]))
    out.append(Case("back-spin", 735, 4097, [Feed(5, [(0, play(ONE), frames(2000.5)), (1, play(-2 * ONE, slew=frames(3.0) // 1000), None), (4, play(ONE, slew=1 << 24), None)])]))
    # loops: a frame long; three frames at step 4 (hundreds of wraps a tick); an edge exactly on a chunk edge; backwards; long enough to stream; set, moved, cleared by events
    out.append(one_shot("loop of one frame", CHUNK + 1, 4097, play(frames(0.37), loop=(77, 78)), frames(77.5), n_ticks=2))
    out.append(one_shot("loop of three frames at step 4", 800, 4097, play(4 * ONE, loop=(1000, 1003)), frames(1001.25), n_ticks=2))
    out.append(one_shot("loop edge on a chunk edge", 800, 4097, play(ONE, loop=(50, 100 + CHUNK)), frames(100), n_ticks=2))
    out.append(one_shot("loop backwards", 735, 4097, play(-frames(1.08), loop=(1000, 1100)), frames(1050.5), n_ticks=2))
    out.append(one_shot("long loop", 800, 4097, play(frames(1.08), loop=(100, 4000)), frames(3000.125), n_ticks=6))
    out.append(Case("loop set, moved, cleared", 735, 4097, [Feed(8, [(0, play(ONE), frames(500)), (1, play(ONE, loop=(1000, 1400)), None), (3, play(ONE, loop=(1100, 1300)), None),
                                                                      (5, play(ONE, loop=(1100, 1300)), frames(3000)), (6, play(ONE), None), (7, play(ONE), frames(20.5))])]))
    out.append(Case("loop passed over, then seek into it", 800, 4097, [Feed(4, [(0, play(4 * ONE, loop=(1000, 1003)), frames(10)), (2, None, frames(1001))])]))
    # paused, and a pause inside a feed
    out.append(Case("pause and resume", CHUNK + 1, 4097, [Feed(2, [(0, play(ONE, on=False), frames(5))]), Feed(4, [(1, play(frames(1.08)), None), (2, play(frames(1.08), on=False), None),
                                                                                                                     (3, play(frames(1.08)), None)])]))
    # every tick length: a seeded command stream of sets, seeks, schedules and loop toggles
    for spt in SPTS:
        out.append(Case(f"random stream, {spt} frames a tick", spt, 4097, random_stream(1000 + spt, 4097, n_feeds=4, max_ticks=6)))
    return out


STEP_POOL = [0, ONE, -ONE, frames(0.92), frames(1.08), -frames(1.5), EDGE1, EDGE1 + 1, 2 * ONE + 1, 4 * ONE, -4 * ONE, frames(0.5), 1]
SLEW_POOL = [0, 0, 1, 1 << 24, frames(1.0) // 2000, frames(2.0) // 600]


def draw_event(rng, n_frames: int, loop, first: bool):
    """one tick's draw of the command stream: ((Params or None, seek or None) or None for a tick without an event, the loop now set).  `first` forces an event with
    params and a seek (a deck's very first tick)"""
    r = rng.random()
    if r < 0.45 and not first:
        return None, loop
    params = seek = None
    if r < 0.85 or first:
        toggle = rng.random()
        if toggle < 0.3:
            a = int(rng.integers(0, max(1, n_frames - 1)))
            loop = (a, int(rng.integers(a + 1, min(n_frames, a + 1 + int(rng.choice([1, 3, 40, 600, 3000]))) + 1)))
        elif toggle < 0.5:
            loop = None
        slew = int(rng.choice(SLEW_POOL))
        params = play(int(rng.choice(STEP_POOL)), slew=slew, loop=loop, on=rng.random() > 0.1)
    if r >= 0.7 or first:
        where = rng.random()
        seek = frames(float(rng.uniform(-60, n_frames + 60))) if where < 0.7 else frames(float(rng.uniform(loop[0], loop[1]))) if loop else frames(n_frames + 3000.5)
    return (params, seek), loop


def random_stream(seed: int, n_frames: int, n_feeds: int, max_ticks: int) -> list:
    """feeds of 1 .. max_ticks ticks with sets, seeks, scheduled events and loop toggles at random ticks"""
    rng = np.random.default_rng(seed)
    feeds, loop = [], None
    for _f in range(n_feeds):
        n_ticks = int(rng.integers(1, max_ticks + 1))
        events = []
        for t in range(n_ticks):
            ev, loop = draw_event(rng, n_frames, loop, _f == 0 and t == 0)
            if ev is not None:
                events.append((t, *ev))
        feeds.append(Feed(n_ticks, events))
    return feeds


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def run_model(case: Case, tables, mis=(), render=True):
    """[(samples float32, [Tick])] per feed of the case"""
    from deck_model import DeckModel
    m = DeckModel(track(case), tables, mis)
    out = []
    for f in case.feeds:
        for (t, p, s) in f.events:
            m.schedule(t, p, s)
        out.append(m.feed(f.n_ticks, case.spt, render))
    return out


# ---- the launch plan, restated (mx_deck.hpp deck_chunk_plan; mx_k_deck.hip) ----
def chunk_form(t, n0: int, cnt: int) -> str:
    """'zero', 'stream' or 'gather' for frames [n0, n0 + cnt) of tick record t"""
    if not t.flags & T_PLAY or t.flags & (T_BEFORE | T_PAST):
        return "zero"
    s0, s1 = t.step + n0 * t.dstep, t.step + (n0 + cnt - 1) * t.dstep
    if (s0 < 0 < s1) or (s1 < 0 < s0):
        return "gather"
    u = lambda n: t.pos + n * t.step + t.dstep * (n * (n - 1) // 2)   # noqa: E731
    ua, ub = sorted((u(n0), u(n0 + cnt - 1)))
    shift = 0
    if t.flags & T_LOOPING:
        in_q, len_q = t.loop_in * ONE, t.loop_len * ONE
        if (ua - in_q) // len_q != (ub - in_q) // len_q:
            return "gather"
        shift = (ua - in_q) // len_q * len_q
    return "stream" if ((ub - shift) >> 32) + 16 - (((ua - shift) >> 32) - 15) + 1 <= WINDOW else "gather"


def launch_counts(recs, spt: int) -> dict:
    """mx_deck_debug_last_feed's six numbers for a feed with these records"""
    c = dict.fromkeys(("ticks_zero", "ticks_stream", "ticks_gather", "chunks_zero", "chunks_stream", "chunks_gather"), 0)
    for t in recs:
        forms = [chunk_form(t, n0, min(CHUNK, spt - n0)) for n0 in range(0, spt, CHUNK)]
        for f in forms:
            c["chunks_" + f] += 1
        c["ticks_" + ("zero" if forms[0] == "zero" else "gather" if "gather" in forms else "stream")] += 1
    return c
