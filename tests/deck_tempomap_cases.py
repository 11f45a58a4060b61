"""The shared cases of the deck's tempo map (tests/test_cpu_deck_tempomap.py, tests/test_gpu_deck_tempomap.py): a track, the settings, and the model's result, which is
computed once per case and shared.  Tracks are generated from seeds; nothing is read from disk.  No track is longer than 300 000 frames."""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

import deck_finegrid_cases as fc
import deck_finegrid_model as fm
import deck_model as dm
import deck_tempomap_model as tm
from deck_finegrid_cases import _rng, bumpy, constant, noise
from deck_tempomap_model import Q16, Settings

RATE, COLUMN = fc.RATE, fc.COLUMN


def _p(h: float) -> int:
    return round(h * Q16)


def silent_middle() -> np.ndarray:
    """300 hops of 16 frames of bumpy noise with the hops [118, 182) digital silence: the window [120, 180) of five of 60 hops is silent, tooth weights included"""
    t = bumpy(4800, "silent middle", 200).copy()
    t[118 * 16:182 * 16] = 0
    return t


def phase_tie() -> np.ndarray:
    """fc.two_equal_bursts (40 hops of 16: the same burst in hops 7 and 9) and 40 hops of silence behind it"""
    return np.concatenate([fc.two_equal_bursts(), np.zeros((640, 2), np.int16)])


def index_tie() -> np.ndarray:
    """fc.periodic_bursts (the same burst every 10 hops of 16 exactly) and a second copy behind it"""
    return np.concatenate([fc.periodic_bursts(), fc.periodic_bursts()])


class Case(NamedTuple):
    name: str
    build: Callable[[], np.ndarray]
    settings: Settings


CASES = [
    Case("a 1-frame track", lambda: noise(1, "tm n1"), Settings(16, 3, _p(4), 7, 10, 3)),
    Case("N < W", lambda: bumpy(30 * 16 - 5, "tm n<w", 70), Settings(16, 4, _p(6.3), 2 * Q16, 40, 7)),
    Case("N = W", lambda: bumpy(40 * 16, "tm n=w", 70), Settings(16, 4, _p(6.3), 2 * Q16, 40, 7)),
    Case("N = W + 1", lambda: bumpy(41 * 16 - 3, "tm n=w+1", 70), Settings(16, 4, _p(6.3), 2 * Q16, 40, 7)),
    Case("T = W: no overlap, and a last window one hop long", lambda: bumpy(97 * 16, "tm t=w", 90), Settings(16, 9, _p(7.7), 0x3001, 32, 32)),
    Case("T = 1 with W = 8 on 40 hops, n_periods 1", lambda: bumpy(40 * 16, "tm t=1", 50), Settings(16, 1, _p(4), 0, 8, 1)),
    Case("a last window shorter than ceil(P)", lambda: bumpy(129 * 32 - 7, "tm short last", 300), Settings(32, 5, _p(20.5), 1234, 64, 60)),
    Case("256 and 257 phases", lambda: bumpy(30000, "tm lanes", 2500), Settings(16, 3, tm.LANES * Q16 - 1, 1, 600, 500)),
    Case("several strides of phases", lambda: bumpy(30000, "tm strides", 2500), Settings(16, 2, _p(2.5 * tm.LANES) + 77, _p(0.75 * tm.LANES), 1700, 100)),
    Case("dperiod 1, 40 periods", lambda: bumpy(20000, "tm d1", 1100), Settings(32, 40, _p(33.3), 1, 80, 33)),
    Case("W at the cap with h = 16", lambda: bumpy(300000, "tm cap", 9000), Settings(16, 9, _p(8000), 3000, tm.MAX_WINDOW, 1000)),
    Case("the longest window that is staged", lambda: bumpy(300000, "tm cap", 9000), Settings(16, 3, _p(99.3), 40000, tm.STAGED_MAX, 9000)),
    Case("one hop longer: read from memory", lambda: bumpy(300000, "tm cap", 9000), Settings(16, 3, _p(99.3), 40000, tm.STAGED_MAX + 1, 9000)),
    Case("V x n_periods = 2^20", lambda: bumpy(1033 * 16, "tm 2^20", 60), Settings(16, 1024, _p(4), 1, 10, 1)),
    Case("silence", lambda: constant(5000, 0), Settings(32, 5, _p(11), 3000, 30, 11)),
    Case("one silent window between loud ones", silent_middle, Settings(16, 10, _p(9.1), 4000, 60, 60)),
    Case("a phase tie inside one window", phase_tie, Settings(16, 3, _p(5), _p(1), 40, 20)),
    Case("an index tie inside one window", index_tie, Settings(16, 3, _p(10) - 1, 1, 88, 44)),
    Case("every sample -32768 at h = 256", lambda: constant(6 * 256 + 100, -32768), Settings(256, 2, _p(4), _p(1.5), 12, 3)),
]
BY_NAME = {c.name: c for c in CASES}
ONE_PAST = (1034 * 16, BY_NAME["V x n_periods = 2^20"].settings)   # one more hop, one more window: refused

_tracks, _truth = {}, {}


def track(case: Case) -> np.ndarray:
    if case.name not in _tracks:
        _tracks[case.name] = case.build()
        _tracks[case.name].setflags(write=False)
    return _tracks[case.name]


def truth(case: Case):
    """(records [v][j] of (score, phase, beats), w) of the model, computed once"""
    if case.name not in _truth:
        recs, w = tm.analyse(track(case), case.settings)
        w.setflags(write=False)
        _truth[case.name] = (recs, w)
    return _truth[case.name]


def flat(recs) -> list:
    return [r for row in recs for r in row]


def forms(case: Case) -> dict:
    return tm.forms(track(case).shape[0], case.settings)


# ---- the property that makes the feature worth having: three click tracks whose tempo is not constant ----
HOP, N_FRAMES, BURST, WINDOW_BEATS, STRIDE_BEATS, WIDTH = 16, 96000, 12, 8, 4, 0.10


class Drift(NamedTuple):
    name: str
    starts: tuple          # the first frame of every burst that sounds
    dp_per_beat: float     # the change of the period from one beat to the next, in frames (the ramp's slope)
    mean_period: float


def _starts(periods, t0=500.0):
    at, out = t0, []
    for p in list(periods) + [0.0]:
        out.append(round(at))
        at += p
    return out


def _drifts():
    ramp = _starts(1900.0 + 300.0 * i / 45.0 for i in range(46))                       # 47 clicks, the period ramping 1900 -> 2200 frames
    step = _starts([2000.37] * 23 + [2140.9] * 23)                                       # 47 clicks, one tempo change in the middle
    slow = [f for f in _starts(2000.0 + 60.0 * i / 45.0 for i in range(46)) if not 32000 - BURST < f < 64000]   # a slow ramp, 32 000 frames of silence in it
    return [Drift("ramp", tuple(ramp), 300.0 / 45.0, 2050.0), Drift("step", tuple(step), 0.0, 2070.0), Drift("gap", tuple(slow), 60.0 / 45.0, 2030.0)]


DRIFTS = _drifts()
DRIFT_BY_NAME = {d.name: d for d in DRIFTS}
_drift_tracks, _drift_maps = {}, {}


def drift_track(d: Drift) -> np.ndarray:
    """+-40 noise with a burst of 12 frames at 15 000 .. 20 000 at every start; the gap track's frames [32 000, 64 000) are digital silence"""
    if d.name not in _drift_tracks:
        t = noise(N_FRAMES, f"drift floor {d.name}", 40)
        burst = _rng(f"drift bursts {d.name}")
        if d.name == "gap":
            t[32000:64000] = 0
        for f in d.starts:
            t[f:f + BURST] = burst.integers(15000, 20001, (BURST, 2))
        t.setflags(write=False)
        _drift_tracks[d.name] = t
    return _drift_tracks[d.name]


def whole_track_pick(d: Drift) -> fm.Pick:
    """FINE GRID's two stages from a coarse period 0.4 % off the track's mean"""
    return fm.refine(drift_track(d), d.mean_period / COLUMN * fc.COARSE_OFF, COLUMN, RATE, HOP)[0]


def drift_map(d: Drift):
    """(segments, Settings, records, path, whole-track Pick) of the model, computed once"""
    if d.name not in _drift_maps:
        pick = whole_track_pick(d)
        _drift_maps[d.name] = tm.map_tempo(drift_track(d), pick.grid.period, HOP, WINDOW_BEATS, STRIDE_BEATS, WIDTH) + (pick,)
    return _drift_maps[d.name]


def misses(d: Drift, lines) -> list[int]:
    """per burst, the distance in hops between its hop and the hop of the nearest of `lines` (Q32 positions: tooth centres)"""
    hops = np.array([b >> 32 for b in lines], np.int64) // HOP
    return [int(np.abs(hops - f // HOP).min()) for f in d.starts]


# ---- warp: the ramp played to a constant output period ----
WARP_SPT, WARP_TICKS, WARP_FEED = 800, 56, 8
WARP_OUT_PERIOD = 2050 << 32


def warp_events(segs, out_period: int, head: dm.Head, n_frames: int, n_ticks: int, spt: int, p: dm.Params | None = None, seek: int | None = None):
    """Deck.schedule_warp's rule on the deck model's state machine: {tick: (Params or None, seek or None)} of one feed, and [(tick, segment, step)] of its step changes"""
    sched, out = {}, []
    for k in range(n_ticks):
        base = p if k == 0 and p is not None else None
        sk = seek if k == 0 else None
        q = base if base is not None else head.params
        (_first, period), seg = tm.at(segs, sk if sk is not None else head.pos)
        new = base
        if period > 0:
            step = tm.step(period, out_period)
            if step != q.step:
                new = q._replace(step=step)
                out.append((k, seg, step))
        if new is not None or sk is not None:
            sched[k] = (new, sk)
        _, head = dm.plan(head, new, sk, spt, n_frames)
    return sched, out


def warp_run(d: Drift, segs, tables, warped: bool = True):
    """the drift track played from frame 0 for WARP_TICKS ticks in feeds of WARP_FEED through the deck model: (output, [Tick], [(absolute tick, segment, step)]);
    warped=False: one constant step, the whole-track answer to the same target"""
    m = dm.DeckModel(drift_track(d), tables)
    outs, ticks, changes = [], [], []
    for first in range(0, WARP_TICKS, WARP_FEED):
        if warped:
            sched, ev = warp_events(segs, WARP_OUT_PERIOD, m.head, m.n_frames, WARP_FEED, WARP_SPT, dm.Params(flags=dm.PLAY) if first == 0 else None, 0 if first == 0 else None)
            for k, (p, sk) in sched.items():
                m.schedule(k, p, sk)
            changes += [(first + k, seg, st) for k, seg, st in ev]
        elif first == 0:
            m.schedule(0, dm.Params(tm.step(int(round(d.mean_period)) << 32, WARP_OUT_PERIOD), flags=dm.PLAY), 0)
        o, t = m.feed(WARP_FEED, WARP_SPT)
        outs.append(o)
        ticks += t
    return np.concatenate(outs), ticks, changes
