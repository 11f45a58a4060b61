"""The shared cases of the deck's fine beat grid (tests/test_cpu_deck_finegrid.py, tests/test_gpu_deck_finegrid.py): a track, the settings, and the model's result, which
is computed once per case and shared.  Tracks are generated from seeds; nothing is read from disk.  No track is longer than 60 000 frames."""
from __future__ import annotations

import zlib
from typing import Callable, NamedTuple

import numpy as np

import deck_finegrid_model as fm
from deck_finegrid_model import LANES, Q16, Settings

RATE = 48000.0


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def noise(n: int, name: str, amp: int = 32767) -> np.ndarray:
    return _rng(name).integers(-amp - 1, amp + 1, (n, 2)).astype(np.int16)


def constant(n: int, value: int) -> np.ndarray:
    return np.full((n, 2), value, np.int16)


def negative_odd(n: int, name: str) -> np.ndarray:
    """every L + R is negative and odd, in bursts of changing level so that there are onsets"""
    level = 1 + (np.arange(n) // 37) % 7
    left = -_rng(name).integers(1, 400, n) * level
    s = -(2 * _rng(name + " sums").integers(0, 300, n) * level + 1)
    return np.stack([left, s - left], axis=1).astype(np.int16)


def bumpy(n: int, name: str, every: int = 5000) -> np.ndarray:
    """noise whose level changes every `every` frames: onsets all along the track, none of them periodic"""
    t = noise(n, name, 400).astype(np.int64)
    gain = _rng(name + " gain").integers(1, 60, n // every + 1)
    return (t * gain[np.arange(n) // every][:, None]).astype(np.int16)


class Clicks(NamedTuple):
    period: float     # frames, not an integer
    t0: float
    hop: int
    n: int = 60000
    length: int = 12


def click_starts(c: Clicks) -> list[int]:
    out, k = [], 0
    while round(c.t0 + k * c.period) + c.length <= c.n:
        out.append(round(c.t0 + k * c.period))
        k += 1
    return out


def clicks(c: Clicks) -> np.ndarray:
    """+-40 noise with a burst of 12 frames at 15 000 .. 20 000 starting at round(t0 + k * period)"""
    t = noise(c.n, f"clicks floor {c}", 40)
    burst = _rng(f"clicks bursts {c}")
    for f in click_starts(c):
        t[f:f + c.length] = burst.integers(15000, 20001, (c.length, 2))
    return t


CLICKS = [Clicks(2000.37, 713.2, 16), Clicks(1733.91, 40.0, 32), Clicks(3001.5, 2999.0, 64), Clicks(2222.22, 1000.0, 32)]
COARSE_OFF = 1.004   # the coarse estimate handed to the span is deliberately 0.4 % off


def click_settings(c: Clicks) -> Settings:
    centre = round(c.period / c.hop * COARSE_OFF * Q16)
    return fm.span(centre, -(-centre // 50), 0, fm.count(c.n, c.hop), c.hop)[0]


def two_equal_bursts() -> np.ndarray:
    """silence but for the same 12 frames at the start of hops 7 and 9 of 40 (h = 16): the phases that put a tooth on either collect the same sum"""
    t = np.zeros((40 * 16, 2), np.int16)
    t[7 * 16:7 * 16 + 12] = t[9 * 16:9 * 16 + 12] = noise(12, "burst", 9000)
    return t


def periodic_bursts() -> np.ndarray:
    """the same burst every 160 frames exactly (10 hops of 16), 8 of them, on silence: the candidates 10 and 10 + 1 / 65536 hops collect the same sum"""
    t = np.zeros((1400, 2), np.int16)
    b = noise(10, "periodic", 12000)
    for k in range(8):
        t[35 + 160 * k:45 + 160 * k] = b
    return t


class Case(NamedTuple):
    name: str
    build: Callable[[], np.ndarray]
    settings: Settings


def _p(hops: float) -> int:
    return round(hops * Q16)


CASES = [
    Case("noise, 1 frame", lambda: noise(1, "n1"), Settings(16, 3, _p(4), 7)),
    Case("noise, h - 1 frames", lambda: noise(63, "h-1"), Settings(64, 2, _p(4), 1)),
    Case("noise, h frames", lambda: noise(64, "h"), Settings(64, 2, _p(5.5), 3)),
    Case("noise, h + 1 frames", lambda: noise(65, "h+1"), Settings(64, 2, _p(4), Q16)),
    Case("N smaller than one period: a single tooth", lambda: bumpy(20 * 32 - 5, "single", 70), Settings(32, 4, _p(30), 2 * Q16)),
    Case("a period of exactly 4 hops", lambda: bumpy(3000, "four", 90), Settings(16, 1, _p(4), 0)),
    Case("an irregular fractional period", lambda: bumpy(9000, "irregular", 300), Settings(16, 5, 7 * Q16 + 0x6A3D, 0x1235)),
    Case("256 and 257 phases", lambda: bumpy(30000, "lanes", 2500), Settings(16, 3, LANES * Q16 - 1, 1)),
    Case("several strides of phases", lambda: bumpy(30000, "strides", 2500), Settings(16, 2, _p(2.5 * LANES) + 77, _p(0.75 * LANES))),
    Case("dperiod 1, 40 periods", lambda: bumpy(20000, "d1", 1100), Settings(32, 40, _p(33.3), 1)),
    Case("first_hop 37", lambda: bumpy(20000, "first", 1300), Settings(64, 6, _p(21.7), 4000, first_hop=37)),
    Case("first_hop the last hop", lambda: bumpy(5000, "last hop", 600), Settings(16, 2, _p(9.2), 999, first_hop=312)),
    Case("max_beats 2", lambda: bumpy(20000, "two", 900), Settings(16, 6, _p(61.3), 5000, max_beats=2)),
    Case("max_beats larger than fits", lambda: bumpy(20000, "many", 900), Settings(16, 6, _p(61.3), 5000, max_beats=1000)),
    Case("every sample -32768 at h = 256", lambda: constant(6 * 256 + 100, -32768), Settings(256, 2, _p(4), _p(1.5))),
    Case("silence", lambda: constant(5000, 0), Settings(32, 5, _p(11), 3000)),
    Case("two equal bursts: a phase tie", two_equal_bursts, Settings(16, 3, _p(5), _p(1))),
    Case("equal scores on two candidates: an index tie", periodic_bursts, Settings(16, 3, _p(10) - 1, 1)),
    Case("negative odd sums", lambda: negative_odd(7001, "odd"), Settings(32, 4, _p(12.4), 2222)),
] + [Case(f"click track {c.period} / {c.t0} / h {c.hop}", (lambda c=c: clicks(c)), click_settings(c)) for c in CLICKS]
BY_NAME = {c.name: c for c in CASES}
CLICK_CASES = [(c, BY_NAME[f"click track {c.period} / {c.t0} / h {c.hop}"]) for c in CLICKS]

_tracks, _truth = {}, {}


def track(case: Case) -> np.ndarray:
    if case.name not in _tracks:
        _tracks[case.name] = case.build()
        _tracks[case.name].setflags(write=False)
    return _tracks[case.name]


def truth(case: Case):
    """(records as abi.DECK_COMB_DTYPE-shaped tuples, w) of the model, computed once"""
    if case.name not in _truth:
        recs, w = fm.analyse(track(case), case.settings)
        w.setflags(write=False)
        _truth[case.name] = (recs, w)
    return _truth[case.name]


def forms(case: Case) -> dict:
    return fm.forms(track(case).shape[0], case.settings)


# ---- the property that makes the feature worth having ----
def grid_misses(c: Clicks, first_q32: int, period_q32: int):
    """(the largest distance in hops between a burst's hop and the nearest tooth of the grid, |P_found - P_true| (K - 1) in frames)"""
    starts = click_starts(c)
    tooth0 = (first_q32 >> 32) // c.hop                     # first_q32 is the centre of tooth 0: its hop
    P16 = period_q32 // (c.hop << 16)                       # the period in hops, Q16
    teeth = [tooth0 + ((k * P16) >> 16) for k in range(len(starts) + 2)]
    worst = max(min(abs(f // c.hop - t) for t in teeth) for f in starts)
    drift = abs(period_q32 / 2.0 ** 32 - c.period) * (len(starts) - 1)
    return worst, drift


# ---- two decks in time: a leader and a follower refined in the header's two stages, synced at tick 0 and played ----
COLUMN = 512
SYNC_SPT, SYNC_TICKS, SYNC_FEED = 800, 56, 8          # 44 800 output frames at 48 kHz in feeds of 8 ticks
SYNC_LEADER, SYNC_FOLLOWER = CLICKS[0], CLICKS[3]     # 2000.37 frames at h = 16 against 2222.22 at h = 32
SYNC_LEADER_POS, SYNC_FOLLOWER_POS = 300 << 32, 0
_pair = {}


def coarse_columns(c: Clicks) -> float:
    """what mx_deck_beatgrid would hand over, 0.4 % off"""
    return c.period / COLUMN * COARSE_OFF


def sync_pair():
    """the model's two-stage picks of both tracks and the sync of the follower to the leader playing at unity from SYNC_LEADER_POS, computed once"""
    if not _pair:
        for who, c in (("leader", SYNC_LEADER), ("follower", SYNC_FOLLOWER)):
            _pair[who] = fm.refine(track(BY_NAME[f"click track {c.period} / {c.t0} / h {c.hop}"]), coarse_columns(c), COLUMN, RATE, c.hop)
        _pair["sync"] = fm.sync(_pair["leader"][0].grid, SYNC_LEADER_POS, 1 << 32, _pair["follower"][0].grid, SYNC_FOLLOWER_POS)
    return _pair


def burst_centroids(samples: np.ndarray) -> list[float]:
    """the energy centroid, in output frames, of every burst of an interleaved stereo output: runs of |L| + |R| > 0.25 no more than 64 frames apart"""
    y = np.abs(np.asarray(samples, np.float64).reshape(-1, 2)).sum(axis=1)
    at = np.flatnonzero(y > 0.25)
    out, start = [], 0
    for k in range(1, len(at) + 1):
        if k == len(at) or at[k] - at[k - 1] > 64:
            idx = np.arange(at[start], at[k - 1] + 1)
            e = y[idx] ** 2
            out.append(float((idx * e).sum() / e.sum()))
            start = k
    return out


# ---- sync: pairs of grids, heads and steps ----
SYNC_FIXED = [
    # (leader beats, leader pos, leader step, follower beats, follower pos)
    (fm.Beats(5 << 32, 2000 << 32), 12345 << 32, 1 << 32, fm.Beats(77 << 32, 1500 << 32), 400 << 32),
    (fm.Beats(5 << 32, 2000 << 32), (5 << 32) + (1000 << 32), 1 << 32, fm.Beats(0, 1500 << 32), 0),                 # delta = +Pf / 2 exactly: it stays
    (fm.Beats(5 << 32, 2000 << 32), 5 << 32, 1 << 32, fm.Beats(0, 1500 << 32), 750 << 32),                           # delta = -Pf / 2 exactly: it folds to +Pf / 2
    (fm.Beats(5 << 32, 2000 << 32), (5 << 32) + (1900 << 32), 1 << 32, fm.Beats(0, 1500 << 32), 0),                 # delta = 1425 frames: it folds to -75
    (fm.Beats(5 << 32, 2000 << 32), (5 << 32) + (100 << 32), 1 << 32, fm.Beats(0, 1500 << 32), 1400 << 32),         # delta = -1325 frames: it folds to +175
    (fm.Beats(9000 << 32, (2000 << 32) + 12345), 100 << 32, -(3 << 31), fm.Beats(700 << 32, (2100 << 32) + 999), -(50 << 32)),   # before both first beats, backwards
    (fm.Beats(0, 3), 1, 1, fm.Beats(0, 2), 0),                                                                         # a = 1, a Pf / Pl = 2 / 3 -> 1; step 2 / 3 -> 1
    (fm.Beats(0, 4), 2, 3, fm.Beats(0, 2), 0),                                                                         # halves: step 3 / 2 -> 2, b = 1 = Pf / 2
    (fm.Beats(0, 1000 << 32), 0, 4 << 32, fm.Beats(0, 1001 << 32), 0),                                                 # the step leaves the range: refused
    (fm.Beats(0, 0), 0, 1 << 32, fm.Beats(0, 1 << 32), 0),                                                             # a period of 0: refused
]


def sync_draws(n: int = 300):
    rng = _rng("sync draws")
    out = []
    for _ in range(n):
        Pl, Pf = (int(rng.integers(1 << 38, 1 << 50)) for _ in range(2))
        if rng.random() < 0.3:
            Pf = Pl + int(rng.integers(-1 << 30, 1 << 30))
        l = fm.Beats(int(rng.integers(-1 << 45, 1 << 50)), Pl)
        f = fm.Beats(int(rng.integers(-1 << 45, 1 << 50)), Pf)
        far = 62 if rng.random() < 0.2 else 52   # positions a few beats before the first beat up to far behind it
        out.append((l, l.first + int(rng.integers(-1 << 51, 1 << far)), int(rng.integers(-(4 << 32), (4 << 32) + 1)), f, f.first + int(rng.integers(-1 << 51, 1 << far))))
    return out
