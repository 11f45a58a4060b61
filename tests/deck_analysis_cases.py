"""The shared cases of the deck's track analysis (tests/test_cpu_deck_analysis.py, tests/test_gpu_deck_analysis.py): a track, the settings, and the model's result, which
is computed once per case and shared.  Tracks are generated from seeds; nothing is read from disk."""
from __future__ import annotations

import zlib
from typing import Callable, NamedTuple

import numpy as np

import deck_analysis_model as am
from deck_analysis_model import Settings

RATE, BPM_LO, BPM_HI = 48000.0, 60.0, 200.0
BANDS_63 = am.settings_bands()                                   # 200 Hz / 2.5 kHz, K = 63, C = 512, L = 256
BANDS_127 = am.settings_bands(taps=127, column=64, max_lag=16)
UNITY = ((16384,), (16384,))                                     # K = 1: low = s, mid = high = 0
EXTREME_TAPS = (520,) * 62 + (527,)                              # 63 positive taps, sum 32767


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def noise(n: int, name: str, amp: int = 32767) -> np.ndarray:
    return _rng(name).integers(-amp - 1, amp + 1, (n, 2)).astype(np.int16)


def constant(n: int, value: int) -> np.ndarray:
    return np.full((n, 2), value, np.int16)


def negative_odd(n: int, name: str) -> np.ndarray:
    """every L + R is negative and odd"""
    left = _rng(name).integers(-3000, 0, n)
    s = -2 * _rng(name + " sums").integers(0, 1500, n) - 1
    return np.stack([left, s - left], axis=1).astype(np.int16)


def clicks(seed: str = "5") -> np.ndarray:
    """20 s at 48 kHz of +-300 noise with 200-frame bursts of +-20 000 every 46 * 512 frames from frame 5000.  The bursts start in column 9 and recur every 46 columns
    exactly, so R[45] and R[47] are the noise's and the parabola's vertex lies a few millionths of a column to either side of 46, by the seed.  At or above 46 (seed "5")
    every beat of phase 9 floors into a burst column: lag 46, phase column 9.  Below 46 (seed "1") the beats of phase 9 fall one column short from the second on and
    phase 10 collects them: the rule's own answer, and a case of its own."""
    n = 20 * 48000
    t = noise(n, "clicks floor " + seed, 300)
    burst = _rng("clicks bursts " + seed)
    for f in range(5000, n - 200, 46 * 512):
        t[f:f + 200] = burst.integers(-20000, 20001, (200, 2))
    return t


def two_equal_bursts() -> np.ndarray:
    """silence but for the same 100 frames in columns 3 and 5 of 8: two equal onsets, so two phases tie for the largest sum"""
    t = np.zeros((8 * 512, 2), np.int16)
    t[3 * 512 + 40:3 * 512 + 140] = t[5 * 512 + 40:5 * 512 + 140] = noise(100, "burst", 9000)
    return t


class Case(NamedTuple):
    name: str
    build: Callable[[], np.ndarray]
    settings: Settings


def _c(name, build, settings, **kw):
    return Case(name, build, settings._replace(**kw))


CASES = [
    _c("noise, 1 frame", lambda: noise(1, "n1"), BANDS_63),
    _c("noise, 5 frames under a 126-frame halo", lambda: noise(5, "n5"), BANDS_127),
    _c("noise, 100 frames in two columns under a 126-frame halo", lambda: noise(100, "n100"), BANDS_127),
    _c("noise, C - 1 frames", lambda: noise(511, "c-1"), BANDS_63),
    _c("noise, C frames", lambda: noise(512, "c"), BANDS_63),
    _c("noise, C + 1 frames", lambda: noise(513, "c+1"), BANDS_63),
    _c("noise, 3 * 4096 + 17 frames at C = 4096", lambda: noise(3 * 4096 + 17, "4096"), BANDS_63, column=4096, max_lag=16),
    _c("noise, 5000 frames at C = 2048, K = 127", lambda: noise(5000, "2048"), BANDS_127, column=2048, max_lag=16),
    _c("noise, 2500 frames at C = 1024", lambda: noise(2500, "1024"), BANDS_63, column=1024, max_lag=16),
    _c("noise, 10 000 frames at C = 64", lambda: noise(10000, "64"), BANDS_63, column=64, max_lag=200),
    _c("noise, 3000 frames at C = 256, K = 1 unity taps", lambda: noise(3000, "unity"), Settings(256, 16, *UNITY)),
    _c("constant track under band tables", lambda: constant(4000, 1000), BANDS_63),
    _c("every sample -32768, 63 positive taps of sum 32767, C = 4096", lambda: constant(3 * 4096, -32768), Settings(4096, 16, EXTREME_TAPS, EXTREME_TAPS)),
    _c("negative odd sums, K = 1 taps 8192 / 12288", lambda: negative_odd(2000, "odd"), Settings(128, 16, (8192,), (12288,))),
    _c("click track", clicks, BANDS_63, max_lag=128),
    _c("click track, the vertex below 46", lambda: clicks("1"), BANDS_63, max_lag=128),
    _c("11 columns under max_lag 256", lambda: noise(10 * 512 + 3, "short", 2000), BANDS_63),
    _c("silence", lambda: constant(5000, 0), BANDS_63),
    _c("two equal bursts", two_equal_bursts, BANDS_63),
    _c("noise, 70 000 frames at max_lag 1024, C = 64", lambda: noise(70000, "lag 1024", 9000), BANDS_63, column=64, max_lag=1024),
]
BY_NAME = {c.name: c for c in CASES}

_tracks, _truth = {}, {}


def track(case: Case) -> np.ndarray:
    if case.name not in _tracks:
        _tracks[case.name] = case.build()
        _tracks[case.name].setflags(write=False)
    return _tracks[case.name]


def truth(case: Case):
    """(columns, R, grid) of the model, computed once"""
    if case.name not in _truth:
        cols, R = am.analyse(track(case), case.settings)
        grid = am.beatgrid(cols["onset"], R, case.settings.max_lag, case.settings.column, RATE, BPM_LO, BPM_HI)
        for v in (cols, R):
            v.setflags(write=False)
        _truth[case.name] = (cols, R, grid)
    return _truth[case.name]


def forms(case: Case) -> dict:
    """what mx_deck_debug_last_analysis says after this case, from the header's description of the counts"""
    n, C, K = track(case).shape[0], case.settings.column, case.settings.taps
    out = dict.fromkeys(("wgs_several_columns", "wgs_tiled_column", "short_track", "wgs_one_column"), 0)
    if n < K - 1:
        out["short_track"] = 1
    else:
        out["wgs_several_columns" if C < 1024 else "wgs_tiled_column" if C > 1024 else "wgs_one_column"] = -(-n // max(C, 1024))
    return out
