"""The deck's track analysis (include/mixlab_gpu.h "ANALYSIS") restated in numpy int64 and Python integers / floats: the bands, the column
records, the onsets, the autocorrelation, the beat grid and the tap tables.  Independent of the library: nothing here imports mixlab_amd.

`mis` names misreadings of the specification (MISREADINGS); the tests show that each changes a compared value on some shared case."""
from __future__ import annotations

import math
from fractions import Fraction
from typing import NamedTuple

import numpy as np

COLUMN_DTYPE = np.dtype([("smin", "<i4"), ("smax", "<i4"), ("peak", "<u4", (3,)), ("onset", "<u4"), ("energy", "<u8", (3,)), ("e", "<u8")])   # 56 bytes

MISREADINGS = ("trunc_shift", "halo_off_by_one", "pad_last_column", "onset_no_shift", "a_minus1_is_a0", "autocorr_to_n", "phase_tie_largest", "high_from_b",
               "fma_index")


class Settings(NamedTuple):
    column: int
    max_lag: int
    lo: tuple
    hi: tuple

    @property
    def taps(self):
        return len(self.lo)


class Grid(NamedTuple):
    bpm: float
    period_columns: float
    confidence: float
    first_beat_frame: int
    lag: int
    phase_column: int


ZERO_GRID = Grid(0.0, 0.0, 0.0, 0, 0, 0)


def check(a: Settings, pad: int = 0, tail=((), ())):
    """None when the settings pass the header's rules, else the rule; tail: what lo / hi hold at index taps and above"""
    C, K, L = a.column, len(a.lo), a.max_lag
    if not (64 <= C <= 4096 and C & (C - 1) == 0):
        return "column"
    if len(a.hi) != K or not (1 <= K <= 127 and K % 2 == 1):
        return "taps"
    if not 16 <= L <= 1024:
        return "max_lag"
    if pad:
        return "_pad"
    for t in tail:
        if any(t):
            return "tail"
    for t in (a.lo, a.hi):
        if sum(abs(int(c)) for c in t) > 32767:
            return "sum"
    return None


def sums(track) -> np.ndarray:
    t = np.asarray(track, np.int16).reshape(-1, 2).astype(np.int64)
    return t[:, 0] + t[:, 1]


def bands(s: np.ndarray, a: Settings, mis=()):
    """(low, mid, high) per frame, int64"""
    K = a.taps
    D = (K - 1) // 2
    before = D + 1 if "halo_off_by_one" in mis else D
    pad = np.concatenate([np.zeros(before, np.int64), s, np.zeros(K, np.int64)])
    a1 = np.correlate(pad, np.asarray(a.lo, np.int64), "valid")[:s.size]   # sum_k lo[k] s[f - D + k]
    a2 = np.correlate(pad, np.asarray(a.hi, np.int64), "valid")[:s.size]
    assert int(np.abs(a1).max(initial=0)) < 1 << 31 and int(np.abs(a2).max(initial=0)) < 1 << 31
    if "trunc_shift" in mis:
        low, b = np.sign(a1) * (np.abs(a1) >> 14), np.sign(a2) * (np.abs(a2) >> 14)
    else:
        low, b = a1 >> 14, a2 >> 14   # arithmetic: floor
    high = b if "high_from_b" in mis else s - b
    return low, b - low, high


def analyse(track, a: Settings, mis=()):
    """(columns as COLUMN_DTYPE[N], R as uint64[L]) of a track"""
    assert check(a) is None
    s = sums(track)
    n, C, L = s.size, a.column, a.max_lag
    N = -(-n // C)
    low, mid, high = bands(s, a, mis)
    at = np.arange(0, n, C)
    cols = np.zeros(N, COLUMN_DTYPE)
    cols["smin"], cols["smax"] = np.minimum.reduceat(s, at), np.maximum.reduceat(s, at)
    if "pad_last_column" in mis and n % C:
        cols["smin"][-1], cols["smax"][-1] = min(int(cols["smin"][-1]), 0), max(int(cols["smax"][-1]), 0)
    for j, band in enumerate((low, mid, high)):
        cols["peak"][:, j] = np.maximum.reduceat(np.abs(band), at)
        cols["energy"][:, j] = np.add.reduceat(band * band, at)
    e = np.add.reduceat(s * s, at)
    cols["e"] = e
    A = [math.isqrt(int(v)) for v in e]
    prev = [A[0] if "a_minus1_is_a0" in mis else 0] + A[:-1]
    shift = 0 if "onset_no_shift" in mis else 6
    o = [max(x - p, 0) >> shift for x, p in zip(A, prev)]
    cols["onset"] = o
    R = np.zeros(L, np.uint64)
    for lag in range(L):
        # "summed to N instead of N - l" needs onset[c + l] for c + l >= N.  Reading those as 0 gives the rule's own sum, so it is no misreading at all; the one that
        # an implementation can really commit -- an index taken modulo N, or a staged block re-read from its start -- wraps round: a circular autocorrelation.
        if "autocorr_to_n" in mis:
            R[lag] = sum(o[c] * o[(c + lag) % N] for c in range(N))
        else:
            R[lag] = sum(o[c] * o[c + lag] for c in range(N - lag))
    return cols, R


def tempo_lag(R, L: int, hop: int, rate: float, bpm_lo: float, bpm_hi: float):
    """mx_tempo_bpm's lag rule: (l*, d), or None with R[0] = 0 or no candidate"""
    Rf = [float(int(v)) for v in R]
    lo = max(1.0, math.ceil(60.0 * rate / (float(hop) * bpm_hi)))
    hi = min(float(L - 2), math.floor(60.0 * rate / (float(hop) * bpm_lo)))
    if Rf[0] == 0.0 or not lo <= hi:
        return None
    best = int(lo)
    for lag in range(best + 1, int(hi) + 1):
        if Rf[lag] > Rf[best]:
            best = lag
    den = Rf[best - 1] - 2.0 * Rf[best] + Rf[best + 1]
    d = 0.5 * (Rf[best - 1] - Rf[best + 1]) / den if den < 0.0 else 0.0
    return best, d


def beat_index(phi: int, k: int, P: float, mis=()) -> int:
    if "fma_index" in mis:   # one rounding: the exact k P + phi rounded to the nearest double
        return math.floor(float(Fraction(k) * Fraction(P) + phi))
    step = float(k) * P
    return math.floor(float(phi) + step)


def beatgrid(onsets, R, L: int, C: int, rate: float, bpm_lo: float, bpm_hi: float, mis=()) -> Grid:
    found = tempo_lag(R, L, C, rate, bpm_lo, bpm_hi)
    if found is None:
        return ZERO_GRID
    best, d = found
    P = float(best) + d
    if not 1.0 <= P <= float(L):
        return ZERO_GRID
    o = [int(v) for v in onsets]
    top, phase = -1, 0
    for phi in range(math.ceil(P)):
        S, k = 0, 0
        while True:
            i = beat_index(phi, k, P, mis)
            if i >= len(o):
                break
            S += o[i]
            k += 1
        if S > top or (S == top and "phase_tie_largest" in mis):
            top, phase = S, phi
    return Grid(60.0 * rate / (float(C) * P), P, float(int(R[best])) / float(int(R[0])), phase * C, best, phase)


def band_taps(rate: float, f: float, K: int):
    """one table of mx_deck_analysis_bands: (the integer taps, 16384 g_k / sum g in f64)"""
    D = (K - 1) // 2
    fc = 2.0 * f / rate
    k = np.arange(K, dtype=np.float64)
    g = fc * np.sinc(fc * (k - D)) * (0.5 - 0.5 * np.cos(2.0 * np.pi * (k + 1.0) / (K + 1.0)))
    ideal = 16384.0 * g / g.sum()
    c = [int(v) for v in np.rint(ideal)]
    c[D] += 16384 - sum(c)
    return c, ideal


def settings_bands(rate=48000.0, f_lo=200.0, f_hi=2500.0, taps=63, column=512, max_lag=256) -> Settings:
    return Settings(column, max_lag, tuple(band_taps(rate, f_lo, taps)[0]), tuple(band_taps(rate, f_hi, taps)[0]))
