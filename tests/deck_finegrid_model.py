"""The deck's fine beat grid and sync, modelled from include/mixlab_gpu.h ("FINE GRID") alone: numpy int64 for the sums, Python integers (math.isqrt for the root) for
everything a rounding could touch, and Python integers throughout for pick, span and sync.

`mis` names ONE deliberate misreading of the header (MISREADINGS); tests/test_cpu_deck_finegrid.py shows that each changes a compared value of some shared case."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

Q16 = 1 << 16
PERIOD_MIN, PERIOD_MAX = 4 * Q16, 32768 * Q16
MAX_PERIODS, LANES = 8192, 256
MAX_FRAMES, MAX_STEP, MAX_SYNC_PERIOD, MAX_POS = 1 << 30, 4 << 32, 1 << 56, 1 << 62

MISREADINGS = ("unweighted_tooth", "round_product", "ignore_max_beats", "tie_largest_phase", "a_minus1_is_a0", "pad_short_hop", "shift_before_subtract",
               "floor_phases", "pick_last_index", "delta_not_folded", "step_truncated")


class Settings(NamedTuple):
    hop: int = 64
    n_periods: int = 1
    period0: int = PERIOD_MIN
    dperiod: int = 0
    first_hop: int = 0
    max_beats: int = 0
    pad: int = 0


class Beats(NamedTuple):
    first: int = 0
    period: int = 0


class Pick(NamedTuple):
    grid: Beats = Beats()
    score: int = 0
    bpm: float = 0.0
    index: int = 0
    n_beats: int = 0


def hop_ok(hop: int) -> bool:
    return 16 <= hop <= 256 and hop & (hop - 1) == 0


def count(n_frames: int, hop: int) -> int:
    return -(-n_frames // hop)


def check(s: Settings, n_frames: int | None) -> str | None:
    """the rule that refuses the settings, or None; n_frames None: every rule but first_hop's"""
    if not hop_ok(s.hop):
        return "hop"
    if not 1 <= s.n_periods <= MAX_PERIODS:
        return "n_periods"
    if s.n_periods > 1 and s.dperiod < 1:
        return "dperiod"
    if not (PERIOD_MIN <= s.period0 <= PERIOD_MAX and s.period0 + (s.n_periods - 1) * s.dperiod <= PERIOD_MAX):
        return "period"
    if s.max_beats == 1:
        return "max_beats"
    if s.pad:
        return "pad"
    if n_frames is not None:
        if not 1 <= n_frames <= MAX_FRAMES:
            return "n_frames"
        if s.first_hop >= count(n_frames, s.hop):
            return "first_hop"
    return None


def onsets(track_i16: np.ndarray, hop: int, mis=()) -> np.ndarray:
    """w as int64[N]"""
    x = np.asarray(track_i16, np.int16).reshape(-1, 2).astype(np.int64)
    s = x[:, 0] + x[:, 1]
    n = len(s)
    N = count(n, hop)
    sq = np.zeros(N * hop, np.int64)
    sq[:n] = s * s
    if "pad_short_hop" in mis and n % hop and N > 1:   # the short last hop filled up with the frames before it
        sq[n:] = sq[n - hop:N * hop - hop]
    e = sq.reshape(N, hop).sum(axis=1)
    A = [math.isqrt(int(v)) for v in e]
    before = [A[0] if "a_minus1_is_a0" in mis else 0] + A[:-1]
    if "shift_before_subtract" in mis:
        o = [max((a >> 4) - (b >> 4), 0) for a, b in zip(A, before)]
    else:
        o = [max(a - b, 0) >> 4 for a, b in zip(A, before)]
    o = np.array([0] + o + [0], np.int64)
    if "unweighted_tooth" in mis:
        return o[1:-1].copy()
    return o[:-2] + 2 * o[1:-1] + o[2:]


def phases(P: int, mis=()) -> int:
    return P >> 16 if "floor_phases" in mis else (P + 65535) >> 16


def comb(w: np.ndarray, s: Settings, mis=()) -> list[tuple[int, int, int]]:
    """(score, phase, beats) per candidate"""
    N = len(w)
    limit = 0 if "ignore_max_beats" in mis else s.max_beats
    half = 32768 if "round_product" in mis else 0
    out = []
    for j in range(s.n_periods):
        P = s.period0 + j * s.dperiod
        d, k = [], 0
        while (not limit or k < limit) and s.first_hop + ((k * P + half) >> 16) < N:   # the teeth of phase 0; every other phase has no more
            d.append((k * P + half) >> 16)
            k += 1
        idx = s.first_hop + np.arange(phases(P, mis), dtype=np.int64)[:, None] + np.array(d, np.int64)[None, :]
        ok = idx < N
        S = np.where(ok, w[np.minimum(idx, N - 1)], 0).sum(axis=1)
        beats = ok.sum(axis=1)
        top = int(S.max())
        hits = np.flatnonzero(S == top)
        phi = int(hits[-1] if "tie_largest_phase" in mis else hits[0])
        out.append((top, phi, int(beats[phi])))
    return out


def analyse(track_i16: np.ndarray, s: Settings, mis=()):
    """(records, w)"""
    assert check(s, np.asarray(track_i16).reshape(-1, 2).shape[0]) is None
    w = onsets(track_i16, s.hop, mis)
    return comb(w, s, mis), w


def pick(recs, s: Settings, rate: float, mis=()) -> Pick:
    assert check(s, None) is None and len(recs) == s.n_periods
    top = max(r[0] for r in recs)
    if top == 0:
        return Pick()
    js = [j for j, r in enumerate(recs) if r[0] == top]
    j = js[-1] if "pick_last_index" in mis else js[0]
    P = s.period0 + j * s.dperiod
    grid = Beats(((s.first_hop + recs[j][1]) * s.hop + s.hop // 2) << 32, (P * s.hop) << 16)
    return Pick(grid, top, (60.0 * rate * 65536.0) / (float(P) * float(s.hop)), j, recs[j][2])


def span(centre: int, halfwidth: int, B: int, N: int, hop: int):
    """(Settings, clipped)"""
    assert hop_ok(hop) and PERIOD_MIN <= centre <= PERIOD_MAX and 1 <= N <= 1 << 26 and B != 1
    halfwidth = min(halfwidth, PERIOD_MAX)
    K = -(-(N << 16) // centre)
    if B and B < K:
        K = B
    d = max(1, 32768 // K)
    want = -(-halfwidth // d)
    m = min(want, 4095)
    below, above = min(m, (centre - PERIOD_MIN) // d), min(m, (PERIOD_MAX - centre) // d)
    return Settings(hop, below + above + 1, centre - below * d, d, 0, B), below < want or above < want


def period_q16(period_columns: float, column: int, hop: int) -> int:
    """the integer nearest to period_columns * C / h * 65536, ties to even -- exactly, from the double's own fraction"""
    num, den = float(period_columns).as_integer_ratio()
    num *= column * Q16
    den *= hop
    return div_half_even(num, den)


def div_half_even(n: int, d: int) -> int:
    q, r = divmod(n, d)
    if 2 * r > d or (2 * r == d and q & 1):
        q += 1
    return q


def sync(leader: Beats, lpos: int, lstep: int, follower: Beats, fpos: int, mis=()):
    """(step, seek, delta), or None where the header says MX_ERR_INVALID"""
    Pl, Pf = leader.period, follower.period
    if not (1 <= Pl <= MAX_SYNC_PERIOD and 1 <= Pf <= MAX_SYNC_PERIOD) or any(abs(v) > MAX_POS for v in (lpos, fpos, leader.first, follower.first)):
        return None
    mag = abs(lstep) * Pf // Pl if "step_truncated" in mis else div_half_even(abs(lstep) * Pf, Pl)
    if mag > MAX_STEP:
        return None
    a = (lpos - leader.first) % Pl
    b = div_half_even(a * Pf, Pl)
    c = (fpos - follower.first) % Pf
    delta = b - c
    if "delta_not_folded" not in mis:
        while 2 * delta > Pf:
            delta -= Pf
        while 2 * delta <= -Pf:
            delta += Pf
    return (-mag if lstep < 0 else mag), fpos + delta, delta


def refine(track_i16: np.ndarray, period_columns: float, column: int, rate: float, hop: int = 64, analyse_fn=None):
    """the header's two stages from a coarse period: (Pick, Settings of stage one, Settings of stage two or None).  analyse_fn(settings) -> records replaces the
    model's own comb (the CPU test hands in the host function)."""
    run = analyse_fn if analyse_fn is not None else (lambda s: analyse(track_i16, s)[0])
    N = count(np.asarray(track_i16).reshape(-1, 2).shape[0], hop)
    centre = period_q16(period_columns, column, hop)
    one, _ = span(centre, -(-centre // 50), 64, N, hop)
    first = pick(run(one), one, rate)
    if not first.score:
        return first, one, None
    two, _ = span(one.period0 + first.index * one.dperiod, 4 * one.dperiod, 0, N, hop)
    return pick(run(two), two, rate), one, two


def forms(n_frames: int, s: Settings) -> dict:
    """what mx_deck_debug_last_finegrid says after these settings, from the header's description of the counts"""
    N = count(n_frames, s.hop)
    one = sum(1 for j in range(s.n_periods) if phases(s.period0 + j * s.dperiod) <= LANES)
    fit = -(-((N - s.first_hop) << 16) // s.period0)
    return {"wgs_one_pass": one, "wgs_strided": s.n_periods - one, "wgs_onset": -(-N // 256), "trip": min(fit, s.max_beats) if s.max_beats else fit}
