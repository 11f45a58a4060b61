"""The deck's bars and phrases, modelled from include/mixlab_gpu.h ("BARS") alone: numpy int64 for the filter and the sums, Python integers (math.isqrt for the root)
for everything a rounding could touch, the whole d matrix for the novelty, and Python integers throughout for the beats, the pick and the next line.  Independent of
the library: nothing here imports mixlab_amd.

`mis` names ONE deliberate misreading of the header (MISREADINGS); tests/test_cpu_deck_bars.py shows that each changes a compared value of the shared case that
tests/deck_bars_cases.py names for it (MISREADING_CASE there).

One misreading CANNOT be shown by any case, NOT_SHOWABLE's "clamp_after_fold" (H = max(sum n, 0) in place of sum max(n, 0)): it differs from the rule only where some
N is negative, and none ever is.  For one component, with P and F the two halves' values, sum_{a in P, b in F} |a - b| = integral of sum_a sum_b [min(a, b) <= t <
max(a, b)] dt = integral of (p (W - f) + f (W - p)) dt, where p(t), f(t) count the values of P, F at or below t; likewise the two within-sums are the integrals of
2 p (W - p) and 2 f (W - f).  So N = integral of 2 p (W - f) + 2 f (W - p) - 2 p (W - p) - 2 f (W - f) dt = 2 integral of (p - f)^2 dt >= 0 -- W^2 times the energy
distance of the two samples -- and d is a sum of six such components.  For the same reason no track can be "built so that some N is negative"; the tests assert
N >= 0 on every case and on random vectors instead, and that this misreading changes nothing."""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np

BEAT_DTYPE = np.dtype([("v", "<u4", (6,)), ("first_frame", "<u4"), ("frames", "<u4"), ("n_bar", "<i8"), ("n_phrase", "<i8")])   # 48 bytes
MAX_BEATS, MAX_FOLDS, BLOCK, TILE = 16384, 136, 4, 1024
PERIOD_MIN, PERIOD_MAX, FAR, MAX_FRAMES, MAX_SYNC_PERIOD = 2048 << 32, 1 << 49, 1 << 62, 1 << 30, 1 << 56

MISREADINGS = ("half_rounded_up",          # h = a + ((c - a + 1) >> 1): an odd beat's first half the longer one
               "lead_added",               # f(j) = (...) + lead
               "n0_strict",                # n0 the smallest j with f(j) > 0: off by one when a line falls on frame 0
               "partial_last_beat",        # a beat that starts inside the track counts, cut at n_frames
               "unordered_within",         # the two within-sums over unordered pairs
               "phrase_free_of_bar",       # the phrase phase the best of all m, not of the m = mb (mod M)
               "novelty_one_further",      # N defined up to k = n_beats - W + 1, the missing beat a zero vector
               "fold_by_grid_index")       # folded by the grid's own index n0 + k, not by k
NOT_SHOWABLE = ("clamp_after_fold",)       # H = max(sum n, 0): see above


class Beats(NamedTuple):
    first: int = 0
    period: int = 0


class Settings(NamedTuple):
    first: int
    period: int
    lo: tuple = (16384,)
    hi: tuple = (16384,)
    lead: int = 128
    M: int = 4
    Q: int = 4
    w_bar: int = 4
    w_phrase: int = 8
    max_beats: int = 0
    taps: int | None = None      # None: len(lo)
    tail: tuple = ((), ())       # what lo / hi hold at index taps and above

    @property
    def K(self):
        return len(self.lo) if self.taps is None else self.taps


class Pick(NamedTuple):
    bars: Beats = Beats()
    phrases: Beats = Beats()
    bar_phase: int = 0
    phrase_phase: int = 0
    bar_best: int = 0
    bar_sum: int = 0
    phrase_best: int = 0
    phrase_sum: int = 0


def line(s: Settings, j: int, mis=()) -> int:
    f = (s.first + j * s.period) >> 32
    return f + s.lead if "lead_added" in mis else f - s.lead


def first_index(s: Settings, mis=()) -> int:
    """n0: it does not depend on the track"""
    ok = (lambda j: line(s, j, mis) > 0) if "n0_strict" in mis else (lambda j: line(s, j, mis) >= 0)
    n0 = -(s.first // s.period)
    while ok(n0 - 1):
        n0 -= 1
    while not ok(n0):
        n0 += 1
    return n0


def beats(s: Settings, n_frames: int, mis=()):
    """(n0, n_beats) before the limit of MAX_BEATS is held"""
    n0 = first_index(s, mis)
    n = 0
    if "partial_last_beat" in mis:
        while line(s, n0 + n, mis) < n_frames:
            n += 1
    else:
        while line(s, n0 + n + 1, mis) <= n_frames:
            n += 1
            if n > (MAX_FRAMES >> 10):
                break
    if s.max_beats:
        n = min(n, s.max_beats)
    return n0, n


def check_static(s: Settings) -> str | None:
    """the rule, of those that need no track, that refuses the settings, or None"""
    if not PERIOD_MIN <= s.period <= PERIOD_MAX:
        return "period_q32"
    if abs(s.first) > FAR:
        return "first_q32"
    if not 0 <= s.lead <= 4096:
        return "lead"
    if not (1 <= s.K <= 127 and s.K % 2 == 1):
        return "taps"
    if not 2 <= s.M <= 8:
        return "beats_per_bar"
    if not 1 <= s.Q <= 16:
        return "bars_per_phrase"
    if not 1 <= s.w_bar <= 64:
        return "w_bar"
    if not 1 <= s.w_phrase <= 64:
        return "w_phrase"
    for name, t, tail in (("lo", s.lo, s.tail[0]), ("hi", s.hi, s.tail[1])):
        if any(t[s.K:]) or any(tail):
            return name
        if sum(abs(int(c)) for c in t) > 32767:
            return name
    return None


def check(s: Settings, n_frames: int) -> str | None:
    rule = check_static(s)
    if rule:
        return rule
    if not 1 <= n_frames <= MAX_FRAMES:
        return "n_frames"
    n = beats(s, n_frames)[1]
    if n == 0:
        return "no whole beat"
    if n > MAX_BEATS:
        return "16384"
    return None


def signal(track, s: Settings):
    """(low, mid, high) per frame of the track, int64 (ANALYSIS' SIGNAL)"""
    t = np.asarray(track, np.int16).reshape(-1, 2).astype(np.int64)
    x = t[:, 0] + t[:, 1]
    K = s.K
    D = (K - 1) // 2
    pad = np.concatenate([np.zeros(D, np.int64), x, np.zeros(D, np.int64)])
    a1 = np.correlate(pad, np.asarray(s.lo[:K], np.int64), "valid")   # sum_k lo[k] s[f - D + k]
    a2 = np.correlate(pad, np.asarray(s.hi[:K], np.int64), "valid")
    assert a1.size == x.size
    low, b = a1 >> 14, a2 >> 14
    return low, b - low, x - b


def novelty(d: np.ndarray, n: int, W: int, mis=()) -> list[int]:
    """N_W[0 .. n) from the (n + 1) x (n + 1) distances (row n: the zero vector a misreading reads past the last beat)"""
    N = [0] * n
    last = n - W + (1 if "novelty_one_further" in mis else 0)
    for k in range(W, min(last, n - 1) + 1):
        P, F = slice(k - W, k), slice(k, k + W)
        within = int(d[P, P].sum()) + int(d[F, F].sum())
        if "unordered_within" in mis:
            within //= 2
        N[k] = 2 * int(d[P, F].sum()) - within
    return N


def analyse(track, s: Settings, mis=()):
    """(records as BEAT_DTYPE[n_beats], the folds as a list of M + M Q integers, n0)"""
    n_frames = np.asarray(track).reshape(-1, 2).shape[0]
    n0, n = beats(s, n_frames, mis)
    assert 1 <= n <= MAX_BEATS
    bands = signal(track, s)
    recs = np.zeros(n, BEAT_DTYPE)
    v = np.zeros((n + 1, 6), np.int64)
    for k in range(n):
        a, c = line(s, n0 + k, mis), min(line(s, n0 + k + 1, mis), n_frames)
        h = a + ((c - a + 1) >> 1) if "half_rounded_up" in mis else a + ((c - a) >> 1)
        for i, band in enumerate(bands):
            v[k, i] = math.isqrt(int((band[a:h] * band[a:h]).sum()))
            v[k, 3 + i] = math.isqrt(int((band[h:c] * band[h:c]).sum()))
        recs[k]["first_frame"], recs[k]["frames"] = a, c - a
    recs["v"] = v[:n]
    d = np.abs(v[:, None, :] - v[None, :, :]).sum(axis=2)
    n_bar, n_phrase = novelty(d, n, s.w_bar, mis), novelty(d, n, s.w_phrase, mis)
    recs["n_bar"], recs["n_phrase"] = n_bar, n_phrase
    assert all(abs(x) < 1 << 44 for x in n_bar + n_phrase)
    M, MQ = s.M, s.M * s.Q
    shift = n0 if "fold_by_grid_index" in mis else 0
    if "clamp_after_fold" in mis:
        H = [max(sum(n_bar[k] for k in range(n) if (k + shift) % M == m), 0) for m in range(M)] + \
            [max(sum(n_phrase[k] for k in range(n) if (k + shift) % MQ == m), 0) for m in range(MQ)]
    else:
        H = [sum(max(n_bar[k], 0) for k in range(n) if (k + shift) % M == m) for m in range(M)] + \
            [sum(max(n_phrase[k], 0) for k in range(n) if (k + shift) % MQ == m) for m in range(MQ)]
    return recs, H, n0


def pick(H, s: Settings, mis=()) -> Pick:
    M, MQ = s.M, s.M * s.Q
    Hb, Hp = [int(x) for x in H[:M]], [int(x) for x in H[M:M + MQ]]
    if sum(Hb) == 0:
        return Pick()
    mb = Hb.index(max(Hb))
    allowed = list(range(MQ)) if "phrase_free_of_bar" in mis else list(range(mb, MQ, M))
    top = max(Hp[m] for m in allowed)
    mp = next(m for m in allowed if Hp[m] == top)
    n0 = first_index(s)
    return Pick(Beats(s.first + (n0 + mb) * s.period, M * s.period), Beats(s.first + (n0 + mp) * s.period, MQ * s.period), mb, mp, Hb[mb], sum(Hb), Hp[mp],
                sum(Hp[m] for m in allowed))


def grid_next(g: Beats, pos: int):
    """(n, line) or None where the header refuses"""
    if not 1 <= g.period <= MAX_SYNC_PERIOD or abs(pos) > FAR or abs(g.first) > FAR:
        return None
    n = -((g.first - pos) // g.period)
    if n >= 1 << 63:
        return None
    return n, g.first + n * g.period


def forms(n_frames: int, s: Settings) -> dict:
    """what mx_deck_debug_last_bars reports of an analysis with these settings"""
    n0, n = beats(s, n_frames)
    one = tiled = 0
    for k in range(n):
        a, c = line(s, n0 + k), line(s, n0 + k + 1)
        h = a + ((c - a) >> 1)
        for length in (h - a, c - h):
            if length <= TILE:
                one += 1
            else:
                tiled += 1
    defined = sum(max(0, n - 2 * W + 1) for W in (s.w_bar, s.w_phrase))
    return {"wgs_half_one_tile": one, "wgs_half_tiled": tiled, "wgs_novelty": -(-n // BLOCK), "novelties_defined": defined}
