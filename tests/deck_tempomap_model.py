"""The deck's tempo map, modelled from include/mixlab_gpu.h ("TEMPO MAP") alone: numpy int64 for the sums, Python integers for path, segments, look-up, warp and
span.  The tooth weights are FINE GRID's (deck_finegrid_model.onsets), as the header says.

`mis` names ONE deliberate misreading of the header (MISREADINGS); tests/test_cpu_deck_tempomap.py shows that each changes a compared value of some shared case."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

from deck_finegrid_model import onsets  # noqa: F401  (ONSETS: "w is FINE GRID's tooth weight, number for number")

Q16 = 1 << 16
PERIOD_MIN, PERIOD_MAX, SPAN_PERIOD_MAX = 4 * Q16, 32768 * Q16, 8192 * Q16
MAX_WINDOW, MAX_PERIODS, MAX_RECORDS, GROUP, LANES, STAGED_MAX = 16384, 1024, 1 << 20, 8, 256, 10112
MAX_FRAMES, MAX_STEP, MAX_PERIOD_Q32, FAR, MAX_PENALTY = 1 << 30, 4 << 32, 1 << 56, 1 << 62, 1 << 40
EMPTY = 1

MISREADINGS = ("window_end_ignored", "phase_from_hop_0", "seam_without_half_period", "start_at_window_first_hop", "empty_not_inherited", "path_ties_largest",
               "penalty_squared", "step_truncated", "tie_largest_phase", "overlap_middle_rounded_up")


class Settings(NamedTuple):
    hop: int = 64
    n_periods: int = 1
    period0: int = PERIOD_MIN
    dperiod: int = 0
    window: int = 8
    stride: int = 8
    pad: int = 0


class Segment(NamedTuple):
    start: int
    first: int
    period: int
    score: int
    window: int
    flags: int


def phases(P: int) -> int:
    return (P + 65535) >> 16


def hops(n_frames: int, hop: int) -> int:
    return -(-n_frames // hop)


def windows(N: int, W: int, T: int) -> int:
    return 1 if N <= W else -(-(N - W) // T) + 1


def check(s: Settings, n_frames: int) -> str | None:
    """the rule that refuses the settings, in the header's order, or None"""
    if not (16 <= s.hop <= 256 and s.hop & (s.hop - 1) == 0):
        return "hop"
    if not 1 <= s.n_periods <= MAX_PERIODS:
        return "n_periods"
    if s.n_periods > 1 and s.dperiod < 1:
        return "dperiod"
    p_max = s.period0 + (s.n_periods - 1) * s.dperiod
    if not (PERIOD_MIN <= s.period0 <= PERIOD_MAX and p_max <= PERIOD_MAX):
        return "period"
    if not 2 * phases(p_max) <= s.window <= MAX_WINDOW:
        return "window_hops"
    if not 1 <= s.stride <= s.window:
        return "stride_hops"
    if s.pad:
        return "pad"
    if not 1 <= n_frames <= MAX_FRAMES:
        return "n_frames"
    if windows(hops(n_frames, s.hop), s.window, s.stride) * s.n_periods > MAX_RECORDS:
        return "n_periods"      # (the message names windows x n_periods)
    return None


def comb(w: np.ndarray, s: Settings, mis=()) -> list:
    """[v][j] = (score, phase, beats)"""
    N = len(w)
    V = windows(N, s.window, s.stride)
    a = np.arange(V, dtype=np.int64) * s.stride
    E = np.full(V, N, np.int64) if "window_end_ignored" in mis else np.minimum(a + s.window, N)
    cols = []
    reach = int((E - a).max())
    for j in range(s.n_periods):
        P = s.period0 + j * s.dperiod
        d, k = [], 0
        while (k * P) >> 16 < reach:   # the teeth of phase 0 in the longest window; no phase of any window has more
            d.append((k * P) >> 16)
            k += 1
        idx = a[:, None, None] + np.arange(phases(P), dtype=np.int64)[None, :, None] + np.array(d, np.int64)[None, None, :]
        ok = idx < E[:, None, None]
        S = np.where(ok, w[np.minimum(idx, N - 1)], 0).sum(axis=2)
        beats = ok.sum(axis=2)
        top = S.max(axis=1)
        hit = S == top[:, None]
        phi = hit.shape[1] - 1 - hit[:, ::-1].argmax(axis=1) if "tie_largest_phase" in mis else hit.argmax(axis=1)   # the last / the first phase that reaches the top
        cols.append(list(zip(top.tolist(), phi.tolist(), beats[np.arange(V), phi].tolist())))
    return [list(row) for row in zip(*cols)]


def analyse(track_i16: np.ndarray, s: Settings, mis=()):
    """(records [v][j], w)"""
    assert check(s, np.asarray(track_i16).reshape(-1, 2).shape[0]) is None
    w = onsets(track_i16, s.hop)
    return comb(w, s, mis), w


def path(score, penalty: int, mis=()) -> list[int] | None:
    """score[v][j] -> one index per window, or None where the header says MX_ERR_INVALID"""
    V, J = len(score), len(score[0])
    if penalty > MAX_PENALTY or V * J > MAX_RECORDS or any(x > 1 << 40 for row in score for x in row):
        return None
    dist = np.abs(np.arange(J)[:, None] - np.arange(J)[None, :]).astype(object)   # [j][i], Python integers throughout
    if "penalty_squared" in mis:
        dist = dist * dist
    D = [int(x) for x in score[0]]
    back = []
    for v in range(1, V):
        nxt, frm = [], []
        for j in range(J):
            cand = [D[i] - penalty * int(dist[j][i]) for i in range(J)]
            top = max(cand)
            at = [i for i in range(J) if cand[i] == top]
            frm.append(at[-1] if "path_ties_largest" in mis else at[0])
            nxt.append(int(score[v][j]) + top)
        D = nxt
        back.append(frm)
    j = D.index(max(D))
    out = [j]
    for frm in reversed(back):
        j = frm[j]
        out.append(j)
    return out[::-1]


def path_value(score, idx, penalty: int) -> int:
    return sum(int(score[v][j]) for v, j in enumerate(idx)) - penalty * sum(abs(a - b) for a, b in zip(idx, idx[1:]))


def grid_next(first: int, period: int, pos: int) -> int:
    """NEXT LINE of BARS: the first line at or after pos"""
    return first + -((first - pos) // period) * period


def segments(recs, s: Settings, n_frames: int, idx, mis=()) -> list[Segment]:
    V = windows(hops(n_frames, s.hop), s.window, s.stride)
    assert len(recs) == V == len(idx)
    own = []
    for v in range(V):
        score, phase, _ = recs[v][idx[v]]
        P = s.period0 + idx[v] * s.dperiod
        at = phase if "phase_from_hop_0" in mis else v * s.stride + phase
        own.append(((at * s.hop + s.hop // 2) << 32, (P * s.hop) << 16) if score else None)
    live = [g for g in own if g is not None]
    last = live[0] if live else (0, 0)
    out = []
    for v in range(V):
        score = recs[v][idx[v]][0]
        if own[v] is not None:
            last = own[v]
        grid = last if "empty_not_inherited" not in mis or own[v] is not None else (0, 0)
        if v == 0:
            start = -FAR
        else:
            half = -(-(s.window - s.stride) // 2) if "overlap_middle_rounded_up" in mis else (s.window - s.stride) // 2
            m = (v * s.stride * s.hop if "start_at_window_first_hop" in mis else (v * s.stride + half) * s.hop) << 32
            start = grid_next(grid[0], grid[1], m) if grid[1] else m
        out.append(Segment(start, grid[0], grid[1], score, v, 0 if score else EMPTY))
    return out


def at(segs, pos: int):
    """(Beats as (first, period), segment), or None where the header says MX_ERR_INVALID"""
    if not segs or abs(pos) > FAR:
        return None
    for v in range(len(segs) - 1, -1, -1):
        if segs[v].start <= pos:
            return (segs[v].first, segs[v].period), v
    return None


def div_half_even(n: int, d: int) -> int:
    q, r = divmod(n, d)
    if 2 * r > d or (2 * r == d and q & 1):
        q += 1
    return q


def step(period: int, out_period: int, mis=()) -> int | None:
    if not (1 <= period <= MAX_PERIOD_Q32 and 1 <= out_period <= MAX_PERIOD_Q32):
        return None
    q = (period << 32) // out_period if "step_truncated" in mis else div_half_even(period << 32, out_period)
    return q if q <= MAX_STEP else None


def beats(segs, end: int, mis=()) -> list[tuple[int, int]]:
    """the map's beats below `end` as (position, segment): per segment the lines b of its grid with start <= b and b + period / 2 <= the next segment's start"""
    out = []
    for v, g in enumerate(segs):
        if not g.period:
            continue
        stop = segs[v + 1].start if v + 1 < len(segs) else end
        b = grid_next(g.first, g.period, max(g.start, 0))     # (positions before the track are not listed)
        while b < end and (v + 1 == len(segs) or b + (0 if "seam_without_half_period" in mis else g.period // 2) <= stop):
            out.append((b, v))
            b += g.period
    return out


def span(centre: int, halfwidth: int, K: int, stride_beats: int, N: int, hop: int):
    """(Settings, clipped), or None where the header says MX_ERR_INVALID"""
    if not (16 <= hop <= 256 and hop & (hop - 1) == 0 and PERIOD_MIN <= centre <= SPAN_PERIOD_MAX and 1 <= N <= 1 << 26 and 1 <= K <= 4096 and 1 <= stride_beats <= 4096):
        return None
    halfwidth = min(halfwidth, PERIOD_MAX)
    d = max(1, 32768 // K)
    want = -(-halfwidth // d)
    m = min(want, 511)
    below, above = min(m, (centre - PERIOD_MIN) // d), min(m, (SPAN_PERIOD_MAX - centre) // d)
    p_max = centre + above * d
    W0 = max(-(-(K * p_max) // Q16), 2 * phases(p_max))
    W = min(W0, MAX_WINDOW)
    T0 = max(1, (stride_beats * centre) >> 16)
    T = min(T0, W)
    s = Settings(hop, below + above + 1, centre - below * d, d, W, T)
    if windows(N, W, T) * s.n_periods > MAX_RECORDS:
        return None
    return s, below < want or above < want or W < W0 or T < T0


def default_penalty(recs) -> int:
    """Deck.map_tempo's: floor(the sum of the windows' best scores / (V * n_periods))"""
    return sum(max(r[0] for r in row) for row in recs) // (len(recs) * len(recs[0]))


def map_tempo(track_i16: np.ndarray, period_q32: int, hop: int = 64, window_beats: int = 16, stride_beats: int = 8, width: float = 0.06, penalty=None):
    """Deck.map_tempo's rule: (segments, Settings, records, path)"""
    n = np.asarray(track_i16).reshape(-1, 2).shape[0]
    centre = (period_q32 >> 16) // hop
    s, _ = span(centre, int(centre * width), window_beats, stride_beats, hops(n, hop), hop)
    recs, _w = analyse(track_i16, s)
    idx = path([[r[0] for r in row] for row in recs], default_penalty(recs) if penalty is None else penalty)
    return segments(recs, s, n, idx), s, recs, idx


def staged(n_frames: int, s: Settings) -> bool:
    """the rule between the two forms of the comb kernel (the header's DEBUG comment)"""
    return s.n_periods >= 2 and min(s.window, hops(n_frames, s.hop)) <= STAGED_MAX


def forms(n_frames: int, s: Settings) -> dict:
    """what mx_deck_debug_last_tempomap says after these settings, from the header's description of the counts"""
    N = hops(n_frames, s.hop)
    wgs, lds = windows(N, s.window, s.stride) * -(-s.n_periods // GROUP), staged(n_frames, s)
    return {"wgs_staged": wgs if lds else 0, "wgs_global": 0 if lds else wgs, "wgs_onset": -(-N // 256), "trip": -(-(min(s.window, N) << 16) // s.period0)}
