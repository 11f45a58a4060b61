"""The key-locked deck, modelled from include/mixlab_gpu.h ("KEY-LOCK") alone: clock, grain positions and the search in Python integers and int64 numpy, the grain
samples through deck_model's filter, the cross-fade in numpy f64 with every operation separate.  The tick rules, the positions and the filter are deck_model's.

`mis` names ONE deliberate misreading of the header (MISREADINGS); tests/test_cpu_deck_keylock.py shows that each changes a sample or a grain record of the shared
cases (tests/deck_keylock_cases.py)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import deck_model as dm
from deck_model import ONE, T_LOOPING, T_PLAY, Tick

Keylock = namedtuple("Keylock", "pitch hop overlap radius", defaults=(ONE, 1024, 256, 512))
Grain = namedtuple("Grain", "a g tick frame delta dist flags")
G_FIRST = 1

MISREADINGS = ("ref_at_a", "frac_from_a", "tie_positive", "tie_first_scanned", "compare_hop", "half_open", "left_only", "squared", "a_unfolded",
               "fade_m_plus_1", "fade_swapped", "old_without_hop", "fade_f32", "no_restart_after_pause", "restart_per_feed", "bank_from_step")


def check(k: Keylock) -> str | None:
    """the rule that refuses k, or None"""
    pow2 = lambda v: v > 0 and v & (v - 1) == 0   # noqa: E731
    if not (1 << 30) <= k.pitch <= 4 * ONE:
        return "pitch"
    if not (pow2(k.hop) and 256 <= k.hop <= 8192):
        return "hop"
    if not (pow2(k.overlap) and 16 <= k.overlap <= min(k.hop // 2, 1024)):
        return "overlap"
    if not 0 <= k.radius <= 1024:
        return "radius"
    return None


def sums(track_i16: np.ndarray, mis=()) -> np.ndarray:
    """s[f] = L[f] + R[f], int64"""
    t = np.asarray(track_i16, np.int16).reshape(-1, 2).astype(np.int64)
    return t[:, 0] if "left_only" in mis else t[:, 0] + t[:, 1]


def span(s: np.ndarray, lo: int, n: int) -> np.ndarray:
    """s[lo .. lo + n), 0 outside the track"""
    out = np.zeros(n, np.int64)
    a, b = max(lo, 0), min(lo + n, len(s))
    if a < b:
        out[a - lo:b - lo] = s[a:b]
    return out


def search(s: np.ndarray, C: int, A: int, V: int, R: int, mis=()) -> tuple[int, int]:
    """(delta, dist) of the header's POSITION rule"""
    ref = span(s, C, V)
    hi = R - 1 if "half_open" in mis and R else R
    win = np.lib.stride_tricks.sliding_window_view(span(s, A - R, V + R + hi), V)   # row e: delta = e - R
    diff = win - ref[None, :]
    D = (diff * diff).sum(axis=1) if "squared" in mis else np.abs(diff).sum(axis=1)
    deltas = np.arange(-R, hi + 1)
    if "tie_first_scanned" in mis:
        e = int(np.argmin(D))
    else:
        tie = 2 * np.abs(deltas) + ((deltas < 0) if "tie_positive" in mis else (deltas > 0))
        e = int(np.lexsort((tie, D))[0])
    return int(deltas[e]), int(D[e])


def grains_of(x: np.ndarray, g: int, m0: int, cnt: int, p: int, bank: int, tables) -> np.ndarray:
    """float32 (cnt, 2): G(m0 .. m0 + cnt) of the grain at g -- the deck's filter at g + m p, never folded"""
    return dm.render_tick(x, Tick(g + m0 * p, p, 0, 0, 0, T_PLAY, bank), cnt, tables)


class KeylockModel:
    """mx_deck_* with mx_deck_set_keylock: feed() returns what mx_deck_feed writes, the tick records and the grain records"""

    def __init__(self, track_i16: np.ndarray, tables, mis=()):
        self.deck = dm.DeckModel(track_i16, tables)
        self.tables, self.mis = tables, mis
        self.s = sums(self.deck.track, mis)
        self.kl = None
        self.t, self.cur, self.prev, self.graph = 0, None, None, None   # the clock; g of the current grain and of the one before it (None: it has none)

    def set_keylock(self, k: Keylock | None):
        assert k is None or check(k) is None
        self.kl, self.t = k, 0

    def schedule(self, tick, params=None, seek=None):
        self.deck.schedule(tick, params, seek)

    def load(self, first_frame: int, interleaved_i16):
        self.deck.load(first_frame, interleaved_i16)
        self.s = sums(self.deck.track, self.mis)

    def feed(self, n_ticks: int, spt: int, graph=0):
        """(float32 [n_ticks * spt * 2], [Tick], [Grain])"""
        d, k, mis = self.deck, self.kl, self.mis
        if k is None:
            self.graph = graph
            return (*d.feed(n_ticks, spt), [])
        assert all(t < n_ticks for t in d.sched)
        if graph != self.graph or "restart_per_feed" in mis:
            self.t = 0
        self.graph = graph
        H, V, R, p = k.hop, k.overlap, k.radius, k.pitch
        out, recs, grains = np.zeros((n_ticks, spt, 2), np.float32), [], []
        for ti in range(n_ticks):
            params, seek = d.sched.get(ti, (None, None))
            tick, d.head = dm.plan(d.head, params, seek, spt, d.n_frames)
            recs.append(tick)
            if not tick.flags & T_PLAY:
                if "no_restart_after_pause" not in mis:
                    self.t = 0
                continue
            bank = tick.bank if "bank_from_step" in mis else dm.bank_of(p)
            us = dm.positions(tick._replace(flags=tick.flags & ~T_LOOPING) if "a_unfolded" in mis else tick, spt)
            n = 0
            while n < spt:
                m = (self.t + n) % H
                if m == 0:                                   # grain j starts at this frame
                    a = us[n]
                    if self.t + n == 0:
                        self.prev, self.cur = None, a
                        grains.append(Grain(a, a, ti, n, 0, 0, G_FIRST))
                    else:
                        c = self.cur + H * p
                        C, A = c >> 32, a >> 32
                        delta, dist = (0, 0) if R == 0 else search(self.s, A if "ref_at_a" in mis else C, A, H if "compare_hop" in mis else V, R, mis)
                        g = (A + delta) * ONE + ((a if "frac_from_a" in mis else c) & (ONE - 1))
                        self.prev, self.cur = self.cur, g
                        grains.append(Grain(a, g, ti, n, delta, dist, 0))
                cnt = min(spt - n, H - m)                    # the frames of this tick that lie in the current grain
                y = grains_of(d.x, self.cur, m, cnt, p, bank, self.tables)
                if self.prev is not None and m < V:
                    nf = min(cnt, V - m)
                    old = grains_of(d.x, self.prev, (0 if "old_without_hop" in mis else H) + m, nf, p, bank, self.tables)
                    ms = np.arange(m, m + nf, dtype=np.float64) + (1.0 if "fade_m_plus_1" in mis else 0.0)
                    if "fade_f32" in mis:
                        w = (ms / float(V)).astype(np.float32)[:, None]
                        y[:nf] = old + w * (y[:nf] - old)
                    else:
                        w = (ms / float(V))[:, None]
                        a64, b64 = old.astype(np.float64), y[:nf].astype(np.float64)
                        if "fade_swapped" in mis:
                            a64, b64 = b64, a64
                        y[:nf] = (a64 + w * (b64 - a64)).astype(np.float32)
                out[ti, n:n + cnt] = y
                n += cnt
            self.t += spt
        d.sched = {}
        return out.reshape(-1), recs, grains
