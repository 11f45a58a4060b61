"""The deck's reverb, modelled from include/mixlab_gpu.h ("REVERB") alone: the clock, the schedule, the ramps and on / off in Python, the samples in numpy f64 with
numpy's casts to f32, one operation per statement in the header's order and association.  A pass over what the deck, the filter and the echo left in the port
(tests/deck_model.py, tests/deck_keylock_model.py, tests/deck_filter_model.py, tests/deck_echo_model.py), tick by tick, that carries the clock and the twelve lines
between calls.  Composed after tests/deck_echo_model.py: the lines here are the whole history of every r_i and q_j, not rings -- a ring that wrapped wrongly would
show -- and lines() lays the specified slots out as the rings of MEMORY for the comparison with mx_deck_read_reverb_lines and mx_deck_reverb_host.

A tick is computed in pieces of at most R frames (R the reach of BLOCKS), each piece as numpy f64 arrays over its frames: no frame of a piece reads what the piece
writes, so each frame's value is the scalar formula's, whatever the cut.  cut() restates BLOCKS for the comparison with mx_deck_reverb_plan.

`mis` names ONE deliberate misreading of the header (MISREADINGS); tests/test_cpu_deck_reverb.py shows that each changes a compared sample or line value of the case
named for it in SHOWN_BY (tests/deck_reverb_cases.py), so those cases tell the model -- and the kernel that must equal it bit for bit -- from every one of them.  One
more misreading, the reverb ahead of the echo, lives where the models meet (deck_reverb_cases.run_model, `reverb_first`).

Two misreadings the issue lists are NOT here, because no f32 sample or line value can show them on input a deck can write.  The damping taps summed in another
order: b r0, a rm and a rp are exact in f64 (a and b come from an f32 damp and carry at most 26 bits, r is an f32), so the two orders differ by one f64 rounding of
the sum, 2^-53 of its size; that reaches the f32 line value or port sample only where m + e (or dry x + wet o) lies within 2^-29 of its size of an f32 rounding
edge, which deck input cannot be tuned to.  The scale before the butterflies: the same -- (h C) summed and (sum h) C differ by a few f64 roundings.  The build pins
both all the same (-ffp-contract=off; the order is written out in mx_deck_reverb.hpp reverb_frame, which the kernel and mx_deck_reverb_host share).  `C as an f32`
IS here: an f32 C is off by 2^-26 of itself, a quarter of an f32 ulp of m, and moves line values."""
from __future__ import annotations

import math
from collections import namedtuple

import numpy as np

MIN_DELAY, MAX_DELAY, MIN_DIFF, MAX_DIFF = 128, 12000, 64, 2000
TANK_RING, DIFF_RING = 16384, 4096
LINE_FLOATS = 8 * TANK_RING + 4 * DIFF_RING
C_MIX = np.float64(float.fromhex("0x1.6a09e667f3bcdp-2"))
Reverb = namedtuple("Reverb", "delay diff gain send dry wet damp diffusion flags", defaults=(1.0, 1.0, 0.5, 0.0, 0.5, 0))
OFF = "off"
ZERO = Reverb((0,) * 8, (0,) * 4, (0.0,) * 8, 0.0, 0.0, 0.0, 0.0, 0.0, 0)

MISREADINGS = ("ramp_n_plus_1", "ramp_f64", "v_for_w", "diffusers_other_order", "diffusers_lr_swapped", "hadamard_in_place", "c_f32", "even_odd_swapped",
               "output_after_gain", "seek_clears", "feed_clears", "clock_stops", "delays_at_tick_end", "no_fade_in")

BASE, DBASE = (1087, 1283, 1447, 1663, 1871, 2053, 2281, 2477), (229, 613, 241, 587)


def check(r: Reverb) -> str | None:
    """the rule that refuses r, or None"""
    if len(r.delay) != 8 or not all(MIN_DELAY <= d <= MAX_DELAY for d in r.delay):
        return "delay"
    if len(r.diff) != 4 or not all(MIN_DIFF <= d <= MAX_DIFF for d in r.diff):
        return "diff"
    f = [np.float32(v) for v in (*r.gain, r.send, r.dry, r.wet, r.damp, r.diffusion)]
    if not all(np.isfinite(v) for v in f):
        return "finite"
    if any(abs(v) > 1 for v in f[:8]):
        return "gain"
    if abs(f[8]) > 1:
        return "send"
    if abs(f[9]) > 1:
        return "dry"
    if abs(f[10]) > 4:
        return "wet"
    if not 0 <= f[11] <= 1:
        return "damp"
    if not 0 <= f[12] <= np.float32(0.75):
        return "diffusion"
    if r.flags:
        return "flags"
    return None


def is_prime(p: int) -> bool:
    return p >= 2 and all(p % d for d in range(2, math.isqrt(p) + 1))


def prime_from(x: int) -> int:
    p = max(2, x)
    while not is_prime(p):
        p += 1
    return p


def design(rate, size, t60, damp, diffusion, send, dry, wet) -> Reverb | None:
    """mx_deck_reverb_design restated: the header's rule in Python floats (f64) and integers; None where the header refuses"""
    vals = (rate, size, t60, damp, diffusion, send, dry, wet)
    if not all(math.isfinite(v) for v in vals) or not rate > 0 or not t60 > 0 or not 0.25 <= size <= 4.0:
        return None
    delays, gains, diffs = [], [], []
    for b in BASE:
        want = math.floor(float(b) * size * rate / 48000.0 + 0.5)
        if want > MAX_DELAY:
            return None
        p = prime_from(int(want))
        while p in delays:
            p = prime_from(p + 1)
        if not MIN_DELAY <= p <= MAX_DELAY:
            return None
        delays.append(p)
        gains.append(float(np.float32(10.0 ** (-3.0 * float(p) / (rate * t60)))))
    for b in DBASE:
        want = math.floor(float(b) * rate / 48000.0 + 0.5)
        if want > MAX_DIFF:
            return None
        p = prime_from(int(want))
        if not MIN_DIFF <= p <= MAX_DIFF:
            return None
        diffs.append(p)
    r = Reverb(tuple(delays), tuple(diffs), tuple(gains), *(float(np.float32(v)) for v in (send, dry, wet, damp, diffusion)), 0)
    return r if check(r) is None else None


def reach(r: Reverb) -> int:
    return min(min(r.delay) - 1, min(r.diff))


def cut(spt: int, reaches) -> list:
    """BLOCKS: [(first frame, frames)] of a feed whose tick k has reach reaches[k] (0: no reverb), frames counted from the feed's first"""
    n_ticks, out, f = len(reaches), [], 0
    while f < n_ticks * spt:
        k = f // spt
        if not reaches[k]:
            f = (k + 1) * spt
            continue
        e = n_ticks * spt
        for kk in range(k, n_ticks):
            # frame g of tick kk belongs while g - R(kk) < f
            if not reaches[kk]:
                e = kk * spt
                break
            limit = f + reaches[kk]
            if limit < (kk + 1) * spt:
                e = max(kk * spt, limit)
                break
        out.append((f, e - f))
        f = e
    return out


def counts_of(spt: int, reaches) -> dict:
    """mx_deck_debug_last_reverb for one deck with these reaches"""
    if not any(reaches):
        return {"decks": 0, "blocks": 0, "blocks_crossing": 0, "largest_block": 0}
    blocks = cut(spt, reaches)
    return {"decks": 1, "blocks": len(blocks), "blocks_crossing": sum(1 for a, n in blocks if a // spt != (a + n - 1) // spt), "largest_block": max(n for _a, n in blocks)}


class ReverbModel:
    """mx_deck_set_reverb / mx_deck_schedule_reverb and the reverb pass of mx_deck_feed on the host"""

    def __init__(self, mis=()):
        assert all(m in MISREADINGS for m in mis), mis
        self.mis = mis
        self.on, self.set, self.t = False, ZERO, 0
        self.tank = np.zeros((1 << 12, 8), np.float32)    # r_i[0 .. t)
        self.dif = np.zeros((1 << 12, 4), np.float32)     # q_j[0 .. t)
        self.sched: dict[int, object] = {}
        self.last_reaches: list = []

    def schedule(self, tick: int, r):
        """r: a Reverb, or OFF"""
        assert r is OFF or check(r) is None
        self.sched[tick] = r

    def state(self):
        return self.t, self.on, self.set

    def lines(self):
        """(the rings as mx_deck_read_reverb_lines lays them out, float32 [LINE_FLOATS]; the mask of the specified slots: those of the clocks in [max(0, t - ring), t))"""
        out, mask = np.zeros(LINE_FLOATS, np.float32), np.zeros(LINE_FLOATS, bool)
        for hist, ring, n, at in ((self.tank, TANK_RING, 8, 0), (self.dif, DIFF_RING, 4, 8 * TANK_RING)):
            s = np.arange(max(0, self.t - ring), self.t)
            for i in range(n):
                out[at + i * ring + (s & (ring - 1))] = hist[s, i]
                mask[at + i * ring + (s & (ring - 1))] = True
        return out, mask

    @staticmethod
    def _read(hist: np.ndarray, i: int, s: np.ndarray) -> np.ndarray:
        """line i at the clocks s as f64, zero for s < 0"""
        out = hist[np.clip(s, 0, None), i].astype(np.float64)
        out[s < 0] = 0.0
        return out

    def _grow(self, need: int):
        if need > self.tank.shape[0]:
            cap = max(need, 2 * self.tank.shape[0])
            for name in ("tank", "dif"):
                old = getattr(self, name)
                grown = np.zeros((cap, old.shape[1]), np.float32)
                grown[:self.t] = old[:self.t]
                setattr(self, name, grown)

    def _clear(self):
        self.tank[:] = 0.0
        self.dif[:] = 0.0
        self.t = 0

    def run(self, x: np.ndarray, spt: int, seeks=(), playing=None) -> np.ndarray:
        """x: float32, n_ticks * spt * 2 interleaved, what the passes before left in the port; the port after the reverb, same shape.  seeks: the ticks at which the
        deck seeks, playing: the ticks whose PLAY flag is set (each read by one misreading only)"""
        mis = self.mis
        x = np.asarray(x, np.float32).reshape(-1, spt, 2)
        n_ticks = x.shape[0]
        assert all(k < n_ticks for k in self.sched)
        y = x.copy()
        sched, self.sched = self.sched, {}
        self.last_reaches = []
        if "feed_clears" in mis:
            self._clear()
        for k in range(n_ticks):
            ramp = False
            old = [np.float32(v) for v in (self.set.send, self.set.dry, self.set.wet, *self.set.gain)]
            prev = self.set if self.on else None
            if k in sched:
                r = sched[k]
                if r is OFF:
                    self.on = False
                else:
                    if not self.on:
                        self.t = 0
                        old = [np.float32(0.0)] * 11
                        if "no_fade_in" in mis:
                            old = [np.float32(v) for v in (r.send, r.dry, r.wet, *r.gain)]
                    self.on, self.set, ramp = True, r, True
            self.last_reaches.append(reach(self.set) if self.on else 0)
            if not self.on:
                continue
            if "seek_clears" in mis and k in seeks:
                self._clear()
            if "clock_stops" in mis and playing is not None and k not in playing:
                continue
            st = self.set
            new = [np.float32(v) for v in (st.send, st.dry, st.wet, *st.gain)]
            damp = np.float64(np.float32(st.damp))
            a = damp * 0.25
            a2 = a + a
            b = 1.0 - a2
            gd = np.float64(np.float32(st.diffusion))
            delays, diffs = st.delay, st.diff
            if "delays_at_tick_end" in mis and ramp and prev is not None:
                delays, diffs = prev.delay, prev.diff
            R =min(min(delays) - 1, min(diffs))
            self._grow(self.t + spt)
            for n0 in range(0, spt, R):
                n1 = min(spt, n0 + R)
                n = np.arange(n0, n1, dtype=np.int64)
                t = self.t + n
                if ramp:
                    w = (n + (1 if "ramp_n_plus_1" in mis else 0)).astype(np.float64) / np.float64(spt)
                    vals = []
                    for o, v in zip(old, new):
                        d = np.float64(v) - np.float64(o)
                        p = d * w
                        g = np.float64(o) + p
                        vals.append(g if "ramp_f64" in mis else g.astype(np.float32).astype(np.float64))
                else:
                    vals = [np.full(n.shape, np.float64(v)) for v in new]
                send, dry, wet, gains = vals[0], vals[1], vals[2], vals[3:]
                xs = x[k, n0:n1].astype(np.float64)
                e = []
                for c in (0, 1):
                    u = send * xs[:, c]
                    j0 = 2 * (1 - c) if "diffusers_lr_swapped" in mis else 2 * c
                    for j in ((j0 + 1, j0) if "diffusers_other_order" in mis else (j0, j0 + 1)):
                        p = self._read(self.dif, j, t - diffs[j])
                        gp = gd * p
                        v = u - gp
                        vf = v.astype(np.float32)
                        self.dif[t, j] = vf
                        wv = v if "v_for_w" in mis else vf.astype(np.float64)
                        gw = gd * wv
                        u = p + gw
                    e.append(u)
                f, h = [], []
                for i in range(8):
                    s = t - delays[i]
                    r0, rm, rp = self._read(self.tank, i, s), self._read(self.tank, i, s - 1), self._read(self.tank, i, s + 1)
                    p0 = b * r0
                    pm = a * rm
                    pp = a * rp
                    s0 = p0 + pm
                    fi = s0 + pp
                    f.append(fi)
                    h.append(gains[i] * fi)
                g_out = list(h)
                for d in (1, 2, 4):
                    for i in range(8):
                        if i & d:
                            continue
                        lo = h[i] + h[i + d]
                        hi = (lo - h[i + d]) if "hadamard_in_place" in mis else (h[i] - h[i + d])
                        h[i], h[i + d] = lo, hi
                cm = np.float64(np.float32(C_MIX)) if "c_f32" in mis else C_MIX
                for i in range(8):
                    m = h[i] * cm
                    ec = e[(i & 1) ^ 1] if "even_odd_swapped" in mis else e[i & 1]
                    self.tank[t, i] = (m + ec).astype(np.float32)
                src = g_out if "output_after_gain" in mis else f
                for c in (0, 1):
                    d0 = src[c] - src[c + 2]
                    d1 = src[c + 4] - src[c + 6]
                    sm = d0 + d1
                    o = sm * 0.5
                    px = dry * xs[:, c]
                    po = wet * o
                    y[k, n0:n1, c] = (px + po).astype(np.float32)
            self.t += spt
        return y.reshape(-1)
