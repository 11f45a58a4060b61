"""The deck's beat echo, modelled from include/mixlab_gpu.h ("ECHO") alone: the clock, the schedule and the ramps in Python integers, the samples in numpy f64 with
numpy's casts to f32, in the header's order.  A pass over what the deck wrote (tests/deck_model.py, tests/deck_keylock_model.py), tick by tick, that carries the clock
and the line between calls.  The line here is the whole history of r, not a ring: a ring that wrapped wrongly would show.

`mis` names ONE deliberate misreading of the header (MISREADINGS); tests/test_cpu_deck_echo.py shows that each changes a compared sample of the shared cases
(tests/deck_echo_cases.py), so those cases tell the model -- and the kernel that must equal it bit for bit -- from every one of them.

Two misreadings the issue lists are NOT here, because no f32 sample can show them on input a deck can write.  A fused multiply-add: send * x and the three tap products
are exact in f64 (24-bit factors), so only fb * f and wet * f round, and fusing them moves the f64 sum by half an ulp at the most -- it reaches the f32 result only when
the sum lies within 2^-29 of its size of an f32 rounding edge, or when x and wet * f cancel to 30 bits, which x cannot be tuned to.  The tap sum in another order: the
same, the three exact products differ from their sum by one f64 rounding.  The build pins both all the same (-ffp-contract=off; the order is written out in the kernel)."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

PINGPONG, MIN_DELAY, MAX_DELAY = 1, 256, 262144
Echo = namedtuple("Echo", "delay send feedback wet damp flags", defaults=(1.0, 0.5, 1.0, 0.0, 0))
OFF = "off"

MISREADINGS = ("r_from_y", "ramp_n_plus_1", "ramp_f32", "delay_from_tick_start", "pingpong_crosses_x", "seek_restarts", "line_kept_off_on", "block_plus_one")
# two more that only a feed of several ticks can show, switched on by the random deck sessions (tests/random_decks.py) alone: the ramp weight running over the whole
# feed instead of the tick, and a feed of several blocks that reads the line as it stood before the feed (what it wrote itself reads as zero)
FEED_MISREADINGS = ("ramp_over_feed", "walk_as_one_block")


def check(e: Echo) -> str | None:
    """the rule that refuses e, or None"""
    if not MIN_DELAY <= e.delay <= MAX_DELAY:
        return "delay"
    g = [np.float32(v) for v in (e.send, e.feedback, e.wet, e.damp)]
    if not all(np.isfinite(v) for v in g):
        return "finite"
    if abs(g[0]) > 1:
        return "send"
    if abs(g[1]) > 1:
        return "feedback"
    if abs(g[2]) > 4:
        return "wet"
    if not 0 <= g[3] <= 1:
        return "damp"
    if e.flags & ~PINGPONG:
        return "flags"
    return None


def echo_delay(period_q32: int, step_q32: int, num: int, den: int) -> int | None:
    """the integer nearest to period * num / (|step| * den), ties to even, in Python integers; None where the header refuses"""
    if not step_q32 or not num or not den or period_q32 <= 0:
        return None
    n, d = period_q32 * num, abs(step_q32) * den
    q, r = divmod(n, d)
    if 2 * r > d or (2 * r == d and q & 1):
        q += 1
    return q if MIN_DELAY <= q <= MAX_DELAY else None


def cut(spt: int, delays, mis=()) -> list:
    """BLOCKS: [(first frame, frames)] of a feed whose tick k has delays[k] (0: no echo), frames counted from the feed's first"""
    slack = 0 if "block_plus_one" in mis else 1
    n_ticks, out, f = len(delays), [], 0
    while f < n_ticks * spt:
        k = f // spt
        if not delays[k]:
            f = (k + 1) * spt
            continue
        e = n_ticks * spt
        for kk in range(k, n_ticks):
            # frame g of tick kk belongs while g - D + 1 < f
            if not delays[kk]:
                e = kk * spt
                break
            limit = f + delays[kk] - slack
            if limit < (kk + 1) * spt:
                e = max(kk * spt, limit)
                break
        out.append((f, e - f))
        f = e
    return out


class EchoModel:
    """mx_deck_set_echo / mx_deck_schedule_echo and the echo pass of mx_deck_feed on the host"""

    def __init__(self, mis=()):
        assert all(m in MISREADINGS + FEED_MISREADINGS for m in mis), mis
        self.mis = mis
        self.on, self.set, self.t = False, Echo(0, 0.0, 0.0, 0.0, 0.0, 0), 0
        self.hist = np.zeros((1 << 12, 2), np.float32)   # r[0 .. t)
        self.sched: dict[int, object] = {}
        self.stale_from = None                           # walk_as_one_block: the clock from which the line reads as zero

    def schedule(self, tick: int, e):
        """e: an Echo, or OFF"""
        assert e is OFF or check(e) is None
        self.sched[tick] = e

    def state(self):
        return self.t, self.on, self.set

    def _line(self, s: np.ndarray) -> np.ndarray:
        """r[s] as f64 (len, 2), zero for s < 0"""
        out = self.hist[np.clip(s, 0, None)].astype(np.float64)
        out[s < 0] = 0.0
        if self.stale_from is not None:
            out[s >= self.stale_from] = 0.0
        return out

    def run(self, x: np.ndarray, spt: int, seeks=()) -> np.ndarray:
        """x: float32, n_ticks * spt * 2 interleaved, what the deck wrote; the port after the echo, same shape.  seeks: the ticks at which the deck seeks
        (read by one misreading only)"""
        x = np.asarray(x, np.float32).reshape(-1, spt, 2)
        n_ticks = x.shape[0]
        assert all(k < n_ticks for k in self.sched)
        y = x.copy()
        sched, self.sched = self.sched, {}
        # the misreading that lives in the block cut: the last frame of a block one frame too long reads its tap at s + 1 before the block's first frame wrote it
        stale = set()
        on, st, delays = self.on, self.set, []
        for k in range(n_ticks):
            if k in sched:
                on = sched[k] is not OFF
                st = sched[k] if on else st
            delays.append(st.delay if on else 0)
        self.stale_from = self.t if "walk_as_one_block" in self.mis and len(cut(spt, delays)) > 1 else None
        if "block_plus_one" in self.mis:
            for first, frames in cut(spt, delays, self.mis):
                stale |= {g for g in range(max(first, first + frames - 2), first + frames) if g - delays[g // spt] + 1 >= first}
        for k in range(n_ticks):
            ramp, old = False, (np.float32(self.set.send), np.float32(self.set.feedback), np.float32(self.set.wet))
            prev_delay = self.set.delay if self.on else None
            if k in sched:
                e = sched[k]
                if e is OFF:
                    self.on = False
                else:
                    if not self.on:
                        old = (np.float32(0.0),) * 3
                        if "line_kept_off_on" not in self.mis:
                            self.t = 0
                            self.stale_from = 0 if self.stale_from is not None else None
                    self.on, self.set, ramp = True, e, True
            if not self.on:
                continue
            if "seek_restarts" in self.mis and k in seeks:
                self.t = 0
            st = self.set
            new = (np.float32(st.send), np.float32(st.feedback), np.float32(st.wet))
            a = np.float64(np.float32(st.damp)) * 0.25
            b = 1.0 - (a + a)
            need = self.t + spt
            if need > self.hist.shape[0]:
                grown = np.zeros((max(need, 2 * self.hist.shape[0]), 2), np.float32)
                grown[:self.t] = self.hist[:self.t]
                self.hist = grown
            n0 = 0
            while n0 < spt:                                  # pieces of at most D - 1 frames read nothing they write themselves
                n1 = min(spt, n0 + st.delay - 1)
                n = np.arange(n0, n1, dtype=np.int64)
                t = self.t + n
                D = np.full(n.shape, st.delay, np.int64)
                if "delay_from_tick_start" in self.mis and prev_delay is not None:
                    D[n < st.delay] = prev_delay
                    n1 = min(n1, n0 + prev_delay - 1)
                    n, t, D = n[:n1 - n0], t[:n1 - n0], D[:n1 - n0]
                s = t - D
                xs = x[k, n0:n1].astype(np.float64)
                r0, rm, rp = self._line(s), self._line(s - 1), self._line(s + 1)
                for i in np.flatnonzero(np.isin(k * spt + n, list(stale))) if stale else ():
                    rp[i] = 0.0
                if st.flags & PINGPONG:
                    if "pingpong_crosses_x" in self.mis:
                        xs = xs[:, ::-1]
                    else:
                        r0, rm, rp = r0[:, ::-1], rm[:, ::-1], rp[:, ::-1]
                if ramp and "ramp_over_feed" in self.mis:
                    w = (k * spt + n).astype(np.float64) / np.float64(n_ticks * spt)
                    g = [(np.float64(o) + (np.float64(v) - np.float64(o)) * w).astype(np.float32) for o, v in zip(old, new)]
                    send, fb, wet = (v.astype(np.float64)[:, None] for v in g)
                elif ramp:
                    if "ramp_f32" in self.mis:
                        w = ((n + (1 if "ramp_n_plus_1" in self.mis else 0)).astype(np.float32) / np.float32(spt)).astype(np.float32)
                        g = [(o + ((v - o) * w).astype(np.float32)).astype(np.float32) for o, v in zip(old, new)]
                    else:
                        w = (n + (1 if "ramp_n_plus_1" in self.mis else 0)).astype(np.float64) / np.float64(spt)
                        g = [(np.float64(o) + (np.float64(v) - np.float64(o)) * w).astype(np.float32) for o, v in zip(old, new)]
                    send, fb, wet = (v.astype(np.float64)[:, None] for v in g)
                else:
                    send, fb, wet = (np.float64(v) for v in new)
                f = b * r0 + a * rm + a * rp                  # ((b r0) + (a rm)) + (a rp)
                yy = (xs + wet * f).astype(np.float32)
                r = (send * (yy.astype(np.float64) if "r_from_y" in self.mis else xs) + fb * f).astype(np.float32)
                self.hist[t] = r
                y[k, n0:n1] = yy
                n0 = n1
            self.t += spt
        self.stale_from = None
        return y.reshape(-1)
