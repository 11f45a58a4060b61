"""The deck, modelled from include/mixlab_gpu.h ("the deck") alone: the tick rules in Python integers, the sums in numpy f64 in the header's order.

`mis` names ONE deliberate misreading of the header (MISREADINGS); the CPU suite shows that each changes some case's samples or records, so the shared cases
can tell the model -- and the kernel that must equal it bit for bit -- from every one of them.  The coefficient tables come from the library (mx_deck_tables), as the
spectrum and loudness models take theirs; tests/test_cpu_deck.py checks them entry by entry against an mpmath evaluation of the header's formula."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

ONE = 1 << 32
TAPS, PHASES, BANKS = 32, 256, 4
PLAY, LOOP = 1, 2
T_PLAY, T_LOOPING, T_BEFORE, T_PAST = 1, 2, 4, 8
MAX_STEP, MAX_SLEW, MARGIN, MAX_FRAMES, MAX_SPT = 4 * ONE, 1 << 24, 1 << 20, 1 << 30, 1 << 20

Params = namedtuple("Params", "step slew loop_in loop_out flags", defaults=(0, 0, 0, 0, 0))
Head = namedtuple("Head", "pos step params last_looping last_loop_in last_loop_out", defaults=(0, 0, Params(), False, 0, 0))
Tick = namedtuple("Tick", "pos step dstep loop_in loop_len flags bank")

MISREADINGS = ("n_plus_1", "round_phase", "tap_offset_16", "fold_taps", "trunc_fold", "bank_from_step", "bank_edge_lt", "blend_from_next", "descending_k",
               "f32_accumulate", "slew_before_event", "clamp_after_loop")


def check(p: Params, n_frames: int) -> str | None:
    """the rule that refuses (p, n_frames), or None"""
    if not 1 <= n_frames <= MAX_FRAMES:
        return "n_frames"
    if abs(p.step) > MAX_STEP:
        return "step"
    if not 0 <= p.slew <= MAX_SLEW:
        return "slew"
    if p.flags & ~(PLAY | LOOP):
        return "flags"
    if p.flags & LOOP and not 0 <= p.loop_in < p.loop_out <= n_frames:
        return "loop"
    return None


def tdiv(a: int, b: int) -> int:
    """C's truncating division"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def clamp(v, lo, hi):
    return min(max(v, lo), hi)


def bank_of(m: int, mis=()) -> int:
    if "bank_edge_lt" in mis:
        return 0 if m < ONE else 1 if 3 * m < 4 * ONE else 2 if m < 2 * ONE else 3
    return 0 if m <= ONE else 1 if 3 * m <= 4 * ONE else 2 if m <= 2 * ONE else 3


def fold(u: int, in_q: int, len_q: int, mis=()) -> int:
    if "trunc_fold" in mis:
        d = u - in_q
        return in_q + (d - tdiv(d, len_q) * len_q)
    return in_q + (u - in_q) % len_q


def slew(step: int, p: Params, spt: int):
    """step 5: (step, dstep)"""
    if p.slew == 0:
        return p.step, 0
    d = clamp(tdiv(p.step - step, spt), -p.slew, p.slew)
    return (p.step, 0) if d == 0 else (step, d)


def plan(h: Head, params: Params | None, seek: int | None, spt: int, n_frames: int, mis=()):
    """one tick: (Tick, Head after it)"""
    assert 1 <= spt <= MAX_SPT and (params is None or check(params, n_frames) is None)
    pos, step, p = h.pos, h.step, h.params
    early = slew(step, p, spt) if "slew_before_event" in mis else None
    if seek is not None:
        pos = seek
    if params is not None:
        p = params
    lo, hi = -MARGIN * ONE, (n_frames + MARGIN) * ONE
    if "clamp_after_loop" not in mis:
        pos = clamp(pos, lo, hi)
    in_q, len_q = p.loop_in * ONE, (p.loop_out - p.loop_in) * ONE
    looping = bool(p.flags & LOOP) and ((h.last_looping and (h.last_loop_in, h.last_loop_out) == (p.loop_in, p.loop_out)) or in_q <= pos < p.loop_out * ONE)
    if "clamp_after_loop" in mis:
        pos = clamp(fold(pos, in_q, len_q), lo, hi) if looping else clamp(pos, lo, hi)
    play = bool(p.flags & PLAY)
    dstep = m = 0
    if play:
        step, dstep = early if early is not None else slew(step, p, spt)
        m = abs(step) if "bank_from_step" in mis else max(abs(step), abs(step + (spt - 1) * dstep))
    flags = (T_PLAY if play else 0) | (T_LOOPING if looping else 0)
    if play and not looping:
        m_true = max(abs(step), abs(step + (spt - 1) * dstep))
        flags |= T_BEFORE if pos + (spt - 1) * m_true < -16 * ONE else 0
        flags |= T_PAST if pos - (spt - 1) * m_true >= (n_frames + 15) * ONE else 0
    tick = Tick(pos, step, dstep, p.loop_in if looping else 0, p.loop_out - p.loop_in if looping else 0, flags, bank_of(m, mis) if play else 0)
    if play:
        pos = pos + spt * step + dstep * (spt * (spt - 1) // 2)
        if looping:
            pos = fold(pos, in_q, len_q, mis)
        step += spt * dstep
    return tick, Head(pos, step, p, looping, p.loop_in if looping else 0, p.loop_out if looping else 0)


def positions(t: Tick, spt: int, mis=()) -> list[int]:
    """u'(n) of a playing tick, n < spt, as Python integers"""
    tri = (lambda n: n * (n + 1) // 2) if "n_plus_1" in mis else (lambda n: n * (n - 1) // 2)
    us = [t.pos + n * t.step + t.dstep * tri(n) for n in range(spt)]
    if t.flags & T_LOOPING:
        us = [fold(u, t.loop_in * ONE, t.loop_len * ONE, mis) for u in us]
    return us


def samples_f64(track_i16: np.ndarray) -> np.ndarray:
    """(n_frames, 2) f64 of the values (float)s / 32768.0f"""
    return (np.asarray(track_i16, np.int16).reshape(-1, 2).astype(np.float32) / np.float32(32768.0)).astype(np.float64)


def render_tick(x: np.ndarray, t: Tick, spt: int, tables: np.ndarray, mis=()) -> np.ndarray:
    """float32 (spt, 2): one tick's output from the track x = samples_f64(...) and tables[bank] = float32 (257, 32)"""
    out = np.zeros((spt, 2), np.float32)
    if not t.flags & T_PLAY:
        return out
    n_frames = x.shape[0]
    u = np.array(positions(t, spt, mis), dtype=object)
    if "round_phase" in mis:
        u = u + (1 << 23)
    idx = np.array([int(v) >> 32 for v in u], np.int64)
    p = np.array([(int(v) >> 24) & 255 for v in u], np.int64)
    w = np.array([int(v) & 0xFFFFFF for v in u], np.float64) * 2.0 ** -24
    T = tables[t.bank].astype(np.float64)
    acc_t = np.float32 if "f32_accumulate" in mis else np.float64
    acc = np.zeros((spt, 2), acc_t)
    off = 16 if "tap_offset_16" in mis else 15
    ks = range(TAPS - 1, -1, -1) if "descending_k" in mis else range(TAPS)
    for k in ks:
        a, b = T[p, k], T[p + 1, k]
        # (the blend started from the next row with the difference left as it stands.  With the difference turned round as well it is the same number: both rows are
        # f32 of like size and w has 24 bits, so either form of c is exact in f64 -- no case can tell those two apart, and none has to)
        c = b + (1.0 - w) * (b - a) if "blend_from_next" in mis else a + w * (b - a)
        f = idx - off + k
        if "fold_taps" in mis and t.flags & T_LOOPING:
            f = t.loop_in + (f - t.loop_in) % t.loop_len
        ok = (f >= 0) & (f < n_frames)
        xs = np.where(ok[:, None], x[np.clip(f, 0, n_frames - 1)], 0.0)
        prod = c[:, None] * xs
        acc = (acc + prod.astype(acc_t)).astype(acc_t)
    return acc.astype(np.float32)


class DeckModel:
    """mx_deck_* on the host: a track, a head, a schedule; feed() returns what mx_deck_feed writes and records"""

    def __init__(self, track_i16: np.ndarray, tables, mis=()):
        self.track = np.asarray(track_i16, np.int16).reshape(-1, 2)
        self.x = samples_f64(self.track)
        self.n_frames = self.x.shape[0]
        self.tables, self.mis = tables, mis
        self.head = Head()
        self.sched: dict[int, list] = {}

    def load(self, first_frame: int, interleaved_i16):
        a = np.asarray(interleaved_i16, np.int16).reshape(-1, 2)
        self.track[first_frame:first_frame + len(a)] = a
        self.x = samples_f64(self.track)

    def schedule(self, tick: int, params: Params | None = None, seek: int | None = None):
        e = self.sched.setdefault(tick, [None, None])
        if params is not None:
            assert check(params, self.n_frames) is None
            e[0] = params
        if seek is not None:
            e[1] = seek

    def feed(self, n_ticks: int, spt: int, render: bool = True):
        """(float32 [n_ticks * spt * 2] interleaved, [Tick])"""
        assert all(t < n_ticks for t in self.sched)
        out, recs = np.zeros((n_ticks, spt, 2), np.float32), []
        for t in range(n_ticks):
            params, seek = self.sched.get(t, (None, None))
            tick, self.head = plan(self.head, params, seek, spt, self.n_frames, self.mis)
            recs.append(tick)
            if render:   # (a BEFORE / PAST tick is rendered like any other: that it comes out as zeros is tested, not assumed)
                out[t] = render_tick(self.x, tick, spt, self.tables, self.mis)
        self.sched = {}
        return out.reshape(-1), recs
