"""The deck's sweep filter, modelled from include/mixlab_gpu.h ("FILTER") alone: the schedule, the ramps and on / off in Python, the samples in numpy f64 with numpy's
casts to f32, one operation per statement in the header's order and association.  A pass over what the deck wrote (tests/deck_model.py, tests/deck_keylock_model.py),
tick by tick, that carries the setting and the four state values between calls; its output is what tests/deck_echo_model.py's EchoModel takes in.

The coefficients of a tick and its wet mix are numpy f64 arrays over the tick's frames (elementwise, so each frame's value is the scalar formula's); the recurrence
itself, serial in time, runs frame by frame in numpy f64 scalars.

`mis` names ONE deliberate misreading of the header (MISREADINGS); tests/test_cpu_deck_filter.py shows that each changes a compared sample or state value of the
case named for it in SHOWN_BY (tests/deck_filter_cases.py), so those cases tell the model -- and the kernel that must equal it bit for bit -- from every one of them.
One more misreading, the filter behind the echo instead of ahead of it, lives where the two models meet (deck_filter_cases.run_model, `echo_first`).

None of the issue's misreadings had to be argued away here: each of them reaches an f32 sample or a state value of a deck-made case.  "gn held in f32" can only show
in a ramp tick (a constant tick's gn IS an f32 widened), which is why its case is the sweep."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

LP, HP, BP, NOTCH = 0, 1, 2, 3
MIN_G, MAX_G, MIN_K, MAX_K = np.float32(2.0 ** -12), np.float32(16.0), np.float32(0.05), np.float32(2.0)
Filt = namedtuple("Filt", "kind g k wet flags pad", defaults=(1.0, 0, 0))
OFF = "off"

MISREADINGS = ("ramp_n_plus_1", "coef_frozen", "gn_f32", "a1_f32", "v2_from_new_s1", "shared_state", "seek_clears", "feed_clears", "kind_change_clears",
               "state_kept_off_on", "no_fade_in", "kind_at_tick_end", "only_playing_ticks", "schedule_late")


def check(f: Filt) -> str | None:
    """the rule that refuses f, or None"""
    if not 0 <= f.kind <= 3:
        return "kind"
    if f.flags:
        return "flags"
    if f.pad:
        return "pad"
    g, k, wet = np.float32(f.g), np.float32(f.k), np.float32(f.wet)
    if not (np.isfinite(g) and np.isfinite(k) and np.isfinite(wet)):
        return "finite"
    if not MIN_G <= g <= MAX_G:
        return "g"
    if not MIN_K <= k <= MAX_K:
        return "k"
    if not 0 <= wet <= 1:
        return "wet"
    return None


def coefficients(old, new, ramp: bool, spt: int, mis=()):
    """(kn, wn, a1, a2, a3) of the frames of one tick, f64 arrays of spt; old, new: (g, k, wet) as f32"""
    g0, k0, w0 = (np.float64(np.float32(v)) for v in old)
    g1, k1, w1 = (np.float64(np.float32(v)) for v in new)
    if ramp:
        n = np.arange(spt, dtype=np.int64)
        if "ramp_n_plus_1" in mis:
            n = n + 1
        if "coef_frozen" in mis:
            n = n * 0
        w = n.astype(np.float64) / np.float64(spt)
        dg = g1 - g0
        dk = k1 - k0
        dw = w1 - w0
        pg = dg * w
        pk = dk * w
        pw = dw * w
        gn = g0 + pg
        kn = k0 + pk
        wn = w0 + pw
    else:
        gn, kn, wn = np.full(spt, g1), np.full(spt, k1), np.full(spt, w1)
    if "gn_f32" in mis:
        gn = gn.astype(np.float32).astype(np.float64)
    gk = gn + kn
    gg = gn * gk
    d = 1.0 + gg
    a1 = 1.0 / d
    if "a1_f32" in mis:
        a1 = a1.astype(np.float32).astype(np.float64)
    a2 = gn * a1
    a3 = gn * a2
    return kn, wn, a1, a2, a3


def step(x, a1, a2, a3, s1, s2, mis=()):
    """one frame of one channel in numpy f64 scalars: (v1, v2, s1, s2)"""
    v3 = x - s2
    p1 = a1 * s1
    p2 = a2 * v3
    v1 = p1 + p2
    d1 = v1 + v1
    s1_new = d1 - s1
    q1 = a2 * (s1_new if "v2_from_new_s1" in mis else s1)
    q2 = a3 * v3
    q = q1 + q2
    v2 = s2 + q
    d2 = v2 + v2
    s2_new = d2 - s2
    return v1, v2, s1_new, s2_new


def response(kind: int, x, kn, v1, v2):
    """f of the header, on arrays or scalars"""
    if kind == LP:
        return v2
    if kind == BP:
        return v1
    kv = kn * v1
    nf = x - kv
    return nf - v2 if kind == HP else nf


class FilterModel:
    """mx_deck_set_filter / mx_deck_schedule_filter and the filter pass of mx_deck_feed on the host"""

    def __init__(self, mis=()):
        assert all(m in MISREADINGS for m in mis), mis
        self.mis = mis
        self.on, self.set = False, Filt(0, 0.0, 0.0, 0.0)
        self.s = np.zeros(4, np.float64)                 # s1 s2 of L, s1 s2 of R
        self.sched: dict[int, object] = {}
        self.late = None                                 # schedule_late: the event that fell off the last feed's end
        self.counts = dict(decks=0, ticks_ramp=0, ticks_constant=0, blocks=0)   # mx_deck_debug_last_filter of the last run

    def schedule(self, tick: int, f):
        """f: a Filt, or OFF"""
        assert f is OFF or check(f) is None
        self.sched[tick] = f

    def state(self):
        """(on, Filt in force) as mx_deck_filter_state reads them"""
        return self.on, self.set

    def state4(self) -> np.ndarray:
        """mx_deck_read_filter_state: the four values, zeros while the filter is off"""
        return self.s.copy() if self.on else np.zeros(4, np.float64)

    def run(self, x: np.ndarray, spt: int, seeks=(), playing=None) -> np.ndarray:
        """x: float32, n_ticks * spt * 2 interleaved, what the deck wrote; the port after the filter, same shape.  seeks: the ticks at which the deck seeks,
        playing: the ticks whose PLAY flag is set (each read by one misreading only)"""
        x = np.asarray(x, np.float32).reshape(-1, spt, 2)
        n_ticks = x.shape[0]
        assert all(k < n_ticks for k in self.sched)
        y = x.copy()
        sched, self.sched = self.sched, {}
        if "schedule_late" in self.mis:
            moved = {k + 1: v for k, v in sched.items()}
            if self.late is not None:
                moved.setdefault(0, self.late)
            self.late = moved.pop(n_ticks, None)
            sched = moved
        if "feed_clears" in self.mis:
            self.s[:] = 0.0
        counts = dict(decks=0, ticks_ramp=0, ticks_constant=0, blocks=0)
        for k in range(n_ticks):
            ramp = False
            old = (self.set.g, self.set.k, self.set.wet)
            kind_before = self.set.kind if self.on else None
            if k in sched:
                f = sched[k]
                if f is OFF:
                    self.on = False
                else:
                    if not self.on:
                        old = (f.g, f.k, f.wet if "no_fade_in" in self.mis else 0.0)
                        if "state_kept_off_on" not in self.mis:
                            self.s[:] = 0.0
                    elif "kind_change_clears" in self.mis and f.kind != self.set.kind:
                        self.s[:] = 0.0
                    self.on, self.set, ramp = True, f, True
            if not self.on:
                continue
            counts["ticks_ramp" if ramp else "ticks_constant"] += 1
            if "seek_clears" in self.mis and k in seeks:
                self.s[:] = 0.0
            if "only_playing_ticks" in self.mis and playing is not None and k not in playing:
                continue
            st = self.set
            kind = kind_before if "kind_at_tick_end" in self.mis and ramp and kind_before is not None else st.kind
            kn, wn, a1, a2, a3 = coefficients(old, (st.g, st.k, st.wet), ramp, spt, self.mis)
            xd = x[k].astype(np.float64)
            v1, v2 = np.empty((spt, 2), np.float64), np.empty((spt, 2), np.float64)
            s = [np.float64(v) for v in self.s]
            shared = "shared_state" in self.mis
            for n in range(spt):
                A1, A2, A3 = a1[n], a2[n], a3[n]
                for c in (0, 1):
                    i = 0 if shared else 2 * c
                    v1[n, c], v2[n, c], s[i], s[i + 1] = step(xd[n, c], A1, A2, A3, s[i], s[i + 1], self.mis)
            self.s[:] = s
            f = response(kind, xd, kn[:, None], v1, v2)
            diff = f - xd
            m = wn[:, None] * diff
            y[k] = (xd + m).astype(np.float32)
        if counts["ticks_ramp"] + counts["ticks_constant"]:
            counts["decks"], counts["blocks"] = 1, -(-n_ticks * spt // 64)
        self.counts = counts
        return y.reshape(-1)
