"""Loudness taps (mixlab_gpu.h mx_graph_set_loudness) restated in numpy, bit for bit.

Per tap and tick: the K-weighted sum of squares of each channel (two f64 biquads in transposed direct form II, every operation rounded on
its own), the window sums over the last momentary_ticks / short_ticks ticks, and the true peak behind a 4 x 12-tap interpolator.  The
recurrence is decomposed per tick exactly as the header states it -- a tick's output is the plain walk from its start state S_k, the next
start state is Z_k + P S_k with Z_k the end state of the walk from zero and P the host's carry matrix -- so the model walks every tick of a
run at once (numpy vectors over ticks, a loop over the tick's frames) and any grouping of ticks into runs gives the same records.

The biquads and the interpolator table come from mx_loudness_tables -- the very ones the kernels use -- so the model needs no libm; the
carry matrix is recomputed here (tests/test_cpu_loudness.py compares it with the library's, and the tables with the standard's printed
ones and a 60-digit evaluation).  Importable without a GPU (the tables are host code).
"""
from __future__ import annotations

import numpy as np

TICK_DTYPE = np.dtype({"names": ["ksq", "momentary_sq", "short_sq", "true_peak", "frames", "channels"],
                       "formats": [("<f8", 2), "<f8", "<f8", ("<f4", 2), "<u4", "<u4"],
                       "offsets": [0, 16, 24, 32, 40, 44], "itemsize": 48})   # mx_loudness_tick
HIST_TICKS = 1023   # the window history: max(momentary_ticks, short_ticks) - 1 <= 1023 ticks
HIST_FRAMES = 11    # the interpolator's history
_tables = {}


def tables(rate: float, frames: int):
    """(biquads f64[10]: shelf b0 b1 b2 a1 a2, high-pass b0 b1 b2 a1 a2; carry f64[4, 4]; interp f32[3, 12]) from the library"""
    key = (float(rate), int(frames))
    if key not in _tables:
        from mixlab_amd import abi
        _tables[key] = abi.loudness_tables(rate, frames)
    return _tables[key]


def step(bq, x, s):
    """one sample through both biquads: x f64 [..], s = [s1, s2, s1', s2'] (updated in place) -> y.  y = b0 x + s1;
    s1 = (b1 x - a1 y) + s2; s2 = b2 x - a2 y, each operation rounded (numpy's float64 ufuncs fuse nothing)"""
    for k in (0, 1):
        b0, b1, b2, a1, a2 = bq[5 * k:5 * k + 5]   # (np.float64 scalars)
        y = b0 * x + s[2 * k]
        s[2 * k] = (b1 * x - a1 * y) + s[2 * k + 1]
        s[2 * k + 1] = b2 * x - a2 * y
        x = y
    return x


_carries = {}


def carry_matrix(bq, frames: int) -> np.ndarray:
    """P[r][c]: component r of the state after `frames` zero samples from unit state c"""
    key = (np.asarray(bq, np.float64).tobytes(), int(frames))
    if key not in _carries:
        _carries[key] = _carry_matrix(np.asarray(bq, np.float64), frames)
    return _carries[key]


def _carry_matrix(bq, frames: int) -> np.ndarray:
    p = np.zeros((4, 4))
    with np.errstate(all="ignore"):
        for c in range(4):
            s = [np.float64(1.0 if r == c else 0.0) for r in range(4)]
            for _ in range(frames):
                step(bq, np.float64(0.0), s)
            p[:, c] = s
    return p


def walk(bq, x: np.ndarray, s0: np.ndarray, energy: bool):
    """x f64 [T, F] (every row a tick), s0 f64 [T, 4] -> (end state [T, 4], ksq [T] or None): the plain recurrence from s0, row by row"""
    s = [s0[:, r].copy() for r in range(4)]
    part = np.zeros((x.shape[0], 8))
    with np.errstate(all="ignore"):
        for i in range(x.shape[1]):
            y = step(bq, x[:, i], s)
            if energy:
                part[:, i & 7] = part[:, i & 7] + y * y   # the product rounds, then the sum
        if energy:
            q = np.arange(8)
            for m in (4, 2, 1):
                part = part + part[:, q ^ m]
    return np.stack(s, axis=1), (part[:, 0] if energy else None)


def advance(p: np.ndarray, z: np.ndarray, s: np.ndarray) -> np.ndarray:
    """S_{k+1} = Z_k + P S_k, row r as ((P[r][0] S0 + P[r][1] S1) + P[r][2] S2) + P[r][3] S3, then Z[r] + that"""
    with np.errstate(all="ignore"):
        return np.array([z[r] + (((p[r, 0] * s[0] + p[r, 1] * s[1]) + p[r, 2] * s[2]) + p[r, 3] * s[3]) for r in range(4)])


def true_peak_bits(interp: np.ndarray, x: np.ndarray, hist: np.ndarray, frames: int) -> np.ndarray:
    """x f32 [n] (one channel of a run), hist f32 [11] -> uint32 [ticks]: the largest magnitude bits of x[m] and v_1..3[m] per tick"""
    ext = np.concatenate([hist, x]).astype(np.float64)
    n = x.shape[0]
    best = x.view(np.uint32) & np.uint32(0x7fffffff)
    with np.errstate(all="ignore"):
        for p in range(3):
            acc = np.zeros(n)
            for j in range(12):
                acc = acc + np.float64(interp[p, j]) * ext[j:j + n]   # exact products: x[m - 11 + j], ascending j
            best = np.maximum(best, acc.astype(np.float32).view(np.uint32) & np.uint32(0x7fffffff))
    return best.reshape(-1, frames).max(axis=1)


class LoudnessModel:
    """one tap: feed it the port's samples run by run (mono: frames, stereo: interleaved 2 * frames); everything starts as +0.0"""

    def __init__(self, channels: int, rate: float, frames: int, momentary_ticks: int = 24, short_ticks: int = 180):
        self.channels, self.frames, self.m, self.s = channels, frames, momentary_ticks, short_ticks
        self.bq, _carry, self.interp = tables(rate, frames)
        self.p = carry_matrix(self.bq, frames)
        self.state = np.zeros((channels, 4))
        self.e_hist = np.zeros(HIST_TICKS)
        self.x_hist = np.zeros((channels, HIST_FRAMES), dtype=np.float32)

    def run(self, samples: np.ndarray, n_ticks: int) -> np.ndarray:
        """-> TICK_DTYPE [n_ticks]"""
        return run_many([self], [samples], n_ticks)[0]

    def _records(self, chans, ksq, n_ticks: int) -> np.ndarray:
        """chans[c]: the run's f32 samples of channel c, ksq[c]: its K-weighted sums, tick by tick"""
        ch, f = self.channels, self.frames
        out = np.zeros(n_ticks, dtype=TICK_DTYPE)
        out["frames"], out["channels"] = f, ch
        for c in range(ch):
            xc = chans[c]
            out["ksq"][:, c] = ksq[c]
            out["true_peak"][:, c] = true_peak_bits(self.interp, xc, self.x_hist[c], f).view(np.float32)
            self.x_hist[c] = np.concatenate([self.x_hist[c], xc])[-HIST_FRAMES:]
        with np.errstate(all="ignore"):
            e = np.concatenate([self.e_hist, out["ksq"][:, 0] + out["ksq"][:, 1]])
            t = HIST_TICKS + np.arange(n_ticks)
            for name, w in (("momentary_sq", self.m), ("short_sq", self.s)):
                acc = np.zeros(n_ticks)
                for back in range(w - 1, -1, -1):   # ascending tick: t - w + 1 .. t
                    acc = acc + e[t - back]
                out[name] = acc
        self.e_hist = e[-HIST_TICKS:].copy()
        return out


def run_many(models, samples, n_ticks: int) -> list:
    """[m.run(x, n_ticks) for m, x in zip(models, samples)] with the walks of the models that share biquads and a tick length done
    together: a row of a walk is one tick of one channel of one tap, rows never meet (numpy's ufuncs work element by element), so every
    record is what the model gives on its own, bit for bit (tests/test_cpu_loudness.py) -- in a fraction of the time, which is the
    Python loop over the tick's frames"""
    out = [None] * len(models)
    groups = {}
    for i, m in enumerate(models):
        groups.setdefault((m.frames, np.asarray(m.bq, np.float64).tobytes()), []).append(i)
    for idx in groups.values():
        f, bq = models[idx[0]].frames, models[idx[0]].bq
        rows = []                                              # (model, channel, the channel's samples)
        for i in idx:
            x = np.ascontiguousarray(samples[i], dtype=np.float32).reshape(n_ticks * f, models[i].channels)
            rows += [(models[i], c, np.ascontiguousarray(x[:, c])) for c in range(models[i].channels)]
        ticks = np.concatenate([xc.astype(np.float64).reshape(n_ticks, f) for _m, _c, xc in rows], axis=0)
        z, _ = walk(bq, ticks, np.zeros((ticks.shape[0], 4)), False)
        starts = np.zeros((ticks.shape[0], 4))
        for r, (m, c, _xc) in enumerate(rows):
            s = m.state[c]
            for k in range(n_ticks):
                starts[r * n_ticks + k] = s
                s = advance(m.p, z[r * n_ticks + k], s)
            m.state[c] = s
        _, ksq = walk(bq, ticks, starts, True)
        r = 0
        for i in idx:
            ch = models[i].channels
            out[i] = models[i]._records([rows[r + c][2] for c in range(ch)], [ksq[(r + c) * n_ticks:(r + c + 1) * n_ticks] for c in range(ch)], n_ticks)
            r += ch
    return out


def records_equal(a: np.ndarray, b: np.ndarray) -> bool:
    """bit for bit, except that any NaN equals any NaN"""
    ok = a["frames"].tobytes() == b["frames"].tobytes() and a["channels"].tobytes() == b["channels"].tobytes()
    for name, bits in (("ksq", np.uint64), ("momentary_sq", np.uint64), ("short_sq", np.uint64), ("true_peak", np.uint32)):
        u, v = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        ok = ok and bool(((u.view(bits) == v.view(bits)) | (np.isnan(u) & np.isnan(v))).all())
    return ok


def first_difference(a: np.ndarray, b: np.ndarray) -> str:
    for name in ("frames", "channels", "ksq", "momentary_sq", "short_sq", "true_peak"):
        u, v = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        bad = u != v
        if u.dtype.kind == "f":
            bits = np.uint64 if u.dtype.itemsize == 8 else np.uint32
            bad = ~((u.view(bits) == v.view(bits)) | (np.isnan(u) & np.isnan(v)))
        if bad.any():
            at = tuple(int(i[0]) for i in np.nonzero(bad))
            return f"{name}{list(at)}: got {u[at]!r}, want {v[at]!r} ({int(bad.sum())} of {bad.size} differ)"
    return "equal"
