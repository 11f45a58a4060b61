"""The look-ahead limiter taps' spec (include/mixlab_gpu.h, mx_graph_set_limiters) restated in numpy, bit for bit: arrays over the frames n,
a loop over the taps k, f32 throughout, every operation rounded on its own.  Importable without a GPU.

A LimiterModel is one tap: it carries the last 2 D input frames from run to run, so feeding it a stream in any grouping gives the same bits
(tests/test_cpu_limiter.py).  `guard_min` and `clamp` switch off step 5's min and step 6's clamp for the negative control only."""
from __future__ import annotations

import numpy as np

from mixlab_amd import abi

F32 = np.float32
MAX_LOOKAHEAD = 512
TICK_DTYPE = abi.LIMITER_TICK_DTYPE


def weights(D: int) -> np.ndarray:
    """w[k] = f32(h[k] / sum h), h[k] = 1 - cos(2 pi (k + 1) / (D + 2)), k = 0 .. D.  Evaluated as 2 sin^2(pi (k + 1) / (D + 2)) / (D + 2):
    1 - cos(2 t) = 2 sin^2(t) without the cancellation, and the sum is D + 2 exactly (the cosines of all D + 2 roots of unity add to 0; the
    one left out is 1).  In f64 the quotient is within 2^-50 relative of the exact one, against the 2^-25 half-spacing of an f32."""
    if D == 0:
        return np.ones(1, F32)
    k = np.arange(D + 1, dtype=np.float64)
    return (2.0 * np.sin(np.pi * (k + 1.0) / (D + 2.0)) ** 2 / (D + 2.0)).astype(F32)


def level_bits(x: np.ndarray) -> np.ndarray:
    """step 1: x [frames, channels] f32 -> bits of a[n]"""
    return (np.ascontiguousarray(x).view(np.uint32) & np.uint32(0x7fffffff)).max(axis=1)


def required_gain(a_bits: np.ndarray, c: np.float32) -> np.ndarray:
    """step 2"""
    a = a_bits.view(F32)
    r = np.ones(a.shape, F32)
    bad = a_bits >= np.uint32(0x7f800000)
    over = ~bad & (a > c)
    r[over] = c / np.minimum(a[over], F32(65536.0))   # numpy's f32 division is IEEE's
    r[bad] = F32(0.0)
    return r


class LimiterModel:
    def __init__(self, ceiling: float, lookahead: int, channels: int, guard_min: bool = True, clamp: bool = True):
        self.c, self.D, self.C = F32(ceiling), int(lookahead), int(channels)
        assert float(self.c) == float(ceiling) and 2.0 ** -20 <= ceiling <= 1.0 and 0 <= self.D <= MAX_LOOKAHEAD and self.C in (1, 2)
        self.w = weights(self.D)
        self.guard_min, self.clamp = guard_min, clamp
        self.hist = np.zeros((2 * self.D, self.C), F32)   # frames before n = 0 are +0.0
        self.last_gain = None                             # g of the last run's frames (tests of the gain's shape)

    def run(self, x, n_ticks: int):
        """x: n_ticks ticks of the port in its logical layout (interleaved when stereo) -> (limited copy, flat f32; records [n_ticks])"""
        c, D, C = self.c, self.D, self.C
        x = np.asarray(x, F32).reshape(-1, C)
        N = len(x)
        assert n_ticks >= 1 and N % n_ticks == 0
        ext = np.concatenate([self.hist, x])            # frames -2 D .. N - 1: frame j at j + 2 D
        r = required_gain(level_bits(ext), c)
        m = r[D:D + N + D].copy()                        # m of frames -D .. N - 1 (frame j at j + D): k = 0
        for k in range(1, D + 1):
            m = np.minimum(m, r[D - k:D - k + N + D])
        acc = np.zeros(N, F32)
        for k in range(D + 1):                           # step 4, ascending k
            p = self.w[k] * m[D - k:D - k + N]
            acc = acc + p
        q = np.minimum(m[D:D + N], m[:N])
        g = np.minimum(acc, r[D:D + N]) if self.guard_min else acc
        g = np.where(q == F32(1.0), F32(1.0), g).astype(F32)
        xd = ext[D:D + N]                                # input[n - D]
        fin = (xd.view(np.uint32) & np.uint32(0x7f800000)) != np.uint32(0x7f800000)
        with np.errstate(invalid="ignore", over="ignore"):
            y = xd * g[:, None]
            if self.clamp:
                y = np.maximum(-c, np.minimum(c, y))
        y = np.where(fin, y, F32(0.0)).astype(F32)
        self.hist = ext[len(ext) - 2 * D:].copy()        # a run shorter than 2 D frames shifts the history
        self.last_gain = g
        F = N // n_ticks
        rec = np.zeros(n_ticks, TICK_DTYPE)
        gt, yt = g.reshape(n_ticks, F), (y.view(np.uint32) & np.uint32(0x7fffffff)).reshape(n_ticks, F * C)
        rec["min_gain"] = gt.view(np.uint32).min(axis=1).view(F32) if F else F32(1.0)
        rec["peak_out"] = yt.max(axis=1).view(F32) if F else F32(0.0)
        rec["limited"] = (gt < F32(1.0)).sum(axis=1)
        rec["nonfinite"] = (~fin).reshape(n_ticks, F * C).sum(axis=1)
        rec["frames"], rec["channels"] = F, C
        return y.reshape(-1), rec


def as_stereo(x_dup) -> np.ndarray:
    """a port stored as one float per frame, in its logical layout"""
    return np.repeat(np.asarray(x_dup, F32), 2)


def to_i16(y) -> np.ndarray:
    """the sinks' format (mx_graph_read_output_i16): clamp to [-1, 1], x 32767 in f32, truncation toward zero"""
    v = np.clip(np.asarray(y, F32), F32(-1.0), F32(1.0)) * F32(32767.0)
    return np.trunc(v).astype(np.int16)


def records_equal(a, b) -> bool:
    return a.tobytes() == b.tobytes()


def first_difference(a, b) -> str:
    for t in range(len(a)):
        for name in TICK_DTYPE.names:
            if a[name][t].tobytes() != b[name][t].tobytes():
                return f"tick {t} {name}: got {a[name][t]!r}, want {b[name][t]!r}"
    return "equal"
