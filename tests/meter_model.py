"""Level meters (mixlab_gpu.h mx_graph_set_meters) restated in numpy, bit for bit.

Per tap, tick and channel:
  peak    the integer maximum of bits(x) & 0x7fffffff over the tick, read as f32
  over    samples with x < -1 or x > 1
  sum_sq  64 f64 partials -- partial j adds (double)x * (double)x for the frames f = j (mod 64) in ascending f, from +0.0 -- then
          s[j] = s[j] + s[j ^ k] for k = 32, 16, 8, 4, 2, 1; the result is s[0].  The partials are built by explicit row-by-row adds, not np.sum
          (whose pairwise order differs).
  hold    h (f32) and age a (u32), both 0 at the start: a = min(a + 1, 2^32 - 1); when a > hold_ticks, h = isfinite(h) ? h * release : 0
          (f32 multiply); when bits(peak) >= bits(h), h = peak and a = 0; record h.
Importable without a GPU.
"""
from __future__ import annotations

import numpy as np

U32_MAX = 0xFFFFFFFF

METER_TICK = np.dtype({"names": ["peak", "hold", "sum_sq", "over", "frames", "channels"],
                       "formats": [(np.float32, 2), (np.float32, 2), (np.float64, 2), (np.uint32, 2), np.uint32, np.uint32],
                       "offsets": [0, 8, 16, 32, 40, 44], "itemsize": 48})


def channel_stats(x: np.ndarray):
    """(peak f32, over, sum_sq f64) of one channel of one tick"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    b = x.view(np.uint32) & np.uint32(0x7FFFFFFF)
    peak = np.array([b.max() if b.size else 0], dtype=np.uint32).view(np.float32)[0]
    over = int(np.count_nonzero((x < np.float32(-1.0)) | (x > np.float32(1.0))))
    s = np.zeros(64, dtype=np.float64)
    d = x.astype(np.float64)
    with np.errstate(all="ignore"):
        for r0 in range(0, d.size, 64):   # row r0 // 64 of frames: each partial takes its next frame, in ascending f
            row = d[r0:r0 + 64]
            s[:row.size] = s[:row.size] + row * row
        lanes = np.arange(64)
        for k in (32, 16, 8, 4, 2, 1):
            s = s + s[lanes ^ k]
    return peak, over, np.float64(s[0])


class MeterModel:
    """one tap: feed it the port's samples tick by tick (mono: (F,), stereo: (F, 2) or interleaved 2F)"""

    def __init__(self, channels: int, hold_ticks: int = 0, release: float = 1.0):
        self.channels = channels
        self.hold_ticks = int(hold_ticks)
        self.release = np.float32(release)
        self.h = [np.float32(0.0), np.float32(0.0)]
        self.a = [0, 0]

    def hold_step(self, c: int, peak: np.float32) -> np.float32:
        self.a[c] = min(self.a[c] + 1, U32_MAX)
        if self.a[c] > self.hold_ticks:
            with np.errstate(all="ignore"):
                self.h[c] = np.float32(self.h[c] * self.release) if np.isfinite(self.h[c]) else np.float32(0.0)
        if int(np.float32(peak).view(np.uint32)) >= int(np.float32(self.h[c]).view(np.uint32)):
            self.h[c] = np.float32(peak)
            self.a[c] = 0
        return self.h[c]

    def tick(self, x: np.ndarray) -> np.ndarray:
        x = np.asarray(x, dtype=np.float32)
        rec = np.zeros((), dtype=METER_TICK)
        if self.channels == 2:
            x = x.reshape(-1, 2)
            chans = [x[:, 0], x[:, 1]]
        else:
            chans = [x.reshape(-1)]
        rec["frames"] = chans[0].size
        rec["channels"] = self.channels
        for c, xc in enumerate(chans):
            peak, over, ss = channel_stats(xc)
            rec["peak"][c] = peak
            rec["over"][c] = over
            rec["sum_sq"][c] = ss
            rec["hold"][c] = self.hold_step(c, peak)
        return rec

    def run(self, port: np.ndarray, n_ticks: int) -> np.ndarray:
        """a run's records from the port's samples of n_ticks ticks, back to back"""
        per = port.size // n_ticks
        return np.array([self.tick(port[k * per:(k + 1) * per]) for k in range(n_ticks)], dtype=METER_TICK)


def records_equal(got: np.ndarray, want: np.ndarray) -> np.ndarray:
    """per record: equal bit for bit, except that any NaN sum_sq equals any NaN"""
    got = np.asarray(got, dtype=METER_TICK)
    want = np.asarray(want, dtype=METER_TICK)
    ok = np.ones(got.shape, dtype=bool)
    for f in ("peak", "hold"):
        ok &= np.all(got[f].view(np.uint32) == want[f].view(np.uint32), axis=-1)
    gs, ws = got["sum_sq"], want["sum_sq"]
    ok &= np.all((gs.view(np.uint64) == ws.view(np.uint64)) | (np.isnan(gs) & np.isnan(ws)), axis=-1)
    ok &= np.all(got["over"] == want["over"], axis=-1)
    ok &= (got["frames"] == want["frames"]) & (got["channels"] == want["channels"])
    return ok
