"""The stereo field taps' spec (include/mixlab_gpu.h, mx_graph_set_stereo) restated in numpy -- what the kernels are held to, bit for bit.

  sum_xy   64 f64 partials -- partial j adds (double)x * (double)y for the frames f = j (mod 64) in ascending f, from +0.0 -- then
           s[j] = s[j] + s[j ^ k] for k = 32 .. 1; the value is s[0] (the meters' order, tests/meter_model.py).
  win_xy   the sum of sum_xy over the last window_ticks ticks in ascending tick from +0.0, every tick afresh; earlier ticks read +0.0.
  gonio    for frames with finite L and R: m = L + R, s = L - R in f32; cell(v) = (int)clamp(floorf(v * z), -grid / 2, grid / 2 - 1) + grid / 2,
           z = 2^zoom_log2 * grid / 4; gon[cell(m)][cell(s)] += 1.  A counter c, +1 per tick; when c mod hop == 0 the grid is emitted and cleared.
"""
import numpy as np

TICK_DTYPE = np.dtype({"names": ["sum_ll", "sum_rr", "sum_lr", "win_ll", "win_rr", "win_lr", "frames", "nonfinite"],
                       "formats": [np.float64] * 6 + [np.uint32] * 2,
                       "offsets": [0, 8, 16, 24, 32, 40, 48, 52], "itemsize": 56})   # mx_stereo_tick
SUMS = ("sum_ll", "sum_rr", "sum_lr")
WINS = ("win_ll", "win_rr", "win_lr")
GRIDS = (0, 64, 128)
HIST_TICKS = 1023


def record_bytes(grid: int) -> int:
    assert grid in GRIDS
    return 32 + 4 * grid * grid


def pair_sum(x: np.ndarray, y: np.ndarray) -> np.float64:
    """sum over one tick of x[f] * y[f] in the spec's order"""
    a, b = np.ascontiguousarray(x, np.float32).astype(np.float64), np.ascontiguousarray(y, np.float32).astype(np.float64)
    s = np.zeros(64, dtype=np.float64)
    with np.errstate(all="ignore"):
        for r0 in range(0, a.size, 64):   # row r0 // 64 of frames: each partial takes its next frame, in ascending f
            ra, rb = a[r0:r0 + 64], b[r0:r0 + 64]
            s[:ra.size] = s[:ra.size] + ra * rb
        lanes = np.arange(64)
        for k in (32, 16, 8, 4, 2, 1):
            s = s + s[lanes ^ k]
    return np.float64(s[0])


def cell(v, grid: int, zoom_log2: int) -> np.ndarray:
    """cell index 0 .. grid - 1 of the f32 value(s) v"""
    v = np.asarray(v, dtype=np.float32)
    z, h = np.float32(2 ** zoom_log2 * grid // 4), np.float32(grid // 2)
    with np.errstate(all="ignore"):
        t = np.floor(v * z).astype(np.float32)   # f32 product (exact unless it overflows to +-inf), floorf
    t = np.minimum(np.maximum(t, -h), h - np.float32(1.0))
    return t.astype(np.int64) + grid // 2


def plot(left: np.ndarray, right: np.ndarray, grid: int, zoom_log2: int):
    """(counts [grid, grid] uint32, plotted, skipped) of one tick"""
    l, r = np.ascontiguousarray(left, np.float32), np.ascontiguousarray(right, np.float32)
    ok = np.isfinite(l) & np.isfinite(r)
    l, r = l[ok], r[ok]
    with np.errstate(all="ignore"):
        m, s = (l + r).astype(np.float32), (l - r).astype(np.float32)   # one f32 rounding each; may overflow to +-inf
    g = np.zeros((grid, grid), dtype=np.uint32)
    np.add.at(g, (cell(m, grid, zoom_log2), cell(s, grid, zoom_log2)), 1)
    return g, int(ok.sum()), int((~ok).sum())


def correlation(ll: float, rr: float, lr: float) -> float:
    """mx_stereo_correlation"""
    with np.errstate(all="ignore"):
        p = np.float64(ll) * np.float64(rr)
        if not (p > 0 and np.isfinite(p)):
            return 0.0
        v = np.float64(lr) / np.sqrt(p)
    if np.isnan(v):
        return 0.0
    return float(min(1.0, max(-1.0, v)))


class StereoModel:
    """one tap: window history, hop counter and grid carried across run() calls"""

    def __init__(self, window_ticks: int = 180, grid: int = 0, zoom_log2: int = 0, hop: int = 1):
        assert 1 <= window_ticks <= 1024 and grid in GRIDS and 0 <= zoom_log2 <= 8 and (grid == 0 or hop >= 1)
        self.window_ticks, self.grid, self.zoom_log2, self.hop = window_ticks, grid, zoom_log2, hop
        self.hist = [(np.float64(0.0),) * 3] * (HIST_TICKS + 1)   # the current tick's sums and the 1023 before it
        self.c = 0
        if grid:
            self.gon = np.zeros((grid, grid), dtype=np.uint32)
            self.plotted = self.skipped = 0

    def run(self, port: np.ndarray, n_ticks: int):
        """port: the run's interleaved L R samples.  Returns (TICK_DTYPE[n_ticks], list of emitted goniometer records as dicts)."""
        x = np.ascontiguousarray(port, np.float32).reshape(n_ticks, -1, 2)
        rec = np.zeros(n_ticks, dtype=TICK_DTYPE)
        emitted = []
        for t in range(n_ticks):
            l, r = x[t, :, 0], x[t, :, 1]
            sums = (pair_sum(l, l), pair_sum(r, r), pair_sum(l, r))
            self.hist = self.hist[1:] + [sums]
            rec[t]["frames"] = l.size
            rec[t]["nonfinite"] = int((~(np.isfinite(l) & np.isfinite(r))).sum())
            with np.errstate(all="ignore"):
                for k in range(3):
                    rec[t][SUMS[k]] = sums[k]
                    w = np.float64(0.0)
                    for h in self.hist[-self.window_ticks:]:
                        w = w + h[k]
                    rec[t][WINS[k]] = w
            if self.grid:
                g, p, s = plot(l, r, self.grid, self.zoom_log2)
                self.gon += g; self.plotted += p; self.skipped += s
                self.c += 1
                if self.c % self.hop == 0:
                    emitted.append({"tick_in_run": t, "ticks": self.hop, "frames": self.plotted, "skipped": self.skipped, "grid": self.grid,
                                    "zoom_log2": self.zoom_log2, "reserved": (0, 0), "gon": self.gon.copy()})
                    self.gon[:] = 0; self.plotted = self.skipped = 0
        return rec, emitted


def records_equal(got: np.ndarray, want: np.ndarray) -> bool:
    """bit for bit; any NaN equals any NaN"""
    if got.shape != want.shape:
        return False
    for f in SUMS + WINS:
        a, b = np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f])
        if not np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))):
            return False
    return bool(np.array_equal(got["frames"], want["frames"]) and np.array_equal(got["nonfinite"], want["nonfinite"]))


def first_difference(got: np.ndarray, want: np.ndarray) -> str:
    for t in range(min(len(got), len(want))):
        if not records_equal(got[t:t + 1], want[t:t + 1]):
            return f"tick {t}: got {got[t]}, want {want[t]}"
    return f"lengths {len(got)} and {len(want)}"


def gonio_equal(got: dict, want: dict) -> bool:
    return all(got[k] == want[k] for k in ("tick_in_run", "ticks", "frames", "skipped", "grid", "zoom_log2", "reserved")) and \
        np.array_equal(got["gon"], want["gon"])
