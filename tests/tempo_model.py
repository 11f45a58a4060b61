"""The tempo taps' spec (include/mixlab_gpu.h, mx_graph_set_tempo) restated in numpy and Python integers -- what the kernels are held to, byte
for byte.

  q      m = L + R in f32 (a mono port: L = R = x); a non-finite m gives q = 0 and counts; else q = trunc(min(|m|, 4) * 2^20)
  E[h]   the sum of q^2 over stream frames [h H, (h + 1) H); A[h] = isqrt(E[h]), A[-1] = 0; o[h] = max(A[h] - A[h - 1], 0) >> 6
  R[l]   at an emission: sum over j < W of o[hl - j] * o[hl - j - l], hl the last hop complete at the end of the emitting tick
  c      one counter, +1 per tick; c mod emit_ticks == 0 emits

`variant` switches in ONE deliberate misreading of the text (tests/test_cpu_tempo.py shows that the shared cases catch each)."""
import math
import struct

import numpy as np

HOPS = (64, 128, 256)
VARIANTS = ("round_q", "no_clamp", "round_root", "shift_first", "keep_negative", "late_hop", "window_minus_1", "lag_forward", "c_per_run",
            "mid_halved")
F32 = np.float32


def record_bytes(max_lag: int) -> int:
    return 32 + 8 * max_lag


def check_params(hop_frames, window_hops, max_lag, emit_ticks) -> bool:
    return hop_frames in HOPS and 64 <= window_hops <= 4096 and 16 <= max_lag <= 1024 and max_lag <= window_hops and emit_ticks >= 1


def quantise(left, right, variant=None):
    """(q uint64[frames], non-finite mask) of one stretch of frames"""
    l, r = np.ascontiguousarray(left, F32), np.ascontiguousarray(right, F32)
    with np.errstate(all="ignore"):
        m = (l + r).astype(F32)                      # one f32 rounding; may overflow to +-inf
        if variant == "mid_halved":
            m = (m * F32(0.5)).astype(F32)
        bad = ~np.isfinite(m)
        a = np.abs(np.where(bad, F32(0.0), m)).astype(F32)
        a = np.minimum(a, F32(4.0) if variant != "no_clamp" else F32(1024.0))   # (the misreading still fits the integers)
        p = a.astype(np.float64) * 1048576.0         # exact (a power of two), as the f32 product is
        q = (np.rint(p) if variant == "round_q" else np.floor(p)).astype(np.uint64)
    return q, bad


def autocorrelation(hist: np.ndarray, W: int, L: int, variant=None) -> np.ndarray:
    """R[0 .. L) from the W + L - 1 onsets that end in o[hl]"""
    s = np.ascontiguousarray(hist, np.int64)
    assert s.size == W + L - 1
    n = W - 1 if variant == "window_minus_1" else W
    u = s[s.size - n:]                               # o[hl - n + 1 .. hl]
    out = np.zeros(L, np.uint64)
    if not u.any():
        return out
    for l in range(L):
        if variant == "lag_forward":                 # o[hl - j + l], what lies beyond hl reading 0
            v = np.concatenate([u[l:], np.zeros(min(l, n), np.int64)])[:n]
        else:
            v = s[s.size - n - l: s.size - l]
        out[l] = int(np.dot(u, v))                   # integer dot: exact, below 2^52
    return out


class TempoModel:
    """one tap: stream position, partial hop, last amplitude, onset history, non-finite count and c carried across run() calls"""

    def __init__(self, hop_frames=128, window_hops=2048, max_lag=512, emit_ticks=6, channels=2, variant=None):
        assert check_params(hop_frames, window_hops, max_lag, emit_ticks) and channels in (1, 2) and (variant is None or variant in VARIANTS)
        self.H, self.W, self.L, self.emit, self.channels, self.variant = hop_frames, window_hops, max_lag, emit_ticks, channels, variant
        self.pos = 0            # frames of the stream so far
        self.part = 0           # energy of the hop in progress
        self.a_prev = 0         # A of the last complete hop
        self.hops = 0           # complete hops
        self.hist = np.zeros(window_hops + max_lag, np.int64)   # ends in the last complete hop's onset (one more than an emission needs)
        self.nonfinite = 0
        self.c = 0

    def _root(self, e: int) -> int:
        if self.variant == "round_root":
            r = math.isqrt(e)
            return r + 1 if e - r * r > r else r     # nearest
        return math.isqrt(e)

    def _hop_done(self):
        a = self._root(self.part)
        if self.variant == "shift_first":
            o = max((a >> 6) - (self.a_prev >> 6), 0)
        elif self.variant == "keep_negative":
            o = abs(a - self.a_prev) >> 6
        else:
            o = max(a - self.a_prev, 0) >> 6
        self.a_prev, self.part = a, 0
        self.hist = np.concatenate([self.hist[1:], [o]])
        self.hops += 1

    def run(self, port, n_ticks: int):
        """port: the run's samples in the port's layout (interleaved L R, or mono).  Returns the run's records, one bytes object each."""
        if n_ticks == 0:
            return []
        x = np.ascontiguousarray(port, F32).reshape(n_ticks, -1, self.channels)
        F = x.shape[1]
        if self.variant == "c_per_run":
            self.c = 0
        out = []
        for t in range(n_ticks):
            l = x[t, :, 0]
            q, bad = quantise(l, x[t, :, self.channels - 1], self.variant)
            self.nonfinite += int(bad.sum())
            sq = q * q
            at = 0
            while at < F:
                take = min(F - at, self.H - self.pos % self.H)
                self.part += int(sq[at:at + take].sum())
                at += take; self.pos += take
                if self.pos % self.H == 0:
                    self._hop_done()
            self.c += 1
            if self.c % self.emit == 0:
                late = self.variant == "late_hop" and self.hops > 0 and self.pos % self.H == 0   # the hop that ends with this tick: not yet
                R = autocorrelation(self.hist[:-1] if late else self.hist[1:], self.W, self.L, self.variant)
                head = struct.pack("<8I", t, min(self.hops - late, 0xffffffff), self.nonfinite, self.H, self.W, self.L, 0, 0)
                out.append(head + R.astype("<u8").tobytes())
                self.nonfinite = 0
        return out


def parse_record(raw) -> dict:
    b = bytes(raw)
    t, hops, nonfinite, H, W, L, r0, r1 = struct.unpack_from("<8I", b, 0)
    return {"tick_in_run": t, "hops_complete": hops, "nonfinite": nonfinite, "hop_frames": H, "window_hops": W, "max_lag": L, "reserved": (r0, r1),
            "acf": np.frombuffer(b, "<u8", L, 32)}


def bpm(record, rate: float, bpm_lo: float, bpm_hi: float):
    """mx_tempo_bpm in f64: (bpm, confidence)"""
    r = parse_record(record)
    H, L, R = r["hop_frames"], r["max_lag"], r["acf"].astype(np.float64)
    lo = max(1, math.ceil(60.0 * rate / (H * bpm_hi)))
    hi = min(L - 2, math.floor(60.0 * rate / (H * bpm_lo)))
    if R[0] == 0.0 or lo > hi:
        return 0.0, 0.0
    ls = lo + int(np.argmax(R[lo:hi + 1]))           # the first maximum
    den = R[ls - 1] - 2.0 * R[ls] + R[ls + 1]
    d = 0.5 * (R[ls - 1] - R[ls + 1]) / den if den < 0.0 else 0.0
    return 60.0 * rate / (H * (ls + d)), R[ls] / R[0]


def click_track(rate: float, tempo: float, frames: int, seed: int = 0, click_frames: int = 4) -> np.ndarray:
    """mono: a click of `click_frames` frames at 0.9 every 60 * rate / tempo frames over noise at -40 dB"""
    rng = np.random.default_rng(seed)
    x = (rng.uniform(-1.0, 1.0, frames) * 0.01).astype(F32)
    period, k = 60.0 * rate / tempo, 0
    while round(k * period) + click_frames <= frames:
        at = round(k * period)
        x[at:at + click_frames] = F32(0.9)
        k += 1
    return x
