"""The tonality taps' spec (include/mixlab_gpu.h, mx_graph_set_tonality) restated in numpy and Python integers -- what the kernels are held to,
byte for byte.  The tables (the decimator's taps c, the kernels' lengths N_b and coefficients K) are taken from mx_tonality_tables, as
spectrum_model.py takes its tables, so the model needs no libm; tests/test_cpu_tonality.py checks the tables themselves against mpmath.

  q      m = L + R in f32 (a mono port: L = R = x); a non-finite m gives q = 0 and counts; else q = trunc(clamp(m, -2, 2) * 2^13)
  d[n]   (sum over k < 8 D of c[k] * q[n D - k]) >> 15 (floor), complete in the tick that holds input frame n D
  M_b[h] isqrt((S_re >> 10)^2 + (S_im >> 10)^2), S = sum over n < N_b of K[b][n] * d[e_h - (N_b - 1) + n], e_h = (h + 1) Hc - 1; complete
         in the tick that holds input frame e_h D
  C[b]   at an emission: the sum of M_b[h] over the hops completed since the previous emission
  c      one counter, +1 per tick; c mod emit_ticks == 0 emits

`variant` switches in ONE deliberate misreading of the text (tests/test_cpu_tonality.py shows that the shared cases catch each)."""
import math
import struct

import numpy as np

from mixlab_amd import abi

VARIANTS = ("round_q", "clamp_4", "shift_to_zero", "late_d", "left_aligned", "len_floored", "late_hop", "nonfinite_per_decimated", "no_reset",
            "left_only", "root_up", "c_per_run")
F32 = np.float32
Q = 17
PROFILES = ((6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88),
            (6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17))


def record_bytes(octaves: int) -> int:
    return 32 + 96 * octaves


def check_params(decim, hop_frames, octaves, f_lo_mhz, emit_ticks) -> bool:
    return decim in (4, 8) and hop_frames in (128, 256, 512) and 2 <= octaves <= 6 and f_lo_mhz >= 1 and emit_ticks >= 1


def quantise(left, right, variant=None):
    """(q int64[frames], non-finite mask) of one stretch of frames"""
    l, r = np.ascontiguousarray(left, F32), np.ascontiguousarray(right, F32)
    with np.errstate(all="ignore"):
        m = l if variant == "left_only" else (l + r).astype(F32)   # one f32 rounding; may overflow to +-inf
        bad = ~np.isfinite(m)
        lim = F32(4.0) if variant == "clamp_4" else F32(2.0)
        a = np.clip(np.where(bad, F32(0.0), m), -lim, lim).astype(np.float64) * 8192.0   # exact (a power of two), as the f32 product is
        q = (np.rint(a) if variant == "round_q" else np.trunc(a)).astype(np.int64)
    return q, bad


_tables = {}


def tables(rate, decim, hop_frames, octaves, f_lo_mhz):
    """(c int64[8 D], N_b list, [K_re int64[N_b]], [K_im int64[N_b]]) from mx_tonality_tables"""
    key = (float(rate), decim, hop_frames, octaves, f_lo_mhz)
    if key not in _tables:
        fir, ln, kern = abi.tonality_tables(rate, decim, hop_frames, octaves, f_lo_mhz)
        off = np.concatenate([[0], np.cumsum(ln.astype(np.int64))])
        k = kern.astype(np.int64)
        _tables[key] = (fir.astype(np.int64), [int(x) for x in ln], [k[off[b]:off[b + 1], 0] for b in range(ln.size)], [k[off[b]:off[b + 1], 1] for b in range(ln.size)])
    return _tables[key]


def floored_kernels(rate, decim, octaves, f_lo_mhz):
    """the len_floored misreading: N_b = floor(Q fs_d / f_b), kernels by the spec's formulas for that length (numpy's libm: only a misreading)"""
    fs_d, out = rate / decim, ([], [], [])
    for b in range(12 * octaves):
        f = f_lo_mhz / 1000.0 * 2.0 ** (b / 12.0)
        N = int(math.floor(Q * fs_d / f))
        n = np.arange(N)
        w = 0.5 - 0.5 * np.cos(2 * np.pi * (n + 1) / (N + 1))
        phi = 2 * np.pi * f * (n - (N - 1)) / fs_d
        out[0].append(N); out[1].append(np.rint(16384 * w * np.cos(phi)).astype(np.int64)); out[2].append(np.rint(-16384 * w * np.sin(phi)).astype(np.int64))
    return out


class TonalityModel:
    """one tap: stream position, quantised and decimated history, sums, counts and c carried across run() calls"""

    def __init__(self, rate, decim=8, hop_frames=512, octaves=5, f_lo_mhz=65406, emit_ticks=30, channels=2, variant=None):
        assert check_params(decim, hop_frames, octaves, f_lo_mhz, emit_ticks) and channels in (1, 2) and (variant is None or variant in VARIANTS)
        self.D, self.Hc, self.O, self.f_lo_mhz, self.emit, self.channels, self.variant = decim, hop_frames, octaves, f_lo_mhz, emit_ticks, channels, variant
        self.B, self.Tf = 12 * octaves, 8 * decim
        self.c_fir, self.N, self.Kre, self.Kim = tables(rate, decim, hop_frames, octaves, f_lo_mhz)
        if variant == "len_floored":
            self.N, self.Kre, self.Kim = floored_kernels(rate, decim, octaves, f_lo_mhz)
        self.pos = 0                                   # frames of the stream so far
        self.qtail = np.zeros(self.Tf - 1, np.int64)   # the newest quantised frames
        self.d = np.zeros(2048, np.int64)              # 2048 zeros (d at a negative index), then every decimated frame so far
        self.hops_done = 0                             # hops whose magnitudes are in C or in an emitted record
        self.C = [0] * self.B
        self.hops = 0                                  # ... since the previous emission
        self.nonfinite = 0
        self.c = 0

    def _decimated(self, frames: int) -> int:
        """decimated frames complete once `frames` frames of the stream have arrived: the n with n D < frames"""
        if self.variant == "late_d":                   # ... with n D + 1 < frames
            return max(0, -(-(frames - 1) // self.D))
        return -(-frames // self.D)

    def _hop(self, h: int):
        e = (h + 1) * self.Hc - 1
        for b in range(self.B):
            N = self.N[b]
            at = 2048 + e - 2047 if self.variant == "left_aligned" else 2048 + e - (N - 1)
            x = self.d[at:at + N]
            re, im = int(np.dot(self.Kre[b], x)), int(np.dot(self.Kim[b], x))   # int64 dots: exact, |S| <= 2^40
            v = (re >> 10) ** 2 + (im >> 10) ** 2
            r = math.isqrt(v)
            self.C[b] += r + 1 if self.variant == "root_up" and r * r < v else r
        self.hops += 1

    def run(self, port, n_ticks: int):
        """port: the run's samples in the port's layout (interleaved L R, or mono).  Returns the run's records, one bytes object each."""
        if n_ticks == 0:
            return []
        x = np.ascontiguousarray(port, F32).reshape(n_ticks, -1, self.channels)
        F, D, Tf = x.shape[1], self.D, self.Tf
        if self.variant == "c_per_run":
            self.c = 0
        q, bad = quantise(x[:, :, 0].reshape(-1), x[:, :, self.channels - 1].reshape(-1), self.variant)
        # every decimated frame whose input frame n D lies in the run (late_d completes the last of them a tick late: it is formed here all the same)
        n0, n1 = -(-self.pos // D), -(-(self.pos + n_ticks * F) // D)
        qbuf = np.concatenate([self.qtail, q])         # qbuf[i] is stream frame pos - (Tf - 1) + i
        if n1 > n0:
            newest = np.arange(n0, n1) * D - self.pos + Tf - 1            # index of q[n D] in qbuf
            win = np.lib.stride_tricks.sliding_window_view(qbuf, Tf)[newest - (Tf - 1)]   # q[n D - (Tf - 1) .. n D]
            acc = win @ self.c_fir[::-1]
            if self.variant == "shift_to_zero":
                dn = np.where(acc < 0, -((-acc) >> 15), acc >> 15)
            else:
                dn = acc >> 15                          # arithmetic: floor
            assert np.abs(dn).max(initial=0) < 32767 or self.variant == "clamp_4"
            self.d = np.concatenate([self.d, dn])
        self.qtail = qbuf[qbuf.size - (Tf - 1):]
        out = []
        for t in range(n_ticks):
            b_t = bad[t * F:(t + 1) * F]
            if self.variant == "nonfinite_per_decimated":
                first = (-self.pos) % D                # only the frames n D count
                self.nonfinite += int(b_t[first::D].sum())
            else:
                self.nonfinite += int(b_t.sum())
            self.pos += F
            done = self._decimated(self.pos) // self.Hc
            if self.variant == "late_hop":             # assigned to the tick after the one that holds its last frame
                done = self._decimated(self.pos - F) // self.Hc
            while self.hops_done < done:
                self._hop(self.hops_done)
                self.hops_done += 1
            self.c += 1
            if self.c % self.emit == 0:
                head = struct.pack("<8I", t, self.hops, self.nonfinite, D, self.Hc, self.O, self.f_lo_mhz, 0)
                out.append(head + struct.pack(f"<{self.B}Q", *self.C))
                self.nonfinite = 0
                if self.variant != "no_reset":
                    self.C, self.hops = [0] * self.B, 0
        return out


def parse_record(raw) -> dict:
    b = bytes(raw)
    t, hops, nonfinite, D, Hc, O, f_lo_mhz, res = struct.unpack_from("<8I", b, 0)
    return {"tick_in_run": t, "hops": hops, "nonfinite": nonfinite, "decim": D, "hop_frames": Hc, "octaves": O, "f_lo_mhz": f_lo_mhz, "reserved": res,
            "cq": np.frombuffer(b, "<u8", 12 * O, 32)}


def chroma(records, rate: float) -> np.ndarray:
    """mx_tonality_chroma in f64"""
    recs = [parse_record(r) for r in records]
    r0 = recs[0]
    assert all((r["decim"], r["hop_frames"], r["octaves"], r["f_lo_mhz"]) == (r0["decim"], r0["hop_frames"], r0["octaves"], r0["f_lo_mhz"]) for r in recs)
    N = tables(rate, r0["decim"], r0["hop_frames"], r0["octaves"], r0["f_lo_mhz"])[1]
    shift = round(12 * math.log2(r0["f_lo_mhz"] / 1000.0 / 16.351597831))
    pc = [0.0] * 12
    for b in range(12 * r0["octaves"]):
        pc[(shift + b) % 12] += float(sum(int(r["cq"][b]) for r in recs)) / N[b]
    total = sum(pc)
    return np.array([v / total if total > 0 else 0.0 for v in pc])


def key(ch):
    """mx_tonality_key in f64: (key, confidence)"""
    ch = np.asarray(ch, np.float64)
    if ch.max() == ch.min():                           # no variance: no correlation
        return -1, 0.0
    rs = [float(np.corrcoef(np.roll(ch, -t), PROFILES[m])[0, 1]) for m in range(2) for t in range(12)]
    best = int(np.argmax(rs))                          # the first maximum
    return best, rs[best] - max(rs[:best] + rs[best + 1:])


def tone(rate: float, freq: float, frames: int, start: int = 0) -> np.ndarray:
    """a four-harmonic tone, amplitudes 1, 1/2, 1/3, 1/4, in f64"""
    t = (np.arange(frames) + start) / rate
    return sum(np.sin(2 * np.pi * freq * k * t) / k for k in (1, 2, 3, 4))


def cadence(rate: float, tonic_pc: int, minor: bool, seconds: float = 8.0) -> np.ndarray:
    """mono f32: I-IV-V-I (minor: i-iv-v-i, the natural minor's triads) in root position around C3 .. C5, each chord a quarter of the time,
    every note a four-harmonic tone, peak about 0.5"""
    third = 3 if minor else 4
    n = int(seconds * rate) // 4
    out = []
    for k, degree in enumerate((0, 5, 7, 0)):
        root = 48 + (tonic_pc + degree) % 12           # MIDI 48 = C3
        chord = sum(tone(rate, 440.0 * 2.0 ** ((root + s - 69) / 12.0), n, k * n) for s in (0, third, 7))
        out.append(chord)
    x = np.concatenate(out)
    return (x * (0.5 / np.abs(x).max())).astype(F32)
