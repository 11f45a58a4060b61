"""Spectrum taps (mixlab_gpu.h mx_graph_set_spectra) restated in numpy, bit for bit.

Per tap, tick and channel: the last N frames of the port's stream that end with the tick (zeros before the taps were set), times the
periodic Hann window in f32, packed as z = L + i R, through the radix-2 decimation-in-time data flow on bit-reversed input with every f32
operation rounded on its own (numpy's float32 ufuncs round each result; nothing here is fused), split into the two channels' bins, bin power
in f64 (exact products, one rounding), bands by the meters' 64-partial order, scaled by the exact 4 / N^2.

The tables come from mx_spectrum_tables -- the very ones the kernels use -- so the model needs no libm; tests/test_cpu_spectrum.py checks
them against a 60-digit evaluation, and the model's accuracy against an f64 transform.  Importable without a GPU (the tables are host code).
"""
from __future__ import annotations

import numpy as np

SIZES = (256, 512, 1024, 2048, 4096)
_tables = {}


def tables(n_fft: int):
    """(window f32[N], twiddle complex as (re f32[N/2], im f32[N/2]))"""
    if n_fft not in _tables:
        from mixlab_amd import abi
        _tables[n_fft] = abi.spectrum_tables(n_fft)
    return _tables[n_fft]


def bit_reverse(n_fft: int) -> np.ndarray:
    bits = n_fft.bit_length() - 1
    i = np.arange(n_fft)
    r = np.zeros(n_fft, dtype=np.int64)
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def fft_f32(re: np.ndarray, im: np.ndarray, n_fft: int):
    """the spec's transform of a batch of frames: re, im float32 [batch, N] (already windowed) -> Z re, im float32 [batch, N]"""
    _w, tre, tim = tables(n_fft)
    rev = bit_reverse(n_fft)
    re = np.ascontiguousarray(re[:, rev], dtype=np.float32)
    im = np.ascontiguousarray(im[:, rev], dtype=np.float32)
    batch = re.shape[0]
    h = 1
    with np.errstate(all="ignore"):
        while h < n_fft:
            step = n_fft // (2 * h)
            wr, wi = tre[::step][:h], tim[::step][:h]           # twiddle[k * N / (2h)], k < h
            r3, i3 = re.reshape(batch, -1, 2 * h), im.reshape(batch, -1, 2 * h)
            ar, ai, br, bi = r3[:, :, :h], i3[:, :, :h], r3[:, :, h:], i3[:, :, h:]
            t_re = br * wr - bi * wi                            # each product and the difference round to f32
            t_im = br * wi + bi * wr
            nr, ni = np.empty_like(r3), np.empty_like(i3)
            nr[:, :, :h], ni[:, :, :h] = ar + t_re, ai + t_im
            nr[:, :, h:], ni[:, :, h:] = ar - t_re, ai - t_im
            re, im = nr.reshape(batch, n_fft), ni.reshape(batch, n_fft)
            h *= 2
    return re, im


def band_powers(zre: np.ndarray, zim: np.ndarray, n_fft: int, edges) -> np.ndarray:
    """Z [batch, N] -> float32 [batch, 2, B]: split, f64 power, 64-partial band sums, exact scale"""
    edges = [int(e) for e in edges]
    k = np.arange(n_fft // 2 + 1)
    n = (n_fft - k) % n_fft
    with np.errstate(all="ignore"):
        l_re, l_im = zre[:, k] + zre[:, n], zim[:, k] - zim[:, n]   # f32
        r_re, r_im = zim[:, k] + zim[:, n], zre[:, n] - zre[:, k]
        out = np.zeros((zre.shape[0], 2, len(edges) - 1), dtype=np.float32)
        lanes = np.arange(64)
        scale = 4.0 / (float(n_fft) * float(n_fft))
        for c, (a, b) in enumerate(((l_re, l_im), (r_re, r_im))):
            a, b = a.astype(np.float64), b.astype(np.float64)
            p = a * a + b * b                                       # exact products, one rounding
            for j in range(len(edges) - 1):
                s = np.zeros((p.shape[0], 64), dtype=np.float64)
                for r0 in range(edges[j], edges[j + 1], 64):        # each partial takes its next bin, in ascending k
                    row = p[:, r0:min(r0 + 64, edges[j + 1])]
                    s[:, :row.shape[1]] = s[:, :row.shape[1]] + row
                for m in (32, 16, 8, 4, 2, 1):
                    s = s + s[:, lanes ^ m]
                out[:, c, j] = (s[:, 0] * scale).astype(np.float32)
    return out


class SpectrumModel:
    """one tap: feed it the port's samples run by run (mono: frames, stereo: interleaved 2 * frames); history starts as silence"""

    def __init__(self, channels: int, n_fft: int, edges):
        self.channels, self.n_fft, self.edges = channels, n_fft, [int(e) for e in edges]
        self.hist = np.zeros((n_fft, 2), dtype=np.float32)

    def run(self, samples: np.ndarray, n_ticks: int) -> np.ndarray:
        """-> float32 [n_ticks, 2, B]"""
        n = self.n_fft
        x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1, self.channels)
        assert n_ticks > 0 and x.shape[0] % n_ticks == 0
        f = x.shape[0] // n_ticks
        if self.channels == 1:
            x = np.concatenate([x, np.zeros_like(x)], axis=1)       # imaginary part +0.0
        stream = np.concatenate([self.hist, x], axis=0)
        ends = n + f * (np.arange(n_ticks) + 1)
        idx = ends[:, None] - n + np.arange(n)[None, :]
        w = tables(n)[0]
        with np.errstate(all="ignore"):
            re = stream[idx, 0] * w
            im = stream[idx, 1] * w if self.channels == 2 else np.zeros_like(re)
        self.hist = stream[-n:].copy()
        out = band_powers(*fft_f32(re, im, n), n, self.edges)
        if self.channels == 1:
            out[:, 1, :] = 0.0
        return out


def records_equal(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """bit for bit, except that any NaN equals any NaN"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
