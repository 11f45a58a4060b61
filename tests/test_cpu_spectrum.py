"""Spectrum taps without a GPU: the tables the kernels use against a 60-digit evaluation, the accuracy of the spec itself (the numpy model,
tests/spectrum_model.py) against an f64 transform, and the ABI as the header declares it."""
import ctypes
import math
import pathlib
import re

import numpy as np
import pytest

import spectrum_model as sm
from mixlab_amd import abi

HEADER = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mixlab_gpu.h").read_text()
f32 = np.float32


def nearest_f32(v) -> np.float32:
    """the f32 nearest to the mpmath real v (ties cannot occur for the irrational entries; the rational ones are exact)"""
    import mpmath
    if v == 0:
        return f32(0.0)
    sign = -1 if v < 0 else 1
    a = abs(v)
    e = int(mpmath.floor(mpmath.log(a, 2)))
    ulp_exp = max(e, -126) - 23
    q = a / mpmath.mpf(2) ** ulp_exp
    n = int(mpmath.nint(q))   # round half to even
    return f32(sign * math.ldexp(n, ulp_exp))


@pytest.mark.parametrize("n_fft", sm.SIZES)
def test_tables_are_correctly_rounded_every_entry(n_fft):
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 60
    w, tre, tim = abi.spectrum_tables(n_fft)
    assert w.shape == (n_fft,) and tre.shape == (n_fft // 2,) and tim.shape == (n_fft // 2,)
    two_pi = 2 * mpmath.pi
    for i in range(n_fft):
        want = nearest_f32(mpmath.mpf("0.5") - mpmath.mpf("0.5") * mpmath.cos(two_pi * i / n_fft))
        assert w[i].view(np.uint32) == want.view(np.uint32), (n_fft, "window", i, w[i], want)
    for k in range(n_fft // 2):
        c, s = nearest_f32(mpmath.cos(two_pi * k / n_fft)), nearest_f32(-mpmath.sin(two_pi * k / n_fft))
        assert tre[k] == c and tim[k] == s, (n_fft, "twiddle", k, tre[k], c, tim[k], s)
    assert tre[0] == 1.0 and tim[0] == 0.0 and tre[n_fft // 4] == 0.0 and tim[n_fft // 4] == -1.0 and w[0] == 0.0 and w[n_fft // 2] == 1.0


def test_tables_refuse_other_sizes():
    buf = np.zeros(8192, np.float32)
    for n in (0, 128, 300, 8192):
        assert abi.lib.mx_spectrum_tables(n, buf.ctypes.data, buf.ctypes.data, buf.ctypes.data) == abi.MX_ERR_INVALID
        with pytest.raises(abi.MxError):
            abi.spectrum_tables(n)
    assert abi.lib.mx_spectrum_tables(256, None, None, None) == abi.MX_OK   # any table may be left out


def f64_bands(x: np.ndarray, n_fft: int, edges):
    """the same quantity in f64: x [N, 2] -> [2, B] band powers and the total power of both channels over all bins"""
    w = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(n_fft) / n_fft)
    out = np.zeros((2, len(edges) - 1))
    total = 0.0
    for c in range(2):
        p = np.abs(np.fft.rfft(x[:, c].astype(np.float64) * w)) ** 2 * 16.0 / (float(n_fft) ** 2)   # the split's L = 2 X; scale 4 / N^2
        total += p.sum()
        for j in range(len(edges) - 1):
            out[c, j] = p[edges[j]:edges[j + 1]].sum()
    return out, total


def bound_c(n_fft: int) -> float:
    """Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2: log2 N (mu + gamma_4 (sqrt 2 + mu)) ~ 6.66 u per stage with
    correctly rounded twiddles; + 4 for the window product, the split and the final roundings.  In units of 2^-24."""
    return 6.66 * math.log2(n_fft) + 4


def model_frame(x: np.ndarray, n_fft: int, edges) -> np.ndarray:
    """the model's [2, B] for the one frame x [N, 2] (a run of one tick of N frames from silence)"""
    return sm.SpectrumModel(2, n_fft, edges).run(x.reshape(-1), 1)[0]


@pytest.mark.parametrize("n_fft", sm.SIZES)
def test_accuracy_of_the_spec_against_f64(n_fft):
    rng = np.random.default_rng(n_fft)
    top = n_fft // 2 + 1
    layouts = [np.arange(top + 1), abi.log_band_edges(n_fft, 31, 20.0, 20000.0, 48000.0), np.array([0, top])]
    i = np.arange(n_fft)
    cases = {
        "noise L, quieter off-bin sine R": np.stack([rng.standard_normal(n_fft) * 0.3, 1e-3 * np.sin(2 * np.pi * 10.37 * i / n_fft)], 1),
        "noise both": rng.standard_normal((n_fft, 2)) * 0.5,
        "loud sine L, silence R": np.stack([np.sin(2 * np.pi * 33 * i / n_fft), np.zeros(n_fft)], 1),
    }
    worst = 0.0
    for name, x in cases.items():
        x = x.astype(np.float32)
        for edges in layouts:
            got = model_frame(x, n_fft, edges).astype(np.float64)
            want, total = f64_bands(x, n_fft, [int(e) for e in edges])
            err = np.abs(np.sqrt(got) - np.sqrt(want)).max()
            unit = 2.0 ** -24 * math.sqrt(total)
            worst = max(worst, err / unit)
            assert err <= bound_c(n_fft) * unit, (name, n_fft, len(edges) - 1, err / unit, bound_c(n_fft))
    print(f"n_fft {n_fft}: worst error {worst:.2f} units of 2^-24 sqrt(total power), bound {bound_c(n_fft):.1f}")


@pytest.mark.parametrize("n_fft", sm.SIZES)
def test_unit_sine_on_a_bin_centre_reads_one_and_silence_reads_zero(n_fft):
    i = np.arange(n_fft)
    k0 = n_fft // 8 + 3
    x = np.stack([np.sin(2 * np.pi * k0 * i / n_fft), np.zeros(n_fft)], 1).astype(np.float32)
    edges = [0, k0 - 1, k0, k0 + 1, k0 + 2, n_fft // 2 + 1]   # the window spreads a bin-centred sine over k0 - 1 .. k0 + 1
    got = model_frame(x, n_fft, edges)
    _, total = f64_bands(x, n_fft, edges)
    unit = 2.0 ** -24 * math.sqrt(total)   # total: 1 + 1/4 + 1/4
    assert abs(total - 1.5) < 1e-6
    assert abs(math.sqrt(float(got[0, 2])) - 1.0) <= bound_c(n_fft) * unit   # the bin's own band: 0 dB
    assert abs(math.sqrt(float(got[0, 1])) - 0.5) <= bound_c(n_fft) * unit and abs(math.sqrt(float(got[0, 3])) - 0.5) <= bound_c(n_fft) * unit
    assert math.sqrt(float(got[0, 0])) <= bound_c(n_fft) * unit and math.sqrt(float(got[0, 4])) <= bound_c(n_fft) * unit
    assert all(math.sqrt(float(v)) <= bound_c(n_fft) * unit for v in got[1])   # the silent channel: the other's rounding floor at most
    mono = sm.SpectrumModel(1, n_fft, edges).run(x[:, 0], 1)[0]
    assert abs(math.sqrt(float(mono[0, 2])) - 1.0) <= bound_c(n_fft) * unit and not mono[1].any()
    zero = model_frame(np.zeros((n_fft, 2), np.float32), n_fft, edges)
    assert not zero.view(np.uint32).any()   # +0.0 exactly, every band, both channels


def test_model_transform_is_the_plain_radix_2_recursion():
    """the vectorised stages against a scalar, element-by-element restatement of the header's data flow (f32 at every step)"""
    n = 256
    rng = np.random.default_rng(1)
    re, im = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    _w, tre, tim = sm.tables(n)
    rev = sm.bit_reverse(n)
    zr, zi = [f32(v) for v in re[rev]], [f32(v) for v in im[rev]]
    h = 1
    while h < n:
        for b in range(0, n, 2 * h):
            for k in range(h):
                wr, wi = tre[k * n // (2 * h)], tim[k * n // (2 * h)]
                br, bi = zr[b + k + h], zi[b + k + h]
                t_re = f32(f32(br * wr) - f32(bi * wi)); t_im = f32(f32(br * wi) + f32(bi * wr))
                ar, ai = zr[b + k], zi[b + k]
                zr[b + k], zi[b + k] = f32(ar + t_re), f32(ai + t_im)
                zr[b + k + h], zi[b + k + h] = f32(ar - t_re), f32(ai - t_im)
        h *= 2
    gr, gi = sm.fft_f32(re[None, :], im[None, :], n)
    assert np.array_equal(gr[0].view(np.uint32), np.array(zr, f32).view(np.uint32))
    assert np.array_equal(gi[0].view(np.uint32), np.array(zi, f32).view(np.uint32))
    # and it is a DFT: close to numpy's
    want = np.fft.fft(re.astype(np.float64) + 1j * im.astype(np.float64))
    assert np.abs((gr[0] + 1j * gi[0]) - want).max() < 1e-4


def test_band_sum_follows_the_partials_and_butterfly():
    n = 1024
    rng = np.random.default_rng(2)
    zr = (rng.standard_normal((1, n)) * np.exp2(rng.integers(-30, 30, n))).astype(f32)
    zi = (rng.standard_normal((1, n)) * np.exp2(rng.integers(-30, 30, n))).astype(f32)
    edges = [3, 4, 200, 513]   # one bin, > 64 bins, > 256 bins
    got = sm.band_powers(zr, zi, n, edges)
    k = np.arange(n // 2 + 1); m = (n - k) % n
    lre, lim = (zr[0, k] + zr[0, m]).astype(f32), (zi[0, k] - zi[0, m]).astype(f32)
    p = [float(a) * float(a) + float(b) * float(b) for a, b in zip(lre, lim)]
    for j in range(3):
        s = [0.0] * 64
        for kk in range(edges[j], edges[j + 1]):
            s[(kk - edges[j]) % 64] = s[(kk - edges[j]) % 64] + p[kk]
        for mm in (32, 16, 8, 4, 2, 1):
            s = [s[q] + s[q ^ mm] for q in range(64)]
        assert got[0, 0, j].view(np.uint32) == f32(s[0] * (4.0 / (n * n))).view(np.uint32), j


def test_model_history_across_runs_and_first_ticks_see_silence():
    n, f = 1024, 735
    x = (np.random.default_rng(3).standard_normal(6 * f * 2)).astype(f32)
    edges = abi.log_band_edges(n, 12, 40.0, 16000.0, 44100.0)
    whole = sm.SpectrumModel(2, n, edges).run(x, 6)
    m = sm.SpectrumModel(2, n, edges)
    parts = np.concatenate([m.run(x[:2 * f], 1), m.run(x[2 * f:8 * f], 3), m.run(x[8 * f:], 2)])
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    # tick 0 is the transform of 289 zeros and the tick's 735 frames
    fr = np.concatenate([np.zeros((n - f, 2), f32), x[:2 * f].reshape(-1, 2)])
    assert np.array_equal(whole[0].view(np.uint32), model_frame(fr, n, edges).view(np.uint32))


def test_log_band_edges_ascend_within_range():
    for n_fft in sm.SIZES:
        for b in (1, 2, 31, 64, 128):
            for lo, hi, rate in ((20.0, 20000.0, 48000.0), (20.0, 22050.0, 44100.0), (1.0, 100.0, 48000.0), (100.0, 96000.0, 48000.0)):
                e = abi.log_band_edges(n_fft, b, lo, hi, rate)
                assert e.dtype == np.uint16 and e.shape == (b + 1,)
                assert (np.diff(e.astype(np.int64)) > 0).all() and int(e[-1]) <= n_fft // 2 + 1, (n_fft, b, lo, hi, e)
    e = abi.log_band_edges(4096, 31, 20.0, 20000.0, 48000.0)
    assert abs(int(e[-1]) - round(20000.0 * 4096 / 48000.0)) <= 1   # where the bins are dense the edges are the log-spaced ones
    for bad in ((256, 0, 20.0, 2e4, 48e3), (256, 129, 20.0, 2e4, 48e3), (256, 4, 0.0, 2e4, 48e3), (256, 4, 30.0, 20.0, 48e3)):
        with pytest.raises(ValueError):
            abi.log_band_edges(*bad)


def test_header_struct_layout_and_symbols():
    body = re.search(r"typedef struct \{([^}]*)\} mx_spectrum_params;", HEADER).group(1)
    fields = [" ".join(ln.split("/*")[0].split()).rstrip(";") for ln in body.strip().splitlines()]
    assert fields == ["uint32_t n_fft", "uint32_t n_bands", "const uint16_t* edges"]

    class Params(ctypes.Structure):   # the header's struct, field by field
        _fields_ = [("n_fft", ctypes.c_uint32), ("n_bands", ctypes.c_uint32), ("edges", ctypes.POINTER(ctypes.c_uint16))]
    assert ctypes.sizeof(Params) == 16 and ctypes.sizeof(abi.SpectrumParams) == 16
    assert [getattr(abi.SpectrumParams, f).offset for f in ("n_fft", "n_bands", "edges")] == [0, 4, 8]
    for name in ("mx_graph_set_spectra", "mx_graph_read_spectra", "mx_spectrum_tables"):
        assert hasattr(abi.lib, name)
    assert re.search(r"int mx_graph_set_spectra\(mx_graph\* g, const mx_port_ref\* ports, size_t n, const mx_spectrum_params\* params\);", HEADER)
    assert re.search(r"int mx_graph_read_spectra\(mx_graph\* g, uint32_t first_tick_in_run, uint32_t n_ticks, float\* dst, size_t cap\);", HEADER)
    assert re.search(r"int mx_spectrum_tables\(uint32_t n_fft, float\* window, float\* twiddle_re, float\* twiddle_im\);", HEADER)
    # taps, not a kind: the kind table, the profile's per-kind floats and the ABI version are what they were
    assert abi.KIND_COUNT == 19 and abi.PROFILE_KINDS == 18
    assert "MX_KIND_COUNT = 19" in HEADER and "#define MX_PROFILE_KINDS 18" in HEADER and "#define MX_ABI_VERSION 4u" in HEADER
    note = HEADER[HEADER.index("#define MX_ABI_VERSION"):HEADER.index("/* ---- status codes")]
    for name in ("mx_spectrum_params", "mx_graph_set_spectra", "mx_graph_read_spectra", "mx_spectrum_tables"):
        assert name in note


def test_null_graph_is_refused_without_a_device():
    assert abi.lib.mx_graph_set_spectra(None, None, 0, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_read_spectra(None, 0, 0, None, 0) == abi.MX_ERR_INVALID
