"""Loudness taps without a GPU: the tables the kernels use against the standard's printed ones and a 60-digit evaluation, the conformance
of the spec (the numpy model, tests/loudness_model.py, with mx_loudness_gate) to EBU Tech 3341 / 3342 style signals, the accuracy of the
tick decomposition and of the interpolator, the model's own invariants, and the ABI as the header declares it."""
import ctypes
import math
import pathlib
import re

import numpy as np
import pytest

import loudness_model as lm
from mixlab_amd import abi
from test_cpu_spectrum import nearest_f32

HEADER = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mixlab_gpu.h").read_text()
RATES = [(48000, 800), (44100, 735)]

# ITU-R BS.1770-4, tables 1 and 2 (48 kHz), to their printed digits
BS1770_SHELF = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
BS1770_HIGH_PASS = (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)


def test_biquads_at_48k_are_the_printed_tables_and_carry_is_the_models():
    bq, carry, interp = abi.loudness_tables(48000.0, 800)
    assert bq.shape == (10,) and carry.shape == (4, 4) and interp.shape == (3, 12)
    for got, want in zip(bq, BS1770_SHELF + BS1770_HIGH_PASS):
        assert abs(got - want) < 5e-15, (got, want)   # half a unit of the 14th printed decimal
    for rate, frames in RATES + [(96000, 1600), (8000, 1), (48000, 48)]:
        bq, carry, _ = abi.loudness_tables(rate, frames)
        assert np.array_equal(carry.view(np.uint64), lm.carry_matrix(bq, frames).view(np.uint64)), (rate, frames)
    # the interpolator depends on neither argument
    assert abi.loudness_tables(44100.0, 735)[2].tobytes() == interp.tobytes()


def test_interpolator_is_correctly_rounded_every_entry():
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 60
    interp = abi.loudness_tables(48000.0, 800)[2]
    for p in (1, 2, 3):
        for j in range(12):
            d = mpmath.mpf(j - 5) - mpmath.mpf(p) / 4
            want = nearest_f32(mpmath.sin(mpmath.pi * d) / (mpmath.pi * d) * (mpmath.mpf("0.5") + mpmath.mpf("0.5") * mpmath.cos(mpmath.pi * d / 6)))
            assert interp[p - 1, j].view(np.uint32) == want.view(np.uint32), (p, j, interp[p - 1, j], want)


def test_tables_refuse_bad_arguments():
    bq, carry, interp = np.zeros(10), np.zeros(16), np.zeros(36, np.float32)
    args = (bq.ctypes.data, carry.ctypes.data, interp.ctypes.data)
    for rate, frames in ((0.0, 800), (-48000.0, 800), (float("nan"), 800), (float("inf"), 800), (3000.0, 50), (48000.0, 0), (48000.0, (1 << 22) + 1)):
        assert abi.lib.mx_loudness_tables(rate, frames, *args) == abi.MX_ERR_INVALID, (rate, frames)
        with pytest.raises(abi.MxError):
            abi.loudness_tables(rate, frames)
    assert abi.lib.mx_loudness_tables(48000.0, 800, None, None, None) == abi.MX_OK   # any table may be left out
    assert abi.lib.mx_loudness_tables(5400.0, 90, *args) == abi.MX_OK               # the lowest rate of tests/tick_shapes.py


# ---- conformance: the tolerances are EBU Tech 3341's (+-0.1 LU) and Tech 3341's true-peak case (+0.2 / -0.4 dB) ----

def sine(rate, seconds, dbfs, freq=1000.0, phase=0.0, start=0):
    t = start + np.arange(int(round(seconds * rate)))
    return (10.0 ** (dbfs / 20.0) * np.sin(2 * np.pi * freq * t / rate + phase)).astype(np.float32)


def measure(rate, frames, mono_stream):
    """the stereo programme with `mono_stream` on both channels through the model: records of whole ticks"""
    n = len(mono_stream) // frames
    x = mono_stream[:n * frames]
    return lm.LoudnessModel(2, rate, frames).run(np.stack([x, x], 1).reshape(-1), n)


def integrated(rec, frames, m=24, hop=6):
    """blocks of m ticks every hop ticks, the first one complete"""
    return abi.loudness_gate(rec["momentary_sq"][m - 1::hop], m * frames)[0]


@pytest.mark.parametrize("rate,frames", RATES)
@pytest.mark.parametrize("level", [-23.0, -33.0])
def test_steady_sine_reads_its_level_in_m_s_and_i(rate, frames, level):
    rec = measure(rate, frames, sine(rate, 20.0, level))
    got_m = abi.lufs(rec["momentary_sq"][-1], 24 * frames)
    got_s = abi.lufs(rec["short_sq"][-1], 180 * frames)
    got_i = integrated(rec, frames)
    print(f"{rate} Hz, {level} dBFS: M {got_m:.4f}, S {got_s:.4f}, I {got_i:.4f} LUFS")
    for got in (got_m, got_s, got_i):
        assert abs(got - level) <= 0.1, (got_m, got_s, got_i)


def sequence(rate, parts):
    out, at = [], 0
    for seconds, dbfs in parts:
        out.append(sine(rate, seconds, dbfs, start=at))
        at += len(out[-1])
    return np.concatenate(out)


@pytest.mark.parametrize("rate,frames", RATES)
@pytest.mark.parametrize("name,parts", [
    ("steps", [(10, -36.0), (60, -23.0), (10, -36.0)]),
    ("absolute gate", [(10, -72.0), (10, -36.0), (60, -23.0), (10, -36.0), (10, -72.0)]),
    ("relative gate", [(20, -26.0), (20.1, -20.0), (20, -26.0)]),
])
def test_gated_integration_reads_minus_23(rate, frames, name, parts):
    rec = measure(rate, frames, sequence(rate, parts))
    got = integrated(rec, frames)
    print(f"{rate} Hz, {name}: I {got:.4f} LUFS")
    assert abs(got - (-23.0)) <= 0.1, got


@pytest.mark.parametrize("rate,frames", RATES)
def test_true_peak_of_a_quarter_rate_sine(rate, frames):
    n = 30
    x = (0.5 * np.sin(2 * np.pi * np.arange(n * frames) / 4.0 + np.pi / 4)).astype(np.float32)
    rec = lm.LoudnessModel(1, rate, frames).run(x, n)
    got = 20.0 * math.log10(float(rec["true_peak"][1:, 0].max()))
    print(f"{rate} Hz: true peak {got:.3f} dBTP (sample peak {20 * math.log10(float(np.abs(x).max())):.3f} dBFS)")
    assert -6.0 - 0.4 <= got <= -6.0 + 0.2, got
    assert np.array_equal(rec["true_peak"][:, 1], np.zeros(n, np.float32)) and (rec["channels"] == 1).all()


def test_gate_edge_cases():
    assert abi.loudness_gate([], 19200) == (-math.inf, 0)
    assert abi.loudness_gate([0.0, 0.0], 19200) == (-math.inf, 0)
    quiet = 19200 * 10.0 ** ((-71.0 + 0.691) / 10.0)   # a block at -71 LUFS: below the absolute gate
    assert abi.loudness_gate([quiet] * 5, 19200) == (-math.inf, 0)
    loud = 19200 * 10.0 ** ((-20.0 + 0.691) / 10.0)
    got, kept = abi.loudness_gate([loud, quiet, loud], [19200, 19200, 19200])
    assert kept == 2 and abs(got - (-20.0)) < 1e-9
    out = ctypes.c_double()
    sq, fr = np.ones(2), np.array([100, 0], np.uint32)
    assert abi.lib.mx_loudness_gate(sq.ctypes.data, fr.ctypes.data, 2, ctypes.byref(out), None) == abi.MX_ERR_INVALID   # a block of 0 frames
    assert abi.lib.mx_loudness_gate(None, None, 2, ctypes.byref(out), None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_loudness_gate(sq.ctypes.data, fr.ctypes.data, 1, None, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_loudness_gate(sq.ctypes.data, fr.ctypes.data, 1, ctypes.byref(out), None) == abi.MX_OK   # blocks_kept may be NULL


# ---- accuracy of the specification, independent of the device ----

# Worst relative deviation of a tick's ksq from the uninterrupted f64 recurrence (scipy lfilter over the whole stream) seen with this
# model: 1.37e-12 of the programme's loudest tick, on a 40 Hz sine at 44.1 kHz.  The bound is twice that.
KSQ_REL_BOUND = 2 * 1.37e-12
# Worst reading of the interpolator against the continuous sine's peak (dense f64 evaluation), 20 Hz .. 20 kHz at 48 kHz, 13 phases:
# under-read -0.256 dB, over-read +0.077 dB.  The bounds are twice those.
TP_UNDER_BOUND_DB, TP_OVER_BOUND_DB = 2 * 0.256, 2 * 0.077


@pytest.mark.parametrize("rate,frames", RATES)
def test_ksq_against_the_uninterrupted_f64_recurrence(rate, frames):
    signal = pytest.importorskip("scipy.signal")
    bq = lm.tables(rate, frames)[0]
    n = 120
    rng = np.random.default_rng(rate)
    cases = {"noise": (rng.standard_normal(n * frames) * 0.25).astype(np.float32), "1 kHz -23 dBFS": sine(rate, n * frames / rate, -23.0),
             "40 Hz -10 dBFS": sine(rate, n * frames / rate, -10.0, freq=40.0)}
    worst = 0.0
    for name, x in cases.items():
        y = x.astype(np.float64)
        for k in (0, 1):
            y = signal.lfilter(bq[5 * k:5 * k + 3], np.concatenate([[1.0], bq[5 * k + 3:5 * k + 5]]), y)
        want = (y * y).reshape(n, frames).sum(axis=1)
        got = lm.LoudnessModel(1, rate, frames).run(x, n)["ksq"][:, 0]
        rel = float(np.abs(got - want).max() / want.max())   # against the programme's loudest tick: a tick at a zero of the envelope has no scale of its own
        worst = max(worst, rel)
        assert rel <= KSQ_REL_BOUND, (name, rel)
    print(f"{rate} Hz: worst |ksq - f64 recurrence| / max ksq = {worst:.3e} (bound {KSQ_REL_BOUND:.1e})")


def test_interpolator_against_the_continuous_sine():
    rate, frames, n = 48000, 800, 4
    under, over = 0.0, 0.0
    t = np.arange(n * frames)
    for freq in (20.0, 100.0, 997.0, 3000.0, 6000.0, 9000.0, 11000.0, 12000.0, 13000.0, 15000.0, 17000.0, 19000.0, 20000.0):
        for ph in range(13):
            phase = 2 * np.pi * ph / 13
            x = (0.5 * np.sin(2 * np.pi * freq * t / rate + phase)).astype(np.float32)
            rec = lm.LoudnessModel(1, rate, frames).run(x, n)
            got = 20.0 * math.log10(float(rec["true_peak"][1:, 0].max()))   # ticks behind the interpolator's run-in
            dense = np.abs(0.5 * np.sin(2 * np.pi * freq * np.arange(frames * 64, n * frames * 64) / (64.0 * rate) + phase)).max()
            err = got - 20.0 * math.log10(float(dense))
            under, over = min(under, err), max(over, err)
    print(f"interpolator vs continuous peak: worst under-read {under:.3f} dB, worst over-read {over:+.3f} dB")
    assert under >= -TP_UNDER_BOUND_DB and over <= TP_OVER_BOUND_DB, (under, over)


# ---- the model itself ----

def test_model_split_anywhere_gives_the_same_records_and_first_ticks_see_silence():
    rate, f, n = 44100, 735, 40
    x = np.random.default_rng(3).standard_normal(n * f * 2).astype(np.float32)
    whole = lm.LoudnessModel(2, rate, f, 5, 17).run(x, n)
    for cuts in ([1] * n, [3, 1, 17, 2, 16, 1], [39, 1]):
        m = lm.LoudnessModel(2, rate, f, 5, 17)
        parts, at = [], 0
        for c in cuts:
            parts.append(m.run(x[at * 2 * f:(at + c) * 2 * f], c)); at += c
        assert lm.records_equal(whole, np.concatenate(parts)), (cuts[:3], lm.first_difference(np.concatenate(parts), whole))
    # the first ticks: windows over fewer ticks than their length hold just those; tick 0's interpolator saw 11 zeros
    e = whole["ksq"][:, 0] + whole["ksq"][:, 1]
    assert whole["momentary_sq"][0] == e[0] and whole["short_sq"][2] == (e[0] + e[1]) + e[2]
    xl = x[0::2]
    want = lm.true_peak_bits(lm.tables(rate, f)[2], xl[:f], np.zeros(11, np.float32), f)
    assert whole["true_peak"][0, 0].view(np.uint32) == want[0]
    assert (whole["frames"] == f).all() and (whole["channels"] == 2).all()


def test_models_run_together_give_each_its_own_records():
    """run_many does the walks of the taps that share a tick length in one loop over the frames (tests/random_taps.py runs its loudness
    models that way): mono and stereo taps, two tick lengths, two runs -- every record and every carried state as from run() alone"""
    rng = np.random.default_rng(77)
    shapes = [(2, 48000.0, 800), (1, 48000.0, 800), (2, 16000.0, 267), (1, 48000.0, 800), (2, 48000.0, 800)]
    alone = [lm.LoudnessModel(ch, rate, f, 2, 5) for ch, rate, f in shapes]
    together = [lm.LoudnessModel(ch, rate, f, 2, 5) for ch, rate, f in shapes]
    for n in (3, 1, 4):
        xs = [(rng.standard_normal(n * f * ch) * 1.5).astype(np.float32) for ch, _rate, f in shapes]
        want = [m.run(x, n) for m, x in zip(alone, xs)]
        got = lm.run_many(together, xs, n)
        for a, b, m, w in zip(got, want, together, alone):
            assert a.tobytes() == b.tobytes() and m.state.tobytes() == w.state.tobytes() and m.e_hist.tobytes() == w.e_hist.tobytes()
    assert want[0]["ksq"].all() and not np.array_equal(want[0]["ksq"], want[4]["ksq"])


def test_window_sums_follow_the_stated_order():
    rate, f, n, m_t, s_t = 48000, 48, 60, 7, 33
    x = (np.random.default_rng(4).standard_normal(n * f) * np.exp2(np.random.default_rng(5).integers(-20, 4, n * f))).astype(np.float32)
    rec = lm.LoudnessModel(1, rate, f, m_t, s_t).run(x, n)
    e = [float(v) for v in rec["ksq"][:, 0]]   # a mono port: ksq[1] is +0.0
    assert not rec["ksq"][:, 1].any()
    for name, w in (("momentary_sq", m_t), ("short_sq", s_t)):
        for t in range(n):
            acc = 0.0
            for u in range(t - w + 1, t + 1):   # ascending tick, from +0.0; ticks before the set read +0.0
                acc = acc + (e[u] if u >= 0 else 0.0)
            assert rec[name][t] == acc, (name, t)


def test_energy_follows_the_partials_and_butterfly_and_the_tick_rule():
    rate, f = 48000, 100
    bq, carry, _ = lm.tables(rate, f)
    x = (np.random.default_rng(6).standard_normal(3 * f) * np.exp2(np.random.default_rng(7).integers(-12, 3, 3 * f))).astype(np.float32)
    rec = lm.LoudnessModel(1, rate, f).run(x, 3)
    state = [0.0] * 4
    for k in range(3):   # a scalar restatement: element by element, Python floats
        s, z = list(state), [0.0] * 4
        part = [0.0] * 8
        for i in range(f):
            xv = float(x[k * f + i])
            for chain, energy in ((s, True), (z, False)):
                v = xv
                for q in (0, 1):
                    b0, b1, b2, a1, a2 = (float(c) for c in bq[5 * q:5 * q + 5])
                    y = b0 * v + chain[2 * q]
                    chain[2 * q] = (b1 * v - a1 * y) + chain[2 * q + 1]
                    chain[2 * q + 1] = b2 * v - a2 * y
                    v = y
                if energy:
                    part[i % 8] = part[i % 8] + v * v
        for m in (4, 2, 1):
            part = [part[j] + part[j ^ m] for j in range(8)]
        assert rec["ksq"][k, 0] == part[0], k
        p = [[float(c) for c in row] for row in carry]
        state = [z[r] + (((p[r][0] * state[0] + p[r][1] * state[1]) + p[r][2] * state[2]) + p[r][3] * state[3]) for r in range(4)]


def test_header_struct_layout_and_symbols():
    body = re.search(r"typedef struct \{([^}]*)\} mx_loudness_tick;", HEADER).group(1)
    fields = [" ".join(ln.split("/*")[0].split()).rstrip(";") for ln in body.strip().splitlines()]
    assert fields == ["double ksq[2]", "double momentary_sq", "double short_sq", "float true_peak[2]", "uint32_t frames", "uint32_t channels"]

    class Tick(ctypes.Structure):   # the header's struct, field by field
        _fields_ = [("ksq", ctypes.c_double * 2), ("momentary_sq", ctypes.c_double), ("short_sq", ctypes.c_double),
                    ("true_peak", ctypes.c_float * 2), ("frames", ctypes.c_uint32), ("channels", ctypes.c_uint32)]
    names = ["ksq", "momentary_sq", "short_sq", "true_peak", "frames", "channels"]
    offsets = [getattr(Tick, f).offset for f in names]
    # the fields as the issue lists them occupy 48 bytes, not the 56 its text names: the header states what the compiler lays out
    assert ctypes.sizeof(Tick) == 48 and offsets == [0, 16, 24, 32, 40, 44]
    assert "/* 48 bytes: ksq 0, momentary_sq 16, short_sq 24, true_peak 32, frames 40, channels 44 */" in HEADER
    for dt in (abi.LOUDNESS_TICK_DTYPE, lm.TICK_DTYPE):
        assert dt.itemsize == 48 and [dt.fields[f][1] for f in names] == offsets
    assert re.search(r"typedef struct \{ uint32_t momentary_ticks; uint32_t short_ticks; \} mx_loudness_params;", HEADER)
    assert ctypes.sizeof(abi.LoudnessParams) == 8 and [getattr(abi.LoudnessParams, f).offset for f in ("momentary_ticks", "short_ticks")] == [0, 4]
    for name in ("mx_graph_set_loudness", "mx_graph_read_loudness", "mx_loudness_tables", "mx_loudness_gate"):
        assert hasattr(abi.lib, name)
    assert re.search(r"int mx_graph_set_loudness\(mx_graph\* g, const mx_port_ref\* ports, size_t n, const mx_loudness_params\* params\);", HEADER)
    assert re.search(r"int mx_graph_read_loudness\(mx_graph\* g, uint32_t first_tick_in_run, uint32_t n_ticks, mx_loudness_tick\* dst, size_t cap\);", HEADER)
    assert re.search(r"int mx_loudness_tables\(double rate, uint32_t frames_per_tick, double\* biquads, double\* carry, float\* interp\);", HEADER)
    assert re.search(r"int mx_loudness_gate\(const double\* block_sq, const uint32_t\* block_frames, size_t n_blocks, double\* lufs_integrated, size_t\* blocks_kept\);", HEADER)
    # taps, not a kind: the kind table, the profile's per-kind floats and the ABI version are what they were
    assert abi.KIND_COUNT == 19 and abi.PROFILE_KINDS == 18
    assert "MX_KIND_COUNT = 19" in HEADER and "#define MX_PROFILE_KINDS 18" in HEADER and "#define MX_ABI_VERSION 4u" in HEADER
    note = HEADER[HEADER.index("#define MX_ABI_VERSION"):HEADER.index("/* ---- status codes")]
    for name in ("mx_loudness_params", "mx_loudness_tick", "mx_graph_set_loudness", "mx_graph_read_loudness", "mx_loudness_tables", "mx_loudness_gate"):
        assert name in note


def test_null_graph_is_refused_without_a_device():
    assert abi.lib.mx_graph_set_loudness(None, None, 0, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_read_loudness(None, 0, 0, None, 0) == abi.MX_ERR_INVALID
