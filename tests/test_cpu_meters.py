"""Level meters without a GPU: the numpy model (tests/meter_model.py) on hand-worked cases, and the ABI as the header declares it."""
import ctypes
import pathlib
import re

import numpy as np

from meter_model import METER_TICK, MeterModel, channel_stats, records_equal
from mixlab_amd import abi

HEADER = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mixlab_gpu.h").read_text()
f32 = np.float32


def bits(v) -> int:
    return int(np.array([v], dtype=np.float32).view(np.uint32)[0])


def from_bits(b) -> np.float32:
    return np.array([b], dtype=np.uint32).view(np.float32)[0]


def spec_sum_sq(x) -> float:
    """the sum-of-squares order in plain Python floats (IEEE binary64, round to nearest even), element by element"""
    s = [0.0] * 64
    for f, v in enumerate(np.asarray(x, dtype=np.float32).tolist()):
        s[f % 64] = s[f % 64] + v * v
    for k in (32, 16, 8, 4, 2, 1):
        s = [s[j] + s[j ^ k] for j in range(64)]
    return s[0]


def test_lengths_1_63_64_65_735_hand_worked():
    for n in (1, 63, 64, 65, 735):
        peak, over, ss = channel_stats(np.full(n, 0.5, np.float32))
        assert peak == f32(0.5) and over == 0 and ss == 0.25 * n, n   # n / 4 is exact
    # one loud frame in the last, partial row
    x = np.full(65, -0.25, np.float32); x[64] = f32(-0.75)
    peak, over, ss = channel_stats(x)
    assert peak == f32(0.75) and over == 0 and ss == 64 * 0.0625 + 0.5625


def test_sum_sq_follows_the_partials_and_butterfly_not_np_sum():
    rng = np.random.default_rng(5)
    for n in (1, 63, 64, 65, 735, 800, 44100):
        # a wide dynamic range: the order of the adds shows in the last bits
        x = (rng.standard_normal(n) * np.exp2(rng.integers(-40, 40, n))).astype(np.float32)
        _, _, ss = channel_stats(x)
        assert np.float64(ss).view(np.uint64) == np.float64(spec_sum_sq(x)).view(np.uint64), n
    x = (rng.standard_normal(44100) * np.exp2(rng.integers(-40, 40, 44100))).astype(np.float32)
    d = x.astype(np.float64)
    assert channel_stats(x)[2] != np.sum(d * d)   # pairwise summation is another order (this input tells them apart)


def test_over_counts_strictly_beyond_one():
    one_up, one_down = np.nextafter(f32(1), f32(2)), np.nextafter(f32(-1), f32(-2))
    x = np.array([1.0, -1.0, one_up, one_down, 0.999, np.nan, np.inf, -np.inf], np.float32)
    assert channel_stats(x)[1] == 4
    assert channel_stats(np.array([1.0, -1.0], np.float32))[1] == 0


def test_signed_zero_subnormal_inf_nan():
    peak, over, ss = channel_stats(np.array([-0.0, 0.0], np.float32))
    assert bits(peak) == 0 and over == 0 and np.float64(ss).view(np.uint64) == 0   # +0.0
    tiny = from_bits(1)   # 2^-149
    peak, over, ss = channel_stats(np.array([-tiny], np.float32))
    assert bits(peak) == 1 and ss == 2.0 ** -298   # the subnormal reaches the f64 square unflushed
    sub = from_bits(0x007FFFFF)   # largest f32 subnormal
    assert channel_stats(np.array([sub, -tiny], np.float32))[2] == float(sub) ** 2 + 2.0 ** -298
    peak, over, ss = channel_stats(np.array([0.5, -np.inf], np.float32))
    assert peak == np.inf and over == 1 and ss == np.inf
    nan_a, nan_b = from_bits(0x7FC00001), from_bits(0xFFC00005)   # magnitudes 0x7fc00001 and 0x7fc00005
    peak, over, ss = channel_stats(np.array([nan_a, 3.0, nan_b], np.float32))
    assert bits(peak) == 0x7FC00005 and over == 1 and np.isnan(ss)
    peak, _, _ = channel_stats(np.array([np.inf, nan_a], np.float32))
    assert bits(peak) == 0x7FC00001   # any NaN pattern lies above +Inf's


def hold_of(peaks, hold_ticks, release):
    m = MeterModel(1, hold_ticks, release)
    return [m.hold_step(0, f32(p)) for p in peaks]


def test_hold_through_hold_ticks_and_release_steps():
    got = hold_of([0.8, 0, 0, 0, 0, 0.1, 0.3], 2, 0.5)
    # t0 takes 0.8; t1, t2 are within hold_ticks = 2; t3..t5 halve it (f32(0.8) / 8 == f32(0.1): equal bits take the peak, the age restarts)
    assert [float(v) for v in got] == [float(f32(v)) for v in (0.8, 0.8, 0.8, 0.4, 0.2, 0.1, 0.3)]
    got = hold_of([0.9, 0, 0, 0], 0, 0.9)   # hold 0: decays on the next tick already, f32 products
    want = [f32(0.9)]
    for _ in range(3):
        want.append(f32(want[-1] * f32(0.9)))
    assert [bits(v) for v in got] == [bits(v) for v in want]


def test_release_one_never_decays():
    assert [float(v) for v in hold_of([0.5, 0, 0, 0, 0.25], 0, 1.0)] == [0.5] * 5


def test_non_finite_hold_drops_to_zero_when_it_decays():
    got = hold_of([np.inf, 0.25, 0.0], 0, 0.5)
    assert got[0] == np.inf and got[1] == f32(0.25) and got[2] == f32(0.125)
    got = hold_of([np.nan, 0.0, 0.0], 1, 0.5)
    assert np.isnan(got[0]) and np.isnan(got[1]) and got[2] == 0.0   # held one tick, then 0 (not NaN * release)


def test_age_saturates():
    m = MeterModel(1, 0xFFFFFFFF, 0.5)   # never older than hold_ticks: no decay ever
    m.hold_step(0, f32(0.5))
    m.a[0] = 0xFFFFFFFE
    for _ in range(3):
        assert m.hold_step(0, f32(0.0)) == f32(0.5)
    assert m.a[0] == 0xFFFFFFFF


def test_model_records_and_stereo_channels():
    m = MeterModel(2, 0, 1.0)
    x = np.array([[0.5, -2.0], [-0.25, 0.0], [1.5, 0.125]], np.float32)
    r = m.tick(x.reshape(-1))
    assert r["frames"] == 3 and r["channels"] == 2
    assert list(r["over"]) == [1, 1] and list(r["peak"]) == [1.5, 2.0]
    assert list(r["sum_sq"]) == [0.25 + 0.0625 + 2.25, 4.0 + 0.0 + 0.015625]
    mono = MeterModel(1).tick(np.array([0.5], np.float32))
    assert mono["channels"] == 1 and mono["peak"][1] == 0 and mono["hold"][1] == 0 and mono["sum_sq"][1] == 0 and mono["over"][1] == 0
    a = np.zeros(2, METER_TICK); b = a.copy()
    a["sum_sq"][0, 0] = np.float64(np.nan); b["sum_sq"][0, 0] = -np.float64(np.nan)
    assert list(records_equal(a, b)) == [True, True]   # any NaN equals any NaN in sum_sq
    b["peak"][1, 1] = f32(-0.0)
    assert list(records_equal(a, b)) == [True, False]


def test_header_struct_layout_and_symbols():
    assert re.search(r"typedef struct \{ uint32_t node, port; \} mx_port_ref;", HEADER)
    assert re.search(r"typedef struct \{ uint32_t hold_ticks; float release; \} mx_meter_params;", HEADER)
    body = re.search(r"typedef struct \{([^}]*)\} mx_meter_tick;", HEADER).group(1)
    fields = [ln.split("/*")[0].strip().rstrip(";") for ln in body.strip().splitlines()]
    assert fields == ["float    peak[2]", "float    hold[2]", "double   sum_sq[2]", "uint32_t over[2]", "uint32_t frames", "uint32_t channels"]

    class Tick(ctypes.Structure):   # the header's struct, field by field
        _fields_ = [("peak", ctypes.c_float * 2), ("hold", ctypes.c_float * 2), ("sum_sq", ctypes.c_double * 2),
                    ("over", ctypes.c_uint32 * 2), ("frames", ctypes.c_uint32), ("channels", ctypes.c_uint32)]
    assert ctypes.sizeof(Tick) == 48
    assert [getattr(Tick, f).offset for f in ("peak", "hold", "sum_sq", "over", "frames", "channels")] == [0, 8, 16, 32, 40, 44]
    for dt in (abi.METER_TICK_DTYPE, METER_TICK):
        assert dt.itemsize == 48 and [dt.fields[f][1] for f in dt.names] == [0, 8, 16, 32, 40, 44]
    assert ctypes.sizeof(abi.PortRef) == 8 and ctypes.sizeof(abi.MeterParams) == 8
    assert hasattr(abi.lib, "mx_graph_set_meters") and hasattr(abi.lib, "mx_graph_read_meters")
    assert re.search(r"int mx_graph_set_meters\(mx_graph\* g, const mx_port_ref\* ports, size_t n, const mx_meter_params\* params\);", HEADER)
    assert re.search(r"int mx_graph_read_meters\(mx_graph\* g, uint32_t first_tick_in_run, uint32_t n_ticks, mx_meter_tick\* dst, size_t cap\);", HEADER)
    # taps, not a kind: the kind table and the profile's per-kind floats are what they were
    assert abi.KIND_COUNT == 19 and abi.PROFILE_KINDS == 18
    assert "MX_KIND_COUNT = 19" in HEADER and "#define MX_PROFILE_KINDS 18" in HEADER and "#define MX_ABI_VERSION 4u" in HEADER


def test_null_graph_is_refused_without_a_device():
    assert abi.lib.mx_graph_set_meters(None, None, 0, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_read_meters(None, 0, 0, None, 0) == abi.MX_ERR_INVALID
