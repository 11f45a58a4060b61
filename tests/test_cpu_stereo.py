"""Stereo field taps without a GPU: the ABI as the header declares it, the host-only helpers, the goniometer's cell rule against a list
written by hand, and the conformance of the spec (the numpy model, tests/stereo_model.py, with mx_stereo_correlation) on signals whose
correlation is known."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import stereo_model as stm
from mixlab_amd import abi

HEADER = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mixlab_gpu.h").read_text()
RATES = [(44100, 735), (48000, 800)]
N_TICKS = 60


# ---- layout ----

class CStereoTick(ctypes.Structure):   # the issue's field list, laid out by the C rules
    _fields_ = [("sum_ll", ctypes.c_double), ("sum_rr", ctypes.c_double), ("sum_lr", ctypes.c_double),
                ("win_ll", ctypes.c_double), ("win_rr", ctypes.c_double), ("win_lr", ctypes.c_double),
                ("frames", ctypes.c_uint32), ("nonfinite", ctypes.c_uint32)]


OFFSETS = {"sum_ll": 0, "sum_rr": 8, "sum_lr": 16, "win_ll": 24, "win_rr": 32, "win_lr": 40, "frames": 48, "nonfinite": 52}


def test_tick_record_is_56_bytes_with_the_stated_offsets():
    assert ctypes.sizeof(CStereoTick) == 56
    for name, off in OFFSETS.items():
        assert getattr(CStereoTick, name).offset == off, name
    for dt in (abi.STEREO_TICK_DTYPE, stm.TICK_DTYPE):
        assert dt.itemsize == 56
        assert {n: dt.fields[n][1] for n in dt.names} == OFFSETS
    assert "/* 56 bytes: sum_ll 0, sum_rr 8, sum_lr 16, win_ll 24, win_rr 32, win_lr 40, frames 48, nonfinite 52 */" in HEADER
    assert ctypes.sizeof(abi.StereoParams) == 16
    assert [f[0] for f in abi.StereoParams._fields_] == ["window_ticks", "grid", "zoom_log2", "hop"]


def test_header_declares_the_prototypes_and_the_version_note_names_them():
    protos = [
        r"int\s+mx_graph_set_stereo\(mx_graph\*\s*g,\s*const mx_port_ref\*\s*ports,\s*size_t n,\s*const mx_stereo_params\*\s*params\);",
        r"int\s+mx_graph_read_stereo\(mx_graph\*\s*g,\s*uint32_t first_tick_in_run,\s*uint32_t n_ticks,\s*mx_stereo_tick\*\s*dst,\s*size_t cap\);",
        r"int\s+mx_graph_read_goniometers\(mx_graph\*\s*g,\s*void\*\s*dst,\s*size_t cap_bytes,\s*uint32_t\*\s*n_records\);",
        r"int\s+mx_stereo_gonio_record_bytes\(const mx_stereo_params\*\s*params,\s*size_t\*\s*bytes\);",
        r"int\s+mx_stereo_correlation\(double ll,\s*double rr,\s*double lr,\s*double\*\s*r\);",
    ]
    for p in protos:
        assert re.search(p, HEADER), p
    note = HEADER[HEADER.index("#define MX_ABI_VERSION"): HEADER.index("/* ---- status codes")]
    for name in ("mx_stereo_params", "mx_stereo_tick", "mx_graph_set_stereo", "mx_graph_read_stereo", "mx_graph_read_goniometers",
                 "mx_stereo_gonio_record_bytes", "mx_stereo_correlation"):
        assert re.search(rf"\b{name}\b", note), name
    assert re.search(r"#define\s+MX_ABI_VERSION\s+4u", HEADER) and abi.lib.mx_abi_version() == 4
    assert abi.KIND_COUNT == 19 and abi.PROFILE_KINDS == 18
    assert re.search(r"#define\s+MX_PROFILE_KINDS\s+18\b", HEADER) and re.search(r"MX_KIND_COUNT\s*=\s*19\b", HEADER)


# ---- helpers ----

def test_every_entry_point_refuses_a_null_graph():
    pa = (abi.PortRef * 1)(abi.PortRef(0, 0))
    par = abi.StereoParams(180, 64, 0, 1)
    out = np.zeros(1, abi.STEREO_TICK_DTYPE)
    n = ctypes.c_uint32()
    assert abi.lib.mx_graph_set_stereo(None, pa, 1, ctypes.byref(par)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_set_stereo(None, None, 0, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_read_stereo(None, 0, 1, out.ctypes.data, 1) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_read_goniometers(None, out.ctypes.data, 56, ctypes.byref(n)) == abi.MX_ERR_INVALID


def test_goniometer_record_bytes():
    assert abi.stereo_gonio_record_bytes(64) == 16416 == stm.record_bytes(64)
    assert abi.stereo_gonio_record_bytes(128) == 65568 == stm.record_bytes(128)
    assert abi.stereo_gonio_record_bytes(0) == 32 == stm.record_bytes(0)
    n = ctypes.c_size_t()
    for grid in (1, 32, 63, 65, 256, 1 << 31):
        assert abi.lib.mx_stereo_gonio_record_bytes(ctypes.byref(abi.StereoParams(1, grid, 0, 1)), ctypes.byref(n)) == abi.MX_ERR_INVALID, grid
        with pytest.raises(abi.MxError):
            abi.stereo_gonio_record_bytes(grid)
    assert abi.lib.mx_stereo_gonio_record_bytes(None, ctypes.byref(n)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_stereo_gonio_record_bytes(ctypes.byref(abi.StereoParams(1, 64, 0, 1)), None) == abi.MX_ERR_INVALID


def test_correlation_helper_is_the_models_and_never_answers_nan():
    rng = np.random.default_rng(5)
    for _ in range(200):
        ll, rr = rng.uniform(0, 1e3, 2)
        lr = rng.uniform(-1.2, 1.2) * np.sqrt(ll * rr)
        got, want = abi.stereo_correlation(ll, rr, lr), stm.correlation(ll, rr, lr)
        assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64) and -1.0 <= got <= 1.0
    assert abi.stereo_correlation(4.0, 9.0, 6.0) == 1.0 and abi.stereo_correlation(4.0, 9.0, -6.0) == -1.0 and abi.stereo_correlation(4.0, 9.0, 3.0) == 0.5
    inf, nan = float("inf"), float("nan")
    for ll, rr, lr in ((0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 0.0), (-1.0, 1.0, 0.5), (inf, 1.0, 1.0), (1e200, 1e200, 1.0), (nan, 1.0, 1.0),
                       (1.0, nan, 1.0), (1.0, 1.0, nan), (1e-200, 1e-200, 1e-200)):
        got = abi.stereo_correlation(ll, rr, lr)
        assert got == 0.0 and stm.correlation(ll, rr, lr) == 0.0, (ll, rr, lr, got)
    assert abi.stereo_correlation(1.0, 1.0, inf) == 1.0 and abi.stereo_correlation(1.0, 1.0, -inf) == -1.0
    assert abi.lib.mx_stereo_correlation(1.0, 1.0, 1.0, None) == abi.MX_ERR_INVALID


# ---- cells ----

def test_cells_at_grid_128_zoom_0_are_the_hand_written_list():
    v = np.array([-2, -1.999, -1e-30, -0.0, 0.0, 1e-30, 1.99, 2.0, 3e38, -3e38], dtype=np.float32)
    by_hand = [0, 0, 63, 64, 64, 64, 127, 127, 127, 0]
    assert stm.cell(v, 128, 0).tolist() == by_hand
    # the same rule one value at a time, in plain Python on the f32 values: floor(v * 32) clamped to [-64, 63], + 64
    for x, want in zip(v, by_hand):
        with np.errstate(over="ignore"):
            t = np.floor(np.float32(x) * np.float32(32.0))
        assert int(min(max(t, -64.0), 63.0)) + 64 == want, x
    # zoom: z doubles per step; at zoom 8 and grid 64 a cell is 2^-12 wide
    assert stm.cell(np.float32(2.0 ** -12), 64, 8) == 33 and stm.cell(np.float32(-(2.0 ** -13)), 64, 8) == 31
    assert stm.cell(np.float32(0.49), 64, 1) == 32 + 15 and stm.cell(np.float32(1.0), 64, 1) == 63
    # an overflowing m from finite L, R clamps to the edge
    g, plotted, skipped = stm.plot(np.array([3e38, -3e38], np.float32), np.array([3e38, -3e38], np.float32), 64, 0)
    assert plotted == 2 and skipped == 0 and g[63, 32] == 1 and g[0, 32] == 1


# ---- conformance ----

def sine(rate, n, phase=0.0, amp=0.5, freq=1000.0):
    return (amp * np.sin(2 * np.pi * freq * np.arange(n) / rate + phase)).astype(np.float32)


def measure(frames, left, right, **kw):
    model = stm.StereoModel(**kw)
    return model.run(np.stack([left, right], 1).reshape(-1), len(left) // frames)


def window_r(rec, t=-1):
    return abi.stereo_correlation(rec["win_ll"][t], rec["win_rr"][t], rec["win_lr"][t])


@pytest.mark.parametrize("rate,frames", RATES)
def test_correlation_of_known_signals(rate, frames):
    n = N_TICKS * frames
    s, c = sine(rate, n), sine(rate, n, np.pi / 2)
    rec, _ = measure(frames, s, s, window_ticks=N_TICKS)
    assert window_r(rec) >= 1 - 1e-12
    rec, _ = measure(frames, s, -s, window_ticks=N_TICKS)
    assert window_r(rec) <= -1 + 1e-12
    rec, _ = measure(frames, s, c, window_ticks=N_TICKS)   # 60 ticks are one second: whole periods
    r_win, r_tick = window_r(rec), abi.stereo_correlation(rec["sum_ll"][0], rec["sum_rr"][0], rec["sum_lr"][0])
    print(f"{rate} Hz: sine against cosine reads {r_win:.3e} over {N_TICKS} ticks, {r_tick:.4f} over one")
    assert abs(r_win) <= 1e-9
    rec, _ = measure(frames, s, np.zeros(n, np.float32), window_ticks=N_TICKS)
    assert window_r(rec) == 0.0 and all(window_r(rec, t) == 0.0 for t in range(N_TICKS))
    rng = np.random.default_rng(rate)
    a, b = rng.uniform(-1, 1, n).astype(np.float32), rng.uniform(-1, 1, n).astype(np.float32)
    rec, _ = measure(frames, a, b, window_ticks=N_TICKS)
    r = window_r(rec)
    print(f"{rate} Hz: independent noises read {r:.4f}, bound {4 / np.sqrt(n):.4f}")
    assert abs(r) <= 4 / np.sqrt(n)


# ---- goniometer ----

@pytest.mark.parametrize("grid", [64, 128])
@pytest.mark.parametrize("rate,frames", RATES)
def test_goniometer_of_mono_and_inverted_signals(rate, frames, grid):
    n_ticks, hop = 12, 4
    s = sine(rate, n_ticks * frames)
    _, em = measure(frames, s, s, grid=grid, hop=hop)
    assert [e["tick_in_run"] for e in em] == [3, 7, 11]
    for e in em:   # L = R: s = 0, every count in column grid / 2
        assert e["gon"].sum() == e["frames"] == hop * frames and e["skipped"] == 0 and e["ticks"] == hop
        assert e["gon"][:, grid // 2].sum() == e["frames"] and np.count_nonzero(e["gon"][:, grid // 2]) > 4
    _, em = measure(frames, s, -s, grid=grid, hop=hop)
    for e in em:   # L = -R: m = 0, every count in row grid / 2
        assert e["gon"].sum() == e["frames"] == hop * frames
        assert e["gon"][grid // 2, :].sum() == e["frames"] and np.count_nonzero(e["gon"][grid // 2, :]) > 4
    x = s.copy(); x[[5, frames + 1, 2 * frames]] = np.nan; y = s.copy(); y[[5, 9]] = np.inf
    rec, em = measure(frames, x, y, grid=grid, hop=hop)
    assert em[0]["skipped"] == 4 and em[0]["frames"] + em[0]["skipped"] == hop * frames and em[0]["gon"].sum() == em[0]["frames"]
    assert rec["nonfinite"][:4].tolist() == [2, 1, 1, 0] and em[1]["skipped"] == 0
    for e in em:
        assert e["frames"] + e["skipped"] == hop * frames


def test_goniometer_counter_runs_across_runs_and_hop_beyond_a_run():
    frames, hop = 48, 5
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, 14 * 2 * frames).astype(np.float32)
    whole = stm.StereoModel(grid=64, hop=hop).run(x, 14)[1]
    parts, at, m = [], 0, stm.StereoModel(grid=64, hop=hop)
    for c in (3, 1, 7, 3):
        em = m.run(x[at * 2 * frames:(at + c) * 2 * frames], c)[1]
        parts += [dict(e, tick_in_run=e["tick_in_run"] + at) for e in em]
        at += c
    assert len(whole) == 2 and len(parts) == 2 and all(stm.gonio_equal(a, b) for a, b in zip(whole, parts))


# ---- window ----

def test_a_window_with_less_behind_it_is_the_sum_of_what_exists():
    frames = 100
    rng = np.random.default_rng(2)
    x = rng.uniform(-1, 1, 10 * 2 * frames).astype(np.float32)
    rec, _ = stm.StereoModel(window_ticks=6).run(x, 10)
    for f_sum, f_win in zip(stm.SUMS, stm.WINS):
        for t in range(10):
            w = np.float64(0.0)
            for u in range(max(0, t - 5), t + 1):
                w = w + rec[f_sum][u]
            assert rec[f_win][t].view(np.uint64) == w.view(np.uint64), (f_win, t)
    # split into runs: the history carries, nothing changes
    m = stm.StereoModel(window_ticks=6)
    parts = np.concatenate([m.run(x[:3 * 2 * frames], 3)[0], m.run(x[3 * 2 * frames:], 7)[0]])
    assert stm.records_equal(parts, rec)
    # and the longest window reaches 1023 ticks back
    y = np.ones(1030 * 2 * 2, np.float32)
    rec, _ = stm.StereoModel(window_ticks=1024).run(y, 1030)
    assert rec["win_ll"][1022] == 2 * 1023 and rec["win_ll"][1023] == 2 * 1024 and rec["win_ll"][1029] == 2 * 1024
