"""The deck's track analysis without a device (include/mixlab_gpu.h "ANALYSIS"): the header's structs and entry points, the setting rules at
both edges of each, mx_deck_columns_host and mx_deck_beatgrid against the model on every shared case, the tap tables' properties, what the specification promises
(low + mid + high = s; the named cases' extremes), and that the shared cases tell the model from each of a list of misreadings."""
import ctypes as C
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import deck_analysis_cases as ac
import deck_analysis_model as am
from deck_analysis_model import Settings

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_analysis_check", "mx_deck_analysis_bands", "mx_deck_analyse", "mx_deck_column_count", "mx_deck_read_columns", "mx_deck_read_autocorr",
                "mx_deck_columns_host", "mx_deck_beatgrid", "mx_deck_debug_last_analysis"}
ANALYSIS_OFFSETS = {"column": 0, "taps": 4, "max_lag": 8, "_pad": 12, "lo": 16, "hi": 270}
COLUMN_OFFSETS = {"smin": 0, "smax": 4, "peak": 8, "onset": 20, "energy": 24, "e": 48}
GRID_OFFSETS = {"bpm": 0, "period_columns": 8, "confidence": 16, "first_beat_frame": 24, "lag": 32, "phase_column": 36}


def c_settings(s: Settings):
    from mixlab_amd import deck
    return deck.analysis(s.column, s.max_lag, s.lo, s.hi)


def grid_bits(g):
    """a grid -- the library's struct or the model's tuple -- with its doubles as bit patterns"""
    v = tuple(g) if isinstance(g, am.Grid) else (g.bpm, g.period_columns, g.confidence, g.first_beat_frame, g.lag, g.phase_column)
    return np.array(v[:3], np.float64).view(np.uint64).tolist() + [int(x) for x in v[3:]]


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    assert lay["mx_deck_analysis"] == {"size": 524, "offsets": ANALYSIS_OFFSETS}
    assert lay["mx_deck_column"] == {"size": 56, "offsets": COLUMN_OFFSETS}
    assert lay["mx_deck_grid"] == {"size": 40, "offsets": GRID_OFFSETS}
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # additions only
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_analyse") == ["mx_deck*", "const mx_deck_analysis*"]
    assert sig("mx_deck_analysis_bands") == ["double", "double", "double", "uint32_t", "mx_deck_analysis*"]
    assert sig("mx_deck_column_count") == ["uint64_t", "uint32_t", "uint64_t*"]
    assert sig("mx_deck_read_columns") == ["mx_deck*", "uint64_t", "uint64_t", "mx_deck_column*"]
    assert sig("mx_deck_read_autocorr") == ["mx_deck*", "uint64_t*", "uint32_t"]
    assert sig("mx_deck_columns_host") == ["const int16_t*", "uint64_t", "const mx_deck_analysis*", "uint64_t", "uint64_t", "mx_deck_column*", "uint64_t*"]
    assert sig("mx_deck_beatgrid") == ["const mx_deck_column*", "uint64_t", "const uint64_t*", "uint32_t", "uint32_t", "double", "double", "double", "mx_deck_grid*"]
    assert re.search(r"int mx_deck_debug_last_analysis\(uint32_t out\[4\]\);", text)
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | {"mx_deck_analysis", "mx_deck_column", "mx_deck_grid"}):
        assert re.search(rf"\b{name}\b", note), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}


def test_ctypes_mirrors_and_the_numpy_record_have_the_headers_layout():
    from mixlab_amd import abi, deck
    for st, size, offs in ((abi.DeckAnalysis, 524, ANALYSIS_OFFSETS), (abi.DeckColumn, 56, COLUMN_OFFSETS), (abi.DeckGrid, 40, GRID_OFFSETS)):
        assert C.sizeof(st) == size and {n: getattr(st, n).offset for n, _t in st._fields_} == offs
    for dt in (deck.COLUMN_DTYPE, am.COLUMN_DTYPE):
        assert dt.itemsize == 56 and {n: dt.fields[n][1] for n in dt.names} == COLUMN_OFFSETS


# ---- the setting rules, accepted at the bound and refused one past it ----
OK = ac.BANDS_63
SUM_32767, SUM_32768 = (32767 - 62,) + (1,) * 30 + (-1,) * 32, (32768 - 62,) + (1,) * 30 + (-1,) * 32
CHECKS = [(OK, True),
          (OK._replace(column=64), True), (OK._replace(column=32), False), (OK._replace(column=4096), True), (OK._replace(column=8192), False),
          (OK._replace(column=96), False), (OK._replace(column=1000), False), (OK._replace(column=0), False),
          (Settings(512, 256, (16384,), (16384,)), True), (Settings(512, 256, (8192, 8192), (8192, 8192)), False), (Settings(512, 256, (), ()), False),
          (Settings(512, 256, (100,) * 127, (100,) * 127), True),
          (OK._replace(lo=SUM_32767), True), (OK._replace(lo=SUM_32768), False), (OK._replace(hi=SUM_32767), True), (OK._replace(hi=SUM_32768), False),
          (OK._replace(lo=(-32768,) + (0,) * 62), False), (OK._replace(lo=(-32767,) + (0,) * 62), True),
          (OK._replace(max_lag=16), True), (OK._replace(max_lag=15), False), (OK._replace(max_lag=1024), True), (OK._replace(max_lag=1025), False)]


@pytest.mark.parametrize("s,ok", CHECKS)
def test_analysis_check_at_the_boundaries(s, ok):
    from mixlab_amd import abi, deck
    assert (am.check(s) is None) == ok
    c = deck.analysis(s.column, s.max_lag, s.lo, s.hi)
    if ok:
        deck.analysis_check(c)
    else:
        with pytest.raises(abi.MxError) as e:
            deck.analysis_check(c)
        assert e.value.code == abi.MX_ERR_INVALID and "deck analysis" in str(e.value)


def test_analysis_check_refuses_129_taps_a_tap_at_or_beyond_k_and_the_pad():
    from mixlab_amd import abi, deck
    for field, value in (("taps", 129), ("taps", 128), ("taps", 0), ("taps", 62), ("_pad", 1)):
        c = c_settings(OK)
        setattr(c, field, value)
        with pytest.raises(abi.MxError):
            deck.analysis_check(c)
    for table in ("lo", "hi"):
        for at in (63, 126):
            c = c_settings(OK)
            getattr(c, table)[at] = 1
            assert am.check(OK, tail=((0,) * (at - 63) + (1,), ())) == "tail"
            with pytest.raises(abi.MxError):
                deck.analysis_check(c)
        c = c_settings(OK)
        getattr(c, table)[62] += 1   # ... while the last tap below K is any tap
        deck.analysis_check(c)
    assert am.check(OK, pad=1) == "_pad"


# ---- columns_host and beatgrid against the model ----
@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_columns_host_and_beatgrid_equal_the_model(case):
    from mixlab_amd import deck
    want_cols, want_R, want_grid = ac.truth(case)
    a = c_settings(case.settings)
    cols, R = deck.columns_host(ac.track(case), a, autocorr=True)
    assert len(cols) == len(want_cols) == deck.column_count(ac.track(case).shape[0], a.column)
    for name in want_cols.dtype.names:
        assert np.array_equal(cols[name], want_cols[name]), (case.name, name)
    assert cols.tobytes() == want_cols.tobytes() and np.array_equal(R, want_R)
    assert grid_bits(deck.beatgrid(cols, R, a.column, ac.RATE, ac.BPM_LO, ac.BPM_HI)) == grid_bits(want_grid), case.name
    # a window names the columns it names (A[first - 1] is recomputed)
    n = len(cols)
    for first, cnt in ((0, 1), (n // 2, n - n // 2), (n - 1, 1), (n, 0)):
        assert deck.columns_host(ac.track(case), a, first, cnt).tobytes() == want_cols[first:first + cnt].tobytes(), (case.name, first, cnt)


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_the_bands_add_up_to_s_on_the_model(case):
    s = am.sums(ac.track(case))
    low, mid, high = am.bands(s, case.settings)
    assert np.array_equal(low + mid + high, s)


def test_the_named_cases_are_what_the_issue_says_they_are():
    cols, R, grid = ac.truth(ac.BY_NAME["click track"])
    assert (grid.lag, grid.phase_column, grid.first_beat_frame) == (46, 9, 9 * 512)
    assert grid.bpm == 60.0 * 48000.0 / (512.0 * grid.period_columns) and round(grid.bpm, 2) == 122.28 and grid.period_columns >= 46.0
    below = ac.truth(ac.BY_NAME["click track, the vertex below 46"])[2]
    assert (below.lag, below.phase_column) == (46, 10) and below.period_columns < 46.0
    # the int32 extreme: a1 = -2 147 418 112 in the interior, e = 2^44 exactly
    case = ac.BY_NAME["every sample -32768, 63 positive taps of sum 32767, C = 4096"]
    cols = ac.truth(case)[0]
    assert [int(v) for v in cols["e"]] == [1 << 44] * 3 and int(cols["smin"][1]) == -65536
    assert int(cols["peak"][1, 0]) == (2147418112 + (1 << 14) - 1) >> 14 == 131068 and sum(case.settings.lo) == 32767
    # K = 1 unity taps: low = s, mid = high = 0
    cols = ac.truth(ac.BY_NAME["noise, 3000 frames at C = 256, K = 1 unity taps"])[0]
    assert not cols["peak"][:, 1:].any() and not cols["energy"][:, 1:].any() and np.array_equal(cols["energy"][:, 0], cols["e"])
    assert np.array_equal(cols["peak"][:, 0], np.maximum(np.abs(cols["smin"].astype(np.int64)), np.abs(cols["smax"].astype(np.int64))))
    # a constant track under band tables: mid = high = 0 away from the ends
    cols = ac.truth(ac.BY_NAME["constant track under band tables"])[0]
    assert not cols["peak"][1:-1, 1:].any() and cols["peak"][0, 1:].all() and (cols["peak"][1:-1, 0] == 2000).all()
    # fewer columns than lags: R[l >= N] = 0
    cols, R, _ = ac.truth(ac.BY_NAME["11 columns under max_lag 256"])
    assert len(cols) == 11 and R[:11].any() and not R[11:].any()
    assert ac.truth(ac.BY_NAME["silence"])[2] == am.ZERO_GRID and not ac.truth(ac.BY_NAME["silence"])[1].any()
    # every kernel form is among the cases
    total = {}
    for c in ac.CASES:
        for k, v in ac.forms(c).items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total


def test_beatgrid_and_columns_host_refuse_what_the_header_says_they_refuse():
    from mixlab_amd import abi, deck
    lib = abi.lib
    case = ac.BY_NAME["11 columns under max_lag 256"]
    cols, R, _ = ac.truth(case)
    g = abi.DeckGrid()
    cp, Rp = cols.ctypes.data_as(C.c_void_p), R.ctypes.data_as(C.c_void_p)
    good = [cp, len(cols), Rp, 256, 512, 48000.0, 60.0, 200.0, C.byref(g)]
    assert lib.mx_deck_beatgrid(*good) == 0
    for k, v in ((0, None), (2, None), (3, 15), (3, 1025), (4, 500), (4, 32), (5, 0.0), (5, float("nan")), (6, -1.0), (6, 300.0), (7, float("inf")), (8, None)):
        args = list(good)
        args[k] = v
        assert lib.mx_deck_beatgrid(*args) == abi.MX_ERR_INVALID, (k, v)
    assert lib.mx_deck_beatgrid(None, 0, Rp, 256, 512, 48000.0, 60.0, 200.0, C.byref(g)) == 0   # no columns: every phase sums to 0
    a = c_settings(case.settings)
    tr = ac.track(case)
    for fn in (lambda: deck.columns_host(tr, a, 12, 0), lambda: deck.columns_host(tr, a, 5, 7), lambda: deck.columns_host(tr, a, 1, 10, autocorr=True),
               lambda: deck.column_count(0, 512), lambda: deck.column_count((1 << 30) + 1, 512), lambda: deck.column_count(100, 100)):
        with pytest.raises(abi.MxError) as e:
            fn()
        assert e.value.code == abi.MX_ERR_INVALID
    assert deck.column_count(1 << 30, 64) == 1 << 24 and deck.column_count(513, 512) == 2


def test_a_runaway_vertex_gives_no_grid():
    """R with its maximum at the edge of the candidate range and a larger neighbour outside it: the parabola's vertex lies far away, P outside [1, L]"""
    from mixlab_amd import deck
    R = np.zeros(64, np.uint64)
    R[0], R[17], R[18], R[19] = 1000, 0, 500, 999   # at C = 512 and 48 kHz, 310 .. 315 BPM leaves lag 18 as the one candidate
    cols = np.zeros(100, deck.COLUMN_DTYPE)
    cols["onset"] = 1
    want = am.beatgrid(cols["onset"], R, 64, 512, 48000.0, 310.0, 315.0)
    assert grid_bits(deck.beatgrid(cols, R, 512, 48000.0, 310.0, 315.0)) == grid_bits(want)
    found = am.tempo_lag(R, 64, 512, 48000.0, 310.0, 315.0)
    assert found is not None and found[0] == 18 and not 1.0 <= 18.0 + found[1] <= 64.0 and want == am.ZERO_GRID


# ---- the tables ----
@pytest.mark.parametrize("rate,f_lo,f_hi,K", [(48000.0, 200.0, 2500.0, 63), (44100.0, 150.0, 4000.0, 127), (48000.0, 200.0, 2500.0, 1), (96000.0, 80.0, 9000.0, 31),
                                              (48000.0, 1000.0, 12000.0, 5)])
def test_analysis_bands_is_symmetric_sums_to_16384_and_lies_within_one_rounding(rate, f_lo, f_hi, K):
    """each tap is round(x), x = 16384 g_k / sum g: at most 0.5 from x as this library evaluates it, and that x is a few ulps from numpy's f64 -- far below the 0.5 more
    that the bound of 1 leaves.  The centre tap alone absorbs the roundings of the others."""
    from mixlab_amd import deck
    a = deck.analysis_bands(rate, f_lo, f_hi, K, column=1024, max_lag=99)
    assert (a.column, a.taps, a.max_lag, a._pad) == (1024, K, 99, 0)
    deck.analysis_check(a)
    for table, f in ((a.lo, f_lo), (a.hi, f_hi)):
        c = [int(v) for v in table]
        assert not any(c[K:]) and c[:K] == c[:K][::-1] and sum(c) == 16384
        model, ideal = am.band_taps(rate, f, K)
        D = (K - 1) // 2
        assert all(abs(c[k] - ideal[k]) <= 1.0 for k in range(K) if k != D), (f, K)
        assert abs(c[D] - ideal[D]) <= 1.0 + K * 0.5
        assert all(abs(c[k] - model[k]) <= 1 for k in range(K) if k != D)


def test_analysis_bands_refuses_bad_arguments_and_leaves_the_settings_alone():
    from mixlab_amd import abi
    lib = abi.lib
    a = c_settings(OK)
    before = bytes(a)
    for args in ((0.0, 200.0, 2500.0, 63), (float("nan"), 200.0, 2500.0, 63), (48000.0, 0.0, 2500.0, 63), (48000.0, 2500.0, 2500.0, 63), (48000.0, 200.0, 24000.0, 63),
                 (48000.0, 200.0, 2500.0, 64), (48000.0, 200.0, 2500.0, 129), (48000.0, 200.0, 2500.0, 0)):
        assert lib.mx_deck_analysis_bands(*args, C.byref(a)) == abi.MX_ERR_INVALID, args
        assert bytes(a) == before
    assert lib.mx_deck_analysis_bands(48000.0, 200.0, 2500.0, 63, None) == abi.MX_ERR_INVALID


# ---- the cases tell the model from every misreading ----
# fma_index -- i_k from one fused multiply-add -- is in the model but not in this list: no case was found in which it shows.  It can differ only where k P lies
# within an ulp of an integer AND adding phi crosses a power of two AND the double rounding hits a tie; 400 000 random parabolas (l* 1 .. 126, R up to 3000, every
# phase, k P up to 2100 columns) and every shared case gave the same indices either way.
SHOWN = tuple(m for m in am.MISREADINGS if m != "fma_index")


def test_the_list_of_misreadings_is_the_issues():
    assert len(SHOWN) == 8 and len(set(am.MISREADINGS)) == 9


@pytest.mark.parametrize("mis", SHOWN)
def test_a_misreading_changes_some_case(mis):
    changed = []
    for c in ac.CASES:
        want_cols, want_R, want_grid = ac.truth(c)
        cols, R = am.analyse(ac.track(c), c.settings, mis=(mis,))
        grid = am.beatgrid(cols["onset"], R, c.settings.max_lag, c.settings.column, ac.RATE, ac.BPM_LO, ac.BPM_HI, mis=(mis,))
        if cols.tobytes() != want_cols.tobytes() or not np.array_equal(R, want_R) or grid_bits(grid) != grid_bits(want_grid):
            changed.append(c.name)
    print(mis, "changes", len(changed), "cases:", changed[:4])
    assert changed, mis


def test_the_fused_index_changes_no_shared_case():
    for c in ac.CASES:
        cols, R, want = ac.truth(c)
        assert am.beatgrid(cols["onset"], R, c.settings.max_lag, c.settings.column, ac.RATE, ac.BPM_LO, ac.BPM_HI, mis=("fma_index",)) == want, c.name
