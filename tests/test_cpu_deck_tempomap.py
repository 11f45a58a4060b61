"""The deck's tempo map without a device (include/mixlab_gpu.h "TEMPO MAP"): the header's structs and entry points, the setting rules at both
edges of each, mx_deck_tempomap_host / _path / _segments / _at / _step / _span against the model (tests/deck_tempomap_model.py) on every shared case
(tests/deck_tempomap_cases.py), the path against a search over all index sequences, look-up and warp against fractions.Fraction, that one window is the fine grid, that
the shared cases tell the text from each of a list of misreadings, the property that makes the feature worth having -- a map that sits on every click of three tracks
whose tempo is not constant, where the whole-track grid is half a beat off -- on the model and on the host functions alike, and the ramp played through the deck model
to a constant output period; and the pure host functions under the host's sanitizers in a program of their own."""
import ctypes as C
import itertools
import math
import pathlib
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import deck_finegrid_cases as fc
import deck_finegrid_model as fm
import deck_tempomap_cases as tc
import deck_tempomap_model as tm
from deck_tempomap_model import PERIOD_MAX, PERIOD_MIN, Q16, Settings

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_tempomap_check", "mx_deck_tempomap_count", "mx_deck_tempomap_span", "mx_deck_tempomap_host", "mx_deck_tempomap_path", "mx_deck_tempomap_segments",
                "mx_deck_tempomap_at", "mx_deck_tempomap_step", "mx_deck_analyse_tempomap", "mx_deck_read_tempomap", "mx_deck_read_tempomap_onsets", "mx_deck_debug_last_tempomap"}
STRUCTS = {"mx_deck_tempomap": (32, {"hop": 0, "n_periods": 4, "period0_q16": 8, "dperiod_q16": 16, "window_hops": 20, "stride_hops": 24, "_pad": 28}),
           "mx_deck_tempo_segment": (40, {"start_q32": 0, "grid": 8, "score": 24, "window": 32, "flags": 36})}
ONE = 1 << 32


def dk():
    from mixlab_amd import deck
    return deck


def c_settings(s: Settings):
    d = dk().tempomap(s.hop, s.n_periods, s.period0, s.dperiod, s.window, s.stride)
    d._pad = s.pad
    return d


def m_settings(c) -> Settings:
    return Settings(c.hop, c.n_periods, c.period0_q16, c.dperiod_q16, c.window_hops, c.stride_hops, c._pad)


def tuples(recs) -> list:
    """[v][j] of (score, phase, beats) from abi.DECK_COMB_DTYPE[V, J]"""
    return [[(int(r["score"]), int(r["phase"]), int(r["beats"])) for r in row] for row in recs]


def comb_array(recs) -> np.ndarray:
    from mixlab_amd import abi
    return np.array([list(row) for row in recs], abi.DECK_COMB_DTYPE)


def seg_tuples(segs) -> list:
    return [tm.Segment(*(int(x) for x in g)) for g in segs]


def seg_array(segs) -> np.ndarray:
    from mixlab_amd import abi
    return np.array([tuple(g) for g in segs], abi.DECK_TEMPO_SEGMENT_DTYPE)


def lib_path(score, penalty):
    from mixlab_amd import abi
    recs = np.zeros((len(score), len(score[0])), abi.DECK_COMB_DTYPE)
    recs["score"] = np.array(score, np.uint64)
    try:
        return dk().tempomap_path(recs, penalty).tolist()
    except abi.MxError as e:
        assert e.code == abi.MX_ERR_INVALID
        return None


def scores(recs):
    return [[r[0] for r in row] for row in recs]


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    for name, (size, offs) in STRUCTS.items():
        assert lay[name] == {"size": size, "offsets": offs}, name
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # additions only
    assert (consts["MX_DECK_TEMPOMAP_MAX_WINDOW"], consts["MX_DECK_TEMPOMAP_MAX_PERIODS"], consts["MX_DECK_TEMPOMAP_MAX_RECORDS"], consts["MX_DECK_TEMPOMAP_GROUP"],
            consts["MX_DECK_TEMPO_EMPTY"], consts["MX_DECK_TEMPOMAP_STAGED_MAX"]) == (tm.MAX_WINDOW, tm.MAX_PERIODS, tm.MAX_RECORDS, tm.GROUP, tm.EMPTY, tm.STAGED_MAX)
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_tempomap_check") == ["const mx_deck_tempomap*", "uint64_t"]
    assert sig("mx_deck_tempomap_count") == ["const mx_deck_tempomap*", "uint64_t", "uint32_t*"]
    assert sig("mx_deck_tempomap_span") == ["uint64_t", "uint64_t", "uint32_t", "uint32_t", "uint64_t", "uint32_t", "mx_deck_tempomap*", "uint32_t*"]
    assert sig("mx_deck_tempomap_host") == ["const int16_t*", "uint64_t", "const mx_deck_tempomap*", "mx_deck_comb*", "uint32_t*"]
    assert sig("mx_deck_tempomap_path") == ["const mx_deck_comb*", "uint32_t", "uint32_t", "uint64_t", "uint32_t*"]
    assert sig("mx_deck_tempomap_segments") == ["const mx_deck_comb*", "const mx_deck_tempomap*", "uint64_t", "const uint32_t*", "mx_deck_tempo_segment*"]
    assert sig("mx_deck_tempomap_at") == ["const mx_deck_tempo_segment*", "uint32_t", "int64_t", "mx_deck_beats*", "uint32_t*"]
    assert sig("mx_deck_tempomap_step") == ["const mx_deck_beats*", "int64_t", "int64_t*"]
    assert sig("mx_deck_analyse_tempomap") == ["mx_deck*", "const mx_deck_tempomap*"]
    assert sig("mx_deck_read_tempomap") == ["mx_deck*", "uint64_t", "uint64_t", "mx_deck_comb*"]
    assert sig("mx_deck_read_tempomap_onsets") == ["mx_deck*", "uint64_t", "uint64_t", "uint32_t*"]
    assert re.search(r"int mx_deck_debug_last_tempomap\(uint32_t out\[4\]\);", text)
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | set(STRUCTS)):
        assert re.search(rf"\b{name}\b", note), name
    # the new comment stands below BARS, whose own declarations are as they were
    assert text.index("---- BARS:") < text.index("int mx_deck_debug_last_bars(uint32_t out[4]);") < text.index("---- TEMPO MAP:") < text.index("pixel path:")
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}


def test_ctypes_mirrors_have_the_headers_layout():
    from mixlab_amd import abi
    for st, name in ((abi.DeckTempomap, "mx_deck_tempomap"), (abi.DeckTempoSegment, "mx_deck_tempo_segment")):
        size, offs = STRUCTS[name]
        assert C.sizeof(st) == size and {n: getattr(st, n).offset for n, _t in st._fields_} == offs, name
    dt = abi.DECK_TEMPO_SEGMENT_DTYPE
    assert dt.itemsize == 40 and [dt.fields[n][1] for n in ("start_q32", "first_q32", "period_q32", "score", "window", "flags")] == [0, 8, 16, 24, 32, 36]
    assert (abi.DECK_TEMPOMAP_MAX_WINDOW, abi.DECK_TEMPOMAP_MAX_PERIODS, abi.DECK_TEMPOMAP_MAX_RECORDS, abi.DECK_TEMPOMAP_GROUP, abi.DECK_TEMPO_EMPTY,
            abi.DECK_TEMPOMAP_STAGED_MAX) == (tm.MAX_WINDOW, tm.MAX_PERIODS, tm.MAX_RECORDS, tm.GROUP, tm.EMPTY, tm.STAGED_MAX)


# ---- the setting rules, accepted at the bound and refused one past it (a track of 1000 frames unless stated: N = 63 at h = 16) ----
BASE = Settings(16, 2, 10 * Q16, 5, 40, 20)
WIDE = {"n_periods": 1, "dperiod": 0, "window": 16384, "stride": 16384}
CHECKS = [({}, 1000, True),
          ({"hop": 16}, 1000, True), ({"hop": 256}, 1000, True), ({"hop": 8}, 1000, False), ({"hop": 512}, 1000, False), ({"hop": 48}, 1000, False), ({"hop": 0}, 1000, False),
          ({"n_periods": 1}, 1000, True), ({"n_periods": 1024}, 1000, True), ({"n_periods": 0}, 1000, False), ({"n_periods": 1025}, 1000, False),
          ({"n_periods": 1, "dperiod": 0}, 1000, True), ({"n_periods": 2, "dperiod": 0}, 1000, False), ({"n_periods": 2, "dperiod": 1}, 1000, True),
          ({"period0": PERIOD_MIN}, 1000, True), ({"period0": PERIOD_MIN - 1}, 1000, False),
          ({**WIDE, "period0": 8192 * Q16}, 1000, True), ({**WIDE, "period0": 8192 * Q16 + 1}, 1000, False),                 # the window rule stops a period the range admits
          ({**WIDE, "period0": PERIOD_MAX}, 1000, False), ({**WIDE, "period0": PERIOD_MAX + 1}, 1000, False),              # ... and the range one beyond it: the rules' order
          ({"n_periods": 3, "period0": PERIOD_MAX - 9}, 1000, False),
          ({"window": 22}, 1000, True), ({"window": 21}, 1000, False), ({"window": 16384}, 1000, True), ({"window": 16385}, 1000, False),
          ({"n_periods": 1, "period0": 11 * Q16, "window": 22}, 1000, True), ({"n_periods": 2, "period0": 11 * Q16, "dperiod": 1, "window": 22, "stride": 5}, 1000, False),
          ({"stride": 1}, 1000, True), ({"stride": 0}, 1000, False), ({"stride": 40}, 1000, True), ({"stride": 41}, 1000, False),
          ({"pad": 1}, 1000, False),
          ({}, 1, True), ({}, 0, False), (WIDE, 1 << 30, True), (WIDE, (1 << 30) + 1, False),
          ({"n_periods": 1024, "period0": 4 * Q16, "dperiod": 1, "window": 10, "stride": 1}, 1033 * 16, True),               # V * n_periods = 2^20
          ({"n_periods": 1024, "period0": 4 * Q16, "dperiod": 1, "window": 10, "stride": 1}, 1033 * 16 + 1, False)]
WORDS = {"hop": "hop", "n_periods": "n_periods", "dperiod": "dperiod_q16", "period": "period", "window_hops": "window_hops", "stride_hops": "stride_hops", "pad": "_pad",
         "n_frames": "n_frames"}


@pytest.mark.parametrize("change,n_frames,ok", CHECKS, ids=lambda v: str(v))
def test_check_rules_at_their_bounds(change, n_frames, ok):
    from mixlab_amd import abi
    s = BASE._replace(**change)
    rule = tm.check(s, n_frames)
    assert (rule is None) == ok
    if ok:
        dk().tempomap_check(c_settings(s), n_frames)
        N = tm.hops(n_frames, s.hop)
        assert dk().tempomap_count(c_settings(s), n_frames) == tm.windows(N, s.window, s.stride)
    else:
        for call in (dk().tempomap_check, dk().tempomap_count):
            with pytest.raises(abi.MxError) as err:
                call(c_settings(s), n_frames)
            assert err.value.code == abi.MX_ERR_INVALID
            assert WORDS[rule] in str(err.value), err.value   # mx_last_error names the broken rule


def test_the_rule_that_refuses_is_the_one_the_order_says():
    from mixlab_amd import abi
    assert tm.check(BASE._replace(**WIDE, period0=PERIOD_MAX), 1000) == "window_hops" and tm.check(BASE._replace(**WIDE, period0=PERIOD_MAX + 1), 1000) == "period"
    with pytest.raises(abi.MxError, match="window_hops"):
        dk().tempomap_check(c_settings(BASE._replace(**WIDE, period0=PERIOD_MAX)), 1000)
    with pytest.raises(abi.MxError, match="windows x n_periods"):
        dk().tempomap_check(c_settings(tc.ONE_PAST[1]), tc.ONE_PAST[0])
    assert tm.windows(1, 8, 8) == 1 and tm.windows(8, 8, 3) == 1 and tm.windows(9, 8, 3) == 2 and tm.windows(11, 8, 3) == 2 and tm.windows(12, 8, 3) == 3


def test_the_other_refusals():
    from mixlab_amd import abi, deck
    s = c_settings(BASE)
    x = np.zeros((100, 2), np.int16)
    rec = np.zeros((2, 2), abi.DECK_COMB_DTYPE)
    idx = np.zeros(2, np.uint32)
    segs = np.zeros(2, abi.DECK_TEMPO_SEGMENT_DTYPE)
    p = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    L = abi.lib
    assert L.mx_deck_tempomap_check(None, 1000) == L.mx_deck_tempomap_count(None, 1000, C.byref(C.c_uint32())) == L.mx_deck_tempomap_count(C.byref(s), 1000, None) == abi.MX_ERR_INVALID
    assert L.mx_deck_tempomap_host(None, 1000, C.byref(s), p(rec), None) == L.mx_deck_tempomap_host(p(x), 1000, None, p(rec), None) == abi.MX_ERR_INVALID
    assert L.mx_deck_tempomap_host(p(x), 1000, C.byref(s), None, None) == abi.MX_ERR_INVALID
    assert L.mx_deck_tempomap_path(None, 2, 2, 0, p(idx)) == L.mx_deck_tempomap_path(p(rec), 2, 2, 0, None) == abi.MX_ERR_INVALID
    assert L.mx_deck_tempomap_path(p(rec), 0, 2, 0, p(idx)) == L.mx_deck_tempomap_path(p(rec), 2, 0, 0, p(idx)) == L.mx_deck_tempomap_path(p(rec), 1 << 11, 1 << 10, 0, p(idx)) \
        == abi.MX_ERR_INVALID
    assert L.mx_deck_tempomap_path(p(rec), 2, 2, (1 << 40) + 1, p(idx)) == abi.MX_ERR_INVALID and L.mx_deck_tempomap_path(p(rec), 2, 2, 1 << 40, p(idx)) == abi.MX_OK
    assert lib_path([[0, (1 << 40) + 1]], 0) is None and lib_path([[0, 1 << 40]], 0) == [1] and tm.path([[0, (1 << 40) + 1]], 0) is None
    n = 800                                                                                                      # N = 50: two windows
    assert L.mx_deck_tempomap_segments(p(rec), C.byref(s), n, p(idx), p(segs)) == abi.MX_OK
    assert L.mx_deck_tempomap_segments(None, C.byref(s), n, p(idx), p(segs)) == L.mx_deck_tempomap_segments(p(rec), None, n, p(idx), p(segs)) == abi.MX_ERR_INVALID
    assert L.mx_deck_tempomap_segments(p(rec), C.byref(s), n, None, p(segs)) == L.mx_deck_tempomap_segments(p(rec), C.byref(s), n, p(idx), None) == abi.MX_ERR_INVALID
    idx[1] = 2
    assert L.mx_deck_tempomap_segments(p(rec), C.byref(s), n, p(idx), p(segs)) == abi.MX_ERR_INVALID          # an index at n_periods
    g, k = abi.DeckBeats(), C.c_uint32()
    assert L.mx_deck_tempomap_at(None, 2, 0, C.byref(g), C.byref(k)) == L.mx_deck_tempomap_at(p(segs), 0, 0, C.byref(g), C.byref(k)) == abi.MX_ERR_INVALID
    segs["start_q32"] = [-tm.FAR, 5]
    assert L.mx_deck_tempomap_at(p(segs), 2, tm.FAR + 1, C.byref(g), C.byref(k)) == L.mx_deck_tempomap_at(p(segs), 2, -tm.FAR - 1, C.byref(g), C.byref(k)) == abi.MX_ERR_INVALID
    assert L.mx_deck_tempomap_at(p(segs), 2, 5, None, None) == abi.MX_OK and L.mx_deck_tempomap_at(p(segs[1:]), 1, 4, C.byref(g), C.byref(k)) == abi.MX_ERR_INVALID
    st = C.c_int64()
    assert L.mx_deck_tempomap_step(None, ONE, C.byref(st)) == L.mx_deck_tempomap_step(C.byref(abi.DeckBeats(0, ONE)), ONE, None) == abi.MX_ERR_INVALID
    assert L.mx_deck_debug_last_tempomap(None) == abi.MX_ERR_INVALID
    assert L.mx_deck_tempomap_span(10 * Q16, 100, 8, 4, 1000, 16, None, None) == abi.MX_ERR_INVALID
    for args in ((PERIOD_MIN - 1, 10, 8, 4, 100, 16), (8192 * Q16 + 1, 10, 8, 4, 100, 16), (10 * Q16, 10, 0, 4, 100, 16), (10 * Q16, 10, 4097, 4, 100, 16),
                 (10 * Q16, 10, 8, 0, 100, 16), (10 * Q16, 10, 8, 4097, 100, 16), (10 * Q16, 10, 8, 4, 0, 16), (10 * Q16, 10, 8, 4, (1 << 26) + 1, 16), (10 * Q16, 10, 8, 4, 100, 20),
                 (4 * Q16, 1 << 30, 1, 1, 1 << 26, 16)):                                                        # the last: 2^20 records would not hold it
        assert tm.span(*args) is None, args
        with pytest.raises(abi.MxError) as err:
            deck.tempomap_span(*args)
        assert err.value.code == abi.MX_ERR_INVALID, args


# ---- the rules against the model on every shared case ----
@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_host_records_and_onsets_equal_the_model(case):
    want, want_w = tc.truth(case)
    recs, w = dk().tempomap_host(tc.track(case), c_settings(case.settings), onsets=True)
    assert w.dtype == np.uint32 and np.array_equal(w.astype(np.int64), want_w), np.flatnonzero(w != want_w)[:4]
    assert tuples(recs) == want
    assert recs.shape == (dk().tempomap_count(c_settings(case.settings), len(tc.track(case))), case.settings.n_periods)


def test_the_cases_hold_what_their_names_say():
    t = {c.name: tc.truth(c) for c in tc.CASES}
    shape = lambda c: (tm.hops(len(tc.track(c)), c.settings.hop), c.settings.window, c.settings.stride)   # noqa: E731
    last_len = lambda c: shape(c)[0] - (len(t[c.name][0]) - 1) * c.settings.stride                         # noqa: E731
    assert all(len(tc.track(c)) <= 300000 for c in tc.CASES)
    assert len(tc.track(tc.BY_NAME["a 1-frame track"])) == 1
    assert shape(tc.BY_NAME["N < W"])[0] == 30 and shape(tc.BY_NAME["N = W"])[0] == 40 and shape(tc.BY_NAME["N = W + 1"])[0] == 41
    assert [len(t[n][0]) for n in ("N < W", "N = W", "N = W + 1")] == [1, 1, 2]
    c = tc.BY_NAME["T = W: no overlap, and a last window one hop long"]
    assert c.settings.window == c.settings.stride and last_len(c) == 1 and len(t[c.name][0]) == 4 and all(r[2] <= 1 for r in t[c.name][0][-1])
    c = tc.BY_NAME["T = 1 with W = 8 on 40 hops, n_periods 1"]
    assert shape(c) == (40, 8, 1) and len(t[c.name][0]) == 33 and c.settings.n_periods == 1
    c = tc.BY_NAME["a last window shorter than ceil(P)"]
    assert last_len(c) == 9 < tm.phases(c.settings.period0) and all(r[2] == 1 for r in t[c.name][0][-1])        # (every phase that has a tooth has one)
    s = tc.BY_NAME["256 and 257 phases"].settings
    assert [tm.phases(s.period0 + j * s.dperiod) for j in range(3)] == [tm.LANES, tm.LANES, tm.LANES + 1]
    s = tc.BY_NAME["several strides of phases"].settings
    assert min(tm.phases(s.period0 + j * s.dperiod) for j in range(2)) > 2 * tm.LANES
    assert tc.BY_NAME["dperiod 1, 40 periods"].settings.dperiod == 1
    c = tc.BY_NAME["W at the cap with h = 16"]
    assert c.settings.window == tm.MAX_WINDOW and c.settings.hop == 16 and len(t[c.name][0]) > 1
    c = tc.BY_NAME["V x n_periods = 2^20"]
    assert len(t[c.name][0]) * c.settings.n_periods == tm.MAX_RECORDS and tm.check(tc.ONE_PAST[1], tc.ONE_PAST[0]) == "n_periods"
    assert all(r[0] == 0 and r[1] == 0 for row in t["silence"][0] for r in row) and not t["silence"][1].any()
    rows = t["one silent window between loud ones"][0]
    assert [max(r[0] for r in row) > 0 for row in rows] == [True, True, False, True, True]
    c = tc.BY_NAME["a phase tie inside one window"]
    w = t[c.name][1]
    S = [sum(int(w[i]) for i in range(phi, 40, 5)) for phi in range(5)]
    assert S.count(max(S)) > 1 and t[c.name][0][0][0][1] == S.index(max(S))
    rows = t["an index tie inside one window"][0]
    assert all(row[1][0] == row[2][0] > row[0][0] for row in rows[:1]) and tm.path(scores(rows), 0)[0] == 1
    w = t["every sample -32768 at h = 256"][1]
    assert w[0] == 2 << 16 and w[1] == 1 << 16
    total = {}
    for c in tc.CASES:
        for k, v in tc.forms(c).items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total          # every kept kernel form occurs among the cases
    on = {n: tc.forms(tc.BY_NAME[n])["wgs_staged"] > 0 for n in ("the longest window that is staged", "one hop longer: read from memory", "W at the cap with h = 16",
                                                                 "T = 1 with W = 8 on 40 hops, n_periods 1", "N < W")}
    assert list(on.values()) == [True, False, False, False, True]      # both sides of the threshold, the cap, a single candidate, min(W, N) = N


@pytest.mark.parametrize("case", [c for c in fc.CASES if c.settings.n_periods <= tm.MAX_PERIODS and c.settings.first_hop == 0 and c.settings.max_beats == 0
                                  and c.settings.period0 + (c.settings.n_periods - 1) * c.settings.dperiod <= 8192 * Q16], ids=lambda c: c.name)
def test_one_window_over_the_whole_track_is_the_fine_grid(case):
    """W >= N: the records equal FINE GRID's at first_hop = 0, max_beats = 0 -- the model's, the fine grid model's and both host functions', byte for byte"""
    from mixlab_amd import deck
    f = case.settings
    N = fm.count(len(fc.track(case)), f.hop)
    s = Settings(f.hop, f.n_periods, f.period0, f.dperiod, max(N, 2 * tm.phases(f.period0 + (f.n_periods - 1) * f.dperiod)), 1)
    got = deck.tempomap_host(fc.track(case), c_settings(s))
    fine = deck.finegrid_host(fc.track(case), deck.finegrid(f.hop, f.n_periods, f.period0, f.dperiod))
    assert got.shape == (1, f.n_periods) and got.tobytes() == fine.tobytes()
    assert tuples(got)[0] == fc.truth(case)[0] == tm.comb(fc.truth(case)[1], s)[0]


# ---- the path ----
def brute(score, penalty):
    """the best of all index sequences; among equals the one the header's ties choose: the smallest last index, then the smallest one before it, ..."""
    V, J = len(score), len(score[0])
    best = max(tm.path_value(score, idx, penalty) for idx in itertools.product(range(J), repeat=V))
    return min((idx for idx in itertools.product(range(J), repeat=V) if tm.path_value(score, idx, penalty) == best), key=lambda idx: idx[::-1])


def test_path_equals_a_search_over_all_sequences():
    rng = np.random.default_rng(22)
    n = 0
    for V, J in ((1, 1), (1, 5), (5, 1), (2, 2), (3, 3), (5, 3), (4, 4), (6, 2), (3, 5)):
        for hi in (2, 4, 1000):                      # small ranges make ties
            for penalty in (0, 1, 2, 7, 1 << 40):
                score = rng.integers(0, hi, (V, J)).tolist()
                want = list(brute(score, penalty))
                assert tm.path(score, penalty) == want and lib_path(score, penalty) == want, (score, penalty)
                n += len(set(map(tuple, score))) < V or hi == 2
    assert n > 20
    flat = [[3, 3, 3]] * 4
    assert lib_path(flat, 0) == [0, 0, 0, 0] == lib_path(flat, 5)                       # every tie to the smallest
    assert lib_path([[0, 9, 0, 0], [0, 0, 0, 9], [0, 9, 0, 0]], 0) == [1, 3, 1]          # penalty 0 is the per-window pick
    assert lib_path([[0, 9, 0, 0], [0, 0, 0, 9], [0, 9, 0, 0]], 5) == [1, 1, 1]          # 9 + 9 against 27 - 20
    assert lib_path([[0, 9, 0, 0], [0, 0, 0, 9], [0, 9, 0, 0]], 1 << 40) == [1, 1, 1]
    assert lib_path([[1 << 40] * 2] * 3, 1 << 40) == [0, 0, 0]
    big = rng.integers(0, 1 << 30, (40, 30)).tolist()
    for penalty in (0, 1 << 20, 1 << 27, 1 << 40):
        assert lib_path(big, penalty) == tm.path(big, penalty)


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_path_and_segments_equal_the_model(case):
    from mixlab_amd import deck
    recs = tc.truth(case)[0]
    if len(recs) * len(recs[0]) > 1 << 16:
        recs = [row[:24] for row in recs[:60]]                                             # (the model's path is Python: a corner of the 2^20 records)
        s, n = case.settings._replace(n_periods=24), (case.settings.window + 59 * case.settings.stride) * case.settings.hop
    else:
        s, n = case.settings, len(tc.track(case))
    arr = comb_array(recs)
    for penalty in (0, tm.default_penalty(recs), 1 << 40):
        idx = tm.path(scores(recs), penalty)
        assert deck.tempomap_path(arr, penalty).tolist() == idx
        want = tm.segments(recs, s, n, idx)
        got = deck.tempomap_segments(arr, c_settings(s), n, np.array(idx, np.uint32))
        assert seg_tuples(got) == want
        for v, g in enumerate(want):                                                        # what the numbers mean, in Fractions
            if v and g.period:
                m = ((v * s.stride + (s.window - s.stride) // 2) * s.hop) << 32
                assert Fraction(g.start - g.first, g.period).denominator == 1 and m <= g.start < m + g.period
            assert bool(g.flags & tm.EMPTY) == (g.score == 0)
        pos = sorted({p for g in want for p in (g.start - 1, g.start, g.start + 1) if abs(p) <= tm.FAR} | {0, -tm.FAR, tm.FAR})
        for q in pos:
            grid, seg = deck.tempomap_at(got, q)
            assert ((grid.first_q32, grid.period_q32), seg) == tm.at(want, q)
            assert want[seg].start <= q and all(g.start > q for g in want[seg + 1:])


def test_empty_windows_inherit_and_an_empty_map_is_zero():
    c = tc.BY_NAME["one silent window between loud ones"]
    recs = tc.truth(c)[0]
    segs = tm.segments(recs, c.settings, len(tc.track(c)), tm.path(scores(recs), 0))
    assert [g.flags for g in segs] == [0, 0, tm.EMPTY, 0, 0] and (segs[2].first, segs[2].period) == (segs[1].first, segs[1].period) and segs[2].score == 0
    lead = [[(0, 0, 3)] * len(recs[0])] * 2 + recs[2:]                                     # leading empties take the first grid there is
    segs = tm.segments(lead, c.settings, len(tc.track(c)), tm.path(scores(lead), 0))
    assert [g.flags for g in segs] == [1, 1, 1, 0, 0] and len({(g.first, g.period) for g in segs[:4]}) == 1
    assert seg_tuples(dk().tempomap_segments(comb_array(lead), c_settings(c.settings), len(tc.track(c)), np.array(tm.path(scores(lead), 0), np.uint32))) == segs
    c = tc.BY_NAME["silence"]
    recs = tc.truth(c)[0]
    segs = tm.segments(recs, c.settings, len(tc.track(c)), [0] * len(recs))
    assert all((g.first, g.period, g.flags) == (0, 0, tm.EMPTY) for g in segs)
    assert [g.start for g in segs[1:]] == [((v * 11 + 9) * 32) << 32 for v in range(1, len(segs))]
    assert dk().tempomap_beats(seg_array(segs), 5000 << 32) == [] == tm.beats(segs, 5000 << 32)


def test_step_equals_the_model_and_fractions():
    from mixlab_amd import abi, deck
    rng = np.random.default_rng(5)
    draws = [(int(rng.integers(1, 1 << 45)), int(rng.integers(1, 1 << 45))) for _ in range(300)]
    draws += [(3, 2 << 32), (1, 2 << 32), (3 * ONE, 2 * ONE), (5, 2 * ONE), (7, 2 * ONE), (4 * ONE, ONE), (4 * ONE + 1, ONE), (1 << 56, 1 << 56), ((1 << 56) + 1, 1 << 56),
              (1 << 56, 1 << 54), (1 << 56, (1 << 54) - 1), (0, ONE), (ONE, 0), (ONE, -5), (ONE, (1 << 56) + 1), (2050 * ONE, 1900 * ONE)]
    live = 0
    for period, out in draws:
        want = tm.step(period, out)
        try:
            got = deck.tempomap_step(abi.DeckBeats(12345, period), out)
        except abi.MxError as e:
            assert e.code == abi.MX_ERR_INVALID
            got = None
        assert got == want, (period, out)
        if want is not None:
            live += 1
            exact = Fraction(period << 32, out)
            assert abs(exact - want) <= Fraction(1, 2) and (abs(exact - want) < Fraction(1, 2) or want % 2 == 0)     # nearest, ties to even
    assert live > 100
    assert tm.step(3, 2 << 32) == 2 and tm.step(1, 2 << 32) == 0 and tm.step(5, 2 * ONE) == 2 and tm.step(7, 2 * ONE) == 4       # 1.5 -> 2, 0.5 -> 0, 2.5 -> 2, 3.5 -> 4
    assert tm.step(4 * ONE, ONE) == 4 * ONE and tm.step(4 * ONE + 1, ONE) is None


SPANS = [(128 * Q16, 12 * Q16, 8, 4, 6000, 16), (351 * Q16 + 999, 21 * Q16, 16, 8, 450000, 64), (10 * Q16, 3000, 16, 8, 500, 16), (PERIOD_MIN, 100, 1, 1, 50, 32),
         (PERIOD_MIN + 7, 1 << 40, 4096, 4096, 5000, 32), (8192 * Q16, 9, 2, 1, 1 << 20, 16), (8000 * Q16, 1 << 30, 3, 4096, 1 << 20, 256), (20 * Q16, 0, 16, 8, 1000, 64),
         (20 * Q16, 511 * 2048, 16, 8, 4000, 64), (20 * Q16, 511 * 2048 + 1, 16, 8, 4000, 64), (1000 * Q16, 50 * Q16, 64, 1, 1 << 18, 16)]


@pytest.mark.parametrize("args", SPANS, ids=lambda a: str(a))
def test_span_equals_the_model_and_passes_the_check(args):
    from mixlab_amd import deck
    s, clipped = deck.tempomap_span(*args)
    want, want_clipped = tm.span(*args)
    assert (m_settings(s), clipped) == (want, want_clipped)
    assert tm.check(want, args[4] * args[5]) is None and want.period0 <= args[0] <= want.period0 + (want.n_periods - 1) * want.dperiod
    assert (args[0] - want.period0) % max(1, want.dperiod) == 0 and want.n_periods <= 1023       # the centre is a candidate; 511 a side


def test_span_says_what_the_header_says():
    s, clipped = tm.span(352 * Q16, 352 * Q16 * 6 // 100, 16, 8, 450000, 64)                       # a ten-minute track at 128 BPM and h = 64
    assert (s.dperiod, s.n_periods, s.stride, clipped) == (2048, 1023, 2816, True) and s.window == -(-16 * (352 * Q16 + 511 * 2048) // Q16)
    s, clipped = tm.span(128 * Q16, 12 * Q16, 8, 4, 6000, 16)
    assert (s.dperiod, s.n_periods, s.window, s.stride, clipped) == (4096, 385, 8 * 140, 512, False)
    assert tm.span(8000 * Q16, 1 << 30, 3, 4096, 1 << 20, 256)[0].window == tm.MAX_WINDOW == tm.span(8000 * Q16, 1 << 30, 3, 4096, 1 << 20, 256)[0].stride   # both cut
    assert tm.span(PERIOD_MIN, 100, 1, 1, 50, 32)[0].window == 2 * tm.phases(PERIOD_MIN + 100 * 1)                                                               # raised


# ---- the shared cases tell the header from its misreadings ----
PATH_TABLES = [([[5, 0, 5], [0, 4, 0], [5, 0, 5]], 1), ([[0, 0, 0, 9], [9, 0, 0, 0]], 2), ([[7, 7], [7, 7]], 0), ([[0, 0, 0, 8], [6, 0, 0, 0], [0, 0, 0, 8]], 2)]


@pytest.mark.parametrize("mis", tm.MISREADINGS)
def test_every_misreading_changes_a_compared_value_of_some_case(mis):
    """a model that misreads the header one way differs from what the LIBRARY computes on some case: the library is the compared value"""
    from mixlab_amd import abi, deck
    drift_cases = [(tc.drift_track(d),) + tc.drift_map(d)[1:4] for d in tc.DRIFTS]
    small = [c for c in tc.CASES if len(tc.truth(c)[0]) * c.settings.n_periods <= 1 << 12]
    if mis in ("window_end_ignored", "tie_largest_phase"):
        hit = [c.name for c in small if tm.analyse(tc.track(c), c.settings, mis=(mis,))[0] != tuples(deck.tempomap_host(tc.track(c), c_settings(c.settings)))]
    elif mis in ("path_ties_largest", "penalty_squared"):
        hit = [k for k, (score, pen) in enumerate(PATH_TABLES) if tm.path(score, pen, mis=(mis,)) != lib_path(score, pen)]
    elif mis == "step_truncated":
        hit = [a for a in ((3, 2 << 32), (2050 * ONE + 1, 1900 * ONE)) if tm.step(*a, mis=(mis,)) != deck.tempomap_step(abi.DeckBeats(0, a[0]), a[1])]
    elif mis == "seam_without_half_period":
        hit = []
        for tr, s, recs, idx in drift_cases:
            segs = tm.segments(recs, s, len(tr), idx)
            if tm.beats(segs, len(tr) << 32, mis=(mis,)) != deck.tempomap_beats(seg_array(segs), len(tr) << 32):
                hit.append(s)
    else:
        hit = []
        every = [(tc.track(c), c.settings, tc.truth(c)[0], tm.path(scores(tc.truth(c)[0]), 0)) for c in small] + drift_cases
        for tr, s, recs, idx in every:
            got = deck.tempomap_segments(comb_array(recs), c_settings(s), len(tr), np.array(idx, np.uint32))
            if tm.segments(recs, s, len(tr), idx, mis=(mis,)) != seg_tuples(got):
                hit.append(s)
    assert hit, mis


# ---- the property that makes the feature worth having ----
def lib_map(d: tc.Drift):
    """Deck.map_tempo's rule restated on the host functions alone: (segments as the model's tuples, beats)"""
    from mixlab_amd import deck
    tr = tc.drift_track(d)
    pick = tc.whole_track_pick(d)
    centre = (pick.grid.period >> 16) // tc.HOP
    s, _ = deck.tempomap_span(centre, int(centre * tc.WIDTH), tc.WINDOW_BEATS, tc.STRIDE_BEATS, deck.finegrid_count(len(tr), tc.HOP), tc.HOP)
    recs = deck.tempomap_host(tr, s)
    penalty = sum(int(v) for v in recs["score"].max(axis=1)) // recs.size
    segs = deck.tempomap_segments(recs, s, len(tr), deck.tempomap_path(recs, penalty))
    return seg_tuples(segs), deck.tempomap_beats(segs, len(tr) << 32)


@pytest.mark.parametrize("d", tc.DRIFTS, ids=lambda d: d.name)
def test_the_map_sits_on_every_click_where_the_whole_track_grid_cannot(d):
    segs, s, recs, idx, pick = tc.drift_map(d)
    end = tc.N_FRAMES << 32
    got_segs, got_beats = lib_map(d)
    beats = tm.beats(segs, end)
    assert got_segs == segs and got_beats == beats                                          # the host functions and the model agree on the whole map
    assert len(d.starts) == (47 if d.name != "gap" else 31) and len(tc.drift_track(d)) == tc.N_FRAMES <= 300000
    # 1. the whole-track grid of FINE GRID's two stages misses some click by more than a quarter beat (on the two tracks that sound throughout)
    beat_hops = (pick.grid.period >> 32) / tc.HOP
    whole = tc.misses(d, [pick.grid.first + k * pick.grid.period for k in range(-2, 60)])
    print(f"{d.name}: whole-track period {pick.grid.period / 2.0 ** 32:.2f} frames, worst click {max(whole)} hops (a beat is {beat_hops:.0f})")
    if d.name != "gap":
        assert max(whole) > beat_hops / 4, "the track proves nothing"
    # 2. the map puts every click within a bound of a beat: one hop of quantisation (a click's hop against a tooth's), one for the tooth's half-width, and the ramp's
    # curvature over half a window -- a window fits ONE period to beats whose period changes by dp a beat, so a beat window_beats / 2 from its middle lies
    # dp * (window_beats / 2)^2 / 2 frames off the straight line, rounded up to hops
    bound = 1 + 1 + math.ceil(d.dp_per_beat * (tc.WINDOW_BEATS / 2) ** 2 / 2 / tc.HOP)
    miss = tc.misses(d, [b for b, _v in beats])
    # 3. on the step track the clicks inside the windows that contain the jump are exempt, 3 of 47 at the most
    exempt = set()
    if d.name == "step":
        jump = d.starts[23] // tc.HOP
        inside = [v for v in range(len(segs)) if v * s.stride <= jump < v * s.stride + s.window]
        lo, hi = max(g.start for g in segs[:inside[0] + 1]), segs[inside[-1] + 1].start if inside[-1] + 1 < len(segs) else end
        exempt = {k for k, f in enumerate(d.starts) if miss[k] > bound and lo <= (f << 32) < hi}
        assert len(exempt) <= 3
    print(f"{d.name}: bound {bound} hops; the map's misses {miss}; exempt {sorted(exempt)}; path {idx}; penalty {tm.default_penalty(recs)}; "
          f"empty windows {[g.window for g in segs if g.flags]}")
    assert all(m <= bound for k, m in enumerate(miss) if k not in exempt), (bound, miss)
    # 4. every interval between consecutive beats of the map lies in [0.75, 1.25] of its segment's period
    ratios = [Fraction(b1 - b0, segs[v1].period) for (b0, _v0), (b1, v1) in zip(beats, beats[1:])]
    print(f"{d.name}: {len(beats)} beats, intervals {float(min(ratios)):.3f} .. {float(max(ratios)):.3f} periods")
    assert len(beats) >= len(d.starts) and Fraction(3, 4) <= min(ratios) and max(ratios) <= Fraction(5, 4)
    if d.name == "gap":                                                                      # the grid is carried across the silence
        assert any(g.flags & tm.EMPTY for g in segs) and all(g.period for g in segs)


# ---- warp ----
def test_the_ramp_comes_out_at_a_constant_beat_length_under_the_warp_and_not_without():
    d = tc.DRIFT_BY_NAME["ramp"]
    segs = tc.drift_map(d)[0]
    tables = np.stack([dk().deck_tables(b) for b in range(4)])
    target = tc.WARP_OUT_PERIOD / 2.0 ** 32
    out, ticks, changes = tc.warp_run(d, segs, tables)
    got = np.diff(fc.burst_centroids(out))
    # The bound, in output frames, for an interval between two clicks that the head plays inside one segment at the step P_seg / target, so that a track interval p
    # comes out as p * target / P_seg:
    #   the ramp inside a segment: a segment plays the beats between two overlap middles, stride_beats of them and one for the seam, centred on its window; the window's
    #     fitted period is its mean interval, and an interval (stride_beats / 2 + 1) beats from the centre differs from it by dp * (stride_beats / 2 + 1) frames;
    #   the fit itself: two teeth 1.5 hops wide at the ends of window_beats - 1 intervals, 2 * 1.5 h / (window_beats - 1), and the candidates' spacing dperiod * h / 65536;
    #   all of it scaled by target / P_min;
    #   the tick: the step changes at the first tick after the head entered a segment, up to spt output frames late, and over those the old step is off by the change of
    #     the period from one segment to the next, dp * stride_beats / P_min;
    #   one frame for the centroids of bursts that the interpolator's 32 taps smear symmetrically, and the roundings.
    s = tc.drift_map(d)[1]
    p_min = 1900.0
    bound = ((d.dp_per_beat * (tc.STRIDE_BEATS / 2 + 1) + 3.0 * tc.HOP / (tc.WINDOW_BEATS - 1) + s.dperiod * tc.HOP / 65536.0) * target / p_min
             + tc.WARP_SPT * d.dp_per_beat * tc.STRIDE_BEATS / p_min + 1.0)
    print(f"bound {bound:.1f} output frames; warped intervals - target: {np.round(got - target, 1).tolist()}; step changes {[(t, v, round(st / 2.0 ** 32, 4)) for t, v, st in changes]}")
    assert len(got) >= 20 and len(changes) >= 4 and len({v for _t, v, _s in changes}) == len(changes)
    assert np.abs(got - target).max() <= bound, (bound, got - target)
    assert bound < 0.03 * target
    flat, _t, _c = tc.warp_run(d, segs, tables, warped=False)
    free = np.diff(fc.burst_centroids(flat))
    print(f"one constant step: intervals - target: {np.round(free - target, 1).tolist()}")
    assert np.abs(free - target).max() > bound
    assert [t.step for t in ticks][:3] == [changes[0][2]] * 3 and ticks[0].pos == 0


# ---- the pure host functions under the host's sanitizers ----
def test_the_host_functions_run_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    import deck_tempomap_check
    try:
        out = deck_tempomap_check.main(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail(f"the sanitized program failed ({e.returncode}):\n{e.stdout or ''}\n{e.stderr or ''}")
    assert out.rstrip().endswith("deck_tempomap_check: ok"), out
