"""The deck's fine beat grid and sync without a device (include/mixlab_gpu.h "FINE GRID"): the header's structs and entry points, the setting
rules at both edges of each, mx_deck_finegrid_host / _pick / _span / _period and mx_deck_sync against the model (tests/deck_finegrid_model.py) on every shared case
(tests/deck_finegrid_cases.py), sync against Python big integers on random draws, that the shared cases tell the text from each of a list of misreadings, the property
that makes the feature worth having -- a grid that sits on every beat of a click track with a non-integer period, to the last one -- on the model and on the host
functions alike, through one stage and through both, and two decks synced and played through the deck model whose bursts coincide to the end of the run."""
import ctypes as C
import pathlib
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import deck_finegrid_cases as fc
import deck_finegrid_model as fm
import deck_model as dm
from deck_finegrid_model import PERIOD_MAX, PERIOD_MIN, Q16, Settings

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_finegrid_check", "mx_deck_finegrid_count", "mx_deck_finegrid_span", "mx_deck_finegrid_period", "mx_deck_analyse_finegrid", "mx_deck_read_finegrid",
                "mx_deck_read_fine_onsets", "mx_deck_finegrid_host", "mx_deck_finegrid_pick", "mx_deck_sync", "mx_deck_debug_last_finegrid"}
STRUCTS = {"mx_deck_finegrid": (32, {"hop": 0, "n_periods": 4, "period0_q16": 8, "dperiod_q16": 16, "first_hop": 20, "max_beats": 24, "_pad": 28}),
           "mx_deck_comb": (16, {"score": 0, "phase": 8, "beats": 12}),
           "mx_deck_beats": (16, {"first_q32": 0, "period_q32": 8}),
           "mx_deck_fine_pick": (40, {"grid": 0, "score": 16, "bpm": 24, "index": 32, "n_beats": 36}),
           "mx_deck_sync_result": (24, {"step_q32": 0, "seek_q32": 8, "delta_q32": 16})}


def dk():
    from mixlab_amd import deck
    return deck


def c_settings(s: Settings):
    d = dk().finegrid(s.hop, s.n_periods, s.period0, s.dperiod, s.first_hop, s.max_beats)
    d._pad = s.pad
    return d


def m_settings(c) -> Settings:
    return Settings(c.hop, c.n_periods, c.period0_q16, c.dperiod_q16, c.first_hop, c.max_beats, c._pad)


def _comb_dtype():
    from mixlab_amd import abi
    return abi.DECK_COMB_DTYPE


def tuples(recs) -> list:
    return [(int(r["score"]), int(r["phase"]), int(r["beats"])) for r in recs]


def c_beats(b: fm.Beats):
    from mixlab_amd import abi
    return abi.DeckBeats(b.first, b.period)


def m_pick(p) -> fm.Pick:
    return fm.Pick(fm.Beats(p.grid.first_q32, p.grid.period_q32), p.score, p.bpm, p.index, p.n_beats)


def host_records(case_or_track, s: Settings) -> list:
    tr = fc.track(case_or_track) if isinstance(case_or_track, fc.Case) else case_or_track
    return tuples(dk().finegrid_host(tr, c_settings(s)))


def c_sync(l, lpos, lstep, f, fpos):
    from mixlab_amd import abi
    try:
        return dk().deck_sync(c_beats(l), lpos, lstep, c_beats(f), fpos)
    except abi.MxError as e:
        assert e.code == abi.MX_ERR_INVALID
        return None


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    for name, (size, offs) in STRUCTS.items():
        assert lay[name] == {"size": size, "offsets": offs}, name
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # additions only
    assert consts["MX_DECK_FINEGRID_LANES"] == fm.LANES and consts["MX_DECK_FINEGRID_MAX_PERIODS"] == fm.MAX_PERIODS
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_finegrid_check") == ["const mx_deck_finegrid*", "uint64_t"]
    assert sig("mx_deck_finegrid_span") == ["uint64_t", "uint64_t", "uint32_t", "uint64_t", "uint32_t", "mx_deck_finegrid*", "uint32_t*"]
    assert sig("mx_deck_analyse_finegrid") == ["mx_deck*", "const mx_deck_finegrid*"]
    assert sig("mx_deck_read_finegrid") == ["mx_deck*", "uint64_t", "uint64_t", "mx_deck_comb*"]
    assert sig("mx_deck_read_fine_onsets") == ["mx_deck*", "uint64_t", "uint64_t", "uint32_t*"]
    assert sig("mx_deck_finegrid_host") == ["const int16_t*", "uint64_t", "const mx_deck_finegrid*", "mx_deck_comb*", "uint32_t*"]
    assert sig("mx_deck_finegrid_pick") == ["const mx_deck_comb*", "const mx_deck_finegrid*", "double", "mx_deck_fine_pick*"]
    assert sig("mx_deck_sync") == ["const mx_deck_beats*", "int64_t", "int64_t", "const mx_deck_beats*", "int64_t", "mx_deck_sync_result*"]
    assert re.search(r"int mx_deck_debug_last_finegrid\(uint32_t out\[4\]\);", text)
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | set(STRUCTS)):
        assert re.search(rf"\b{name}\b", note), name
    # the new comment stands below KEY AND LOUDNESS, whose own declarations are as they were
    assert text.index("---- KEY AND LOUDNESS:") < text.index("int mx_tonality_camelot(int key, uint32_t* number, uint32_t* minor);") < text.index("---- FINE GRID:")
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}


def test_ctypes_mirrors_have_the_headers_layout():
    from mixlab_amd import abi
    for st, name in ((abi.DeckFinegrid, "mx_deck_finegrid"), (abi.DeckComb, "mx_deck_comb"), (abi.DeckBeats, "mx_deck_beats"), (abi.DeckFinePick, "mx_deck_fine_pick"),
                     (abi.DeckSyncResult, "mx_deck_sync_result")):
        size, offs = STRUCTS[name]
        assert C.sizeof(st) == size and {n: getattr(st, n).offset for n, _t in st._fields_} == offs, name
    assert abi.DECK_COMB_DTYPE.itemsize == 16 and [abi.DECK_COMB_DTYPE.fields[n][1] for n in ("score", "phase", "beats")] == [0, 8, 12]
    assert abi.DECK_FINEGRID_LANES == fm.LANES and abi.DECK_FINEGRID_MAX_PERIODS == fm.MAX_PERIODS


# ---- the setting rules, accepted at the bound and refused one past it (a track of 1000 frames: N = 63 at h = 16, 4 at h = 256) ----
BASE = Settings(16, 2, 10 * Q16, 5)
CHECKS = [({}, True),
          ({"hop": 16}, True), ({"hop": 256}, True), ({"hop": 8}, False), ({"hop": 512}, False), ({"hop": 48}, False), ({"hop": 0}, False),
          ({"n_periods": 1}, True), ({"n_periods": 8192}, True), ({"n_periods": 0}, False), ({"n_periods": 8193}, False),
          ({"n_periods": 1, "dperiod": 0}, True), ({"n_periods": 2, "dperiod": 0}, False), ({"n_periods": 2, "dperiod": 1}, True),
          ({"period0": PERIOD_MIN}, True), ({"period0": PERIOD_MIN - 1}, False), ({"n_periods": 1, "period0": PERIOD_MAX}, True),
          ({"n_periods": 1, "period0": PERIOD_MAX + 1}, False), ({"period0": PERIOD_MAX - 5}, True), ({"period0": PERIOD_MAX - 4}, False),
          ({"n_periods": 8192, "period0": PERIOD_MAX - 8191 * 5}, True), ({"n_periods": 8192, "period0": PERIOD_MAX - 8191 * 5 + 1}, False),
          ({"first_hop": 62}, True), ({"first_hop": 63}, False), ({"hop": 256, "first_hop": 3}, True), ({"hop": 256, "first_hop": 4}, False),
          ({"max_beats": 0}, True), ({"max_beats": 2}, True), ({"max_beats": 1}, False), ({"max_beats": 0xFFFFFFFF}, True),
          ({"pad": 1}, False)]


@pytest.mark.parametrize("change,ok", CHECKS, ids=lambda v: str(v))
def test_check_rules_at_their_bounds(change, ok):
    from mixlab_amd import abi
    s = BASE._replace(**change)
    assert (fm.check(s, 1000) is None) == ok
    if ok:
        dk().finegrid_check(c_settings(s), 1000)
    else:
        with pytest.raises(abi.MxError) as err:
            dk().finegrid_check(c_settings(s), 1000)
        assert err.value.code == abi.MX_ERR_INVALID
        words = {"hop": "hop", "n_periods": "n_periods", "dperiod": "dperiod_q16", "period": "period", "max_beats": "max_beats", "pad": "_pad", "first_hop": "first_hop"}
        assert words[fm.check(s, 1000)] in str(err.value), err.value   # mx_last_error names the broken rule


def test_check_count_and_the_other_refusals():
    from mixlab_amd import abi, deck
    assert deck.finegrid_count(1, 16) == 1 and deck.finegrid_count(1 << 30, 16) == 1 << 26 and deck.finegrid_count(257, 256) == 2
    bad = [lambda: deck.finegrid_count(0, 16), lambda: deck.finegrid_count((1 << 30) + 1, 16), lambda: deck.finegrid_count(100, 24),
           lambda: deck.finegrid_check(c_settings(BASE), 0), lambda: deck.finegrid_check(c_settings(BASE), (1 << 30) + 1),
           lambda: deck.finegrid_span(PERIOD_MIN - 1, 10, 0, 100, 16), lambda: deck.finegrid_span(PERIOD_MAX + 1, 10, 0, 100, 16),
           lambda: deck.finegrid_span(10 * Q16, 10, 1, 100, 16), lambda: deck.finegrid_span(10 * Q16, 10, 0, 0, 16), lambda: deck.finegrid_span(10 * Q16, 10, 0, (1 << 26) + 1, 16),
           lambda: deck.finegrid_span(10 * Q16, 10, 0, 100, 20),
           lambda: deck.finegrid_period(float("nan"), 512, 64), lambda: deck.finegrid_period(46.0, 500, 64), lambda: deck.finegrid_period(46.0, 512, 8),
           lambda: deck.finegrid_period(0.4, 512, 64), lambda: deck.finegrid_period(5000.0, 512, 64),
           lambda: deck.finegrid_host(np.zeros((100, 2), np.int16), c_settings(BASE._replace(first_hop=7))),
           lambda: deck.finegrid_pick(np.zeros(2, abi.DECK_COMB_DTYPE), c_settings(BASE), 0.0),
           lambda: deck.finegrid_pick(np.zeros(2, abi.DECK_COMB_DTYPE), c_settings(BASE), float("inf")),
           lambda: deck.finegrid_pick(np.zeros(2, abi.DECK_COMB_DTYPE), c_settings(BASE._replace(hop=17)), 48000.0)]
    for k, fn in enumerate(bad):
        with pytest.raises(abi.MxError) as err:
            fn()
        assert err.value.code == abi.MX_ERR_INVALID, k
    s = c_settings(BASE)
    rec = np.zeros(2, abi.DECK_COMB_DTYPE)
    x = np.zeros((100, 2), np.int16)
    assert abi.lib.mx_deck_finegrid_check(None, 1000) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_finegrid_host(None, 100, C.byref(s), rec.ctypes.data_as(C.c_void_p), None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_finegrid_host(x.ctypes.data_as(C.c_void_p), 100, C.byref(s), None, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_finegrid_host(x.ctypes.data_as(C.c_void_p), 100, None, rec.ctypes.data_as(C.c_void_p), None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_finegrid_host(x.ctypes.data_as(C.c_void_p), 100, C.byref(s), rec.ctypes.data_as(C.c_void_p), None) == abi.MX_OK
    assert abi.lib.mx_deck_finegrid_pick(None, C.byref(s), 48000.0, C.byref(abi.DeckFinePick())) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_sync(None, 0, 0, C.byref(abi.DeckBeats(0, 1)), 0, C.byref(abi.DeckSyncResult())) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_debug_last_finegrid(None) == abi.MX_ERR_INVALID
    # first_hop is not held against a track by the pick
    assert deck.finegrid_pick(rec, c_settings(BASE._replace(first_hop=1 << 30)), 48000.0).score == 0


# ---- the rules against the model on every shared case ----
@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_host_records_onsets_and_pick_equal_the_model(case):
    from mixlab_amd import deck
    want, want_w = fc.truth(case)
    recs, w = deck.finegrid_host(fc.track(case), c_settings(case.settings), onsets=True)
    assert w.dtype == np.uint32 and np.array_equal(w.astype(np.int64), want_w), np.flatnonzero(w != want_w)[:4]
    assert tuples(recs) == want
    assert len(w) == deck.finegrid_count(fc.track(case).shape[0], case.settings.hop) == fm.count(fc.track(case).shape[0], case.settings.hop)
    for rate in (48000.0, 44100.0):
        assert m_pick(deck.finegrid_pick(recs, c_settings(case.settings), rate)) == fm.pick(want, case.settings, rate)   # the bpm bit for bit: == on floats


def test_the_cases_hold_what_their_names_say():
    t = {}
    for c in fc.CASES:   # what the library's host function gives: held to the model in the test above, and what the device is held to
        recs, w = dk().finegrid_host(fc.track(c), c_settings(c.settings), onsets=True)
        t[c.name] = (tuples(recs), w.astype(np.int64))
    assert all(len(fc.track(c)) <= 60000 for c in fc.CASES)
    assert all(r == (0, 0, 15) for r in t["silence"][0]) and not t["silence"][1].any()
    w = t["every sample -32768 at h = 256"][1]
    assert w[0] == 2 << 16 and w[1] == 1 << 16                                            # A[0] = 2^20, o[0] = 2^16: the largest root and onset
    recs = t["equal scores on two candidates: an index tie"][0]
    assert recs[1][0] == recs[2][0] > recs[0][0] and fm.pick(recs, fc.BY_NAME["equal scores on two candidates: an index tie"].settings, fc.RATE).index == 1
    case = fc.BY_NAME["two equal bursts: a phase tie"]
    w = t[case.name][1]
    S = [sum(int(w[i]) for i in range(phi, len(w), 5)) for phi in range(5)]
    assert S.count(max(S)) > 1 and t[case.name][0][0][1] == S.index(max(S))
    assert all(r[2] == 1 for r in t["N smaller than one period: a single tooth"][0])
    assert all(r[2] == 2 for r in t["max_beats 2"][0]) and max(r[2] for r in t["max_beats larger than fits"][0]) < 1000
    s = fc.BY_NAME["an irregular fractional period"].settings
    assert len({((k + 1) * s.period0 >> 16) - (k * s.period0 >> 16) for k in range(40)}) == 2      # the teeth step by 7 and by 8 hops
    x = fc.track(fc.BY_NAME["negative odd sums"]).astype(np.int64).sum(axis=1)
    assert (x < 0).all() and (x % 2 == 1).all()
    assert [fm.phases(s.period0 + j * s.dperiod) for s in [fc.BY_NAME["256 and 257 phases"].settings] for j in range(3)] == [fm.LANES, fm.LANES, fm.LANES + 1]
    assert min(fm.phases(s.period0 + j * s.dperiod) for s in [fc.BY_NAME["several strides of phases"].settings] for j in range(2)) > 2 * fm.LANES
    assert sorted({c.settings.n_periods for c in fc.CASES})[0] == 1 and any(290 <= c.settings.n_periods <= 310 for c in fc.CASES)
    total = {}
    for c in fc.CASES:
        for k, v in fc.forms(c).items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total


SPANS = [(10 * Q16, 3000, 0, 500, 16), (10 * Q16, 3000, 64, 100000, 16), (375 * Q16, 375 * Q16 // 50, 64, 450000, 64), (375 * Q16 + 12345, 512, 0, 450000, 64),
         (PERIOD_MIN, 100, 0, 50, 32), (PERIOD_MIN + 7, 100, 2, 50, 32), (PERIOD_MAX, 9, 0, 1 << 26, 16), (PERIOD_MAX - 3, 9, 0, 7, 256), (20 * Q16, 0, 0, 1000, 64),
         (20 * Q16, 1 << 40, 0, 1000, 64), (20 * Q16, 4095 * 1638, 0, 400, 64), (20 * Q16, 4095 * 1638 + 1, 0, 400, 64), (4 * Q16 + 100, 5000, 0, 1 << 26, 16)]


@pytest.mark.parametrize("args", SPANS, ids=lambda a: str(a))
def test_span_equals_the_model_and_passes_the_check(args):
    from mixlab_amd import deck
    s, clipped = deck.finegrid_span(*args)
    want, want_clipped = fm.span(*args)
    assert (m_settings(s), clipped) == (want, want_clipped)
    assert fm.check(want, None) is None and want.period0 <= args[0] <= want.period0 + (want.n_periods - 1) * want.dperiod
    assert (args[0] - want.period0) % max(1, want.dperiod) == 0          # the centre is a candidate


def test_span_and_period_say_what_the_header_says():
    # a ten-minute track at 128 BPM and h = 64: 2 % round 375 hops over 64 beats, then four of stage one's steps to either side over all 1 200
    one, clipped = fm.span(375 * Q16, 375 * Q16 // 50, 64, 450000, 64)
    assert (one.dperiod, one.n_periods, clipped) == (512, 1921, False)
    two, clipped = fm.span(375 * Q16, 4 * one.dperiod, 0, 450000, 64)
    assert (two.dperiod, two.n_periods, clipped) == (27, 153, False)
    assert fm.span(20 * Q16, 1 << 40, 0, 1000, 64)[1] and fm.span(PERIOD_MIN, 100, 0, 50, 32)[1]
    from mixlab_amd import deck
    for pc, column, hop in ((46.0, 512, 64), (46.000003, 512, 16), (3.9999999, 64, 64), (1.0 / 3.0, 4096, 16), (100.0 + 2.0 ** -20, 64, 256), (46.87134, 512, 32)):
        assert deck.finegrid_period(pc, column, hop) == fm.period_q16(pc, column, hop)
    assert fm.period_q16(100.0 + 2.0 ** -17, 64, 64) == 100 * Q16 and fm.period_q16(100.0 + 3 * 2.0 ** -17, 64, 64) == 100 * Q16 + 2      # ties to even
    assert deck.finegrid_period(100.0 + 2.0 ** -17, 64, 64) == 100 * Q16 and deck.finegrid_period(100.0 + 3 * 2.0 ** -17, 64, 64) == 100 * Q16 + 2


# ---- sync ----
def test_sync_equals_the_model_on_the_fixed_cases_and_on_random_draws():
    got = [c_sync(*a) for a in fc.SYNC_FIXED]
    assert got == [fm.sync(*a) for a in fc.SYNC_FIXED]
    ONE = 1 << 32
    assert got[1] == (ONE * 3 // 4, 750 * ONE, 750 * ONE)                    # +Pf / 2 stays
    assert got[2] == (ONE * 3 // 4, 1500 * ONE, 750 * ONE)                   # -Pf / 2 folds to +Pf / 2
    assert got[3][2] == -75 * ONE and got[4][2] == 175 * ONE
    assert got[5][0] < 0 and got[6] == (1, 1, 1) and got[7] == (2, 1, 1)                      # 2 / 3 -> 1; 3 / 2 -> 2 (ties to even), b = 1 = Pf / 2 stays
    assert got[-2] is None and got[-1] is None
    draws = fc.sync_draws(300)
    want = [fm.sync(*a) for a in draws]
    assert [c_sync(*a) for a in draws] == want
    live = [(a, w) for a, w in zip(draws, want) if w is not None]
    assert len(live) > 200 and any(a[2] < 0 for a, _w in live) and any(a[1] < a[0].first for a, _w in live) and any(a[4] < a[3].first for a, _w in live)
    for (l, lpos, lstep, f, fpos), (step, seek, delta) in live:
        # what the three numbers mean, in Python's big integers: the follower stands at the leader's fraction of a beat (to the rounding), by the shortest way
        assert -f.period < 2 * delta <= f.period and seek == fpos + delta
        target = Fraction(((lpos - l.first) % l.period) * f.period, l.period)          # the leader's fraction of a beat, in the follower's frames, exactly
        off = (Fraction((seek - f.first) % f.period) - target) % f.period
        assert min(off, f.period - off) <= Fraction(1, 2)
        assert abs(Fraction(abs(step)) - Fraction(abs(lstep) * f.period, l.period)) <= Fraction(1, 2) and (step < 0) == (lstep < 0 and step != 0)
    # the bounds of the header
    b = fm.Beats(0, 1 << 32)
    for args in ((fm.Beats(0, (1 << 56) + 1), 0, 1, b, 0), (b, (1 << 62) + 1, 1, b, 0), (b, 0, 1, fm.Beats(-(1 << 62) - 1, 1 << 32), 0), (b, 0, 1, fm.Beats(0, -5), 0)):
        assert c_sync(*args) is None and fm.sync(*args) is None
    assert c_sync(fm.Beats(0, 1 << 56), 1 << 62, -(4 << 32), fm.Beats(-(1 << 62), 1 << 56), -(1 << 62)) == fm.sync(fm.Beats(0, 1 << 56), 1 << 62, -(4 << 32),
                                                                                                                  fm.Beats(-(1 << 62), 1 << 56), -(1 << 62)) is not None


# ---- the shared cases tell the header from its misreadings ----
@pytest.mark.parametrize("mis", fm.MISREADINGS)
def test_every_misreading_changes_a_compared_value_of_some_case(mis):
    """a model that misreads the header one way differs from what the LIBRARY computes on some case: the library is the compared value"""
    from mixlab_amd import deck
    if mis in ("delta_not_folded", "step_truncated"):
        hit = [k for k, a in enumerate(fc.SYNC_FIXED) if fm.sync(*a, mis=(mis,)) != c_sync(*a)]
    elif mis == "pick_last_index":
        hit = [c.name for c in fc.CASES
               if fm.pick(fc.truth(c)[0], c.settings, fc.RATE, mis=(mis,)) != m_pick(deck.finegrid_pick(np.array(fc.truth(c)[0], _comb_dtype()), c_settings(c.settings), fc.RATE))]
    else:
        hit = []
        for c in fc.CASES:
            recs, w = fm.analyse(fc.track(c), c.settings, mis=(mis,))
            got, got_w = deck.finegrid_host(fc.track(c), c_settings(c.settings), onsets=True)
            if recs != tuples(got) or not np.array_equal(w, got_w):
                hit.append(c.name)
    assert hit, mis


# ---- the property that makes the feature worth having ----
@pytest.mark.parametrize("clicks,case", fc.CLICK_CASES, ids=lambda v: getattr(v, "name", None))
def test_the_picked_grid_sits_on_every_burst_to_the_last(clicks, case):
    """a click track with a non-integer period, a coarse estimate 0.4 % off, one stage of +-2 %: every burst's hop is within 1 of a tooth, and the last grid line within
    a tooth of the last beat -- the tooth's half-width of one hop plus one hop of quantisation, not tuned"""
    from mixlab_amd import deck
    assert abs(case.settings.period0 + (case.settings.n_periods // 2) * case.settings.dperiod - clicks.period / clicks.hop * Q16) > 0.003 * clicks.period / clicks.hop * Q16
    picks = {"model": fm.pick(fc.truth(case)[0], case.settings, fc.RATE), "host": m_pick(deck.finegrid_pick(deck.finegrid_host(fc.track(case), c_settings(case.settings)),
                                                                                                         c_settings(case.settings), fc.RATE))}
    assert picks["model"] == picks["host"]
    for who, p in picks.items():
        worst, drift = fc.grid_misses(clicks, *p.grid)
        print(f"{who}: {clicks}: period {p.grid.period / 2.0 ** 32:.4f} frames, largest miss {worst} hops, drift of the last beat {drift / clicks.hop:.3f} hops")
        assert worst <= 1, (who, worst)
        assert drift <= 2 * clicks.hop, (who, drift)
        assert abs(p.bpm - 60.0 * fc.RATE / clicks.period) < 60.0 * fc.RATE / clicks.period * 2e-3


@pytest.mark.parametrize("clicks,case", fc.CLICK_CASES, ids=lambda v: getattr(v, "name", None))
def test_the_same_through_both_stages_on_host_functions_only(clicks, case):
    """Deck.refine_grid's rule restated on mx_deck_finegrid_period / _span / _host / _pick: equal to the model's two stages, and the same two bounds"""
    from mixlab_amd import deck
    tr = fc.track(case)
    N = deck.finegrid_count(len(tr), clicks.hop)
    centre = deck.finegrid_period(fc.coarse_columns(clicks), fc.COLUMN, clicks.hop)
    one, _ = deck.finegrid_span(centre, (centre + 49) // 50, 64, N, clicks.hop)
    first = deck.finegrid_pick(deck.finegrid_host(tr, one), one, fc.RATE)
    two, _ = deck.finegrid_span(one.period0_q16 + first.index * one.dperiod_q16, 4 * one.dperiod_q16, 0, N, clicks.hop)
    last = m_pick(deck.finegrid_pick(deck.finegrid_host(tr, two), two, fc.RATE))
    want, m_one, m_two = fm.refine(tr, fc.coarse_columns(clicks), fc.COLUMN, fc.RATE, clicks.hop)
    assert (m_settings(one), m_settings(two), last) == (m_one, m_two, want)
    assert fm.refine(tr, fc.coarse_columns(clicks), fc.COLUMN, fc.RATE, clicks.hop, analyse_fn=lambda s: host_records(tr, s))[0] == want
    worst, drift = fc.grid_misses(clicks, *last.grid)
    print(f"{clicks}: two stages: period {last.grid.period / 2.0 ** 32:.4f} frames, largest miss {worst} hops, drift of the last beat {drift / clicks.hop:.3f} hops")
    assert worst <= 1 and drift <= 2 * clicks.hop


# ---- two decks in time ----
def test_two_synced_decks_play_their_bursts_together_to_the_end_of_the_run():
    from mixlab_amd import deck
    pair = fc.sync_pair()
    lead, follow = pair["leader"][0], pair["follower"][0]
    step, seek, delta = pair["sync"]
    assert (step, seek, delta) == deck.deck_sync(c_beats(lead.grid), fc.SYNC_LEADER_POS, dm.ONE, c_beats(follow.grid), fc.SYNC_FOLLOWER_POS)
    tables = np.stack([deck.deck_tables(b) for b in range(4)])
    outs = []
    for c, pos, st in ((fc.SYNC_LEADER, fc.SYNC_LEADER_POS, dm.ONE), (fc.SYNC_FOLLOWER, seek, step)):
        m = dm.DeckModel(fc.track(fc.BY_NAME[f"click track {c.period} / {c.t0} / h {c.hop}"]), tables)
        m.schedule(0, dm.Params(st, flags=dm.PLAY), pos)
        outs.append(m.feed(fc.SYNC_TICKS, fc.SYNC_SPT)[0])
    a, b = (fc.burst_centroids(o) for o in outs)
    # The bound, in output frames.  A burst's first frame f lies in a hop within 1 of its tooth's, so f - (the tooth's centre) is in [-1.5 h, 1.5 h); the grid line
    # first + k * period lies at or less than one hop after that centre (floor(k P) against k P), so f - line is in (-2.5 h, 1.5 h).  The centroid of a burst of 12
    # frames lies less than 12 frames after f, and the interpolator's 32 taps move it by at most 16 track frames either way.  A track frame is 1 / step output frames,
    # and sync puts the two lines of a beat on the same output frame to within a rounding of 2^-32.  So the two centroids differ by at most
    #     (2.5 h_l + 12 + 16) / step_l + (2.5 h_f + 12 + 16) / step_f  (+ 1 for the roundings)
    # and since the first property holds for EVERY beat of the track, the last pair of the run is held to it like the first: that is what the period's precision buys.
    bound = (2.5 * fc.SYNC_LEADER.hop + 28) / 1.0 + (2.5 * fc.SYNC_FOLLOWER.hop + 28) / (step / 2.0 ** 32) + 1.0
    n_out = fc.SYNC_SPT * fc.SYNC_TICKS
    assert len(a) >= 20 and len(b) >= 20 and a[-1] > n_out - 2200 and b[-1] > n_out - 2200        # both play bursts to the end of the run
    gaps = [min(abs(x - y) for y in b) for x in a]
    print(f"bound {bound:.1f} output frames; centroid gaps: first {gaps[0]:.1f}, last {gaps[-1]:.1f}, largest {max(gaps):.1f}")
    assert abs(len(a) - len(b)) <= 1 and max(gaps) <= bound, (gaps, bound)
    assert bound < 0.004 * fc.RATE                                                                # "a few milliseconds"
    # ... and without the sync the same two decks are a flam from the first beat on
    free = dm.DeckModel(fc.track(fc.BY_NAME[f"click track {fc.SYNC_FOLLOWER.period} / {fc.SYNC_FOLLOWER.t0} / h {fc.SYNC_FOLLOWER.hop}"]), tables)
    free.schedule(0, dm.Params(dm.ONE, flags=dm.PLAY), fc.SYNC_FOLLOWER_POS)
    c = fc.burst_centroids(free.feed(fc.SYNC_TICKS, fc.SYNC_SPT)[0])
    assert max(min(abs(x - y) for y in c) for x in a) > bound
