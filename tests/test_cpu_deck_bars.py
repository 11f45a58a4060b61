"""The deck's bars and phrases without a device (include/mixlab_gpu.h "BARS"): the header's structs and entry points, the setting rules at both
edges of each, mx_deck_bars_host / _count / _tables against the model (tests/deck_bars_model.py) on every shared case (tests/deck_bars_cases.py) byte for byte,
mx_deck_bars_pick and mx_deck_grid_next against Python integers on random draws, that the model finds the constructed bar and phrase phase of every section track,
that the named cases tell the text from each of a list of misreadings (and why one misreading cannot be told), the end-to-end chain of the four models on a section
track, bar-aligned sync of two such tracks through the deck model, and the pure host functions under the host's sanitizers in a program of their own."""
import ctypes as C
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import deck_analysis_model as am
import deck_bars_cases as bc
import deck_bars_model as bm
import deck_finegrid_model as fm
import deck_model as dm
from deck_bars_model import Settings

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_bars_check", "mx_deck_bars_count", "mx_deck_bars_tables", "mx_deck_analyse_bars", "mx_deck_read_bars", "mx_deck_read_bar_folds", "mx_deck_bars_host",
                "mx_deck_bars_pick", "mx_deck_grid_next", "mx_deck_debug_last_bars"}
STRUCTS = {"mx_deck_bars": (552, {"grid": 0, "lead": 16, "taps": 20, "beats_per_bar": 24, "bars_per_phrase": 28, "w_bar": 32, "w_phrase": 36, "max_beats": 40, "lo": 44,
                                  "hi": 298}),
           "mx_deck_beat": (48, {"v": 0, "first_frame": 24, "frames": 28, "n_bar": 32, "n_phrase": 40}),
           "mx_deck_bar_pick": (72, {"bars": 0, "phrases": 16, "bar_phase": 32, "phrase_phase": 36, "bar_best": 40, "bar_sum": 48, "phrase_best": 56, "phrase_sum": 64})}


def dk():
    from mixlab_amd import deck
    return deck


# how mx_last_error words each rule the model names: the whole phrase, so that no other message can pass for it
RULE_PHRASES = {"period_q32": ("deck bars: grid.period_q32 outside 2048 .. 131072 frames",), "first_q32": ("deck bars: grid.first_q32 beyond 2^62 in magnitude",),
                "lead": ("deck bars: lead above 4096",), "taps": ("deck bars: taps is not odd in 1 .. 127",), "beats_per_bar": ("deck bars: beats_per_bar outside 2 .. 8",),
                "bars_per_phrase": ("deck bars: bars_per_phrase outside 1 .. 16",), "w_bar": ("deck bars: w_bar outside 1 .. 64",),
                "w_phrase": ("deck bars: w_phrase outside 1 .. 64",),
                "lo": ("deck bars: lo has a non-zero entry at index taps or above", "deck bars: the sum of |lo[k]| is above 32767"),
                "hi": ("deck bars: hi has a non-zero entry at index taps or above", "deck bars: the sum of |hi[k]| is above 32767"),
                "n_frames": ("deck bars: n_frames outside 1 .. 2^30",), "no whole beat": ("deck bars: the grid places no whole beat in the track",),
                "16384": ("deck bars: more than 16384 beats (set max_beats)",)}


def names_rule(err, rule) -> bool:
    return any(str(err).endswith(phrase) for phrase in RULE_PHRASES[rule])


def host(case_or_track, s: Settings):
    tr = bc.track(case_or_track) if isinstance(case_or_track, bc.Case) else case_or_track
    return dk().bars_host(tr, bc.c_settings(s))


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    for name, (size, offs) in STRUCTS.items():
        assert lay[name] == {"size": size, "offsets": offs}, name
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # additions only
    assert (consts["MX_DECK_BARS_MAX_BEATS"], consts["MX_DECK_BARS_MAX_FOLDS"], consts["MX_DECK_BARS_BLOCK"]) == (bm.MAX_BEATS, bm.MAX_FOLDS, bm.BLOCK)
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_bars_check") == ["const mx_deck_bars*", "uint64_t"]
    assert sig("mx_deck_bars_count") == ["const mx_deck_bars*", "uint64_t", "uint32_t*", "int64_t*"]
    assert sig("mx_deck_bars_tables") == ["const mx_deck_analysis*", "mx_deck_bars*"]
    assert sig("mx_deck_analyse_bars") == ["mx_deck*", "const mx_deck_bars*"]
    assert sig("mx_deck_read_bars") == ["mx_deck*", "uint64_t", "uint64_t", "mx_deck_beat*"]
    assert sig("mx_deck_read_bar_folds") == ["mx_deck*", "uint64_t*", "uint32_t"]
    assert sig("mx_deck_bars_host") == ["const int16_t*", "uint64_t", "const mx_deck_bars*", "mx_deck_beat*", "uint64_t*"]
    assert sig("mx_deck_bars_pick") == ["const uint64_t*", "const mx_deck_bars*", "mx_deck_bar_pick*"]
    assert sig("mx_deck_grid_next") == ["const mx_deck_beats*", "int64_t", "int64_t*", "int64_t*"]
    assert re.search(r"int mx_deck_debug_last_bars\(uint32_t out\[4\]\);", text)
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | set(STRUCTS)):
        assert re.search(rf"\b{name}\b", note), name
    # the new section stands below FINE GRID, whose own declarations are as they were, and the two "out of scope" remarks point at it
    assert text.index("---- FINE GRID:") < text.index("int mx_deck_debug_last_finegrid(uint32_t out[4]);") < text.index("---- BARS:") < text.index("pixel path:")
    assert "downbeat / bar detection (BARS below has it)" in text and "downbeats and bars (BARS below)" in text
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}


def test_ctypes_mirrors_have_the_headers_layout():
    from mixlab_amd import abi
    for st, name in ((abi.DeckBars, "mx_deck_bars"), (abi.DeckBeat, "mx_deck_beat"), (abi.DeckBarPick, "mx_deck_bar_pick")):
        size, offs = STRUCTS[name]
        assert C.sizeof(st) == size and {n: getattr(st, n).offset for n, _t in st._fields_} == offs, name
    assert abi.DECK_BEAT_DTYPE == bm.BEAT_DTYPE and abi.DECK_BEAT_DTYPE.itemsize == 48
    assert [abi.DECK_BEAT_DTYPE.fields[n][1] for n in ("v", "first_frame", "frames", "n_bar", "n_phrase")] == [0, 24, 28, 32, 40]
    assert (abi.DECK_BARS_MAX_BEATS, abi.DECK_BARS_MAX_FOLDS, abi.DECK_BARS_BLOCK) == (bm.MAX_BEATS, bm.MAX_FOLDS, bm.BLOCK)


# ---- the setting rules, accepted at the bound and refused one past it (a track of 100 000 frames) ----
BASE = Settings(300 << 32, 2400 << 32, *bc.T63)
N_BASE = 100000
HALF = tuple([16383] + [0] * 61 + [16384])      # sum |c| = 32767
CHECKS = [({}, True),
          ({"period": bm.PERIOD_MIN}, True), ({"period": bm.PERIOD_MIN - 1}, False), ({"period": 98000 << 32}, True), ({"period": bm.PERIOD_MAX + 1}, False),
          ({"period": bm.PERIOD_MAX, "first": 0, "lead": 0}, False),                                 # within the period rule, but no whole beat in 100 000 frames
          ({"first": bm.FAR}, True), ({"first": bm.FAR + 1}, False), ({"first": -bm.FAR}, True), ({"first": -bm.FAR - 1}, False),
          ({"lead": 0}, True), ({"lead": 4096}, True), ({"lead": 4097}, False),
          ({"lo": (16384,), "hi": (16384,)}, True), ({"lo": bc.T127[0], "hi": bc.T127[1]}, True), ({"taps": 62}, False), ({"taps": 0}, False), ({"taps": 129}, False),
          ({"M": 2}, True), ({"M": 8}, True), ({"M": 1}, False), ({"M": 9}, False),
          ({"Q": 1}, True), ({"Q": 16}, True), ({"Q": 0}, False), ({"Q": 17}, False),
          ({"w_bar": 1}, True), ({"w_bar": 64}, True), ({"w_bar": 0}, False), ({"w_bar": 65}, False),
          ({"w_phrase": 1}, True), ({"w_phrase": 64}, True), ({"w_phrase": 0}, False), ({"w_phrase": 65}, False),
          ({"lo": HALF}, True), ({"lo": HALF[:-1] + (16385,)}, False), ({"hi": HALF[:-1] + (-16385,)}, False),
          ({"tail": ((0, 1), ())}, False), ({"tail": ((), (0,) * 63 + (-1,))}, False), ({"taps": 61}, False),       # (taps 61: lo[61], lo[62] are not zero)
          ({"max_beats": 0}, True), ({"max_beats": 1}, True), ({"max_beats": 0xFFFFFFFF}, True),
          ({"first": 97727 << 32}, True), ({"first": 97729 << 32, "period": 98000 << 32}, False)]                   # the one beat that fits; none does


@pytest.mark.parametrize("change,ok", CHECKS, ids=lambda v: str(v)[:60])
def test_check_rules_at_their_bounds(change, ok):
    from mixlab_amd import abi
    s = BASE._replace(**change)
    rule = bm.check(s, N_BASE)
    assert (rule is None) == ok, rule
    if ok:
        dk().bars_check(bc.c_settings(s), N_BASE)
        assert dk().bars_count(bc.c_settings(s), N_BASE) == bm.beats(s, N_BASE)[::-1]
    else:
        with pytest.raises(abi.MxError) as err:
            dk().bars_check(bc.c_settings(s), N_BASE)
        assert err.value.code == abi.MX_ERR_INVALID
        assert names_rule(err.value, rule), (rule, err.value)   # mx_last_error names the broken rule
        with pytest.raises(abi.MxError):
            dk().bars_count(bc.c_settings(s), N_BASE)


def test_the_track_rules_count_tables_and_the_other_refusals():
    from mixlab_amd import abi, deck
    ok = bc.c_settings(BASE)
    # n_frames, and the two rules about the beats a grid places: 16 384 beats pass, one more does not unless max_beats cuts it
    long_track = 300 - 128 + 2400 * 16384
    for n_frames, max_beats, rule in ((0, 0, "n_frames"), ((1 << 30) + 1, 0, "n_frames"), (2571, 0, "no whole beat"), (2572, 0, None), (long_track, 0, None),
                                      (long_track + 2400, 0, "16384"), (long_track + 2400, 16384, None), (1 << 30, 16384, None), (1 << 30, 16385, "16384")):
        s = BASE._replace(max_beats=max_beats)
        assert bm.check(s, n_frames) == rule
        if rule is None:
            deck.bars_check(bc.c_settings(s), n_frames)
            assert deck.bars_count(bc.c_settings(s), n_frames) == bm.beats(s, n_frames)[::-1]
        else:
            with pytest.raises(abi.MxError) as err:
                deck.bars_check(bc.c_settings(s), n_frames)
            assert err.value.code == abi.MX_ERR_INVALID and names_rule(err.value, rule), (rule, err.value)
    assert deck.bars_count(ok, 2572) == (1, 0) and deck.bars_count(ok, long_track) == (16384, 0)
    # tables: taken over from analysis settings, which must pass their own check; everything else in the settings stays
    a = deck.analysis_bands(rate=bc.RATE, taps=63)
    s = deck.bars(abi.DeckBeats(BASE.first, BASE.period), a, lead=77, beats_per_bar=3, bars_per_phrase=5, w_bar=6, w_phrase=7, max_beats=9)
    assert (tuple(s.lo[:63]), tuple(s.hi[:63]), s.taps) == (bc.T63[0], bc.T63[1], 63) and not any(s.lo[63:]) and not any(s.hi[63:])
    assert (s.lead, s.beats_per_bar, s.bars_per_phrase, s.w_bar, s.w_phrase, s.max_beats, s.grid.first_q32, s.grid.period_q32) == (77, 3, 5, 6, 7, 9, BASE.first, BASE.period)
    plain = deck.bars(abi.DeckBeats(BASE.first, BASE.period))
    assert (plain.taps, plain.lo[0], plain.hi[0], plain.beats_per_bar, plain.bars_per_phrase, plain.w_bar, plain.w_phrase, plain.lead) == (1, 16384, 16384, 4, 4, 4, 8, 128)
    a.taps = 62
    before = bytes(s)
    assert abi.lib.mx_deck_bars_tables(C.byref(a), C.byref(s)) == abi.MX_ERR_INVALID and bytes(s) == before
    # NULL pointers
    x = np.zeros((N_BASE, 2), np.int16)
    rec = np.zeros(64, abi.DECK_BEAT_DTYPE)
    H = np.zeros(20, np.uint64)
    p = lambda arr: arr.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert abi.lib.mx_deck_bars_check(None, N_BASE) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_bars_count(None, N_BASE, None, None) == abi.MX_ERR_INVALID and abi.lib.mx_deck_bars_count(C.byref(ok), N_BASE, None, None) == abi.MX_OK
    assert abi.lib.mx_deck_bars_tables(None, C.byref(s)) == abi.MX_ERR_INVALID and abi.lib.mx_deck_bars_tables(C.byref(a), None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_bars_host(None, N_BASE, C.byref(ok), p(rec), p(H)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_bars_host(p(x), N_BASE, None, p(rec), p(H)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_bars_host(p(x), N_BASE, C.byref(ok), None, p(H)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_bars_host(p(x), N_BASE, C.byref(ok), p(rec), None) == abi.MX_OK
    assert abi.lib.mx_deck_bars_pick(None, C.byref(ok), C.byref(abi.DeckBarPick())) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_bars_pick(p(H), None, C.byref(abi.DeckBarPick())) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_bars_pick(p(H), C.byref(ok), None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_grid_next(None, 0, None, None) == abi.MX_ERR_INVALID and abi.lib.mx_deck_grid_next(C.byref(abi.DeckBeats(0, 5)), 0, None, None) == abi.MX_OK
    assert abi.lib.mx_deck_debug_last_bars(None) == abi.MX_ERR_INVALID
    # the pick holds every rule that needs no track, and no other
    for change, passes in (({"M": 9}, False), ({"w_bar": 0}, False), ({"period": 5}, False), ({"first": 1 << 61, "max_beats": 7}, True)):
        call = lambda: deck.bars_pick(np.zeros(20, np.uint64), bc.c_settings(BASE._replace(**change)))   # noqa: E731
        if passes:
            assert call().bar_sum == 0
        else:
            with pytest.raises(abi.MxError) as err:
                call()
            assert err.value.code == abi.MX_ERR_INVALID


# ---- the rules against the model on every shared case ----
@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name[:60])
def test_host_records_folds_count_and_pick_equal_the_model(case):
    from mixlab_amd import deck
    want, want_H, n0 = bc.truth(case)
    tr = bc.track(case)
    assert len(tr) <= 400000 and bm.check(case.settings, len(tr)) is None
    recs, H = host(case, case.settings)
    assert recs.tobytes() == want.tobytes(), [k for k in range(len(want)) if recs[k] != want[k]][:4]
    assert H.dtype == np.uint64 and [int(v) for v in H] == list(want_H)
    assert deck.bars_count(bc.c_settings(case.settings), len(tr)) == (len(want), n0)
    assert bc.m_pick(deck.bars_pick(H, bc.c_settings(case.settings))) == bm.pick(want_H, case.settings)
    assert int(min(want["n_bar"].min(), want["n_phrase"].min())) >= 0      # never negative: the model's docstring


def test_the_cases_hold_what_their_names_say():
    t = {c.name: bc.truth(c) for c in bc.CASES}
    f = {c.name: bc.forms(c) for c in bc.CASES}
    lens = {c.name: [int(v) for v in t[c.name][0]["frames"]] for c in bc.CASES}
    name = "period exactly 2048: every half one tile"
    assert set(lens[name]) == {2048} and f[name]["wgs_half_tiled"] == 0
    name = "period 2049.37: every half a tile and a frame or two"
    assert set(lens[name]) == {2049, 2050} and f[name]["wgs_half_one_tile"] > 0 and f[name]["wgs_half_tiled"] > 0      # 1024 + 1025, and 1025 + 1025
    assert set(lens["period 5000.7: several tiles a half, odd beats"]) == {5000, 5001}
    k127 = next(c for c in bc.CASES if c.name.startswith("K = 127"))
    recs = t[k127.name][0]
    assert k127.settings.K == 127 and recs["first_frame"][0] == 0 and int(recs["first_frame"][-1]) + int(recs["frames"][-1]) == len(bc.track(k127))
    short = bc.BY_NAME["the last beat one frame short of n_frames' reach"]
    assert len(t[short.name][0]) == len(recs) - 1 and len(bc.track(short)) == len(bc.track(k127)) - 1
    assert {bc.BY_NAME[n].settings.lead for n in (k127.name, "lead 4096")} == {0, 4096}
    assert t["a negative first_q32"][2] > 0 and t["first_q32 several periods into the track: n0 < 0"][2] < -3
    assert t["first_q32 several periods into the track: n0 < 0"][2] % 4 != 0                                               # ... so that folding by the grid's index differs
    cut = bc.BY_NAME["max_beats cutting the track"]
    assert len(t[cut.name][0]) == 13 < bm.beats(cut.settings._replace(max_beats=0), len(bc.track(cut)))[1]
    assert {len(r[0]) % bm.BLOCK for r in t.values()} == {0, 1, 2, 3}                                                       # full and part-full novelty blocks
    w = bc.BY_NAME["W = 1 and W = 64 over 141 beats"]
    recs = t[w.name][0]
    assert (w.settings.w_bar, w.settings.w_phrase) == (1, 64) and np.count_nonzero(recs["n_phrase"]) == 141 - 128 + 1 and recs["n_phrase"][64] and recs["n_phrase"][77]
    assert recs["n_bar"][0] == 0 and np.count_nonzero(recs["n_bar"][1:]) == 140
    none = "2 W above n_beats: every N is 0 and the pick all zero"
    assert not t[none][0]["n_bar"].any() and not t[none][0]["n_phrase"].any() and not any(t[none][1]) and bm.pick(t[none][1], bc.BY_NAME[none].settings) == bm.Pick()
    assert t[none][0]["v"].any() and f[none]["novelties_defined"] == 0
    assert (bc.BY_NAME["M = 3, Q = 1"].settings.M, bc.BY_NAME["M = 3, Q = 1"].settings.Q, len(t["M = 3, Q = 1"][1])) == (3, 1, 6)
    assert len(t["M = 8, Q = 16"][1]) == bm.MAX_FOLDS and sum(1 for v in t["M = 8, Q = 16"][1][8:] if v) > 64
    v = t["a constant track"][0]["v"]
    assert (v[1:-1, [1, 2, 4, 5]] == 0).all() and (v[:, [0, 3]] > 0).all()          # DC passes the low band at gain 1: mid = high = 0 away from the track's ends
    assert t["a noise track"][0]["v"].min() > 0
    name = "the best phrase phase of all lies off the bar phase"
    Hp = t[name][1][4:]
    assert Hp.index(max(Hp)) % 4 != bm.pick(t[name][1], bc.BY_NAME[name].settings).bar_phase
    total = {}
    for c in bc.CASES:
        for k, n in f[c.name].items():
            total[k] = total.get(k, 0) + n
    assert all(n > 0 for n in total.values()), total


# ---- pick and next line against Python integers ----
def test_pick_equals_python_integers_on_random_draws_ties_included():
    from mixlab_amd import deck
    draws = bc.pick_draws(300)
    got = [bc.m_pick(deck.bars_pick(np.array(H, np.uint64), bc.c_settings(s))) for H, s in draws]
    want = [bm.pick(H, s) for H, s in draws]
    assert got == want
    live = [(H, s, w) for (H, s), w in zip(draws, want) if w.bar_sum]
    assert len(live) > 200 and any(w == bm.Pick() and any(H) for (H, _s), w in zip(draws, want))     # H_bar all zero, H_phrase not: everything is zero
    assert sum(1 for H, s, w in live if H[:s.M].count(w.bar_best) > 1) > 20                          # ties of the bar fold ...
    assert sum(1 for H, s, w in live if [H[s.M + m] for m in range(w.bar_phase, s.M * s.Q, s.M)].count(w.phrase_best) > 1) > 20     # ... and of the phrase fold
    assert any(w.phrase_best < max(H[s.M:]) for H, s, w in live)                                     # a better phrase phase off the bar phase, not taken
    for H, s, w in live:
        n0 = bm.first_index(s)
        assert bm.line(s, n0) >= 0 > bm.line(s, n0 - 1)
        assert (w.bars.first - s.first) % s.period == 0 and (w.phrases.first - w.bars.first) % w.bars.period == 0 and w.phrases.period == s.Q * w.bars.period
        assert w.bar_phase == min(m for m in range(s.M) if H[m] == max(H[:s.M])) and w.phrase_phase % s.M == w.bar_phase


def test_grid_next_equals_python_integers_on_random_draws_and_at_the_range_edges():
    from mixlab_amd import abi, deck
    draws = bc.next_draws(400)

    def c_next(g, pos):
        try:
            return deck.grid_next(abi.DeckBeats(g.first, g.period), pos)
        except abi.MxError as e:
            assert e.code == abi.MX_ERR_INVALID
            return None

    got, want = [c_next(*a) for a in draws], [bm.grid_next(*a) for a in draws]
    assert got == want
    assert want[0] is None and want[1] == (1 << 62, 1 << 62) and want[2] == (-128, -(1 << 62)) and want[3] == (0, 1 << 62) and all(w is None for w in want[4:9])
    assert want[9:15] == [(-1, -5), (0, 5), (1, 15), (-1, -5), (-2, -15), (-2, -15)]
    live = [(g, pos, w) for (g, pos), w in zip(draws, want) if w is not None]
    assert len(live) > 300 and any(w[0] < 0 for _g, _p, w in live) and any(w[1] == pos for _g, pos, w in live)
    for g, pos, (n, ln) in live:
        assert ln == g.first + n * g.period and pos <= ln < pos + g.period


# ---- the rule finds what was constructed ----
@pytest.mark.parametrize("sec,case", bc.SECTION_CASES, ids=lambda v: getattr(v, "name", None))
def test_the_model_finds_the_constructed_bar_and_phrase_phase(sec, case):
    recs, H, n0 = bc.truth(case)
    p = bm.pick(H, case.settings)
    Hb = sorted(H[:4])
    print(f"{sec.name}: n0 {n0}, {len(recs)} beats, bar phase {p.bar_phase}, phrase phase {p.phrase_phase}, winner / runner-up {Hb[-1] / Hb[-2]:.2f}")
    assert (p.bar_phase, p.phrase_phase) == bc.section_truth(sec, n0)
    # ... which puts the `bars` grid on the constructed downbeats, to the frame the grid itself was given with
    first_down = sec.first + sec.pickup * sec.period
    assert abs(((p.bars.first / 2.0 ** 32 - first_down) + 2 * sec.period) % (4 * sec.period) - 2 * sec.period) < 1.0
    assert abs(((p.phrases.first / 2.0 ** 32 - first_down) + 8 * sec.period) % (16 * sec.period) - 8 * sec.period) < 1.0


# ---- the shared cases tell the header from its misreadings ----
@pytest.mark.parametrize("mis", bm.MISREADINGS)
def test_every_misreading_changes_a_compared_value_of_the_case_named_for_it(mis):
    """a model that misreads the header one way differs from what the LIBRARY computes on the case named for it: the library is the compared value"""
    from mixlab_amd import deck
    case = bc.BY_NAME[bc.MISREADING_CASE[mis]]
    recs, H = host(case, case.settings)
    if mis == "phrase_free_of_bar":
        assert bm.pick([int(v) for v in H], case.settings, mis=(mis,)) != bc.m_pick(deck.bars_pick(H, bc.c_settings(case.settings)))
    else:
        m_recs, m_H, _n0 = bm.analyse(bc.track(case), case.settings, mis=(mis,))
        assert m_recs.tobytes() != recs.tobytes() or list(m_H) != [int(v) for v in H]
        if mis == "fold_by_grid_index":
            assert m_recs.tobytes() == recs.tobytes()        # (the folds alone)


def test_the_clamp_after_the_fold_cannot_be_told_because_no_novelty_is_negative():
    assert set(bm.MISREADINGS) == set(bc.MISREADING_CASE) and len(bm.MISREADINGS) >= 8 and bm.NOT_SHOWABLE == ("clamp_after_fold",)
    for case in bc.CASES[:6]:
        assert tuple(bm.analyse(bc.track(case), case.settings, mis=bm.NOT_SHOWABLE)[1]) == bc.truth(case)[1]
    # random vectors, wild ones included: the novelty of the model's own d matrix is never negative
    rng = np.random.default_rng(21)
    for W, top in ((1, 5), (2, 1 << 27), (3, 3), (7, 1 << 27), (64, 1 << 27), (64, 2)):
        v = rng.integers(0, top, (2 * W + 9, 6)).astype(np.int64)
        d = np.abs(v[:, None, :] - v[None, :, :]).sum(axis=2)
        N = bm.novelty(np.pad(d, ((0, 1), (0, 1))), len(v), W)
        assert min(N) >= 0 and max(N) < 1 << 44 and N[W - 1] == 0 and N[len(v) - W + 1:] == [0] * (W - 1)


# ---- end to end on the models: analyse -> beat grid -> fine grid -> bars ----
def test_the_composed_models_put_the_downbeats_within_two_fine_hops_of_the_constructed_ones():
    e = bc.end_to_end()
    sec, p, n0 = bc.END_TO_END, e["pick"], e["n0"]
    print(f"coarse {e['coarse'].bpm:.3f} BPM, fine period {e['fine'].grid.period / 2.0 ** 32:.3f} frames (true {sec.period}), first {e['fine'].grid.first / 2.0 ** 32:.1f}, "
          f"n0 {n0}, bar phase {p.bar_phase}, phrase phase {p.phrase_phase}, H_bar {e['folds'][:4]}")
    assert p.bar_sum > 0
    misses = bc.downbeat_misses(sec, p.bars)
    print(f"downbeat misses in frames: first {misses[0]:.1f}, last {misses[-1]:.1f}, largest {max(misses):.1f}; bound {2 * bc.E2E_HOP}")
    assert max(misses) <= 2 * bc.E2E_HOP
    # the phrase lines are downbeats of the constructed sections
    first_phrase = sec.first + sec.pickup * sec.period
    off = ((p.phrases.first / 2.0 ** 32 - first_phrase) + 8 * sec.period) % (16 * sec.period) - 8 * sec.period
    assert abs(off) <= 2 * bc.E2E_HOP, off
    # the same chain on the library's host functions
    from mixlab_amd import abi, deck
    tr = bc.section_track(sec)
    a = deck.analysis_bands(rate=bc.RATE, column=bc.E2E_COLUMN, max_lag=bc.E2E_LAG)
    cols, R = deck.columns_host(tr, a, autocorr=True)
    coarse = deck.beatgrid(cols, R, a.column, bc.RATE, *bc.E2E_BPM)
    N = deck.finegrid_count(len(tr), bc.E2E_HOP)
    centre = deck.finegrid_period(coarse.period_columns, a.column, bc.E2E_HOP)
    one, _ = deck.finegrid_span(centre, (centre + 49) // 50, 64, N, bc.E2E_HOP)
    first = deck.finegrid_pick(deck.finegrid_host(tr, one), one, bc.RATE)
    two, _ = deck.finegrid_span(one.period0_q16 + first.index * one.dperiod_q16, 4 * one.dperiod_q16, 0, N, bc.E2E_HOP)
    fine = deck.finegrid_pick(deck.finegrid_host(tr, two), two, bc.RATE)
    assert (fine.grid.first_q32, fine.grid.period_q32) == tuple(e["fine"].grid)
    s = deck.bars(fine.grid, a)
    recs, H = deck.bars_host(tr, s)
    assert recs.tobytes() == e["records"].tobytes() and bc.m_pick(deck.bars_pick(H, s)) == p
    n, ln = deck.grid_next(p_beats := abi.DeckBeats(*p.phrases), 40000 << 32)
    assert ln == p.phrases.first + n * p.phrases.period and ln - p_beats.period_q32 < (40000 << 32) <= ln


def test_two_tracks_synced_on_their_bars_grids_have_their_downbeats_together():
    """mx_deck_sync on the two `bars` grids puts the follower's "1" on the leader's "1"; on the beat grids alone it leaves the follower's "3" there (the GPU suite
    plays the pair)"""
    from mixlab_amd import abi, deck
    pair = bc.bar_sync_pair()
    step, seek, _delta = pair["sync"]
    lp, fp = pair["leader"]["pick"], pair["follower"]["pick"]
    assert (step, seek) == deck.deck_sync(abi.DeckBeats(*lp.bars), bc.BAR_SYNC_LEADER_POS, dm.ONE, abi.DeckBeats(*fp.bars), bc.BAR_SYNC_FOLLOWER_POS)[:2]
    gaps, bound = bc.bar_sync_gaps(step, seek)
    print(f"{len(gaps)} leader downbeats with a follower bar round them; gaps: first {gaps[0]:.1f}, last {gaps[-1]:.1f}, largest {max(gaps):.1f} output frames; bound {bound:.1f}")
    assert bound == 2 * bc.E2E_HOP and len(gaps) >= 12 and max(gaps) <= bound
    # beat-aligned sync alone is free to put the "1" elsewhere: from these two positions it keeps the follower on the "3" it stood next to
    bstep, bseek, _ = deck.deck_sync(abi.DeckBeats(*pair["leader"]["fine"].grid), bc.BAR_SYNC_LEADER_POS, dm.ONE, abi.DeckBeats(*pair["follower"]["fine"].grid),
                                     bc.BAR_SYNC_FOLLOWER_POS)
    assert min(bc.bar_sync_gaps(bstep, bseek)[0]) > 1.5 * bc.BAR_SYNC_FOLLOWER.period / (bstep / 2.0 ** 32)


# ---- the pure host functions under the host's sanitizers ----
def test_the_host_functions_run_clean_under_the_address_and_undefined_behaviour_sanitizers(tmp_path):
    import deck_bars_check
    try:
        out = deck_bars_check.main(tmp_path)
    except subprocess.CalledProcessError as e:
        pytest.fail(f"the sanitized program failed ({e.returncode}):\n{e.stdout or ''}\n{e.stderr or ''}")
    assert out.rstrip().endswith("deck_bars_check: ok"), out
