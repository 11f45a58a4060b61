"""Key-lock without a device (include/mixlab_gpu.h "KEY-LOCK"): the header's structs and entry points, the setting rules at both edges,
mx_deck_keylock_search against the model on random and constructed tracks, the identities and the independence from feed grouping on the model, that the shared
cases tell the model from each of a list of misreadings, and what the search is for: a tone keeps its pitch at another tempo."""
import ctypes as C
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import deck_cases as dc
import deck_keylock_cases as kc
import deck_keylock_model as km
import deck_model as dm
from deck_keylock_model import Keylock
from deck_model import ONE, PLAY, Params

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_set_keylock", "mx_deck_keylock_check", "mx_deck_keylock_search", "mx_deck_grain_count", "mx_deck_read_grains", "mx_deck_debug_last_keylock"}
KEYLOCK_OFFSETS = {"pitch_q32": 0, "hop": 8, "overlap": 12, "radius": 16, "_pad": 20}
GRAIN_OFFSETS = {"a_q32": 0, "g_q32": 8, "tick": 16, "frame": 20, "delta": 24, "dist": 28, "flags": 32, "_pad": 36}


@pytest.fixture(scope="module")
def tables():
    from mixlab_amd import deck
    return np.stack([deck.deck_tables(b) for b in range(4)])


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    assert lay["mx_deck_keylock"]["size"] == 24 and lay["mx_deck_keylock"]["offsets"] == KEYLOCK_OFFSETS
    assert lay["mx_deck_grain"]["size"] == 40 and lay["mx_deck_grain"]["offsets"] == GRAIN_OFFSETS
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_DECK_GRAIN_FIRST"] == 1
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19   # additions only
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_set_keylock") == ["mx_deck*", "const mx_deck_keylock*"]
    assert sig("mx_deck_keylock_check") == ["const mx_deck_keylock*"]
    assert sig("mx_deck_keylock_search") == ["const int16_t*", "uint64_t", "int64_t", "int64_t", "uint32_t", "uint32_t", "int32_t*", "uint32_t*"]
    assert sig("mx_deck_grain_count") == ["const mx_deck*", "uint32_t*"]
    assert sig("mx_deck_read_grains") == ["mx_deck*", "uint32_t", "uint32_t", "mx_deck_grain*"]
    assert re.search(r"int mx_deck_debug_last_keylock\(uint32_t out\[4\]\);", text)
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | {"mx_deck_keylock", "mx_deck_grain"}):
        assert re.search(rf"\b{name}\b", note), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi
    for st, size, offs in ((abi.DeckKeylock, 24, KEYLOCK_OFFSETS), (abi.DeckGrain, 40, GRAIN_OFFSETS)):
        assert C.sizeof(st) == size and {n: getattr(st, n).offset for n, _t in st._fields_} == offs
    assert abi.DECK_GRAIN_FIRST == km.G_FIRST


# ---- the setting rules, at both edges of each ----
OK_SET = Keylock(ONE, 1024, 256, 512)
CHECKS = [(OK_SET, True),
          (OK_SET._replace(pitch=1 << 30), True), (OK_SET._replace(pitch=(1 << 30) - 1), False), (OK_SET._replace(pitch=4 * ONE), True), (OK_SET._replace(pitch=4 * ONE + 1), False),
          (OK_SET._replace(pitch=0), False), (OK_SET._replace(pitch=-ONE), False),
          (OK_SET._replace(hop=256, overlap=128), True), (OK_SET._replace(hop=128, overlap=64), False), (OK_SET._replace(hop=8192), True), (OK_SET._replace(hop=16384), False),
          (OK_SET._replace(hop=1000), False), (OK_SET._replace(hop=0), False), (OK_SET._replace(hop=1025), False),
          (OK_SET._replace(overlap=16), True), (OK_SET._replace(overlap=8), False), (OK_SET._replace(overlap=512), True), (OK_SET._replace(overlap=1024), False),
          (OK_SET._replace(hop=2048, overlap=1024), True), (OK_SET._replace(hop=8192, overlap=2048), False), (OK_SET._replace(hop=4096, overlap=1024), True),
          (OK_SET._replace(overlap=48), False), (OK_SET._replace(overlap=0), False), (OK_SET._replace(hop=256, overlap=256), False),
          (OK_SET._replace(radius=0), True), (OK_SET._replace(radius=1024), True), (OK_SET._replace(radius=1025), False), (OK_SET._replace(radius=0xFFFFFFFF), False)]


@pytest.mark.parametrize("k,ok", CHECKS)
def test_keylock_check_at_the_boundaries(k, ok):
    from mixlab_amd import abi, deck
    assert (km.check(k) is None) == ok
    c = deck.keylock(*k)
    if ok:
        deck.keylock_check(c)
    else:
        with pytest.raises(abi.MxError) as e:
            deck.keylock_check(c)
        assert e.value.code == abi.MX_ERR_INVALID
    bad_pad = deck.keylock(*OK_SET)
    bad_pad._pad = 1
    with pytest.raises(abi.MxError):
        deck.keylock_check(bad_pad)


def test_deck_check_still_refuses_every_flag_bit_outside_play_and_loop():
    from mixlab_amd import abi, deck
    for bit in range(2, 32):
        with pytest.raises(abi.MxError):
            deck.deck_check(deck.params(flags=1 << bit), 100)


# ---- the search, against the model ----
def lib_search(tr, Cf, Af, V, R):
    from mixlab_amd import deck
    return deck.keylock_search(tr, Cf, Af, V, R)


def test_search_equals_the_model_on_random_tracks():
    rng = np.random.default_rng(11)
    for trial in range(60):
        n = int(rng.choice([1, 2, 15, 100, 700, 3000]))
        tr = kc.track("music" if trial % 2 else "noise", n, f"search {trial}")
        V, R = int(rng.choice([1, 16, 17, 64, 256, 1024])), int(rng.choice([0, 1, 5, 300, 1024]))
        Cf, Af = (int(v) for v in rng.integers(-1200, n + 1200, 2))
        assert lib_search(tr, Cf, Af, V, R) == km.search(km.sums(tr), Cf, Af, V, R), (trial, n, V, R, Cf, Af)


def test_search_on_a_silent_track_stays_where_it_is():
    tr = kc.track("silent", 500)
    assert lib_search(tr, 100, 240, 64, 300) == (0, 0) == km.search(km.sums(tr), 100, 240, 64, 300)


def test_search_tie_between_minus_q_and_plus_q_goes_to_minus_q():
    tr = kc.track("period 16", 2000)
    s = km.sums(tr)
    Cf, Af, V, R = 400, 808, 64, 12
    D = {d: int(np.abs(s[Cf:Cf + V] - s[Af + d:Af + d + V]).sum()) for d in (-8, 0, 8)}
    assert D[-8] == D[8] == 0 < D[0]
    assert lib_search(tr, Cf, Af, V, R) == (-8, 0) == km.search(s, Cf, Af, V, R)
    assert km.search(s, Cf, Af, V, R, mis=("tie_positive",)) == (8, 0)


def test_search_at_extreme_amplitudes_stays_within_32_bits():
    tr = kc.track("extreme", 4000)
    # an odd offset puts every -32768 - 32768 against a 32767 + 32767: 131 070 per frame, 1024 frames
    got = lib_search(tr, 1000, 2001, 1024, 0)
    assert got == (0, 1024 * 131070) and got[1] < 1 << 32
    assert lib_search(tr, 1000, 2001, 1024, 0) == km.search(km.sums(tr), 1000, 2001, 1024, 0)
    assert lib_search(tr, 1000, 2001, 1024, 4) == (-1, 0) == km.search(km.sums(tr), 1000, 2001, 1024, 4)


def test_search_with_c_or_a_outside_the_track_and_a_track_of_one_frame():
    tr = kc.track("noise", 300, "outside")
    s = km.sums(tr)
    for Cf, Af in ((-5000, 100), (100, -5000), (299, 290), (-10, -3), (295, 5000), (1 << 40, -(1 << 40))):
        for V, R in ((16, 5), (1024, 1024)):
            assert lib_search(tr, Cf, Af, V, R) == km.search(s, Cf, Af, V, R), (Cf, Af, V, R)
    one = np.array([[-32768, -32768]], np.int16)
    for Cf, Af, V, R in ((0, 0, 16, 5), (0, 3, 16, 5), (-3, 2, 16, 5), (0, 100, 16, 5), (0, 1024, 1024, 1024)):
        assert lib_search(one, Cf, Af, V, R) == km.search(km.sums(one), Cf, Af, V, R), (Cf, Af, V, R)
    assert lib_search(one, 0, 3, 16, 5) == (-3, 0)


def test_search_refuses_what_the_header_says_it_refuses():
    from mixlab_amd import abi
    lib = abi.lib
    tr = np.zeros(20, np.int16)
    d, D = C.c_int32(), C.c_uint32()
    ptr = tr.ctypes.data_as(C.c_void_p)
    good = (ptr, 10, 0, 0, 16, 5, C.byref(d), C.byref(D))
    assert lib.mx_deck_keylock_search(*good) == 0
    for k, v in ((0, None), (1, 0), (1, (1 << 30) + 1), (2, (1 << 40) + 1), (3, -(1 << 40) - 1), (4, 0), (4, 1025), (5, 1025), (6, None), (7, None)):
        args = list(good)
        args[k] = v
        assert lib.mx_deck_keylock_search(*args) == abi.MX_ERR_INVALID, (k, v)


# ---- what the header says follows ----
@pytest.mark.parametrize("step", (ONE, kc.STEP_441), ids=("unity", "44.1 in 48"))
def test_pitch_equal_to_a_constant_step_gives_the_plain_decks_bits(tables, step):
    tr = kc.track("noise", 4097, "identity")
    for seek in (0, frames_q(300.37)):
        plain, m = dm.DeckModel(tr, tables), km.KeylockModel(tr, tables)
        m.set_keylock(Keylock(step, 256, 128, 300))
        p = Params(step, 0, 0, 0, PLAY)
        plain.schedule(0, p, seek); m.schedule(0, p, seek)
        want, _ = plain.feed(6, 800)
        got, _recs, grains = m.feed(6, 800)
        assert len(grains) == 6 * 800 // 256 + 1 and all(g.delta == 0 and g.dist == 0 for g in grains)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
        if step == ONE and seek == 0:   # ... which at unity from an integer position is the track itself
            track = np.zeros((6 * 800, 2), np.float32)
            track[:4097] = tr.astype(np.float32) / np.float32(32768.0)
            assert np.array_equal(got.view(np.uint32), track.reshape(-1).view(np.uint32))


def frames_q(f):
    return int(round(f * ONE))


@pytest.mark.parametrize("name", ("spt 257, hop 256", "seek mid-feed", "pause between playing ticks", "spt 800, hop 256, more candidates than lanes"))
def test_the_result_does_not_depend_on_how_ticks_are_grouped_into_feeds(tables, name):
    case = kc.BY_NAME[name]
    total = sum(f.n_ticks for f in case.feeds)
    ref = kc.run_model(case, tables)
    ref_s = np.concatenate([r[0] for r in ref])
    ref_g = [(total_tick(ref, i, g), g.frame, g.a, g.g, g.delta, g.dist, g.flags) for i, r in enumerate(ref) for g in r[2]]
    for split in ([1] * total, [total] if total <= 8 else [8] * (total // 8) + ([total % 8] if total % 8 else [])):
        got = kc.run_model(case, tables, split=split)
        assert np.array_equal(np.concatenate([r[0] for r in got]).view(np.uint32), ref_s.view(np.uint32)), split
        assert [(total_tick(got, i, g), g.frame, g.a, g.g, g.delta, g.dist, g.flags) for i, r in enumerate(got) for g in r[2]] == ref_g, split


def total_tick(results, feed_index, grain):
    return sum(len(r[1]) for r in results[:feed_index]) + grain.tick


# ---- the cases tell the model from every misreading ----
@pytest.fixture(scope="module")
def truth(tables):
    return {c.name: kc.run_model(c, tables) for c in kc.CASES}


def test_the_list_of_misreadings_is_the_issues():
    assert len(km.MISREADINGS) == 16 and len(set(km.MISREADINGS)) == 16


@pytest.mark.parametrize("mis", km.MISREADINGS)
def test_a_misreading_changes_some_case(tables, truth, mis):
    changed = []
    for c in kc.CASES:
        for (got, recs, grains), (want, wrecs, wgrains) in zip(kc.run_model(c, tables, mis=(mis,)), truth[c.name]):
            if recs != wrecs or grains != wgrains or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                changed.append(c.name)
                break
    print(mis, "changes", len(changed), "cases")
    assert changed, mis


def test_the_cases_reach_every_path_the_debug_counts_name(truth):
    total = dict.fromkeys(("grains_searched", "grains_unsearched", "chunks_fading", "chunks_straddling"), 0)
    for c in kc.CASES:
        for k, v in kc.keylock_counts(c, truth[c.name]).items():
            total[k] += v
    assert all(v > 0 for v in total.values()), total
    deltas = {g.delta for c in kc.CASES for r in truth[c.name] for g in r[2]}
    assert min(deltas) < 0 < max(deltas)
    # a first grain in the middle of a feed, a feed without a grain start, ticks with several
    assert any(g.flags & km.G_FIRST and g.tick > 0 for c in kc.CASES for r in truth[c.name] for g in r[2])
    assert any(not r[2] and any(t.flags & dm.T_PLAY for t in r[1]) for c in kc.CASES for r in truth[c.name][1:] if c.name.startswith("spt"))
    assert any(sum(1 for g in r[2] if g.tick == 0) >= 3 for c in kc.CASES for r in truth[c.name])


def test_the_cases_read_both_end_rows_of_the_bank_at_a_fractional_pitch(truth):
    """with a fractional pitch the render kernel stages the bank in LDS; row 0 is the first word of that array and row 255 blends into the last row.  (Row 0 was
    where the first version of the kernel faulted on a device: no other case read it.)"""
    rows = set()
    for c in kc.CASES:
        rows |= kc.fractional_pitch_phase_rows(c, truth[c.name])
    assert {0, 255} <= rows, sorted(rows)[:4]


# ---- what it is for: a tone at another tempo keeps its pitch ----
# The energy outside +-8 bins of the spectral peak, in dB relative to the whole, of a 997 Hz half-scale tone (48 kHz, i16 track, both channels) played at each tempo with
# pitch 2^32 and the recommended 1024 / 256 / 512, measured FROM THE MODEL over 16384 frames (Hann window, 2.93 Hz a bin) after 2 ticks of run-in, and the same with
# radius 0 (plain overlap-add); recorded in DESIGN.md section 0.16 and asserted with 3 dB of margin.  A property of the header's rule, not of any device.
TONE_DB = {0.92: (-63.6, -7.3), 1.08: (-63.3, -7.3), 1.5: (-61.7, -5.4)}   # tempo: (radius 512, radius 0)


def tone_figure(tables, tempo, radius):
    from mixlab_amd import deck
    rate, spt, f0, amp, n_win = 48000, 800, 997.0, 0.5, 16384
    n_ticks = 2 + -(-n_win // spt)
    n_frames = int(n_ticks * spt * tempo) + 4000
    tr = np.round(amp * 32768.0 * np.sin(2 * np.pi * f0 * np.arange(n_frames) / rate)).astype(np.int16)
    m = km.KeylockModel(np.stack([tr, tr], axis=1), tables)
    m.set_keylock(Keylock(ONE, 1024, 256, radius))
    m.schedule(0, Params(deck.deck_step(rate, rate, tempo), 0, 0, 0, PLAY), 100 * ONE)
    got, _recs, grains = m.feed(n_ticks, spt)
    y = got.reshape(-1, 2)[2 * spt:2 * spt + n_win].astype(np.float64)
    assert np.array_equal(y[:, 0], y[:, 1])
    spec = np.abs(np.fft.rfft(y[:, 0] * np.hanning(n_win))) ** 2
    peak = int(np.argmax(spec))
    outside = spec.sum() - spec[max(0, peak - 8):peak + 9].sum()
    return peak * rate / n_win, 10 * np.log10(outside / spec.sum()), grains


@pytest.mark.parametrize("tempo", sorted(TONE_DB))
def test_a_tone_at_another_tempo_keeps_its_pitch(tables, tempo):
    bin_hz = 48000 / 16384
    peak, db, grains = tone_figure(tables, tempo, 512)
    peak0, db0, _ = tone_figure(tables, tempo, 0)
    print(f"tempo {tempo}: radius 512 peak {peak:.1f} Hz, outside {db:.2f} dB; radius 0 peak {peak0:.1f} Hz, outside {db0:.2f} dB")
    assert any(g.delta for g in grains)
    assert abs(peak - 997.0) <= bin_hz, peak
    want, want0 = TONE_DB[tempo]
    assert db <= want + 3.0, db
    assert db0 >= db + 40.0, (db0, db)
