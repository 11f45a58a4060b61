"""The deck's whole-track tonality and loudness without a device (include/mixlab_gpu.h "KEY AND LOUDNESS"): the header's structs and entry
points, the setting rules at both edges of each, mx_deck_tonality_host and mx_deck_loudness_host against the TAPS' models on every shared case
(tests/deck_loudkey_cases.py), the counts, the refusals, the two read-outs, that the shared cases tell the text from each of a list of misreadings, and conformance
through the host paths: four cadences named, a sine's programme loudness, a true peak between the samples."""
import ctypes as C
import math
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import deck_loudkey_cases as lk
import loudness_model as lm
import tonality_model as tm

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_tonality_check", "mx_deck_tonality_count", "mx_deck_analyse_tonality", "mx_deck_read_tonality", "mx_deck_tonality_host",
                "mx_deck_debug_last_tonality", "mx_deck_loudness_check", "mx_deck_loudness_count", "mx_deck_analyse_loudness", "mx_deck_read_loudness",
                "mx_deck_loudness_host", "mx_deck_debug_last_loudness", "mx_deck_loudness_gain", "mx_tonality_camelot"}
TONALITY_OFFSETS = {"rate": 0, "decim": 8, "hop_frames": 12, "octaves": 16, "f_lo_mhz": 20, "segment_hops": 24, "_pad": 28}
LOUDNESS_OFFSETS = {"rate": 0, "block_frames": 8, "momentary_blocks": 12, "short_blocks": 16, "_pad": 20}


def raw(recs) -> bytes:
    return b"".join(r["raw"] for r in recs)


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    assert lay["mx_deck_tonality"] == {"size": 32, "offsets": TONALITY_OFFSETS}
    assert lay["mx_deck_loudness"] == {"size": 24, "offsets": LOUDNESS_OFFSETS}
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # additions only
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_analyse_tonality") == ["mx_deck*", "const mx_deck_tonality*"]
    assert sig("mx_deck_tonality_count") == ["uint64_t", "const mx_deck_tonality*", "uint64_t*"]
    assert sig("mx_deck_read_tonality") == ["mx_deck*", "uint64_t", "uint64_t", "void*", "size_t"]
    assert sig("mx_deck_tonality_host") == ["const int16_t*", "uint64_t", "const mx_deck_tonality*", "uint64_t", "uint64_t", "void*"]
    assert sig("mx_deck_analyse_loudness") == ["mx_deck*", "const mx_deck_loudness*"]
    assert sig("mx_deck_loudness_count") == ["uint64_t", "uint32_t", "uint64_t*"]
    assert sig("mx_deck_read_loudness") == ["mx_deck*", "uint64_t", "uint64_t", "mx_loudness_tick*"]
    assert sig("mx_deck_loudness_host") == ["const int16_t*", "uint64_t", "const mx_deck_loudness*", "mx_loudness_tick*", "uint64_t"]
    assert sig("mx_deck_loudness_gain") == ["const mx_loudness_tick*", "uint64_t", "uint32_t", "uint32_t", "double", "double", "double*", "double*", "double*"]
    assert sig("mx_tonality_camelot") == ["int", "uint32_t*", "uint32_t*"]
    for name in ("tonality", "loudness"):
        assert re.search(rf"int mx_deck_debug_last_{name}\(uint32_t out\[4\]\);", text)
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | {"mx_deck_tonality", "mx_deck_loudness"}):
        assert re.search(rf"\b{name}\b", note), name
    # the new comment stands below ANALYSIS, whose own text is as it was
    assert text.index("---- ANALYSIS:") < text.index("mx_deck_debug_last_analysis(uint32_t out[4]);") < text.index("---- KEY AND LOUDNESS:")
    assert "Out of scope: gated-loudness (LUFS) auto-gain and whole-track key (the columns' e and peaks serve a plain gain; key can follow on the same pass)" in text
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}


def test_ctypes_mirrors_have_the_headers_layout():
    from mixlab_amd import abi
    for st, size, offs in ((abi.DeckTonality, 32, TONALITY_OFFSETS), (abi.DeckLoudness, 24, LOUDNESS_OFFSETS)):
        assert C.sizeof(st) == size and {n: getattr(st, n).offset for n, _t in st._fields_} == offs
    assert abi.LOUDNESS_TICK_DTYPE.itemsize == 48


# ---- the setting rules, accepted at the bound and refused one past it ----
# at 8 kHz and D 4 (fs_d = 2000): N_0 = ceil(34000 / f_lo) <= 2048 down to 16.602 Hz; two octaves end below 0.45 fs_d = 900 Hz up to f_lo < 900 / 2^(47/24) = 231.59 Hz
TON_CHECKS = [({}, True),
              ({"decim": 8, "f_lo_mhz": 110000}, True), ({"decim": 2}, False), ({"decim": 16}, False), ({"decim": 0}, False), ({"decim": 6}, False),
              ({"hop_frames": 256}, True), ({"hop_frames": 512}, True), ({"hop_frames": 64}, False), ({"hop_frames": 1024}, False), ({"hop_frames": 129}, False),
              # (six octaves pass the parameter rule but no rate has kernels for them: 2^(71/12 + 1/24) x 17 / 2048 = 0.516 > 0.45; five is the most that exists)
              ({"octaves": 5, "decim": 8, "rate": 48000.0, "f_lo_mhz": 65406}, True), ({"octaves": 6, "decim": 8, "rate": 48000.0, "f_lo_mhz": 65406}, False),
              ({"octaves": 7, "decim": 8, "rate": 48000.0, "f_lo_mhz": 32703}, False), ({"octaves": 1}, False),
              ({"f_lo_mhz": 16602}, True), ({"f_lo_mhz": 16601}, False), ({"f_lo_mhz": 0}, False), ({"f_lo_mhz": 1}, False),
              ({"f_lo_mhz": 231000}, True), ({"f_lo_mhz": 232000}, False), ({"f_lo_mhz": 440000}, False), ({"f_lo_mhz": 440000, "rate": 16000.0}, True),
              ({"segment_hops": 1}, True), ({"segment_hops": 65536}, True), ({"segment_hops": 0}, False), ({"segment_hops": 65537}, False),
              ({"rate": 0.0}, False), ({"rate": -8000.0}, False), ({"rate": float("nan")}, False), ({"rate": float("inf")}, False), ({"_pad": 1}, False)]
LOUD_CHECKS = [({}, True),
               ({"block_frames": 64}, True), ({"block_frames": 63}, False), ({"block_frames": 65536}, True), ({"block_frames": 65537}, False),
               ({"momentary_blocks": 1}, True), ({"momentary_blocks": 0}, False), ({"momentary_blocks": 1024}, True), ({"momentary_blocks": 1025}, False),
               ({"short_blocks": 1}, True), ({"short_blocks": 0}, False), ({"short_blocks": 1024}, True), ({"short_blocks": 1025}, False),
               ({"rate": 3364.0}, True), ({"rate": 3363.948901911066}, False), ({"rate": float("nan")}, False), ({"rate": float("inf")}, False), ({"_pad": 1}, False)]


@pytest.mark.parametrize("change,ok", TON_CHECKS)
def test_tonality_check_at_the_boundaries(change, ok):
    from mixlab_amd import abi, deck
    t = deck.tonality(8000.0, 4, 128, 2, 220000, 3)
    for k, v in change.items():
        setattr(t, k, v)
    # the rules that are the taps': what mx_tonality_tables says of the same numbers
    if "segment_hops" not in change and "_pad" not in change:
        par = abi.TonalityParams(t.decim, t.hop_frames, t.octaves, t.f_lo_mhz, 1)
        fir, ln = np.zeros(64, np.int16), np.zeros(96, np.uint32)
        taps_ok = abi.lib.mx_tonality_tables(t.rate, C.byref(par), fir.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p), None, None) == abi.MX_OK
        assert taps_ok == ok, change
    if ok:
        deck.tonality_check(t)
        assert deck.tonality_count(1, t) == 1
    else:
        for fn in (lambda: deck.tonality_check(t), lambda: deck.tonality_count(1000, t), lambda: deck.tonality_host(np.zeros((10, 2), np.int16), t)):
            with pytest.raises(abi.MxError) as e:
                fn()
            assert e.value.code == abi.MX_ERR_INVALID


@pytest.mark.parametrize("change,ok", LOUD_CHECKS)
def test_loudness_check_at_the_boundaries(change, ok):
    from mixlab_amd import abi, deck
    l = deck.loudness(48000.0, 4800, 4, 30)
    for k, v in change.items():
        setattr(l, k, v)
    if ok:
        deck.loudness_check(l)
    else:
        with pytest.raises(abi.MxError) as e:
            deck.loudness_check(l)
        assert e.value.code == abi.MX_ERR_INVALID and "deck loudness" in str(e.value)
        out = np.zeros(4, abi.LOUDNESS_TICK_DTYPE)
        assert abi.lib.mx_deck_loudness_host(np.zeros(200, np.int16).ctypes.data_as(C.c_void_p), 100, C.byref(l), out.ctypes.data_as(C.c_void_p), 4) == abi.MX_ERR_INVALID


def test_the_base_setting_is_the_nearest_to_the_issues_that_the_tables_accept():
    """D 4, Hc 128, O 2 from 440 Hz at 8 kHz is refused (the top bin lies beyond 0.45 fs_d); one octave lower is the setting of the shared cases"""
    from mixlab_amd import abi
    with pytest.raises(abi.MxError) as e:
        abi.tonality_tables(8000.0, 4, 128, 2, 440000)
    assert "0.45" in str(e.value)
    fir, ln, kern = abi.tonality_tables(8000.0, 4, 128, 2, 220000)
    assert int(ln[0]) == 155 and len(ln) == 24 and kern.shape[0] == int(ln.sum())
    assert all((c.rate, c.D, c.Hc, c.O, c.f_lo_mhz) == (8000.0, 4, 128, 2, 220000) for c in lk.TON_CASES[:-1])


# ---- the host functions against the taps' models ----
@pytest.mark.parametrize("case", lk.TON_CASES, ids=lambda c: c.name)
def test_tonality_host_equals_the_model_whole_and_windowed(case):
    from mixlab_amd import deck
    t, tr, want = lk.c_tonality(case), lk.track(case), lk.ton_truth(case)
    n, rb = lk.ton_segments(case), 32 + 96 * case.O
    assert deck.tonality_count(case.n_frames, t) == n and len(want) == n * rb
    got = deck.tonality_host(tr, t)
    for g, r in enumerate(got):
        assert r["raw"] == want[g * rb:(g + 1) * rb], (case.name, g)
        assert (r["tick_in_run"], r["hops"], r["nonfinite"], r["decim"], r["hop_frames"], r["octaves"], r["f_lo_mhz"], r["reserved"]) == \
               (g, case.G, 0, case.D, case.Hc, case.O, case.f_lo_mhz, 0)
    for first, cnt in ((0, 1), (n // 2, n - n // 2), (n - 1, 1), (n, 0)):
        assert raw(deck.tonality_host(tr, t, first, cnt)) == want[first * rb:(first + cnt) * rb], (case.name, first, cnt)
    # the records are the taps': the chroma and key calls take them as they are
    from mixlab_amd import abi
    if np.frombuffer(want, np.uint8).reshape(n, rb)[:, 32:].any():
        assert np.array_equal(abi.tonality_chroma(got, case.rate), tm.chroma([r["raw"] for r in got], case.rate))


@pytest.mark.parametrize("case", lk.LOUD_CASES, ids=lambda c: c.name)
def test_loudness_host_equals_the_model_bit_for_bit(case):
    from mixlab_amd import deck
    got, want = deck.loudness_host(lk.track(case), lk.c_loudness(case)), lk.loud_truth(case)
    assert len(got) == len(want) == lk.loud_blocks(case) == deck.loudness_count(case.n_frames, case.F)
    assert lm.records_equal(got, want), (case.name, lm.first_difference(got, want))
    assert (got["frames"] == case.F).all() and (got["channels"] == 2).all()


def test_the_named_cases_are_what_the_issue_says_they_are():
    q = lambda s: np.trunc(s / 4.0)   # noqa: E731
    tr = lk.track(lk.TON_BY_NAME["every sample -32768"]).astype(np.int64)
    assert (q(tr.sum(axis=1)) == -16384).all()                                   # the decimator's extreme
    s = lk.track(lk.TON_BY_NAME["odd negative s throughout"]).astype(np.int64).sum(axis=1)
    assert (s < 0).all() and (s & 1).all() and (q(s) != (s >> 2)).all()           # where s / 4 and s >> 2 part
    a, b = (lk.ton_truth(lk.TON_BY_NAME[n]) for n in ("508 frames: the first hop's last input frame absent", "509 frames: ... present"))
    assert len(a) == len(b) == 224 and a != b                                    # one padded segment each, whose sums differ
    assert lk.ton_segments(lk.TON_BY_NAME["20 hops of noise, G = 7: a short last segment"]) == 3 and lk.ton_segments(lk.TON_BY_NAME["20 hops of noise, G = 65536: one record"]) == 1
    assert not np.frombuffer(lk.ton_truth(lk.TON_BY_NAME["silence"]), np.uint8).reshape(2, 224)[:, 32:].any()
    rec = lk.loud_truth(lk.LOUD_BY_NAME["full-scale alternating square"])
    assert float(rec["true_peak"].max()) > 32767.0 / 32768.0                     # the true peak lies above the sample peak
    assert float(lk.loud_truth(lk.LOUD_BY_NAME["every sample -32768"])["true_peak"].max()) >= 1.0
    rec = lk.loud_truth(lk.LOUD_BY_NAME["silence"])
    assert not rec["ksq"].any() and not rec["true_peak"].any() and not rec["momentary_sq"].any()
    long_w = lk.loud_truth(lk.LOUD_BY_NAME["71 blocks, windows 1 and 1024"])
    e = long_w["ksq"].sum(axis=1)
    assert len(long_w) == 71 and np.array_equal(long_w["momentary_sq"], e) and long_w["short_sq"][-1] == np.add.accumulate(e)[-1]
    assert len(lk.loud_truth(lk.LOUD_BY_NAME["F = 4800 over 3.5 blocks"])) == 4


# ---- the refusals ----
def test_the_host_functions_and_counts_refuse_what_the_header_says_they_refuse():
    from mixlab_amd import abi, deck
    lib = abi.lib
    case = lk.TON_BY_NAME["F + 1 frames, G = 3"]
    t, tr = lk.c_tonality(case), np.ascontiguousarray(lk.track(case))
    xp, buf = tr.ctypes.data_as(C.c_void_p), np.zeros(2 * 224, np.uint8)
    bp = buf.ctypes.data_as(C.c_void_p)
    assert lib.mx_deck_tonality_host(xp, case.n_frames, C.byref(t), 0, 2, bp) == abi.MX_OK and buf.tobytes() == lk.ton_truth(case)
    for args in ((None, case.n_frames, C.byref(t), 0, 2, bp), (xp, case.n_frames, None, 0, 2, bp), (xp, case.n_frames, C.byref(t), 0, 2, None),
                 (xp, case.n_frames, C.byref(t), 0, 3, bp), (xp, case.n_frames, C.byref(t), 3, 0, bp), (xp, case.n_frames, C.byref(t), 2, 1, bp),
                 (xp, 0, C.byref(t), 0, 0, bp), (xp, (1 << 30) + 1, C.byref(t), 0, 1, bp)):
        assert lib.mx_deck_tonality_host(*args) == abi.MX_ERR_INVALID, args
    assert lib.mx_deck_tonality_host(xp, case.n_frames, C.byref(t), 2, 0, None) == abi.MX_OK   # an empty window at the end names nothing
    n = C.c_uint64()
    for args in ((0, C.byref(t), C.byref(n)), ((1 << 30) + 1, C.byref(t), C.byref(n)), (100, None, C.byref(n)), (100, C.byref(t), None)):
        assert lib.mx_deck_tonality_count(*args) == abi.MX_ERR_INVALID, args
    assert deck.tonality_count(1 << 30, deck.tonality(8000.0, 4, 128, 2, 220000, 1)) == 1 << 21 and deck.tonality_count(1537, t) == 2
    assert deck.tonality_count(1 << 30, deck.tonality(48000.0, 8, 512, 5, 65406, 65536)) == 4 and deck.tonality_count(1 << 28, deck.tonality(48000.0, 8, 512, 5, 65406, 65536)) == 1
    assert lib.mx_deck_tonality_check(None) == abi.MX_ERR_INVALID and lib.mx_deck_loudness_check(None) == abi.MX_ERR_INVALID

    lc = lk.LOUD_BY_NAME["65 frames"]
    l, tr = lk.c_loudness(lc), np.ascontiguousarray(lk.track(lc))
    xp, out = tr.ctypes.data_as(C.c_void_p), np.zeros(2, abi.LOUDNESS_TICK_DTYPE)
    op = out.ctypes.data_as(C.c_void_p)
    assert lib.mx_deck_loudness_host(xp, 65, C.byref(l), op, 2) == abi.MX_OK and lm.records_equal(out, lk.loud_truth(lc))
    for args in ((None, 65, C.byref(l), op, 2), (xp, 65, None, op, 2), (xp, 65, C.byref(l), None, 2), (xp, 65, C.byref(l), op, 1), (xp, 0, C.byref(l), op, 2),
                 (xp, (1 << 30) + 1, C.byref(l), op, 1 << 30)):
        assert lib.mx_deck_loudness_host(*args) == abi.MX_ERR_INVALID, args
    for args in ((0, 64, C.byref(n)), ((1 << 30) + 1, 64, C.byref(n)), (100, 63, C.byref(n)), (100, 65537, C.byref(n)), (100, 64, None)):
        assert lib.mx_deck_loudness_count(*args) == abi.MX_ERR_INVALID, args
    assert deck.loudness_count(1 << 30, 64) == 1 << 24 and deck.loudness_count(65, 64) == 2 and deck.loudness_count(64, 64) == 1 and deck.loudness_count(1, 65536) == 1
    for fn in (lib.mx_deck_debug_last_tonality, lib.mx_deck_debug_last_loudness):
        assert fn(None) == abi.MX_ERR_INVALID


# ---- the read-outs ----
CAMELOT = ["8B", "3B", "10B", "5B", "12B", "7B", "2B", "9B", "4B", "11B", "6B", "1B",      # C, C#, D, Eb, E, F, F#, G, Ab, A, Bb, B major
           "5A", "12A", "7A", "2A", "9A", "4A", "11A", "6A", "1A", "8A", "3A", "10A"]      # C, C#, D, Eb, E, F, F#, G, G#, A, Bb, B minor


def test_camelot_names_all_24_keys_and_refuses_the_rest():
    from mixlab_amd import abi, deck
    assert [deck.camelot(k) for k in range(24)] == CAMELOT
    assert (deck.camelot(0), deck.camelot(21), deck.camelot(11)) == ("8B", "8A", "1B")
    for k in range(12):   # a major key and its relative minor, a minor third below, share a number
        assert deck.camelot(k)[:-1] == deck.camelot(12 + (k + 9) % 12)[:-1]
    number, minor = C.c_uint32(), C.c_uint32()
    for key in (-1, 24, -2, 1 << 20):
        assert abi.lib.mx_tonality_camelot(key, C.byref(number), C.byref(minor)) == abi.MX_ERR_INVALID, key
    assert abi.lib.mx_tonality_camelot(0, None, C.byref(minor)) == abi.MX_ERR_INVALID and abi.lib.mx_tonality_camelot(0, C.byref(number), None) == abi.MX_ERR_INVALID


def gain_restated(recs, m, hop, target, ceiling):
    from mixlab_amd import abi
    n = len(recs)
    idx = list(range(min(m - 1, n - 1), n, hop))
    lufs = abi.loudness_gate([float(recs["momentary_sq"][i]) for i in idx], [m * int(recs["frames"][i]) for i in idx])[0]
    pk = float(recs["true_peak"].max())
    peak = 20.0 * math.log10(pk) if pk > 0 else -math.inf
    return lufs, peak, (0.0 if lufs == -math.inf else min(target - lufs, ceiling - peak))


def test_loudness_gain_equals_its_restatement():
    """lufs is mx_loudness_gate's own number, so equal bit for bit; the peak and the gain go through log10, which this test takes from Python's libm and the library
    from its own: 1e-9 dB is far above an ulp of either and far below anything a host would show"""
    from mixlab_amd import deck
    sine = (10.0 ** (-12.0 / 20.0) * 32767.0 * np.sin(2 * np.pi * 1000.0 * np.arange(48000) / 48000.0)).round().astype(np.int16)
    loud = deck.loudness_host(np.stack([sine, sine], axis=1), deck.loudness(48000.0, 4800, 4, 30))
    cases = [(lk.loud_truth(lk.LOUD_BY_NAME["71 blocks: 64 * 70 + 5 frames"]), 4, 1, -14.0, -1.0),
             (lk.loud_truth(lk.LOUD_BY_NAME["71 blocks: 64 * 70 + 5 frames"]), 4, 3, -14.0, -1.0),
             (lk.loud_truth(lk.LOUD_BY_NAME["65 frames"]), 4, 1, -14.0, -1.0),            # n = 2 < M: the one block is the last record
             (lk.loud_truth(lk.LOUD_BY_NAME["1 frame"]), 4, 1, -14.0, -1.0),
             (lk.loud_truth(lk.LOUD_BY_NAME["silence"]), 4, 1, -14.0, -1.0),              # nothing passes the gate: gain 0
             (loud, 4, 1, -23.0, -1.0),                                                    # the target binds: a -12 dBFS sine turned down
             (loud, 4, 1, -6.0, -10.0)]                                                    # the ceiling binds: +6 LU would lift the peak above -10 dBTP
    for recs, m, hop, target, ceiling in cases:
        got, want = deck.loudness_gain(recs, m, hop, target, ceiling), gain_restated(recs, m, hop, target, ceiling)
        assert got[0] == want[0] or (math.isnan(got[0]) and math.isnan(want[0])), (got, want)
        for a, b in zip(got[1:], want[1:]):
            assert a == b or abs(a - b) <= 1e-9, (got, want)
    silent = deck.loudness_gain(lk.loud_truth(lk.LOUD_BY_NAME["silence"]))
    assert silent == (-math.inf, -math.inf, 0.0)
    lufs, peak, gain = deck.loudness_gain(loud, 4, 1, -23.0, -1.0)
    assert abs(lufs - (-12.0)) < 0.1 and abs(peak - (-12.0)) < 0.1 and gain == -23.0 - lufs
    lufs, peak, gain = deck.loudness_gain(loud, 4, 1, -6.0, -10.0)
    assert gain == -10.0 - peak and gain < -6.0 - lufs


def test_loudness_gain_refuses_what_the_header_says_it_refuses():
    from mixlab_amd import abi
    recs = np.ascontiguousarray(lk.loud_truth(lk.LOUD_BY_NAME["65 frames"]))
    rp = recs.ctypes.data_as(C.c_void_p)
    a, b, c = C.c_double(), C.c_double(), C.c_double()
    good = [rp, 2, 4, 1, -14.0, -1.0, C.byref(a), C.byref(b), C.byref(c)]
    assert abi.lib.mx_deck_loudness_gain(*good) == abi.MX_OK
    for k, v in ((0, None), (1, 0), (2, 0), (2, 1025), (3, 0), (4, float("nan")), (4, float("inf")), (5, float("nan")), (5, -float("inf")), (6, None), (7, None), (8, None)):
        args = list(good)
        args[k] = v
        assert abi.lib.mx_deck_loudness_gain(*args) == abi.MX_ERR_INVALID, (k, v)
    good[2] = 1024
    assert abi.lib.mx_deck_loudness_gain(*good) == abi.MX_OK


# ---- the cases tell the text from every misreading ----
@pytest.mark.parametrize("mis", lk.TON_MISREADINGS)
def test_a_tonality_misreading_changes_some_case(mis):
    changed = [c.name for c in lk.TON_CASES if b"".join(lk.ton_records(c, mis)) != lk.ton_truth(c)]
    print(mis, "changes", len(changed), "cases:", changed[:4])
    assert changed, mis


@pytest.mark.parametrize("mis", lk.LOUD_MISREADINGS)
def test_a_loudness_misreading_changes_some_case(mis):
    changed = [c.name for c in lk.LOUD_CASES if not lm.records_equal(lk.loud_records(c, mis), lk.loud_truth(c))]
    print(mis, "changes", len(changed), "cases:", changed[:4])
    assert changed, mis


def test_the_list_of_misreadings_is_the_issues():
    assert len(lk.TON_MISREADINGS) + len(lk.LOUD_MISREADINGS) == 8


# ---- conformance, through the host paths ----
def as_i16(x) -> np.ndarray:
    """mono f32 in [-1, 1] -> stereo int16, rounded to nearest"""
    v = np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767).astype(np.int16)
    return np.stack([v, v], axis=1)


@pytest.mark.parametrize("tonic,minor,name", [(0, False, "8B"), (9, True, "8A"), (6, False, "2B"), (3, True, "2A")], ids=["C major", "A minor", "F sharp major", "E flat minor"])
def test_a_cadence_is_named(tonic, minor, name):
    """the four cadences of DESIGN.md section 0.10 as stereo int16 tracks, 8 s at 48 kHz; the confidences are reported in section 0.18"""
    from mixlab_amd import abi, deck
    recs = deck.tonality_host(as_i16(tm.cadence(48000.0, tonic, minor)), deck.tonality(48000.0, 8, 512, 5, 65406, 64))
    key, conf = abi.tonality_key(abi.tonality_chroma(recs, 48000.0))
    print(f"cadence on {tonic} {'minor' if minor else 'major'}: key {key}, confidence {conf:.4f}, {len(recs)} records")
    assert key == tonic + (12 if minor else 0) and conf > 0 and deck.camelot(key) == name


def test_a_minus_23_dbfs_sine_reads_minus_23_lufs_integrated():
    """EBU Tech 3341's tolerance, +-0.1 LU, the one tests/test_cpu_loudness.py uses"""
    from mixlab_amd import deck
    x = 10.0 ** (-23.0 / 20.0) * np.sin(2 * np.pi * 1000.0 * np.arange(480000) / 48000.0)
    recs = deck.loudness_host(as_i16(x), deck.loudness(48000.0, 4800, 4, 30))
    lufs, peak, _gain = deck.loudness_gain(recs, 4, 1)
    print(f"1 kHz at -23 dBFS, 10 s: I {lufs:.4f} LUFS, true peak {peak:.4f} dBTP")
    assert len(recs) == 100 and abs(lufs - (-23.0)) <= 0.1, lufs


def test_the_true_peak_of_a_quarter_rate_sine():
    """the taps' case: rate / 4, phase 45 degrees, amplitude 0.5 -- every sample is 0.354, the peak between them 0.5 = -6.02 dBTP; Tech 3341's +0.2 / -0.4 dB"""
    from mixlab_amd import deck
    x = 0.5 * np.sin(2 * np.pi * np.arange(30 * 800) / 4.0 + np.pi / 4)
    recs = deck.loudness_host(as_i16(x), deck.loudness(48000.0, 800, 4, 30))
    _lufs, peak, _gain = deck.loudness_gain(recs, 4, 1)
    print(f"true peak {peak:.3f} dBTP (sample peak {20 * math.log10(float(np.abs(x).max())):.3f} dBFS)")
    assert -6.0 - 0.4 <= peak <= -6.0 + 0.2, peak
    assert np.array_equal(recs["true_peak"][:, 0], recs["true_peak"][:, 1])
