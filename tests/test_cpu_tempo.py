"""The tempo taps' spec without a GPU: the model against a slow and obvious restatement, independence of how a stream is cut into runs, the
deliberate misreadings the shared cases catch, mx_tempo_bpm on click tracks, and the ABI as the header declares it.
tests/test_gpu_tempo.py holds the device to the same model byte for byte."""
import ctypes as C
import math
import pathlib
import re
import struct

import numpy as np
import pytest

import tempo_cases as tc
import tempo_model as tm
from mixlab_amd import abi

HEADER = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mixlab_gpu.h").read_text()
F32 = np.float32


def run_model(case, x, cuts, variant=None):
    """the records of the whole stream, fed in runs of `cuts` ticks, as (absolute tick, record bytes without the tick word)"""
    m = tm.TempoModel(case.H, case.W, case.L, case.emit, case.channels, variant)
    per, out, at = case.F * case.channels, [], 0
    while at < case.n_ticks:
        k = min(cuts, case.n_ticks - at)
        for rec in m.run(x[at * per:(at + k) * per], k):
            out.append((at + struct.unpack_from("<I", rec)[0], rec[4:]))
        at += k
    return out


_spec = {}


def spec_records(case):
    if case.id not in _spec:
        _spec[case.id] = run_model(case, tc.stream(case), case.n_ticks)
    return _spec[case.id]


# ---- the slow and obvious restatement ----

def brute(case, x):
    """frame by frame, in Python integers"""
    H, W, L = case.H, case.W, case.L
    onsets, out = [], []
    energy = a_prev = bad = c = 0
    frame = 0
    for t in range(case.n_ticks):
        for f in range(case.F):
            i = (t * case.F + f) * case.channels
            with np.errstate(all="ignore"):
                m = float(F32(x[i]) + F32(x[i + case.channels - 1]))
            if math.isnan(m) or math.isinf(m):
                bad += 1
                q = 0
            else:
                q = int(min(abs(m), 4.0) * 1048576.0)   # exact in f64 as in f32; int() truncates
            energy += q * q
            frame += 1
            if frame % H == 0:
                a = math.isqrt(energy)
                onsets.append(max(a - a_prev, 0) >> 6)
                a_prev, energy = a, 0
        c += 1
        if c % case.emit == 0:
            hl = len(onsets) - 1
            o = lambda h: onsets[h] if h >= 0 else 0
            R = []
            for l in range(L):
                acc = 0
                for j in range(W):
                    if o(hl - j):
                        acc += o(hl - j) * o(hl - j - l)
                R.append(acc)
            out.append((t, struct.pack("<7I", len(onsets), bad, H, W, L, 0, 0) + struct.pack(f"<{L}Q", *R)))
            bad = 0
    return out


@pytest.mark.parametrize("case", [c for c in tc.CASES if c.id != "one_frame"] + [tc.Case("one_frame_short", 64, 64, 16, 7, 1, 700, 1)], ids=lambda c: c.id)
def test_model_equals_the_frame_by_frame_restatement(case):
    x = tc.stream(case)
    got = run_model(case, x, case.n_ticks)
    want = brute(case, x)
    assert len(got) == len(want) == case.n_ticks // case.emit
    for a, b in zip(got, want):
        assert a == b, f"tick {a[0]} / {b[0]}"
    recs = [tm.parse_record(b"\0\0\0\0" + r) for _, r in got]
    assert sum(r["nonfinite"] for r in recs) > 0 and any(r["acf"][1:].any() for r in recs) and all(r["acf"].max() < 2 ** 52 for r in recs)


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.id)
def test_tick_by_tick_in_runs_and_in_one_piece_give_identical_bytes(case):
    x = tc.stream(case)
    for cuts in (1, 3, 64):
        if case.id == "one_frame" and cuts == 1:
            cuts = 5   # (9000 one-tick runs of the model are slow; the device test makes them)
        assert run_model(case, x, cuts) == spec_records(case), cuts
    assert [t for t, _ in spec_records(case)] == list(range(case.emit - 1, case.n_ticks, case.emit))


def test_one_frame_ticks_emit_zero_tables_until_a_hop_completes():
    case = tc.by_id("one_frame")
    recs = [(t, tm.parse_record(b"\0\0\0\0" + r)) for t, r in spec_records(case)]
    early = [r for t, r in recs if t + 1 < case.H]
    assert len(early) == 9 and all(r["hops_complete"] == 0 and not r["acf"].any() for r in early)
    assert all(r["hops_complete"] == (t + 1) // case.H for t, r in recs) and recs[-1][1]["acf"][0] > 0


# ---- deliberate misreadings ----

@pytest.mark.parametrize("variant", tm.VARIANTS)
def test_every_misreading_is_caught_by_the_shared_cases(variant):
    """each variant changes one clause of the text; runs of 4 ticks, so that a counter reset per run shows"""
    caught = [case.id for case in tc.CASES if case.id != "one_frame" and run_model(case, tc.stream(case), 4, variant) != spec_records(case)]
    print(variant, "caught by", caught)
    assert caught, f"{variant} gives the spec's records on every shared case"
    if variant == "late_hop":
        assert "l_equals_w" in caught


def test_values_at_the_edges_of_the_quantiser():
    v = F32([4.0, 4.0000005, 3.9999998, 100.0, 3e38, 2.0 ** -20, 2.0 ** -21, 0.99999994 * 2.0 ** -20, 0.0, -0.0, -2.5, 1.5 * 2.0 ** -20])
    q, bad = tm.quantise(v * F32(0.5), v * F32(0.5))
    assert q.tolist() == [1 << 22, 1 << 22, 4194303, 1 << 22, 1 << 22, 1, 0, 0, 0, 0, 2621440, 1] and not bad.any()
    q, bad = tm.quantise(F32([3e38, np.inf, np.nan, np.inf, 1.0]), F32([3e38, 1.0, 1.0, -np.inf, 1.0]))
    assert bad.tolist() == [True, True, True, True, False] and q.tolist() == [0, 0, 0, 0, 2 << 20]
    sub = np.array([1, 0x7fffff], np.uint32).view(F32)
    assert tm.quantise(sub, sub)[0].tolist() == [0, 0]


# ---- mx_tempo_bpm ----

BPM_CASES = [(rate, tempo) for rate in (48000, 44100) for tempo in (90, 120, 128, 174)]


def click_record(rate, tempo, H=128, W=2048, L=512):
    F = rate // 60
    n_ticks = -(-(W + 40) * H // F)   # the window is full of the track
    x = tm.click_track(rate, tempo, n_ticks * F, seed=tempo)
    return tm.TempoModel(H, W, L, n_ticks, 1).run(x, n_ticks)[0]


def bpm_bound(rate, tempo, H=128):
    """the tempo step of half a hop of lag at the true lag 60 rate / (H tempo), towards the slower side (the smaller of the two steps)"""
    lag = 60.0 * rate / (H * tempo)
    return tempo - 60.0 * rate / (H * (lag + 0.5))


@pytest.mark.parametrize("rate,tempo", BPM_CASES)
def test_bpm_of_a_click_track(rate, tempo):
    rec = click_record(rate, tempo)
    lo, hi = tempo * 0.7, tempo * 1.4   # brackets the tempo; excludes its half and its double
    assert lo > tempo / 2 and hi < tempo * 2
    bound = bpm_bound(rate, tempo)
    want, want_conf = tm.bpm(rec, rate, lo, hi)
    print(f"{rate} Hz {tempo} BPM: model {want:.4f} (off by {abs(want - tempo):.4f}, bound {bound:.4f}), confidence {want_conf:.3f}")
    assert abs(want - tempo) <= bound, "the model alone misses the bound"
    got, conf = abi.tempo_bpm(rec, rate, lo, hi)
    assert abs(got - tempo) <= bound
    assert got == pytest.approx(want, rel=1e-13) and conf == pytest.approx(want_conf, rel=1e-13) and 0.3 < conf < 1.5


def test_bpm_of_silence_and_of_nothing_but_nonfinite_frames_is_zero():
    n_ticks, F = 24, 800
    for x in (np.zeros(n_ticks * F, F32), np.full(n_ticks * F, np.nan, F32), np.tile(F32([np.inf, -np.inf]), n_ticks * F // 2)):
        rec = tm.TempoModel(128, 128, 64, n_ticks, 1).run(x, n_ticks)[0]
        assert abi.tempo_bpm(rec, 48000.0, 60.0, 200.0) == (0.0, 0.0) == tm.bpm(rec, 48000.0, 60.0, 200.0)
        assert tm.parse_record(rec)["nonfinite"] == (0 if x[0] == 0 else n_ticks * F)


def test_bpm_lag_range_first_maximum_and_refusals():
    L = 32
    R = np.zeros(L, np.uint64); R[0] = 1000; R[10] = 500; R[9] = 300; R[11] = 400; R[20] = 500
    rec = struct.pack("<8I", 0, 99, 0, 128, 64, L, 0, 0) + R.tobytes()
    rate = 48000.0
    at = lambda l: 60.0 * rate / (128 * l)
    got, conf = abi.tempo_bpm(rec, rate, at(25), at(5))          # lags 5 .. 25: the first of the two equal maxima
    d = 0.5 * (300 - 400) / (300 - 1000 + 400)
    assert got == pytest.approx(at(10 + d), rel=1e-14) and conf == 0.5
    assert abi.tempo_bpm(rec, rate, at(25), at(15))[0] == pytest.approx(at(20), rel=1e-14)   # a peak between zeros: the denominator is negative, d = 0
    assert abi.tempo_bpm(rec, rate, at(10.5), at(9.5))[0] == pytest.approx(at(10 + d), rel=1e-14)   # a range of one lag
    assert abi.tempo_bpm(rec, rate, at(10.9), at(10.1)) == (0.0, 0.0)                         # no integer lag inside
    assert abi.tempo_bpm(rec, rate, at(500), at(31)) == (0.0, 0.0)                            # beyond L - 2
    assert abi.tempo_bpm(rec, rate, at(500), at(30))[0] == at(30)                             # lag 30 = L - 2: R is flat there, d = 0
    assert abi.tempo_bpm(rec, rate, at(0.9), at(0.1)) == (0.0, 0.0)                           # below lag 1
    b, c = C.c_double(), C.c_double()
    buf = C.create_string_buffer(rec, len(rec))
    call = lambda r, *a: abi.lib.mx_tempo_bpm(r, *a)
    assert call(buf, rate, 60.0, 200.0, C.byref(b), C.byref(c)) == abi.MX_OK
    assert call(None, rate, 60.0, 200.0, C.byref(b), C.byref(c)) == abi.MX_ERR_INVALID
    assert call(buf, rate, 60.0, 200.0, None, C.byref(c)) == abi.MX_ERR_INVALID and call(buf, rate, 60.0, 200.0, C.byref(b), None) == abi.MX_ERR_INVALID
    for args in ((0.0, 60.0, 200.0), (-1.0, 60.0, 200.0), (float("nan"), 60.0, 200.0), (float("inf"), 60.0, 200.0), (rate, 0.0, 200.0), (rate, -5.0, 200.0),
                 (rate, 200.0, 60.0), (rate, 60.0, float("inf")), (rate, float("nan"), 200.0)):
        assert call(buf, *args, C.byref(b), C.byref(c)) == abi.MX_ERR_INVALID, args
    for head in ((100, 64, 32), (128, 63, 32), (128, 64, 15), (128, 64, 65), (128, 5000, 32), (128, 4096, 1025), (0, 0, 0)):   # not a record
        bad = C.create_string_buffer(struct.pack("<8I", 0, 0, 0, *head, 0, 0) + bytes(8 * 1025))
        assert call(bad, rate, 60.0, 200.0, C.byref(b), C.byref(c)) == abi.MX_ERR_INVALID, head
    with pytest.raises(abi.MxError):
        abi.tempo_bpm(rec[:100], rate, 60.0, 200.0)   # shorter than its header says


# ---- constants and header ----

def test_record_bytes_and_parameter_errors():
    for H, W, L, e in ((64, 64, 16, 1), (128, 2048, 512, 6), (256, 4096, 1024, 1 << 31), (128, 64, 64, 1)):
        assert abi.tempo_record_bytes(H, W, L, e) == tm.record_bytes(L) == 32 + 8 * L and tm.check_params(H, W, L, e)
    n = C.c_size_t()
    for H, W, L, e in ((0, 64, 16, 1), (32, 64, 16, 1), (96, 64, 16, 1), (512, 64, 16, 1), (128, 63, 16, 1), (128, 4097, 16, 1), (128, 64, 15, 1), (128, 2048, 1025, 1),
                       (128, 64, 65, 1), (128, 64, 16, 0)):
        assert abi.lib.mx_tempo_record_bytes(C.byref(abi.TempoParams(H, W, L, e)), C.byref(n)) == abi.MX_ERR_INVALID, (H, W, L, e)
        assert not tm.check_params(H, W, L, e)
    assert abi.lib.mx_tempo_record_bytes(None, C.byref(n)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_tempo_record_bytes(C.byref(abi.TempoParams(128, 64, 16, 1)), None) == abi.MX_ERR_INVALID
    parsed = abi.parse_tempo_records(np.frombuffer(struct.pack("<8I", 3, 9, 1, 64, 64, 16, 0, 0) + struct.pack("<16Q", *range(16)), np.uint8), 16)
    assert len(parsed) == 1 and parsed[0]["tick_in_run"] == 3 and parsed[0]["hops_complete"] == 9 and parsed[0]["acf"].tolist() == list(range(16))


def test_header_carries_the_spec_and_constants_are_unchanged():
    assert C.sizeof(abi.TempoParams) == 16 and [getattr(abi.TempoParams, f).offset for f, _ in abi.TempoParams._fields_] == [0, 4, 8, 12]
    assert re.search(r"typedef struct \{ uint32_t hop_frames /\*.*?\*/, window_hops /\*.*?\*/, max_lag /\*.*?\*/, emit_ticks /\*.*?\*/; \} mx_tempo_params;", HEADER)
    for p in (r"int mx_graph_set_tempo\(mx_graph\* g, const mx_port_ref\* ports, size_t n, const mx_tempo_params\* params\);",
              r"int mx_graph_read_tempo\(mx_graph\* g, void\* dst, size_t cap_bytes, uint32_t\* n_records\);",
              r"int mx_tempo_record_bytes\(const mx_tempo_params\* params, size_t\* bytes\);",
              r"int mx_tempo_bpm\(const void\* record, double rate, double bpm_lo, double bpm_hi, double\* bpm, double\* confidence\);"):
        assert re.search(p, HEADER), p
    spec = HEADER[HEADER.index("/* Tempo taps on audio output ports"): HEADER.index("} mx_tempo_params;")]
    for clause in ("m = L + R in f32, rounded once", "(uint32_t)(fminf(fabsf(m), 4.0f) * 1048576.0f)", "floor(sqrt(E[h]))", "A[-1] = 0",
                   "max(A[h] - A[h - 1], 0) >> 6", "c mod emit_ticks == 0", "o[hl - j] * o[hl - j - l]", "W + L - 1", "no running sum",
                   "tick_in_run", "hops_complete", "nonfinite", "reserved[2]", "32 + 8 L bytes", "BUILD-SPECIFIED", "tests/tempo_model.py",
                   "resets every tap and c", "MX_FLAG_NO_FUSE"):
        assert clause in spec, clause
    for name in ("mx_graph_set_tempo", "mx_graph_read_tempo", "mx_tempo_record_bytes", "mx_tempo_bpm"):
        assert hasattr(abi.lib, name)
    note = HEADER[HEADER.index("#define MX_ABI_VERSION"): HEADER.index("/* ---- status codes")]
    assert "later, without a bump (only additions)" in note
    for name in ("mx_tempo_params", "mx_graph_set_tempo", "mx_graph_read_tempo", "mx_tempo_record_bytes", "mx_tempo_bpm"):
        assert name in note, name
    # additions only: no version bump, no module kind
    assert re.search(r"#define\s+MX_ABI_VERSION\s+4u", HEADER) and abi.lib.mx_abi_version() == 4
    assert abi.KIND_COUNT == 19 and abi.PROFILE_KINDS == 18
    assert re.search(r"#define\s+MX_PROFILE_KINDS\s+18\b", HEADER) and re.search(r"MX_KIND_COUNT\s*=\s*19\b", HEADER)
