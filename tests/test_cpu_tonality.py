"""The tonality taps' spec without a GPU: the tables against mpmath, the model against a slow and obvious restatement and against an f64
evaluation within a derived bound, independence of how a stream is cut into runs, the deliberate misreadings the shared cases catch, the key
of cadences, and the ABI as the header declares it.  tests/test_gpu_tonality.py holds the device to the same model byte for byte."""
import ctypes as C
import math
import pathlib
import re
import struct

import mpmath
import numpy as np
import pytest

import tonality_cases as tc
import tonality_model as tm
from mixlab_amd import abi

HEADER = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mixlab_gpu.h").read_text()
F32 = np.float32
NAMES = "C C# D D# E F F# G G# A A# B".split()


def run_model(case, x, cuts, variant=None):
    """the records of the whole stream, fed in runs of `cuts` ticks, as (absolute tick, record bytes without the tick word)"""
    m = tm.TonalityModel(case.rate, case.D, case.Hc, case.O, case.f_lo_mhz, case.emit, case.channels, variant)
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


# ---- the tables ----

TABLE_SETS = [(48000, 8, 5, 65406), (44100, 8, 5, 65406), (48000, 4, 2, 440000), (48000, 8, 2, 50000), (30540, 4, 2, 440000), (8000, 4, 2, 100000)]


@pytest.mark.parametrize("rate,D,O,f_lo_mhz", TABLE_SETS)
def test_tables_against_mpmath(rate, D, O, f_lo_mhz):
    """every entry within 0.5 + 2^-20 of the scaled exact value; sum |c| <= 65534; the lengths are the exact ceilings"""
    mpmath.mp.dps = 40
    fir, ln, kern = abi.tonality_tables(rate, D, 128, O, f_lo_mhz)
    tol = 0.5 + 2.0 ** -20
    Tf, fs_d, f_lo = 8 * D, mpmath.mpf(rate) / D, mpmath.mpf(f_lo_mhz) / 1000
    h = []
    for k in range(Tf):
        t = mpmath.mpf(k) - mpmath.mpf(Tf - 1) / 2
        h.append(mpmath.sin(2 * mpmath.pi * (mpmath.mpf("0.45") / D) * t) / (mpmath.pi * t) * (0.5 - 0.5 * mpmath.cos(2 * mpmath.pi * (k + 1) / (Tf + 1))))
    total = sum(h)
    assert fir.size == Tf and max(abs(int(fir[k]) - 32768 * h[k] / total) for k in range(Tf)) <= tol
    assert int(np.abs(fir.astype(np.int64)).sum()) <= 65534
    at = 0
    for b in range(12 * O):
        f = f_lo * mpmath.power(2, mpmath.mpf(b) / 12)
        N = int(mpmath.ceil(17 * fs_d / f))
        assert int(ln[b]) == N and N <= 2048
        n = np.arange(N)
        w = [0.5 - 0.5 * mpmath.cos(2 * mpmath.pi * (int(i) + 1) / (N + 1)) for i in n]
        phi = [2 * mpmath.pi * f * (int(i) - (N - 1)) / fs_d for i in n]
        err_re = max(abs(int(kern[at + i, 0]) - 16384 * w[i] * mpmath.cos(phi[i])) for i in range(N))
        err_im = max(abs(int(kern[at + i, 1]) + 16384 * w[i] * mpmath.sin(phi[i])) for i in range(N))
        assert err_re <= tol and err_im <= tol, (b, float(err_re), float(err_im))
        at += N
    assert at == kern.shape[0]


# ---- the slow and obvious restatement ----

def brute(case, x):
    """frame by frame, in Python integers"""
    c_fir, N, Kre, Kim = tm.tables(case.rate, case.D, case.Hc, case.O, case.f_lo_mhz)
    c_fir, Kre, Kim = [int(v) for v in c_fir], [[int(v) for v in k] for k in Kre], [[int(v) for v in k] for k in Kim]
    D, Hc, Tf, B = case.D, case.Hc, 8 * case.D, 12 * case.O
    q, d, out = [], [], []
    C_, hops, bad, c, hops_done = [0] * B, 0, 0, 0, 0
    qa = lambda i: q[i] if i >= 0 else 0
    da = lambda i: d[i] if i >= 0 else 0
    for t in range(case.n_ticks):
        for f in range(case.F):
            i = (t * case.F + f) * case.channels
            with np.errstate(all="ignore"):
                m = float(F32(x[i]) + F32(x[i + case.channels - 1]))
            if math.isnan(m) or math.isinf(m):
                bad += 1
                q.append(0)
            else:
                q.append(int(min(max(m, -2.0), 2.0) * 8192.0))   # exact in f64 as in f32; int() truncates
            frame = len(q) - 1
            if frame % D == 0:                                   # decimated frame frame / D is complete
                n = frame // D
                d.append(sum(c_fir[k] * qa(n * D - k) for k in range(Tf)) >> 15)
                if (n + 1) % Hc == 0:                            # and with it a hop
                    for b in range(B):
                        re = sum(Kre[b][j] * da(n - (N[b] - 1) + j) for j in range(N[b]))
                        im = sum(Kim[b][j] * da(n - (N[b] - 1) + j) for j in range(N[b]))
                        C_[b] += math.isqrt((re >> 10) ** 2 + (im >> 10) ** 2)
                    hops += 1
                    hops_done += 1
        c += 1
        if c % case.emit == 0:
            out.append((t, struct.pack("<7I", hops, bad, D, Hc, case.O, case.f_lo_mhz, 0) + struct.pack(f"<{B}Q", *C_)))
            C_, hops, bad = [0] * B, 0, 0
    return out


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.id)
def test_model_equals_the_frame_by_frame_restatement(case):
    x = tc.stream(case)
    got = run_model(case, x, case.n_ticks)
    want = brute(case, x)
    assert len(got) == len(want) == case.n_ticks // case.emit
    for a, b in zip(got, want):
        assert a == b, f"tick {a[0]} / {b[0]}"
    recs = [tm.parse_record(b"\0\0\0\0" + r) for _, r in got]
    assert sum(r["nonfinite"] for r in recs) > 0 and sum(r["hops"] for r in recs) >= 1 and any(r["cq"].any() for r in recs)


@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.id)
def test_runs_of_1_3_7_64_ticks_and_one_piece_give_identical_bytes(case):
    x = tc.stream(case)
    for cuts in (1, 3, 7, 64):
        assert run_model(case, x, cuts) == spec_records(case), cuts
    assert [t for t, _ in spec_records(case)] == list(range(case.emit - 1, case.n_ticks, case.emit))


def test_one_frame_ticks_emit_zero_tables_until_a_hop_completes():
    case = tc.by_id("one_frame")
    recs = [(t, tm.parse_record(b"\0\0\0\0" + r)) for t, r in spec_records(case)]
    early = [r for t, r in recs if t < 508]
    assert len(early) == 72 and all(r["hops"] == 0 and not r["cq"].any() for r in early)
    assert [r["hops"] for t, r in recs if t >= 508] == [1] + [0] * (len(recs) - 73) and recs[72][1]["cq"].any()


def test_the_tick_boundary_cases_sit_on_the_boundary():
    """hop 0's last input frame, 508, is tick 0's last frame (F = 509) or tick 1's first (F = 508)"""
    a = [tm.parse_record(b"\0\0\0\0" + r)["hops"] for _, r in spec_records(tc.by_id("last_frame_509"))]
    b = [tm.parse_record(b"\0\0\0\0" + r)["hops"] for _, r in spec_records(tc.by_id("first_frame_508"))]
    assert a[:2] == [1, 0] and b[:2] == [0, 1]


def test_the_long_kernel_reads_the_far_end_of_the_history():
    case = tc.by_id("long_kernel")
    assert tm.tables(case.rate, case.D, case.Hc, case.O, case.f_lo_mhz)[1][0] == 2040
    assert sum(tm.parse_record(b"\0\0\0\0" + r)["hops"] for _, r in spec_records(case)) == 4   # hop 3 ends at decimated frame 2047


# ---- accuracy of the model against an f64 evaluation ----

def test_model_against_an_f64_evaluation_within_the_derived_bound():
    """The same decimator and transform in f64 on benign input (no clamp, nothing non-finite), with the exact (unrounded) tables.  The bound
    on |M - M_exact| follows from the quantisation steps, in units of M (2^-10 of S):
      q    truncation: |q - 8192 m| < 1, so d's sum is off by less than sum |c| ... and c itself is off by at most 0.5 per tap from
           2^15 h / sum h, against |q| <= 2^14: in d's units (after >> 15) e_d <= (sum |c| x 1 + Tf x 0.5 x 2^14) / 2^15 + 1 (the floor)
      K    off by at most 0.5 per entry against |d| <= d_max, and d off by e_d against |K| <= 16384 w: per component of S
           e_S <= N (0.5 d_max + e_d x 16384 x mean(w)), with mean(w) = 1/2 for the Hann window, so e_S <= N (0.5 d_max + 8192 e_d)
      >>10 floor: less than 1 per component in M's units; the root of a sum of two squares moves by at most sqrt(2) x the larger component
           error; the final floor adds less than 1
    so |M - M_exact| <= sqrt(2) (e_S / 1024 + 1) + 1."""
    rate, D, Hc, O, f_lo_mhz, F, n_ticks = 48000, 8, 512, 5, 65406, 800, 30
    rng = np.random.default_rng(7)
    t = np.arange(F * n_ticks) / rate
    x = (0.3 * np.sin(2 * np.pi * 220.0 * t) + 0.2 * np.sin(2 * np.pi * 523.25 * t + 1.0) + 0.05 * rng.standard_normal(t.size)).astype(F32)
    m = tm.TonalityModel(rate, D, Hc, O, f_lo_mhz, n_ticks, 1)
    rec = tm.parse_record(m.run(x, n_ticks)[0])
    hops = rec["hops"]
    assert hops == F * n_ticks // D // Hc and rec["nonfinite"] == 0
    # f64: exact tables, no rounding anywhere
    Tf, fs_d = 8 * D, rate / D
    k = np.arange(Tf); tt = k - (Tf - 1) / 2
    h = np.sin(2 * np.pi * (0.45 / D) * tt) / (np.pi * tt) * (0.5 - 0.5 * np.cos(2 * np.pi * (k + 1) / (Tf + 1)))
    c = 32768.0 * h / h.sum()
    mid = (x.astype(np.float64) * 2.0) * 8192.0                 # m = x + x, exact in f32 for these values' doubling
    n_dec = -(-mid.size // D)
    padded = np.concatenate([np.zeros(Tf - 1), mid])
    d = np.array([np.dot(c[::-1], padded[n * D:n * D + Tf]) for n in range(n_dec)]) / 32768.0
    dpad = np.concatenate([np.zeros(2048), d])
    d_max = float(np.abs(d).max())
    sum_c = float(np.abs(m.c_fir).sum())
    e_d = (sum_c + Tf * 0.5 * 16384.0) / 32768.0 + 1.0
    worst = 0.0
    for b in range(12 * O):
        N = m.N[b]
        f = f_lo_mhz / 1000.0 * 2.0 ** (b / 12.0)
        n = np.arange(N)
        w = 0.5 - 0.5 * np.cos(2 * np.pi * (n + 1) / (N + 1))
        phi = 2 * np.pi * f * (n - (N - 1)) / fs_d
        exact = 0.0
        for hh in range(hops):
            e = (hh + 1) * Hc - 1
            seg = dpad[2048 + e - (N - 1):2048 + e + 1]
            exact += math.hypot(np.dot(16384 * w * np.cos(phi), seg), np.dot(-16384 * w * np.sin(phi), seg)) / 1024.0
        e_S = N * (0.5 * d_max + 8192.0 * e_d)
        bound = hops * (math.sqrt(2.0) * (e_S / 1024.0 + 1.0) + 1.0)
        err = abs(float(rec["cq"][b]) - exact)
        worst = max(worst, err / bound)
        assert err <= bound, (b, err, bound)
    print(f"worst |C - C_f64| / bound over {12 * O} bins: {worst:.4f}")
    assert float(rec["cq"].max()) > 1000 * hops   # the bound is small against the signal: the comparison says something


# ---- deliberate misreadings ----

@pytest.mark.parametrize("variant", tm.VARIANTS)
def test_every_misreading_is_caught_by_the_shared_cases(variant):
    """each variant changes one clause of the text; runs of 4 ticks, so that a counter reset per run shows"""
    caught = [case.id for case in tc.CASES if case.id != "one_frame" and run_model(case, tc.stream(case), 4, variant) != spec_records(case)]
    print(variant, "caught by", caught)
    assert caught, f"{variant} gives the spec's records on every shared case"
    if variant == "late_d":
        assert "last_frame_509" in caught
    if variant == "left_aligned":
        assert "short_50" in caught


def test_values_at_the_edges_of_the_quantiser():
    v = F32([2.0, 2.0000002, 1.9999999, 100.0, 3e38, 2.0 ** -13, 2.0 ** -14, 0.99999994 * 2.0 ** -13, 0.0, -0.0, -1.25, 1.5 * 2.0 ** -13, -2.0, -2.0000002, -1.9999999])
    q, bad = tm.quantise(v * F32(0.5), v * F32(0.5))
    assert q.tolist() == [16384, 16384, 16383, 16384, 16384, 1, 0, 0, 0, 0, -10240, 1, -16384, -16384, -16383] and not bad.any()
    q, bad = tm.quantise(F32([3e38, np.inf, np.nan, np.inf, 1.0, -0.7]), F32([3e38, 1.0, 1.0, -np.inf, 1.0, 0.69995]))
    assert bad.tolist() == [True, True, True, True, False, False] and q.tolist() == [0, 0, 0, 0, 16384, 0]   # -0.00005 x 8192 truncates to 0, not -1
    sub = np.array([1, 0x7fffff], np.uint32).view(F32)
    assert tm.quantise(sub, sub)[0].tolist() == [0, 0]


# ---- the key ----

KEY_CASES = [(rate, pc, minor) for rate in (48000, 44100) for pc, minor in ((0, False), (9, True), (6, False), (3, True))]


@pytest.mark.parametrize("rate,pc,minor", KEY_CASES, ids=lambda v: str(v))
def test_key_of_a_cadence(rate, pc, minor):
    """I-IV-V-I of four-harmonic tones, 8 s, D 8, Hc 512, O 5 from C2, through the model and both sets of helpers"""
    F = rate // 60
    x = tm.cadence(rate, pc, minor)
    n = x.size // F
    recs = tm.TonalityModel(rate, 8, 512, 5, 65406, 30, 1).run(x[:n * F], n)
    assert len(recs) == n // 30
    want, want_conf = tm.key(tm.chroma(recs, rate))
    ch = abi.tonality_chroma(recs, rate)
    got, conf = abi.tonality_key(ch)
    print(f"{rate} Hz {NAMES[pc]} {'minor' if minor else 'major'}: {NAMES[got % 12]} {'minor' if got >= 12 else 'major'}, confidence {conf:.3f}")
    assert got == want == pc + 12 * minor
    assert ch == pytest.approx(tm.chroma(recs, rate), rel=1e-12) and conf == pytest.approx(want_conf, rel=1e-9) and conf > 0 and abs(ch.sum() - 1) < 1e-12


def test_a_pure_tone_peaks_at_its_bin():
    rate, F, n = 48000, 800, 30
    for b in (0, 17, 33, 59):
        f = 65.406 * 2.0 ** (b / 12.0)
        x = (0.4 * np.sin(2 * np.pi * f * np.arange(n * F) / rate)).astype(F32)
        m = tm.TonalityModel(rate, 8, 512, 5, 65406, n, 1)
        rec = tm.parse_record(m.run(x, n)[0])
        assert int(np.argmax(rec["cq"])) == b, b
        ch = abi.tonality_chroma([m.run(x, n)[0]], rate)   # (the next 30 ticks of the same tone)
        assert int(np.argmax(ch)) == b % 12


# ---- helpers ----

def test_silence_and_nothing_but_nonfinite_frames_have_no_key():
    n_ticks, F = 12, 800
    for x in (np.zeros(n_ticks * F, F32), np.full(n_ticks * F, np.nan, F32), np.tile(F32([np.inf, -np.inf]), n_ticks * F // 2)):
        recs = tm.TonalityModel(48000, 4, 128, 2, 440000, 4, 1).run(x, n_ticks)
        ch = abi.tonality_chroma(recs, 48000.0)
        assert len(recs) == 3 and not ch.any() and abi.tonality_key(ch) == (-1, 0.0) == tm.key(ch)
        assert sum(tm.parse_record(r)["nonfinite"] for r in recs) == (0 if x[0] == 0 else n_ticks * F)
        assert sum(tm.parse_record(r)["hops"] for r in recs) == n_ticks * F // 4 // 128
    assert abi.tonality_key([1.0 / 12] * 12) == (-1, 0.0)


def test_key_first_maximum_rotations_and_refusals():
    for m in range(2):
        for t in range(12):
            ch = np.roll(np.array(tm.PROFILES[m]), t)
            k, conf = abi.tonality_key(ch / ch.sum())
            assert k == 12 * m + t and conf > 0.1 and tm.key(ch)[0] == k
    k, conf, ch = C.c_int(), C.c_double(), (C.c_double * 12)(*([0.0] * 11 + [1.0]))
    assert abi.lib.mx_tonality_key(ch, C.byref(k), C.byref(conf)) == abi.MX_OK and k.value >= 0
    assert abi.lib.mx_tonality_key(None, C.byref(k), C.byref(conf)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_tonality_key(ch, None, C.byref(conf)) == abi.MX_ERR_INVALID and abi.lib.mx_tonality_key(ch, C.byref(k), None) == abi.MX_ERR_INVALID
    for bad in (float("nan"), float("inf")):
        ch[3] = bad
        assert abi.lib.mx_tonality_key(ch, C.byref(k), C.byref(conf)) == abi.MX_ERR_INVALID


def test_chroma_folds_sums_and_refuses():
    O, B = 2, 24
    N = tm.tables(48000, 4, 128, O, 440000)[1]
    c1 = [0] * B; c1[0] = 5 * N[0]; c1[12] = 3 * N[12]; c1[4] = 2 * N[4]
    r1 = struct.pack("<8I", 2, 1, 0, 4, 128, O, 440000, 0) + struct.pack(f"<{B}Q", *c1)
    r2 = struct.pack("<8I", 5, 1, 7, 4, 128, O, 440000, 0) + struct.pack(f"<{B}Q", *c1)
    ch = abi.tonality_chroma([r1, r2], 48000.0)
    want = np.zeros(12); want[9] = 0.8; want[1] = 0.2                     # 440 Hz is an A: bin 0 and bin 12 fold to pitch class 9, bin 4 to C#
    assert ch == pytest.approx(want, abs=1e-15) and tm.chroma([r1, r2], 48000.0) == pytest.approx(want, abs=1e-15)
    big = struct.pack("<8I", 0, 1, 0, 4, 128, O, 440000, 0) + struct.pack(f"<{B}Q", *([2 ** 64 - 1] + [0] * (B - 1)))
    assert abi.tonality_chroma([big, big], 48000.0)[9] == 1.0             # summed as integers: no wrap
    out = (C.c_double * 12)()
    buf = C.create_string_buffer(r1 + r2, len(r1 + r2))
    call = abi.lib.mx_tonality_chroma
    assert call(buf, 2, 48000.0, out) == abi.MX_OK
    assert call(None, 2, 48000.0, out) == abi.MX_ERR_INVALID and call(buf, 0, 48000.0, out) == abi.MX_ERR_INVALID and call(buf, 2, 48000.0, None) == abi.MX_ERR_INVALID
    for rate in (0.0, -1.0, float("nan"), float("inf"), 250000.0):       # at 250 kHz N_0 = ceil(17 x 62500 / 440) > 2048
        assert call(buf, 2, rate, out) == abi.MX_ERR_INVALID, rate
    for head in ((4, 128, O, 440001), (8, 128, O, 440000), (4, 256, O, 440000)):   # the second record's header disagrees
        other = C.create_string_buffer(r1 + struct.pack("<8I", 5, 1, 7, *head, 0) + bytes(8 * B), len(r1) * 2)
        assert call(other, 2, 48000.0, out) == abi.MX_ERR_INVALID, head
    for head in ((3, 128, 2, 440000), (4, 100, 2, 440000), (4, 128, 1, 440000), (4, 128, 7, 440000), (4, 128, 2, 0), (0, 0, 0, 0)):   # not a record
        bad = C.create_string_buffer(struct.pack("<8I", 0, 0, 0, *head, 0) + bytes(8 * 72))
        assert call(bad, 1, 48000.0, out) == abi.MX_ERR_INVALID, head
    with pytest.raises(abi.MxError):
        abi.tonality_chroma([r1[:100]], 48000.0)   # shorter than its header says


def test_record_bytes_tables_sizes_and_parameter_errors():
    for D, Hc, O, f, e in ((4, 128, 2, 440000, 1), (8, 512, 5, 65406, 30), (8, 256, 6, 1, 1 << 31)):
        assert abi.tonality_record_bytes(D, Hc, O, f, e) == tm.record_bytes(O) == 32 + 96 * O and tm.check_params(D, Hc, O, f, e)
    n = C.c_size_t()
    fir, ln = (C.c_int16 * 64)(), (C.c_uint32 * 72)()
    for par in ((0, 128, 2, 440000, 1), (2, 128, 2, 440000, 1), (16, 128, 2, 440000, 1), (4, 64, 2, 440000, 1), (4, 1024, 2, 440000, 1), (4, 129, 2, 440000, 1),
                (4, 128, 1, 440000, 1), (4, 128, 7, 440000, 1), (4, 128, 2, 0, 1), (4, 128, 2, 440000, 0)):
        assert abi.lib.mx_tonality_record_bytes(C.byref(abi.TonalityParams(*par)), C.byref(n)) == abi.MX_ERR_INVALID, par
        assert abi.lib.mx_tonality_tables(48000.0, C.byref(abi.TonalityParams(*par)), fir, ln, None, C.byref(n)) == abi.MX_ERR_INVALID, par
        assert not tm.check_params(*par)
    ok = abi.TonalityParams(4, 128, 2, 440000, 1)
    assert abi.lib.mx_tonality_record_bytes(None, C.byref(n)) == abi.MX_ERR_INVALID and abi.lib.mx_tonality_record_bytes(C.byref(ok), None) == abi.MX_ERR_INVALID
    tables = abi.lib.mx_tonality_tables
    assert tables(48000.0, C.byref(ok), fir, ln, None, None) == abi.MX_OK and ln[0] == 464                 # sizes only, kern_pairs may be NULL
    assert tables(48000.0, C.byref(ok), fir, ln, None, C.byref(n)) == abi.MX_OK and n.value == sum(ln[:24])
    assert tables(48000.0, None, fir, ln, None, C.byref(n)) == abi.MX_ERR_INVALID and tables(48000.0, C.byref(ok), None, ln, None, C.byref(n)) == abi.MX_ERR_INVALID
    assert tables(48000.0, C.byref(ok), fir, None, None, C.byref(n)) == abi.MX_ERR_INVALID
    for rate in (0.0, -48000.0, float("nan"), float("inf")):
        assert tables(rate, C.byref(ok), fir, ln, None, C.byref(n)) == abi.MX_ERR_INVALID, rate
    assert tables(48000.0, C.byref(abi.TonalityParams(4, 128, 2, 99000, 1)), fir, ln, None, C.byref(n)) == abi.MX_ERR_INVALID    # N_0 = 2061
    assert tables(48000.0, C.byref(abi.TonalityParams(4, 128, 2, 99610, 1)), fir, ln, None, C.byref(n)) == abi.MX_OK and ln[0] == 2048
    assert tables(48000.0, C.byref(abi.TonalityParams(8, 128, 6, 65406, 1)), fir, ln, None, C.byref(n)) == abi.MX_ERR_INVALID    # the top bin at 3951 Hz, 0.45 fs_d = 2700 Hz
    parsed = abi.parse_tonality_records(np.frombuffer(struct.pack("<8I", 3, 9, 1, 4, 128, 2, 440000, 0) + struct.pack("<24Q", *range(24)), np.uint8), 2)
    assert len(parsed) == 1 and parsed[0]["tick_in_run"] == 3 and parsed[0]["hops"] == 9 and parsed[0]["f_lo_mhz"] == 440000 and parsed[0]["cq"].tolist() == list(range(24))


def test_header_carries_the_spec_and_constants_are_unchanged():
    assert C.sizeof(abi.TonalityParams) == 20 and [getattr(abi.TonalityParams, f).offset for f, _ in abi.TonalityParams._fields_] == [0, 4, 8, 12, 16]
    assert re.search(r"typedef struct \{ uint32_t decim /\*.*?\*/, hop_frames /\*.*?\*/, octaves /\*.*?\*/, f_lo_mhz /\*.*?\*/, emit_ticks /\*.*?\*/; \} mx_tonality_params;", HEADER)
    for p in (r"int mx_graph_set_tonality\(mx_graph\* g, const mx_port_ref\* ports, size_t n, const mx_tonality_params\* params\);",
              r"int mx_graph_read_tonality\(mx_graph\* g, void\* dst, size_t cap_bytes, uint32_t\* n_records\);",
              r"int mx_tonality_record_bytes\(const mx_tonality_params\* params, size_t\* bytes\);",
              r"int mx_tonality_tables\(double rate, const mx_tonality_params\* params, int16_t\* fir /\*.*?\*/, uint32_t\* len /\*.*?\*/,\s+int16_t\* kern /\*.*?\*/, size_t\* kern_pairs\);",
              r"int mx_tonality_chroma\(const void\* records, size_t n_records, double rate, double chroma\[12\]\);",
              r"int mx_tonality_key\(const double chroma\[12\], int\* key, double\* confidence\);"):
        assert re.search(p, HEADER), p
    spec = HEADER[HEADER.index("/* Tonality taps on audio output ports"): HEADER.index("} mx_tonality_params;")]
    for clause in ("m = L + R in f32, rounded once", "(int32_t)(fminf(fmaxf(m, -2.0f), 2.0f) * 8192.0f)", ">> 15", "sum |c[k]| <= 65534", "Q = 17",
                   "N_b = ceil(Q * fs_d / f_b)", "0.5 - 0.5 cos(2 pi (n + 1) / (N_b + 1))", "round(-16384 w_b[n] sin(phi))", "e_h = (h + 1) Hc - 1",
                   "floor(sqrt((S_re >> 10)^2 + (S_im >> 10)^2))", "c mod emit_ticks == 0", "Nothing is windowed", "tick_in_run", "nonfinite", "f_lo_mhz",
                   "32 + 8 B bytes", "BUILD-SPECIFIED", "tests/tonality_model.py", "resets every tap and c", "MX_FLAG_NO_FUSE", "2047 + Hc - 1"):
        assert clause in spec, clause
    names = ("mx_graph_set_tonality", "mx_graph_read_tonality", "mx_tonality_record_bytes", "mx_tonality_tables", "mx_tonality_chroma", "mx_tonality_key")
    for name in names:
        assert hasattr(abi.lib, name)
    note = HEADER[HEADER.index("#define MX_ABI_VERSION"): HEADER.index("/* ---- status codes")]
    assert "later, without a bump (only additions)" in note
    for name in ("mx_tonality_params",) + names:
        assert name in note, name
    # additions only: no version bump, no module kind
    assert re.search(r"#define\s+MX_ABI_VERSION\s+4u", HEADER) and abi.lib.mx_abi_version() == 4
    assert abi.KIND_COUNT == 19 and abi.PROFILE_KINDS == 18
    assert re.search(r"#define\s+MX_PROFILE_KINDS\s+18\b", HEADER) and re.search(r"MX_KIND_COUNT\s*=\s*19\b", HEADER)
