"""The limiter taps' spec without a GPU: the weights the library exports against the model's and against the exact quotient, the model's own
invariants (the guarantee, transparency, the gain's shape, independence of how a stream is cut into runs), a negative control, and the ABI
as the header declares it.  tests/test_gpu_limiter.py holds the device to the same model bit for bit."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import limiter_model as lm
from mixlab_amd import abi

HEADER = (pathlib.Path(__file__).resolve().parents[1] / "include" / "mixlab_gpu.h").read_text()
LOOKAHEADS = (0, 1, 2, 7, 64, 240, 512)
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- weights ----

@pytest.mark.parametrize("D", LOOKAHEADS)
def test_exported_weights_are_the_models(D):
    w = abi.limiter_weights(D)
    assert w.dtype == np.float32 and w.shape == (D + 1,)
    assert w.tobytes() == lm.weights(D).tobytes()
    assert (w > 0).all() and np.array_equal(w, w[::-1])   # a raised cosine without its zero end points
    if D == 0:
        assert w[0] == 1.0


@pytest.mark.parametrize("D", LOOKAHEADS)
def test_weights_are_correctly_rounded_every_entry(D):
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 60
    w = abi.limiter_weights(D)
    h = [1 - mpmath.cos(2 * mpmath.pi * (k + 1) / (D + 2)) for k in range(D + 1)]
    total = mpmath.fsum(h)
    for k in range(D + 1):
        q = h[k] / total
        near = F32(float(q))   # within an ulp of the answer: the nearest of it and its neighbours is the correctly rounded one
        want = min((near, np.nextafter(near, F32(2.0)), np.nextafter(near, F32(-1.0))), key=lambda v: abs(mpmath.mpf(float(v)) - q))
        assert w[k].view(np.uint32) == want.view(np.uint32), (D, k, w[k], want)


def test_weights_refusals():
    w = np.zeros(600, np.float32)
    assert abi.lib.mx_limiter_weights(513, w.ctypes.data) == abi.MX_ERR_INVALID
    assert abi.lib.mx_limiter_weights(1 << 31, w.ctypes.data) == abi.MX_ERR_INVALID
    assert abi.lib.mx_limiter_weights(4, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_limiter_weights(512, w.ctypes.data) == abi.MX_OK and w[513:].sum() == 0
    with pytest.raises(abi.MxError):
        abi.limiter_weights(513)


# ---- the guarantee ----

def hostile(seed, n, c, channels):
    """seeded noise at +12 dB over c with louder bursts, +-Inf, NaN, subnormals and values above 65536, flat in the port's layout"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n * channels) * (4.0 * c)).astype(F32)
    for _ in range(6):
        at = int(rng.integers(0, n * channels - 40))
        x[at:at + 40] *= F32(30.0)
    idx = rng.choice(n * channels, 24, replace=False)
    x[idx[0:3]] = np.inf; x[idx[3:6]] = -np.inf; x[idx[6:9]] = np.nan
    x[idx[9:12]] = np.array([1, 77, 0x7fffff], np.uint32).view(F32)            # subnormals
    x[idx[12:15]] = F32(-1e-41)
    x[idx[15:24]] = np.array([65536.5, -70000.0, 1e9, -3e38, 3.4e38, 65537.0, -65536.0, 131072.0, 1e20], F32)
    return x


def recount(x, y, g, c, n_ticks, channels):
    """the record from the samples alone"""
    F = len(g) // n_ticks
    rec = np.zeros(n_ticks, lm.TICK_DTYPE)
    yb = (bits(y) & 0x7fffffff).reshape(n_ticks, F * channels)
    for t in range(n_ticks):
        rec["min_gain"][t] = g[t * F:(t + 1) * F].min()
        rec["peak_out"][t] = np.array([yb[t].max()], np.uint32).view(F32)[0]
        rec["limited"][t] = int((g[t * F:(t + 1) * F] < 1).sum())
    rec["frames"], rec["channels"] = F, channels
    return rec


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("D", LOOKAHEADS)
def test_no_output_exceeds_the_ceiling_and_the_record_is_a_plain_recount(D, channels):
    for c in (F32(0.5), F32(1.0), F32(2.0 ** -20), F32(0.70794576)):
        n_ticks, F = 5, 801
        x = hostile(100 + D, n_ticks * F, float(c), channels)
        m = lm.LimiterModel(float(c), D, channels)
        y, rec = m.run(x, n_ticks)
        assert y.shape == x.shape
        assert ((bits(y) & 0x7fffffff) <= bits(c)).all(), "an output above the ceiling"
        want = recount(x, y, m.last_gain, c, n_ticks, channels)
        delayed = np.concatenate([np.zeros(D * channels, F32), x])[:len(x)]   # the samples the outputs were made of
        want["nonfinite"] = (~np.isfinite(delayed)).reshape(n_ticks, -1).sum(axis=1)
        assert lm.records_equal(rec, want), lm.first_difference(rec, want)
        assert rec["limited"].sum() > F and rec["nonfinite"].sum() > 0 and (rec["peak_out"] <= c).all()
        assert (y[~np.isfinite(delayed)].view(np.uint32) == 0).all()          # a replaced sample is +0.0


def test_ceiling_and_lookahead_ranges():
    for c, D in ((1.5, 4), (0.0, 4), (2.0 ** -21, 4), (0.5, 513), (0.5, -1)):
        with pytest.raises(AssertionError):
            lm.LimiterModel(c, D, 2)


# ---- transparency ----

@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("D", LOOKAHEADS)
def test_a_stream_within_the_ceiling_comes_out_delayed_bit_for_bit(D, channels):
    c = F32(0.25)
    rng = np.random.default_rng(D)
    n_ticks, F = 4, 735
    x = (rng.uniform(-1.0, 1.0, n_ticks * F * channels) * 0.25).astype(F32)
    x[::97] = c; x[5::101] = -c                                     # |x| == c exactly
    x[3::89] = np.array([5], np.uint32).view(F32)[0]                # a subnormal, and both zeros
    x[7::83] = F32(-0.0); x[11::79] = F32(0.0)
    assert (np.abs(x) <= c).all()
    m = lm.LimiterModel(float(c), D, channels)
    out = []
    for t in range(n_ticks):
        y, rec = m.run(x[t * F * channels:(t + 1) * F * channels], 1)
        assert rec["min_gain"][0] == 1.0 and rec["limited"][0] == 0 and rec["nonfinite"][0] == 0
        out.append(y)
    want = np.concatenate([np.zeros(D * channels, F32), x])[:len(x)]
    assert np.concatenate(out).tobytes() == want.tobytes()


# ---- the gain's shape ----

# Worst deviation of the model's g from the f64 evaluation in the case below, per D, in units of 2^-25 (against derived bounds of 5, 6, 7, 12,
# 69, 245 and 517: the roundings mostly cancel).  The bound asserted beside the derived one is twice the worst.
SHAPE_WORST_2P25 = {0: 0.0, 1: 1.0, 2: 0.5, 7: 2.47, 64: 2.79, 240: 11.07, 512: 26.32}


@pytest.mark.parametrize("D", LOOKAHEADS)
def test_gain_around_one_peak_follows_the_overlapped_weights(D):
    """One sample of height A > c at frame p in a sine below c.  m is rho = f32(c / A) on frames p .. p + D and 1 elsewhere, so
    s[n] = sum w - (1 - rho) x (the sum of the w[k] with p <= n - k <= p + D), and g = min(s, r[n - D]) wherever that sum is not empty.

    Tolerance against the f64 evaluation 1 - (1 - rho) sum_overlap w[k] (the f32 w[k] and rho, summed in f64), derived:
      - each of the D + 1 products w[k] m[n - k] rounds by at most 2^-24 relative; the products add up to at most sum w, so together 2^-24;
      - each of the D + 1 additions rounds a partial sum below 1 by at most half an ulp of [0.5, 1): 2^-25 each;
      - the f64 evaluation starts from 1 where the kernel's terms start from sum w; every w[k] is within 2^-24 relative of the exact weight and
        the exact weights add to 1: 2^-24.
    Together (D + 1 + 2 + 2) x 2^-25 = (D + 5) x 2^-25."""
    c, A, n, p = F32(0.5), F32(1.7), 4 * D + 300, 2 * D + 100
    x = (0.45 * np.sin(0.05 * np.arange(n))).astype(F32)
    x[p] = A
    m = lm.LimiterModel(float(c), D, 1)
    y, rec = m.run(x, 1)
    g = m.last_gain
    rho, w = float(c / A), lm.weights(D).astype(np.float64)
    want = np.ones(n)
    for f in range(n):
        ks = [k for k in range(D + 1) if p <= f - k <= p + D]
        if ks:
            want[f] = 1.0 - (1.0 - rho) * sum(w[k] for k in ks)
    want[p + D] = min(want[p + D], rho)
    tol = (D + 5) * 2.0 ** -25
    worst = float(np.abs(g.astype(np.float64) - want).max())
    print(f"D {D}: worst |g - f64| {worst / 2.0 ** -25:.2f} x 2^-25 (derived bound {D + 5})")
    assert worst <= tol
    assert worst <= 2 * SHAPE_WORST_2P25[D] * 2.0 ** -25
    assert (g[:p] == 1.0).all() and (g[p + 2 * D + 1:] == 1.0).all()           # exactly transparent beyond 2 D frames
    assert g[p + D] == g.min() and g[p + D] <= F32(rho)                         # the minimum is on the frame that outputs the peak
    assert y[p + D] == F32(A) * g[p + D] <= c and rec["limited"][0] == (2 * D + 1 if D else 1)
    if D >= 7:   # a smooth dip: falling to the peak, rising after it
        assert (np.diff(g[p:p + D + 1].astype(np.float64)) <= tol).all() and (np.diff(g[p + D:p + 2 * D + 1].astype(np.float64)) >= -tol).all()


# ---- independence of the grouping into runs ----

@pytest.mark.parametrize("F,D,channels", [(735, 240, 2), (800, 512, 1), (1, 64, 2), (37, 64, 1), (100, 7, 2), (5, 0, 1)])
def test_tick_by_tick_in_runs_and_in_one_piece_give_identical_bits(F, D, channels):
    n_ticks = 192 if F < 100 else 66
    x = hostile(7, n_ticks * F, 0.5, channels)
    results = []
    for run in (n_ticks, 1, 3, 64):
        m = lm.LimiterModel(0.5, D, channels)
        ys, recs, at = [], [], 0
        while at < n_ticks:
            k = min(run, n_ticks - at)
            y, rec = m.run(x[at * F * channels:(at + k) * F * channels], k)
            ys.append(y); recs.append(rec); at += k
        results.append((np.concatenate(ys), np.concatenate(recs)))
    for y, rec in results[1:]:
        assert y.tobytes() == results[0][0].tobytes() and lm.records_equal(rec, results[0][1])
    assert results[0][1]["limited"].sum() > 0


# ---- negative control ----

def test_without_the_min_the_gain_alone_does_not_hold_the_ceiling():
    """Step 5's min is what makes x * g <= c hold by the gain itself, before step 6's clamp (which is a hard clip: where it acts it
    distorts).  With the clamp switched off in both, a steady level of 0.515625 against c = 0.5 -- r = c / a rounds so that a * r <= c --
    shows it: the smoothed sum alone rounds above r for D = 7, 64, 240 and 512 (a search over levels at development time; D <= 2 has too
    few terms to), the spec's gain never.  The guarantee inputs show the same for the larger D."""
    c, level = F32(0.5), F32(0.515625)
    exceeded = []
    for D in LOOKAHEADS:
        x = np.full(4 * D + 64, level, F32)
        y_spec, _ = lm.LimiterModel(0.5, D, 1, clamp=False).run(x, 1)
        y_var, _ = lm.LimiterModel(0.5, D, 1, guard_min=False, clamp=False).run(x, 1)
        assert (np.abs(y_spec) <= c).all(), D
        if (np.abs(y_var) > c).any():
            exceeded.append(D)
    assert exceeded == [7, 64, 240, 512]
    over = 0
    for D in (64, 240, 512):
        x = hostile(100 + D, 4005, 0.5, 1)
        y_var, _ = lm.LimiterModel(0.5, D, 1, guard_min=False, clamp=False).run(x, 1)
        delayed = np.concatenate([np.zeros(D, F32), x])[:len(x)]
        over += int(((np.abs(y_var) > c) & (np.abs(delayed) <= 65536.0)).sum())
    assert over > 0


# ---- constants and header ----

def test_record_layout_and_unchanged_constants():
    d = abi.LIMITER_TICK_DTYPE
    assert d.itemsize == 24 and [d.fields[n][1] for n in d.names] == [0, 4, 8, 12, 16, 20]
    assert d.names == ("min_gain", "peak_out", "limited", "nonfinite", "frames", "channels")
    assert "/* 24 bytes: min_gain 0, peak_out 4, limited 8, nonfinite 12, frames 16, channels 20 */" in HEADER
    assert C.sizeof(abi.LimiterParams) == 8 and abi.LimiterParams.ceiling.offset == 0 and abi.LimiterParams.lookahead.offset == 4
    assert re.search(r"typedef struct \{ float ceiling; uint32_t lookahead; \} mx_limiter_params;", HEADER)
    assert re.search(r"#define\s+MX_LIMITER_MAX_LOOKAHEAD\s+512u", HEADER) and abi.LIMITER_MAX_LOOKAHEAD == lm.MAX_LOOKAHEAD == 512
    for p in (r"int mx_graph_set_limiters\(mx_graph\* g, const mx_port_ref\* ports, size_t n, const mx_limiter_params\* params\);",
              r"int mx_graph_read_limiters\(mx_graph\* g, uint32_t first_tick_in_run, uint32_t n_ticks, mx_limiter_tick\* dst, size_t cap\);",
              r"int mx_graph_read_limited\(mx_graph\* g, size_t tap, uint32_t first_tick_in_run, uint32_t n_ticks, float\* samples, size_t cap, size_t\* n_samples\);",
              r"int mx_graph_read_limited_i16\(mx_graph\* g, size_t tap, uint32_t first_tick_in_run, uint32_t n_ticks, int16_t\* samples, size_t cap, size_t\* n_samples\);",
              r"int mx_graph_limited_device_ptr\(mx_graph\* g, size_t tap, void\*\* dev, size_t\* floats_per_tick\);",
              r"int mx_limiter_weights\(uint32_t lookahead, float\* w\);"):
        assert re.search(p, HEADER), p
    for name in ("mx_graph_set_limiters", "mx_graph_read_limiters", "mx_graph_read_limited", "mx_graph_read_limited_i16",
                 "mx_graph_limited_device_ptr", "mx_limiter_weights"):
        assert hasattr(abi.lib, name)
    note = HEADER[HEADER.index("#define MX_ABI_VERSION"): HEADER.index("/* ---- status codes")]
    assert "mx_graph_set_limiters" in note and "mx_limiter_weights" in note
    # additions only: no version bump, no module kind
    assert re.search(r"#define\s+MX_ABI_VERSION\s+4u", HEADER) and abi.lib.mx_abi_version() == 4
    assert abi.KIND_COUNT == 19 and abi.PROFILE_KINDS == 18
    assert re.search(r"#define\s+MX_PROFILE_KINDS\s+18\b", HEADER) and re.search(r"MX_KIND_COUNT\s*=\s*19\b", HEADER)
    assert abi.LIMITER_TILE == 2048


def test_i16_form_of_a_limited_copy_never_clamps():
    y = np.array([1.0, -1.0, 0.5, -0.5, 0.99999994, 3.0517578e-05, -0.0], F32)
    assert lm.to_i16(y).tolist() == [32767, -32767, 16383, -16383, 32766, 0, 0]
