"""The deck's sweep filter without a device (include/mixlab_gpu.h "FILTER"): the header's structs and entry points, the setting rules one
refusal a rule, mx_deck_filter_host against the model bit for bit over the shared cases and through the carried block, the design helpers against libm, the model
against the mathematics (the analytic response of each kind, exact rational arithmetic of the recurrence), what the header says follows -- on the model -- and that
the shared cases tell the model from each of a list of misreadings."""
import ctypes as C
import math
import pathlib
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import deck_filter_cases as fc
import deck_filter_model as fm
from deck_filter_model import BP, HP, LP, NOTCH, OFF, Filt, FilterModel

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_set_filter", "mx_deck_schedule_filter", "mx_deck_filter_check", "mx_deck_filter_state", "mx_deck_read_filter_state", "mx_deck_filter_design",
                "mx_deck_filter_knob", "mx_deck_filter_host", "mx_deck_debug_last_filter"}
FILTER_OFFSETS = {"kind": 0, "flags": 4, "g": 8, "k": 12, "wet": 16, "_pad": 20}
CARRY_OFFSETS = {"s": 0, "last": 32, "on": 56, "_pad": 60}


@pytest.fixture(scope="module")
def tables():
    from mixlab_amd import deck
    return np.stack([deck.deck_tables(b) for b in range(4)])


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def c_filt(f: Filt):
    from mixlab_amd import abi
    return abi.DeckFilter(f.kind, f.flags, f.g, f.k, f.wet, f.pad)


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    assert lay["mx_deck_filter"]["size"] == 24 and lay["mx_deck_filter"]["offsets"] == FILTER_OFFSETS
    assert lay["mx_deck_filter_carry"]["size"] == 64 and lay["mx_deck_filter_carry"]["offsets"] == CARRY_OFFSETS
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert [consts[f"MX_DECK_FILTER_{n}"] for n in ("LP", "HP", "BP", "NOTCH")] == [LP, HP, BP, NOTCH] == [0, 1, 2, 3]
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19   # additions only
    for name, want in (("MIN_G", 2.0 ** -12), ("MAX_G", 16.0), ("MIN_K", 0.05), ("MAX_K", 2.0)):
        assert float(re.search(rf"#define MX_DECK_FILTER_{name} ([0-9.]+)f", text).group(1)) == want
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_set_filter") == ["mx_deck*", "const mx_deck_filter*"]
    assert sig("mx_deck_schedule_filter") == ["mx_deck*", "uint32_t", "const mx_deck_filter*"]
    assert sig("mx_deck_filter_state") == ["const mx_deck*", "uint32_t*", "mx_deck_filter*"]
    assert sig("mx_deck_filter_design") == ["uint32_t", "double", "double", "double", "double", "mx_deck_filter*"]
    assert sig("mx_deck_filter_knob") == ["double", "double", "double", "mx_deck_filter*", "uint32_t*"]
    assert sig("mx_deck_filter_host")[1:3] == ["uint32_t", "uint32_t"] and sig("mx_deck_filter_host")[-1] == "mx_deck_filter_carry*"
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | {"mx_deck_filter", "mx_deck_filter_carry"}):
        assert re.search(rf"\b{name}\b", note), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}
    # the echo no longer names the filter as missing
    echo = text[text.index("---- ECHO"):text.index("---- FILTER")]
    assert "sweep filter" not in echo


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi
    assert C.sizeof(abi.DeckFilter) == 24 and {n: getattr(abi.DeckFilter, n).offset for n, _t in abi.DeckFilter._fields_} == FILTER_OFFSETS
    assert C.sizeof(abi.DeckFilterCarry) == 64 and {n: getattr(abi.DeckFilterCarry, n).offset for n, _t in abi.DeckFilterCarry._fields_} == CARRY_OFFSETS
    assert (abi.DECK_FILTER_LP, abi.DECK_FILTER_HP, abi.DECK_FILTER_BP, abi.DECK_FILTER_NOTCH) == (LP, HP, BP, NOTCH)
    assert (np.float32(abi.DECK_FILTER_MIN_G), np.float32(abi.DECK_FILTER_MAX_G), np.float32(abi.DECK_FILTER_MIN_K), np.float32(abi.DECK_FILTER_MAX_K)) == (fm.MIN_G, fm.MAX_G, fm.MIN_K, fm.MAX_K)
    assert float(abi.DECK_FILTER_MIN_K) == float(fm.MIN_K)


# ---- the setting rules: one refusal per rule, and the edges that pass ----
OK_SET = Filt(LP, 0.1, 0.5, 1.0)
below = lambda v: float(np.nextafter(np.float32(v), np.float32(-np.inf)))   # noqa: E731
above = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))    # noqa: E731
CHECKS = [(OK_SET, True), (OK_SET._replace(kind=NOTCH), True), (OK_SET._replace(kind=4), False), (OK_SET._replace(kind=1 << 31), False),
          (OK_SET._replace(flags=1), False), (OK_SET._replace(pad=1), False),
          (OK_SET._replace(g=float("nan")), False), (OK_SET._replace(k=float("inf")), False), (OK_SET._replace(wet=float("nan")), False), (OK_SET._replace(g=float("inf")), False),
          (OK_SET._replace(g=2.0 ** -12), True), (OK_SET._replace(g=below(2.0 ** -12)), False), (OK_SET._replace(g=16.0), True), (OK_SET._replace(g=above(16.0)), False),
          (OK_SET._replace(g=0.0), False), (OK_SET._replace(g=-0.1), False),
          (OK_SET._replace(k=0.05), True), (OK_SET._replace(k=below(0.05)), False), (OK_SET._replace(k=2.0), True), (OK_SET._replace(k=above(2.0)), False),
          (OK_SET._replace(wet=0.0), True), (OK_SET._replace(wet=1.0), True), (OK_SET._replace(wet=-1e-6), False), (OK_SET._replace(wet=above(1.0)), False)]


@pytest.mark.parametrize("f,ok", CHECKS)
def test_filter_check_refuses_what_each_rule_refuses(f, ok):
    from mixlab_amd import abi, deck
    assert (fm.check(f) is None) == ok
    if ok:
        deck.filter_check(c_filt(f))
    else:
        with pytest.raises(abi.MxError) as err:
            deck.filter_check(c_filt(f))
        assert err.value.code == abi.MX_ERR_INVALID


# ---- mx_deck_filter_host equals the model bit for bit, in one call and through the carried block ----
def filter_only(case, tables, split, mis=()):
    """the filter alone (no echo) over the case's deck samples: (port float32, FilterModel)"""
    total, deck_ev, filt_ev, _e = fc.flatten(case)
    xs, m, out, at = fc.deck_samples(case, tables), FilterModel(mis), [], 0
    for n in split:
        for t in range(at, at + n):
            if t in filt_ev:
                m.schedule(t - at, filt_ev[t])
        out.append(m.run(xs[at:at + n].reshape(-1), case.spt))
        at += n
    return np.concatenate(out), m


def host_run(case, tables, split):
    from mixlab_amd import deck
    xs, per_tick, carry, out, at = fc.deck_samples(case, tables), fc.settings_per_tick(case), None, [], 0
    for n in split:
        y, carry = deck.filter_host(xs[at:at + n].reshape(-1), case.spt, [c_filt(f) if f is not None else None for f in per_tick[at:at + n]], carry)
        out.append(y)
        at += n
    return np.concatenate(out), carry


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_filter_host_equals_the_model_bit_for_bit_whole_and_through_the_carried_block(case, tables):
    total = fc.flatten(case)[0]
    want, m = filter_only(case, tables, [total])
    for split in ([total], [5, total - 5], [1] * total):
        got, carry = host_run(case, tables, split)
        assert np.array_equal(bits(got), bits(want)), (case.name, split)
        assert np.array_equal(np.array(carry.s[:]).view(np.uint64), m.state4().view(np.uint64)), (case.name, split)
        assert bool(carry.on) == m.on and (carry.last.kind, carry.last.g, carry.last.k, carry.last.wet) == (m.set.kind, *(float(np.float32(v)) for v in (m.set.g, m.set.k, m.set.wet)))


def test_filter_host_refuses_bad_arguments():
    from mixlab_amd import abi, deck
    x = np.linspace(-1, 1, 64, dtype=np.float32)
    for spt, settings in ((0, [c_filt(OK_SET)]), (8, [c_filt(OK_SET), c_filt(OK_SET._replace(g=17.0)), None, None])):
        with pytest.raises(abi.MxError) as err:
            deck.filter_host(x[:len(settings) * spt * 2], spt, settings)
        assert err.value.code == abi.MX_ERR_INVALID
    bad = abi.DeckFilterCarry()
    bad.on = 2
    with pytest.raises(abi.MxError):
        deck.filter_host(x[:16], 8, [c_filt(OK_SET)], bad)


# ---- the design helpers ----
def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def test_filter_design_lies_within_one_f32_ulp_of_libm_and_refuses_what_falls_outside():
    from mixlab_amd import abi, deck
    rng = np.random.default_rng(23)
    for _ in range(300):
        rate = float(rng.choice([26460.0, 44100.0, 48000.0, 96000.0]))
        hz = float(np.exp(rng.uniform(np.log(10.0), np.log(0.47 * rate))))
        q = float(np.exp(rng.uniform(np.log(0.5), np.log(20.0))))
        f = deck.filter_design(BP, hz, q, rate, 0.75)
        assert ulps(f.g, math.tan(math.pi * hz / rate)) <= 1 and ulps(f.k, 1.0 / q) <= 1, (hz, q, rate)
        assert (f.kind, f.flags, f.wet, f._pad) == (BP, 0, 0.75, 0)
    for bad in ((LP, 24000.0, 1.0, 48000.0, 1.0), (LP, 0.0, 1.0, 48000.0, 1.0), (LP, 1.0, 1.0, 48000.0, 1.0), (LP, 23990.0, 1.0, 48000.0, 1.0), (LP, 1000.0, 0.49, 48000.0, 1.0),
                (LP, 1000.0, 21.0, 48000.0, 1.0), (LP, 1000.0, 1.0, 0.0, 1.0), (LP, 1000.0, 1.0, 48000.0, 1.5), (4, 1000.0, 1.0, 48000.0, 1.0), (LP, float("nan"), 1.0, 48000.0, 1.0)):
        with pytest.raises(abi.MxError) as err:     # (1 Hz: g under 2^-12; 23990 Hz: g above 16)
            deck.filter_design(*bad)
        assert err.value.code == abi.MX_ERR_INVALID, bad


def test_filter_knob_dead_zone_ends_monotone_cutoff_and_clamp():
    from mixlab_amd import abi, deck
    rate = 48000.0
    hz_of = lambda f: math.atan(f.g) * rate / math.pi   # noqa: E731
    for knob in (0.0, 1 / 128, -1 / 128, below(1 / 64), -below(1 / 64)):
        assert deck.filter_knob(knob, rate) is None
    first = deck.filter_knob(-1 / 64, rate)
    assert first is not None and first.kind == LP and deck.filter_knob(1 / 64, rate).kind == HP
    lo, hi = deck.filter_knob(-1.0, rate, 2.0), deck.filter_knob(1.0, rate, 2.0)
    assert (lo.kind, lo.wet, lo.k) == (LP, 1.0, 0.5) and abs(hz_of(lo) - 80.0) < 1e-3
    assert (hi.kind, hi.wet, hi.k) == (HP, 1.0, 0.5) and abs(hz_of(hi) - 8000.0) < 1e-1
    knobs = np.linspace(1 / 64, 1.0, 200)
    lp = [deck.filter_knob(-v, rate).g for v in knobs]
    hp = [deck.filter_knob(v, rate).g for v in knobs]
    assert all(a > b for a, b in zip(lp, lp[1:])) and all(a < b for a, b in zip(hp, hp[1:]))    # the low-pass closes, the high-pass opens, strictly
    assert abs(hz_of(deck.filter_knob(-1 / 64, rate)) - 20000.0 * (80.0 / 20000.0) ** (1 / 64)) < 1.0
    # the clamp: at 16 kHz the open end of the low-pass (18.3 kHz at the dead zone's edge) and the high-pass's top (8 kHz) both stop at 0.45 x rate = 7200 Hz
    assert ulps(deck.filter_knob(-1 / 64, 16000.0).g, math.tan(math.pi * 0.45)) <= 1 and ulps(deck.filter_knob(1.0, 16000.0).g, math.tan(math.pi * 0.45)) <= 1
    for bad in (1.0001, -1.5, float("nan")):
        with pytest.raises(abi.MxError):
            deck.filter_knob(bad, rate)


# ---- the model against the mathematics ----
def biquad(kind, g, k):
    """the filter as a ratio of polynomials in z, from H(s) with s = (z - 1) / (g (z + 1)): (b[3], a[3]) over the common denominator g^2 (z + 1)^2, highest power first"""
    p, q, c = np.array([1.0, -2.0, 1.0]), np.array([1.0, 0.0, -1.0]), np.array([1.0, 2.0, 1.0])     # (z - 1)^2, (z - 1)(z + 1), (z + 1)^2
    a = p + k * g * q + g * g * c
    b = {LP: g * g * c, BP: g * q, HP: p, NOTCH: p + g * g * c}[kind]
    return b / a[0], a / a[0]


def impulse_response(b, a, n):
    """the direct form in f64: another realisation than the state-variable one"""
    h, x1, x2, y1, y2 = np.zeros(n), 0.0, 0.0, 0.0, 0.0
    for i in range(n):
        x0 = 1.0 if i == 0 else 0.0
        y0 = b[0] * x0 + b[1] * x1 + b[2] * x2 - a[1] * y1 - a[2] * y2
        h[i], x2, x1, y2, y1 = y0, x1, x0, y1, y0
    return h


@pytest.mark.parametrize("kind", (LP, HP, BP, NOTCH))
def test_a_sine_through_each_kind_at_rest_reaches_the_analytic_amplitude_and_phase(kind):
    """The filter at rest is linear and time-invariant, y[n] = sum_m h[m] x[n - m], and the steady state of sin(w n) is |H| sin(w n + arg H) with H at
    s = j tan(w / 2) / g.  What the model gives differs from it by: the part of the sum the switch-on at n = 0 cut off, at most sum_{m > n} |h[m]| (|x| <= 1); the
    rounding of the input to f32, at most 2^-25 sum |h| (half an ulp below 1); the rounding of the output to f32, at most 2^-24 |y|; and f64 rounding, 2^-53 an
    operation, far below these.  h comes from the same H(s) in direct form; beyond the horizon M with r^M < 2^-60 (r the pole radius) it is below f64's sight.
    The wait is the first n whose cut-off part is under 2^-24."""
    g, k, w = float(np.float32(0.3)), float(np.float32(0.5)), 0.21
    b, a = biquad(kind, g, k)
    r = max(abs(z) for z in np.roots(a))
    assert r < 1
    M = int(math.ceil(-60 * math.log(2) / math.log(r)))
    h = np.abs(impulse_response(b, a, M))
    tail = np.cumsum(h[::-1])[::-1]                         # tail[n] = sum_{m >= n} |h[m]|
    wait = int(np.argmax(tail < 2.0 ** -24))
    s = 1j * math.tan(w / 2) / g
    H = {LP: 1.0, BP: s, HP: s * s, NOTCH: s * s + 1.0}[kind] / (s * s + k * s + 1.0)
    spt = wait + 256
    n = np.arange(2 * spt)
    x = np.sin(w * n).astype(np.float32)
    m = FilterModel()
    m.schedule(0, Filt(kind, g, k))
    y = m.run(np.stack([x, x], axis=1).reshape(-1), spt).reshape(-1, 2)[:, 0].astype(np.float64)
    want = abs(H) * np.sin(w * n + np.angle(H))
    at = slice(spt, 2 * spt)                                # the second tick: wet stands at 1, and spt > wait frames have passed
    tol = tail[wait] + 2.0 ** -25 * tail[0] + 2.0 ** -24 * abs(H) + 2.0 ** -53 * 32 * len(n) * (1.0 + tail[0])
    assert np.max(np.abs(y[at] - want[at])) <= tol, (np.max(np.abs(y[at] - want[at])), tol)
    assert abs(H) > 0.05 and tol < 1e-6                     # the comparison is not empty: eight digits of an amplitude that is there


@pytest.mark.parametrize("kind", (LP, HP, BP, NOTCH))
def test_the_first_32_samples_of_an_impulse_equal_exact_rational_arithmetic_within_the_rounding_of_the_operations(kind):
    """The same recurrence in fractions.  One frame is 13 f64 operations a channel on the way to s1, s2 and f (v3, two products and a sum for v1, two products and
    two sums for v2, two doublings and two differences, up to three more for f), each off by at most u = 2^-53 of its result, all results at most M in size; an error
    made on the way is at most doubled before it lands in the state (the coefficients a1, a2, a3 lie under 1), and one that landed in the state j frames ago has
    since gone through A^j, A the update matrix of (s1, s2).  So E[n] = sum_j |A^j| 32 u M (row-sum norms) bounds the state's error, and 2 E + 32 u M that of f."""
    g, k = Fraction(float(np.float32(0.3))), Fraction(float(np.float32(0.2)))
    d = 1 + g * (g + k)
    a1 = 1 / d
    a2, a3 = g * a1, g * g * a1
    A = np.array([[float(2 * a1 - 1), float(-2 * a2)], [float(2 * a2), float(1 - 2 * a3)]])
    norms = [float(np.max(np.sum(np.abs(np.linalg.matrix_power(A, j)), axis=1))) for j in range(64)]
    m = FilterModel()
    m.schedule(0, Filt(kind, float(g), float(k)))
    x = np.zeros((32, 2), np.float32)
    x[0] = (0.75, -0.5)
    y0 = m.run(x.reshape(-1), 32).reshape(-1, 2)            # tick 0: the impulse, wet fading in by n / 32 (exact in f64)
    s_mid = m.s.copy()
    y1 = m.run(np.zeros(64, np.float32), 32).reshape(-1, 2)  # tick 1: wet 1, y = (float)(x + (f - x)) = (float)f with x = 0
    y, u = np.concatenate([y0, y1]), 2.0 ** -53
    for c, x0 in ((0, Fraction(3, 4)), (1, Fraction(-1, 2))):
        s1, s2, E, M = Fraction(0), Fraction(0), 0.0, Fraction(0)
        for n in range(64):
            xx = x0 if n == 0 else Fraction(0)
            v3 = xx - s2
            v1 = a1 * s1 + a2 * v3
            v2 = s2 + (a2 * s1 + a3 * v3)
            s1, s2 = 2 * v1 - s1, 2 * v2 - s2
            f = {LP: v2, BP: v1, HP: (xx - k * v1) - v2, NOTCH: xx - k * v1}[kind]
            M = max(M, abs(v3), abs(v1), abs(v2), 2 * abs(v1), 2 * abs(v2), abs(s1), abs(s2), abs(f), abs(xx), abs(f - xx))
            E = sum(norms[:n + 1]) * 32 * u * float(M)
            want = xx + min(Fraction(n, 32), Fraction(1)) * (f - xx)
            assert abs(Fraction(float(y[n, c])) - want) <= abs(want) * Fraction(1, 1 << 24) + Fraction(2 * E + 32 * u * float(M)) + Fraction(1, 1 << 149), (kind, n, c)
            if n == 31:
                assert abs(Fraction(float(s_mid[2 * c])) - s1) <= E and abs(Fraction(float(s_mid[2 * c + 1])) - s2) <= E
        assert abs(Fraction(float(m.s[2 * c])) - s1) <= E and abs(Fraction(float(m.s[2 * c + 1])) - s2) <= E and E < 1e-12
    assert np.count_nonzero(y) > 100


# ---- what the header says follows, on the model ----
def test_the_result_does_not_depend_on_how_ticks_are_grouped_into_feeds(tables):
    for name in ("schedules inside a feed", "lp sweep 20 kHz to 80 Hz", "65 frames a tick", "echo-out under a closing low-pass"):
        case = fc.BY_NAME[name]
        (ref,), (ref_state,), _f, _e = fc.run_model(case, tables)
        for split in ([5, 7], [1] * 12):
            ports, states, _f, _e = fc.run_model(case, tables, split=split)
            assert np.array_equal(bits(np.concatenate(ports)), bits(ref)), (name, split)
            assert states[-1][:2] == ref_state[:2] and np.array_equal(states[-1][2].view(np.uint64), ref_state[2].view(np.uint64))


def test_with_wet_0_the_port_holds_the_decks_own_samples_as_numbers_and_the_state_moves_on(tables):
    case = fc.BY_NAME["wet 0"]
    (y,), (st,), _f, _e = fc.run_model(case, tables)
    x = fc.deck_samples(case, tables).reshape(-1)
    assert np.array_equal(y, x) and st[2].any()
    # ... a -0 the deck wrote comes back as +0: x + 0 * (f - x) is +0 for x = -0
    m = FilterModel()
    m.schedule(0, Filt(LP, 0.1, 0.5, 0.0))
    out = m.run(np.array([-0.0, -0.0, 0.5, -0.5], np.float32), 2)
    assert np.array_equal(bits(out), bits(np.array([0.0, 0.0, 0.5, -0.5], np.float32)))


def test_the_channels_never_meet(tables):
    case = fc.BY_NAME["lp sweep 20 kHz to 80 Hz"]
    x = fc.deck_samples(case, tables).reshape(-1, 2).copy()
    ev = fc.flatten(case)[2]

    def run(x):
        m = FilterModel()
        for t, f in ev.items():
            m.schedule(t, f)
        return m.run(x.reshape(-1), case.spt).reshape(-1, 2), m.s.copy()
    (y, s), other = run(x), x.copy()
    other[:, 1] = other[::-1, 1] * np.float32(0.5)
    y2, s2 = run(other)
    assert np.array_equal(bits(y[:, 0]), bits(y2[:, 0])) and np.array_equal(s[:2], s2[:2]) and not np.array_equal(y[:, 1], y2[:, 1])


def test_the_kind_can_change_without_touching_the_state(tables):
    case = fc.BY_NAME["63 frames a tick"]                          # low-pass until tick 8, then high-pass at the same g, k and wet
    x = fc.deck_samples(case, tables).reshape(-1)
    total, _d, ev, _e = fc.flatten(case)
    a, b = FilterModel(), FilterModel()
    for t, f in ev.items():
        a.schedule(t, f)
        b.schedule(t, f._replace(kind=LP) if f is not OFF else f)
    ya, yb = a.run(x, case.spt), b.run(x, case.spt)
    assert np.array_equal(a.s.view(np.uint64), b.s.view(np.uint64))
    assert np.array_equal(bits(ya[:8 * 63 * 2]), bits(yb[:8 * 63 * 2])) and not np.array_equal(ya[8 * 63 * 2:], yb[8 * 63 * 2:])


def test_a_deck_whose_play_flag_is_cleared_keeps_ringing(tables):
    case = fc.BY_NAME["ring-out"]
    (y,), _s, _f, _e = fc.run_model(case, tables)
    x = fc.deck_samples(case, tables)
    assert not x[4:].any()                                         # the deck writes zeros from tick 4 on ...
    ring = y.reshape(12, -1)[4:]
    assert all(np.max(np.abs(t)) > 1e-4 for t in ring)             # ... and the band-pass at Q = 20 is heard in every one of the eight ticks that follow


def test_the_subnormal_ring_out_passes_through_the_subnormals_into_zero(tables):
    case = fc.BY_NAME["subnormal ring-out"]
    (y,), _s, _f, _e = fc.run_model(case, tables)
    a = np.abs(y)
    assert np.count_nonzero((a > 0) & (a < np.finfo(np.float32).tiny)) > 100 and not y[-441 * 2:].any()


# ---- the misreadings ----
@pytest.mark.parametrize("mis", sorted(fc.SHOWN_BY))
def test_each_misreading_changes_samples_or_state_of_the_case_named_for_it(mis, tables):
    name, split = fc.SHOWN_BY[mis]
    case = fc.BY_NAME[name]
    ports, states, _f, _e = fc.run_model(case, tables, split=split)
    if mis == "echo_first":
        wrong, wrong_states, _f, _e = fc.run_model(case, tables, split=split, echo_first=True)
    else:
        wrong, wrong_states, _f, _e = fc.run_model(case, tables, mis=(mis,), split=split)
    differs = not np.array_equal(bits(np.concatenate(ports)), bits(np.concatenate(wrong)))
    differs = differs or not np.array_equal(states[-1][2].view(np.uint64), wrong_states[-1][2].view(np.uint64))
    assert differs, mis


def test_the_list_of_misreadings_is_the_models_and_one_at_the_seam():
    assert set(fc.SHOWN_BY) == set(fm.MISREADINGS) | {"echo_first"} and len(fc.SHOWN_BY) >= 10
