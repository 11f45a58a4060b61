"""The deck's reverb without a device (include/mixlab_gpu.h "REVERB"): the header's structs and entry points, the setting rules one refusal
a rule, mx_deck_reverb_host against the model bit for bit over the shared cases -- port, lines and carried block; whole, split and tick by tick --,
mx_deck_reverb_plan against the model's own cut, mx_deck_reverb_design against a Python restatement, what the header says follows -- on the model --, two physical
checks of the tank's energy whose bounds are derived from the gains, the delays and f32's 2^-24, and that the shared cases tell the model from each of a list of
misreadings."""
import ctypes as C
import math
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import deck_reverb_cases as rc
import deck_reverb_model as rm
from deck_reverb_model import OFF, Reverb, ReverbModel

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_set_reverb", "mx_deck_schedule_reverb", "mx_deck_reverb_check", "mx_deck_reverb_state", "mx_deck_read_reverb_lines", "mx_deck_reverb_plan",
                "mx_deck_reverb_host", "mx_deck_reverb_design", "mx_deck_debug_last_reverb"}
REVERB_OFFSETS = {"delay": 0, "diff": 32, "gain": 48, "send": 80, "dry": 84, "wet": 88, "damp": 92, "diffusion": 96, "flags": 100}
CARRY_OFFSETS = {"t": 0, "last": 8, "on": 112, "_pad": 116}


@pytest.fixture(scope="module")
def tables():
    from mixlab_amd import deck
    return np.stack([deck.deck_tables(b) for b in range(4)])


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def c_rev(r: Reverb):
    from mixlab_amd import abi
    return abi.DeckReverb((C.c_uint32 * 8)(*r.delay), (C.c_uint32 * 4)(*r.diff), (C.c_float * 8)(*r.gain), r.send, r.dry, r.wet, r.damp, r.diffusion, r.flags)


def as_tuple(r):
    """an abi.DeckReverb as the model's Reverb, floats as the f32 they are"""
    return Reverb(tuple(r.delay), tuple(r.diff), tuple(r.gain), r.send, r.dry, r.wet, r.damp, r.diffusion, r.flags)


def f32_tuple(r: Reverb):
    f = lambda v: float(np.float32(v))   # noqa: E731
    return Reverb(tuple(r.delay), tuple(r.diff), tuple(f(v) for v in r.gain), f(r.send), f(r.dry), f(r.wet), f(r.damp), f(r.diffusion), r.flags)


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    assert lay["mx_deck_reverb"]["size"] == 104 and lay["mx_deck_reverb"]["offsets"] == REVERB_OFFSETS
    assert lay["mx_deck_reverb_carry"]["size"] == 120 and lay["mx_deck_reverb_carry"]["offsets"] == CARRY_OFFSETS
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert [consts[f"MX_DECK_REVERB_{n}"] for n in ("MIN_DELAY", "MAX_DELAY", "MIN_DIFF", "MAX_DIFF", "TANK_RING", "DIFF_RING", "LINE_FLOATS")] == \
        [rm.MIN_DELAY, rm.MAX_DELAY, rm.MIN_DIFF, rm.MAX_DIFF, rm.TANK_RING, rm.DIFF_RING, rm.LINE_FLOATS] == [128, 12000, 64, 2000, 16384, 4096, 147456]
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19   # additions only
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_set_reverb") == ["mx_deck*", "const mx_deck_reverb*"]
    assert sig("mx_deck_schedule_reverb") == ["mx_deck*", "uint32_t", "const mx_deck_reverb*"]
    assert sig("mx_deck_reverb_state") == ["const mx_deck*", "uint64_t*", "uint32_t*", "mx_deck_reverb*"]
    assert sig("mx_deck_read_reverb_lines") == ["mx_deck*", "float*"]
    assert sig("mx_deck_reverb_design") == ["double"] * 8 + ["mx_deck_reverb*"]
    assert sig("mx_deck_reverb_host")[1:3] == ["uint32_t", "uint32_t"] and sig("mx_deck_reverb_host")[-2:] == ["float*", "mx_deck_reverb_carry*"]
    assert sig("mx_deck_reverb_plan")[0] == "uint32_t" and sig("mx_deck_reverb_plan")[2:] == ["uint32_t", "uint64_t*", "uint32_t", "uint32_t*"]
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | {"mx_deck_reverb", "mx_deck_reverb_carry"}):
        assert re.search(rf"\b{name}\b", note), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}
    # the echo no longer names the reverb as missing, and the reverb names what it leaves out
    echo = text[text.index("---- ECHO"):text.index("---- FILTER")]
    assert "interpolated delay, reverb," not in echo
    rev = text[text.index("---- REVERB"):text.index("#define MX_DECK_REVERB_MIN_DELAY")]
    for word in ("pre-delay", "modulated or interpolated", "one-pole damping", "bit-exact freeze", "other than a deck's source", "more than two channels"):
        assert word in rev, word


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi
    assert C.sizeof(abi.DeckReverb) == 104 and {n: getattr(abi.DeckReverb, n).offset for n, _t in abi.DeckReverb._fields_} == REVERB_OFFSETS
    assert C.sizeof(abi.DeckReverbCarry) == 120 and {n: getattr(abi.DeckReverbCarry, n).offset for n, _t in abi.DeckReverbCarry._fields_} == CARRY_OFFSETS
    assert (abi.DECK_REVERB_MIN_DELAY, abi.DECK_REVERB_MAX_DELAY, abi.DECK_REVERB_MIN_DIFF, abi.DECK_REVERB_MAX_DIFF) == (rm.MIN_DELAY, rm.MAX_DELAY, rm.MIN_DIFF, rm.MAX_DIFF)
    assert (abi.DECK_REVERB_TANK_RING, abi.DECK_REVERB_DIFF_RING, abi.DECK_REVERB_LINE_FLOATS) == (rm.TANK_RING, rm.DIFF_RING, rm.LINE_FLOATS)


# ---- the setting rules: one refusal per rule, and the edges that pass ----
OK_SET = rc.MID
above = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))    # noqa: E731


def with_at(r: Reverb, field: str, i: int, v):
    t = list(getattr(r, field))
    t[i] = v
    return r._replace(**{field: tuple(t)})


CHECKS = [(OK_SET, True), (rc.FLOOR, True), (rc.CEILING, True), (rc.DEFAULT, True),
          (with_at(OK_SET, "delay", 0, 127), False), (with_at(OK_SET, "delay", 7, 12001), False), (with_at(OK_SET, "delay", 3, 0), False),
          (with_at(OK_SET, "delay", 3, 128), True), (with_at(OK_SET, "delay", 3, 12000), True),
          (with_at(OK_SET, "diff", 0, 63), False), (with_at(OK_SET, "diff", 3, 2001), False), (with_at(OK_SET, "diff", 1, 64), True), (with_at(OK_SET, "diff", 2, 2000), True),
          (with_at(OK_SET, "gain", 5, float("nan")), False), (OK_SET._replace(send=float("inf")), False), (OK_SET._replace(dry=float("nan")), False),
          (OK_SET._replace(wet=float("inf")), False), (OK_SET._replace(damp=float("nan")), False), (OK_SET._replace(diffusion=float("nan")), False),
          (with_at(OK_SET, "gain", 0, 1.0), True), (with_at(OK_SET, "gain", 0, -1.0), True), (with_at(OK_SET, "gain", 7, above(1.0)), False), (with_at(OK_SET, "gain", 2, -above(1.0)), False),
          (OK_SET._replace(send=-1.0), True), (OK_SET._replace(send=above(1.0)), False),
          (OK_SET._replace(dry=-1.0), True), (OK_SET._replace(dry=-above(1.0)), False),
          (OK_SET._replace(wet=-4.0), True), (OK_SET._replace(wet=above(4.0)), False),
          (OK_SET._replace(damp=0.0), True), (OK_SET._replace(damp=1.0), True), (OK_SET._replace(damp=-1e-6), False), (OK_SET._replace(damp=above(1.0)), False),
          (OK_SET._replace(diffusion=0.0), True), (OK_SET._replace(diffusion=0.75), True), (OK_SET._replace(diffusion=-1e-6), False), (OK_SET._replace(diffusion=above(0.75)), False),
          (OK_SET._replace(flags=1), False), (OK_SET._replace(flags=1 << 31), False)]


@pytest.mark.parametrize("k", range(len(CHECKS)))
def test_reverb_check_refuses_what_each_rule_refuses(k):
    from mixlab_amd import abi, deck
    r, ok = CHECKS[k]
    assert (rm.check(r) is None) == ok
    if ok:
        deck.reverb_check(c_rev(r))
    else:
        with pytest.raises(abi.MxError) as err:
            deck.reverb_check(c_rev(r))
        assert err.value.code == abi.MX_ERR_INVALID


# ---- mx_deck_reverb_host equals the model bit for bit: port, lines and carried block; whole, split, tick by tick ----
def host_run(case, tables, split):
    from mixlab_amd import deck
    _p, _s, _l, inputs = rc.run_model(case, tables)
    xs, per_tick, lines, carry, out, at = np.concatenate(inputs).reshape(-1, case.spt * 2), rc.settings_per_tick(case), None, None, [], 0
    for n in split:
        y, lines, carry = deck.reverb_host(xs[at:at + n].reshape(-1), case.spt, [c_rev(r) if r is not None else None for r in per_tick[at:at + n]], lines, carry)
        out.append(y)
        at += n
    return np.concatenate(out), lines, carry


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_reverb_host_equals_the_model_bit_for_bit_whole_split_and_tick_by_tick(case, tables):
    total = rc.flatten(case)[0]
    ports, states, lines, _x = rc.run_model(case, tables)
    want, (t, on, st, _c), (want_lines, mask) = np.concatenate(ports), states[-1], lines[-1]
    for split in ([total], [5, total - 5], [1] * total):
        got, got_lines, carry = host_run(case, tables, split)
        assert np.array_equal(bits(got), bits(want)), (case.name, split)
        assert np.array_equal(bits(got_lines)[mask], bits(want_lines)[mask]), (case.name, split)
        assert (carry.t, bool(carry.on), carry._pad) == (t, on, 0) and as_tuple(carry.last) == f32_tuple(st), (case.name, split)


def test_reverb_host_refuses_bad_arguments_and_writes_nothing():
    from mixlab_amd import abi, deck
    x = np.linspace(-1, 1, 64, dtype=np.float32)
    for spt, settings in ((0, [c_rev(OK_SET)]), (8, [c_rev(OK_SET), c_rev(with_at(OK_SET, "delay", 0, 100)), None, None])):
        with pytest.raises(abi.MxError) as err:
            deck.reverb_host(x[:len(settings) * spt * 2], spt, settings)
        assert err.value.code == abi.MX_ERR_INVALID
    bad = abi.DeckReverbCarry()
    bad.on = 2
    with pytest.raises(abi.MxError):
        deck.reverb_host(x[:16], 8, [c_rev(OK_SET)], None, bad)


# ---- mx_deck_reverb_plan against the model's own cut ----
def test_reverb_plan_equals_the_models_cut_on_every_case_and_on_random_schedules():
    from mixlab_amd import abi, deck
    for case in rc.CASES:
        per_tick = rc.settings_per_tick(case)
        reaches = [rm.reach(r) if r is not None else 0 for r in per_tick]
        assert deck.reverb_plan(case.spt, [c_rev(r) if r is not None else None for r in per_tick]) == rm.cut(case.spt, reaches), case.name
    rng = np.random.default_rng(5)
    pool = [rc.FLOOR, rc.STAGGER, rc.MID, rc.CEILING, rc.DEFAULT, None]
    crossing = 0
    for _ in range(200):
        spt, n = int(rng.choice([1, 16, 63, 64, 65, 441, 800, 2500])), int(rng.integers(1, 30))
        per_tick, cur = [], None
        for _k in range(n):
            if rng.random() < 0.4:
                cur = pool[int(rng.integers(len(pool)))]
            per_tick.append(cur)
        want = rm.cut(spt, [rm.reach(r) if r is not None else 0 for r in per_tick])
        assert deck.reverb_plan(spt, [c_rev(r) if r is not None else None for r in per_tick]) == want
        crossing += sum(1 for a, m in want if a // spt != (a + m - 1) // spt)
        # the rule itself: every frame of a block reads below the block's first, and one more frame would not (or the tick has no reverb, or the feed ends)
        for a, m in want:
            for g in (a, a + m - 1):
                assert g - rm.reach(per_tick[g // spt]) < a
            if a + m < n * spt and per_tick[(a + m) // spt] is not None:
                assert a + m - rm.reach(per_tick[(a + m) // spt]) >= a
    assert crossing > 100
    assert deck.reverb_plan(800, []) == []
    with pytest.raises(abi.MxError):
        deck.reverb_plan(0, [c_rev(OK_SET)])
    with pytest.raises(abi.MxError):
        deck.reverb_plan(800, [c_rev(with_at(OK_SET, "diff", 0, 10))])


# ---- the design helper ----
def ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def test_reverb_design_gives_the_restatements_integers_exactly_and_its_gains_within_one_f32_ulp():
    from mixlab_amd import abi, deck
    rng = np.random.default_rng(31)
    given = refused = 0
    for _ in range(300):
        rate = float(rng.choice([22050.0, 26460.0, 44100.0, 48000.0, 96000.0, 192000.0]))
        size = float(rng.uniform(0.2, 4.2)) if rng.random() < 0.8 else float(rng.choice([0.25, 4.0, 1.0]))
        t60 = float(np.exp(rng.uniform(np.log(0.05), np.log(30.0))))
        args = (rate, size, t60, float(rng.uniform(0, 1)), float(rng.uniform(0, 0.75)), float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)), float(rng.uniform(-4, 4)))
        want = rm.design(*args)
        if want is None:
            with pytest.raises(abi.MxError) as err:
                deck.reverb_design(*args)
            assert err.value.code == abi.MX_ERR_INVALID
            refused += 1
            continue
        got = as_tuple(deck.reverb_design(*args))
        assert (got.delay, got.diff, got.flags) == (want.delay, want.diff, 0), args
        assert all(ulps(a, b) <= 1 for a, b in zip(got.gain, want.gain)), args
        assert (got.send, got.dry, got.wet, got.damp, got.diffusion) == (want.send, want.dry, want.wet, want.damp, want.diffusion)
        assert all(rm.is_prime(d) for d in got.delay + got.diff) and len(set(got.delay)) == 8
        given += 1
    assert given > 100 and refused > 30
    d = as_tuple(deck.reverb_design(48000.0, 1.0, 2.0, 0.3, 0.5, 1.0, 1.0, 0.5))
    assert d.delay == (1087, 1283, 1447, 1663, 1871, 2053, 2281, 2477) and d.diff == (229, 613, 241, 587) == rc.DEFAULT.diff     # the bases are primes
    for bad in ((0.0, 1.0, 2.0), (48000.0, 0.2, 2.0), (48000.0, 4.1, 2.0), (48000.0, 1.0, 0.0), (float("nan"), 1.0, 2.0), (192000.0, 2.0, 2.0), (4000.0, 0.25, 2.0)):
        with pytest.raises(abi.MxError):     # (192 kHz at size 2: the last delay would be 19 816 frames; 4 kHz at size 1/4: the first would be 23)
            deck.reverb_design(*bad, 0.3, 0.5, 1.0, 1.0, 0.5)
    with pytest.raises(abi.MxError):
        deck.reverb_design(48000.0, 1.0, 2.0, 0.3, 0.8, 1.0, 1.0, 0.5)     # a diffusion the check refuses


# ---- what the header says follows, on the model ----
def test_the_result_does_not_depend_on_how_ticks_are_grouped_into_feeds(tables):
    for name in ("schedules inside a feed", "reach lowered mid-feed", "65 frames a tick", "behind a filter and an echo"):
        case = rc.BY_NAME[name]
        (ref,), (ref_state,), ((ref_lines, mask),), _x = rc.run_model(case, tables)
        for split in ([5, 7], [1] * 12):
            ports, states, lines, _x = rc.run_model(case, tables, split=split)
            assert np.array_equal(bits(np.concatenate(ports)), bits(ref)), (name, split)
            assert states[-1][:3] == ref_state[:3] and np.array_equal(bits(lines[-1][0])[mask], bits(ref_lines)[mask])


def test_with_wet_0_and_dry_1_the_port_holds_the_decks_samples_as_numbers_and_the_lines_move_on(tables):
    case = rc.BY_NAME["wet 0"]
    (y,), _s, ((lines, mask),), _x = rc.run_model(case, tables)
    x = rc.deck_samples(case, tables).reshape(12, -1)
    assert np.array_equal(y.reshape(12, -1)[1:], x[1:]) and lines[mask].any()          # (tick 0 fades dry in from 0: RAMPS)
    assert not np.array_equal(y.reshape(12, -1)[0], x[0])


def test_with_all_gains_0_and_no_diffusion_the_wet_signal_is_the_four_tap_delay_of_the_sent_input(tables):
    case = rc.BY_NAME["gain 0 multi-tap"]
    (y,), _s, _l, _x = rc.run_model(case, tables)
    r = rc.settings_per_tick(case)[0]
    spt, x = case.spt, rc.deck_samples(case, tables).reshape(-1, 2)
    n = np.arange(len(x))
    ramp = np.where(n < spt, n / spt, 1.0)                                        # tick 0 fades send, dry and wet in; exact in f64, then one rounding to f32
    send = (np.float64(np.float32(r.send)) * ramp).astype(np.float32).astype(np.float64)
    dry = (np.float64(np.float32(r.dry)) * ramp).astype(np.float32).astype(np.float64)
    wet = (np.float64(np.float32(r.wet)) * ramp).astype(np.float32).astype(np.float64)
    want = np.zeros_like(x)
    for c in (0, 1):
        sent = (send * x[:, c].astype(np.float64)).astype(np.float32).astype(np.float64)
        u = np.concatenate([np.zeros(r.diff[2 * c] + r.diff[2 * c + 1]), sent])[:len(x)]      # the two diffusers at diffusion 0: a pure delay
        tap = lambda D: np.concatenate([np.zeros(D), u])[:len(x)]   # noqa: E731
        o = 0.5 * ((tap(r.delay[c]) - tap(r.delay[c + 2])) + (tap(r.delay[c + 4]) - tap(r.delay[c + 6])))
        want[:, c] = (dry * x[:, c].astype(np.float64) + wet * o).astype(np.float32)
    assert np.array_equal(bits(y), bits(want)) and np.count_nonzero(y.reshape(-1, 2) != x) > 1000


def test_a_deck_whose_play_flag_is_cleared_keeps_sounding_its_tail(tables):
    case = rc.BY_NAME["reverb-out"]
    (y,), _s, _l, _x = rc.run_model(case, tables)
    x = rc.deck_samples(case, tables)
    assert not x[4:].any()                                         # the deck writes zeros from tick 4 on ...
    assert all(np.max(np.abs(t)) > 1e-3 for t in y.reshape(12, -1)[4:])     # ... and the two-second tail is heard in every one of the eight ticks that follow


def test_the_subnormal_ring_out_passes_through_the_subnormals_into_zero(tables):
    case = rc.BY_NAME["subnormal ring-out"]
    (y,), _s, ((lines, mask),), _x = rc.run_model(case, tables)
    a = np.abs(y)
    assert np.count_nonzero((a > 0) & (a < np.finfo(np.float32).tiny)) > 100 and not y[-800 * 2:].any()


# ---- two physical checks: bounds from the gains, the delays and f32's 2^-24 ----
def tank_energy(m: ReverbModel, r: Reverb) -> float:
    """the energy the tank holds at clock t: line i holds its last delay_i values"""
    return float(sum(np.sum(m.tank[max(0, m.t - r.delay[i]):m.t, i].astype(np.float64) ** 2) for i in range(8)))


def test_with_damp_0_the_energy_held_after_an_impulse_lies_between_the_bounds_of_the_gains_and_delays():
    """No diffusion, damp 0, one impulse on L and R.  Line i holds its last D_i values: those not yet read.  A frame reads f_i = r_i[t - D_i] out of that set and
    writes r_i[t] = C H (g o f) into it; C H is orthogonal, so the squares written sum to sum (g_i f_i)^2: every reading multiplies the energy it reads by a factor
    between gmin^2 and gmax^2 and hands it to lines that are read again D_j frames later.  Energy that entered at clock t1 has, by clock t, been read at most
    ceil((t - t1) / Dmin) times and at least floor((t - t1) / Dmax) - 1 times, so
        E0 gmin^(2 ceil((t - t1) / Dmin)) <= E(t) <= E0 gmax^(2 (floor((t - t1) / Dmax) - 1)).
    E0 is exact: the impulse stands in four lines a channel, unread.  Every line write rounds to f32, a relative 2^-24 at the most, so (1 +- 2^-24)^2 on its
    square; both bounds are widened by (1 +- 2^-22) for each of the at most ceil((t - t1) / Dmin) readings -- 2^-23 for the square, as much again for the f64
    operations of a frame (2^-53 each) and the products' second-order terms."""
    r = Reverb((211, 307, 401, 503, 601, 701, 809, 907), (64, 64, 64, 64), (0.9, 0.8, 0.95, 0.85, 0.9, 0.8, 0.95, 0.85), 1.0, 0.0, 1.0, 0.0, 0.0)
    spt = 128
    m = ReverbModel()
    m.schedule(0, r)
    m.run(np.zeros(spt * 2, np.float32), spt)                       # the fade-in tick passes in silence: every ramped value stands at its setting from tick 1 on
    x = np.zeros(spt * 2, np.float32)
    x[:2] = (0.75, -0.5)
    m.run(x, spt)
    m.run(np.zeros(spt * 2, np.float32), spt)                       # the impulse has left the diffusers (128 frames) and stands in the lines, not yet read (Dmin = 211 > 130)
    e0, t1 = tank_energy(m, r), 2 * spt                             # the impulse entered the lines at clock 256, the first frame of this tick
    assert e0 == 4 * (0.75 ** 2 + 0.5 ** 2)                         # four lines a channel hold the impulse whole
    gmin, gmax, dmin, dmax = float(np.float32(min(r.gain))), float(np.float32(max(r.gain))), min(r.delay), max(r.delay)
    for _ in range(40):
        m.run(np.zeros(spt * 2, np.float32), spt)
        most, least = math.ceil((m.t - t1) / dmin), max(0, (m.t - t1) // dmax - 1)
        lo = e0 * gmin ** (2 * most) * (1 - 2.0 ** -22) ** most
        hi = e0 * gmax ** (2 * least) * (1 + 2.0 ** -22) ** most
        e = tank_energy(m, r)
        assert lo <= e <= hi, (m.t, lo, e, hi)
    assert hi < 0.7 * e0 and lo > 0                                 # the bounds are not empty: by the end the upper one has fallen by a third


def test_with_all_gains_1_and_send_0_the_energy_stays_constant_within_the_accumulated_rounding():
    """Lossless: gain 1, damp 0, send 0 after the tank is filled.  Each frame reads eight values and writes eight whose squares sum to the same number, but for the
    rounding of each written value to f32 (relative 2^-24 at the most, so 2^-23 on its square; as much again covers the f64 operations and second-order terms).
    After T frames the energy has been rewritten at most ceil(T / Dmin) times: |E(T) / E0 - 1| <= (1 + 2^-22)^ceil(T / Dmin) - 1."""
    fill = Reverb((211, 307, 401, 503, 601, 701, 809, 907), (64, 64, 64, 64), (1.0,) * 8, 1.0, 0.0, 1.0, 0.0, 0.0)
    hold = fill._replace(send=0.0)
    spt = 256
    rng = np.random.default_rng(3)
    m = ReverbModel()
    m.schedule(0, fill)
    m.run(rng.uniform(-0.1, 0.1, spt * 2 * 4).astype(np.float32), spt)
    m.schedule(0, hold)
    m.run(np.zeros(spt * 2, np.float32), spt)                       # send ramps to 0 over this tick
    m.run(np.zeros(spt * 2, np.float32), spt)                       # ... and what the diffusers still held (128 frames) has entered the tank
    e0, t0 = tank_energy(m, hold), m.t
    assert e0 > 1.0
    for _ in range(30):
        m.run(np.zeros(spt * 2, np.float32), spt)
        passes = math.ceil((m.t - t0) / min(hold.delay))
        e = tank_energy(m, hold)
        assert abs(e / e0 - 1.0) <= (1 + 2.0 ** -22) ** passes - 1, (m.t, e / e0 - 1.0)
    assert (1 + 2.0 ** -22) ** passes - 1 < 1e-5                    # the bound is not empty: five digits of the energy after 37 passes


# ---- the misreadings ----
@pytest.mark.parametrize("mis", sorted(rc.SHOWN_BY))
def test_each_misreading_changes_samples_or_lines_of_the_case_named_for_it(mis, tables):
    name, split = rc.SHOWN_BY[mis]
    case = rc.BY_NAME[name]
    ports, _s, lines, _x = rc.run_model(case, tables, split=split)
    if mis == "reverb_first":
        wrong, _s, wrong_lines, _x = rc.run_model(case, tables, split=split, reverb_first=True)
    else:
        wrong, _s, wrong_lines, _x = rc.run_model(case, tables, mis=(mis,), split=split)
    differs = not np.array_equal(bits(np.concatenate(ports)), bits(np.concatenate(wrong)))
    mask = lines[-1][1] & wrong_lines[-1][1]
    differs = differs or not np.array_equal(bits(lines[-1][0])[mask], bits(wrong_lines[-1][0])[mask])
    assert differs, mis


def test_the_list_of_misreadings_is_the_models_and_one_at_the_seam():
    assert set(rc.SHOWN_BY) == set(rm.MISREADINGS) | {"reverb_first"} and len(rc.SHOWN_BY) >= 14
