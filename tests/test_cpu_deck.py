"""The deck without a device (include/mixlab_gpu.h "the deck"): the header's structs and entry points, the coefficient tables against an
mpmath evaluation of the header's formula, the host state machine mx_deck_plan against the Python model tick by tick, the parameter rules and the step helper at
their boundaries, the properties the header promises (transparency at unity, a tone played at another speed), that the shared cases tell the model from each of a
list of misreadings, and that they draw every form of the kernel's launch plan."""
import ctypes as C
import math
import pathlib
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import deck_cases as dc
import deck_model as dm
from deck_model import LOOP, ONE, PLAY, Head, Params

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_create", "mx_deck_destroy", "mx_deck_load_i16", "mx_deck_set", "mx_deck_seek", "mx_deck_schedule", "mx_deck_check", "mx_deck_plan", "mx_deck_feed",
                "mx_deck_read_ticks", "mx_deck_state", "mx_deck_step", "mx_deck_tables", "mx_deck_debug_last_feed"}
PARAMS_OFFSETS = {"step_q32": 0, "slew_q32": 8, "loop_in": 16, "loop_out": 24, "flags": 32, "_pad": 36}
HEAD_OFFSETS = {"pos_q32": 0, "step_q32": 8, "params": 16, "last_loop_in": 56, "last_loop_out": 64, "last_looping": 72, "_pad": 76}
TICK_OFFSETS = {"pos_q32": 0, "step_q32": 8, "dstep_q32": 16, "loop_in": 24, "loop_len": 32, "flags": 40, "bank": 44}


@pytest.fixture(scope="module")
def tables():
    from mixlab_amd import deck
    return np.stack([deck.deck_tables(b) for b in range(4)])


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    assert lay["mx_deck_params"]["size"] == 40 and lay["mx_deck_params"]["offsets"] == PARAMS_OFFSETS
    assert lay["mx_deck_head"]["size"] == 80 and lay["mx_deck_head"]["offsets"] == HEAD_OFFSETS
    assert lay["mx_deck_tick"]["size"] == 48 and lay["mx_deck_tick"]["offsets"] == TICK_OFFSETS
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert [consts[n] for n in ("MX_DECK_PLAY", "MX_DECK_LOOP", "MX_DECK_TICK_PLAY", "MX_DECK_TICK_LOOPING", "MX_DECK_TICK_BEFORE", "MX_DECK_TICK_PAST")] == [1, 2, 1, 2, 4, 8]
    assert [consts[n] for n in ("MX_DECK_TAPS", "MX_DECK_PHASES", "MX_DECK_BANKS", "MX_DECK_CHUNK", "MX_DECK_MAX_SPT")] == [32, 256, 4, dc.CHUNK, 1 << 20]
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # a feeder: not a module kind, not a profile kind, no new ABI version
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared) and "mx_deck" in h.opaque
    assert [c for _n, c, _a in declared["mx_deck_plan"][2]] == ["const mx_deck_head*", "const mx_deck_params*", "const int64_t*", "uint32_t", "uint64_t", "mx_deck_tick*", "mx_deck_head*"]
    assert [c for _n, c, _a in declared["mx_deck_feed"][2]] == ["mx_deck*const*", "const uint32_t*", "size_t", "mx_graph*", "uint32_t"]
    assert [c for _n, c, _a in declared["mx_deck_schedule"][2]] == ["mx_deck*", "uint32_t", "const mx_deck_params*", "const int64_t*"]
    assert [c for _n, c, _a in declared["mx_deck_step"][2]] == ["uint32_t", "uint32_t", "double", "int64_t*"]
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | {"mx_deck_params", "mx_deck_head", "mx_deck_tick"}):
        assert re.search(rf"\b{name}\b", note), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi
    for st, size, offs in ((abi.DeckParams, 40, PARAMS_OFFSETS), (abi.DeckHead, 80, HEAD_OFFSETS), (abi.DeckTick, 48, TICK_OFFSETS)):
        assert C.sizeof(st) == size and {n: getattr(st, n).offset for n, _t in st._fields_} == offs
    assert (abi.DECK_CHUNK, abi.DECK_MAX_SPT, abi.DECK_PLAY, abi.DECK_LOOP) == (dc.CHUNK, dm.MAX_SPT, PLAY, LOOP)
    assert abi.lib.mx_abi_version() == 4


# ---- the tables ----
def test_every_table_entry_is_the_nearest_f32_of_the_headers_formula(tables):
    """T[b][p][k] = g / (row sum of g), g(fc, x) = fc sinc(fc x) I0(9 sqrt(1 - (x / 16)^2)) / I0(9), at 50 digits; an entry passes when no neighbouring f32 is nearer"""
    import mpmath as mp
    mp.mp.dps = 50
    win = [[mp.besseli(0, 9 * mp.sqrt(1 - (mp.mpf((k - 15) * 256 - p) / 4096) ** 2)) / mp.besseli(0, 9) for k in range(32)] for p in range(257)]
    worst = mp.mpf(0)
    for b, fc in enumerate((mp.mpf(1), mp.mpf(3) / 4, mp.mpf(1) / 2, mp.mpf(1) / 4)):
        got = tables[b]
        for p in range(257):
            g = []
            for k in range(32):
                x = mp.mpf((k - 15) * 256 - p) / 256
                t = fc * x
                g.append(fc * (mp.sinpi(t) / (mp.pi * t) if t != 0 else 1) * win[p][k])
            s = mp.fsum(g)
            for k in range(32):
                v, have = g[k] / s, got[p, k]
                err = abs(v - mp.mpf(float(have)))
                for other in (np.nextafter(have, np.float32(np.inf)), np.nextafter(have, np.float32(-np.inf))):
                    assert err <= abs(v - mp.mpf(float(other))), (b, p, k, float(have), mp.nstr(v, 20))
                worst = max(worst, err / abs(v)) if v != 0 else worst
    assert worst < mp.mpf(2) ** -24   # (half an ulp at the most, relative)


def test_the_impulse_rows_are_exact_and_every_row_passes_dc(tables):
    e15, e16 = np.zeros(32, np.float32), np.zeros(32, np.float32)
    e15[15] = e16[16] = 1.0
    assert np.array_equal(tables[0][0], e15) and np.array_equal(tables[0][256], e16)
    assert np.abs(tables.astype(np.float64).sum(axis=2) - 1.0).max() < 32 * 2.0 ** -24   # each of 32 entries rounded once
    from mixlab_amd import abi, deck
    with pytest.raises(abi.MxError):
        deck.deck_tables(4)


# ---- the state machine ----
def c_params(p: Params):
    from mixlab_amd import abi
    return abi.DeckParams(p.step, p.slew, p.loop_in, p.loop_out, p.flags, 0)


def c_head(h: Head):
    from mixlab_amd import abi
    return abi.DeckHead(h.pos, h.step, c_params(h.params), h.last_loop_in, h.last_loop_out, 1 if h.last_looping else 0, 0)


def head_tuple(h):
    return (h.pos_q32, h.step_q32, h.params.step_q32, h.params.slew_q32, h.params.loop_in, h.params.loop_out, h.params.flags, h.last_loop_in, h.last_loop_out, h.last_looping)


def model_head_tuple(h: Head):
    return (h.pos, h.step, h.params.step, h.params.slew, h.params.loop_in, h.params.loop_out, h.params.flags, h.last_loop_in, h.last_loop_out, 1 if h.last_looping else 0)


def tick_tuple(t):
    return (t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank)


def walk(case):
    """the case through mx_deck_plan and through the model side by side: yields (label, library tick, model tick, library head, model head)"""
    from mixlab_amd import deck
    mh, ch = Head(), c_head(Head())
    for fi, f in enumerate(case.feeds):
        ev = {t: (p, s) for (t, p, s) in f.events}
        for t in range(f.n_ticks):
            p, s = ev.get(t, (None, None))
            want, mh = dm.plan(mh, p, s, case.spt, case.n_frames)
            got, ch = deck.deck_plan(ch, case.spt, case.n_frames, c_params(p) if p is not None else None, s)
            yield f"{case.name}: feed {fi} tick {t}", got, want, ch, mh


STREAMS = [dc.Case(f"stream {seed} at {spt}", spt, n, dc.random_stream(seed, n, n_feeds=6, max_ticks=8))
           for seed, spt, n in ((1, 735, 4097), (2, 800, 4097), (3, 1, 33), (4, 255, 31), (5, 256, 1), (6, 257, 100000), (7, 800, 1 << 30), (8, 1 << 20, 4097))]


@pytest.mark.parametrize("case", dc.CASES + STREAMS, ids=lambda c: c.name)
def test_plan_equals_the_model_on_every_field(case):
    for label, got, want, ch, mh in walk(case):
        assert tick_tuple(got) == tuple(want), label
        assert head_tuple(ch) == model_head_tuple(mh), label


def test_the_streams_and_cases_reach_every_rule_of_the_tick():
    """clamp at both ends, a slew that reaches its target and snaps, loop catch and release, seeks into and out of a loop, seek before params at one tick"""
    seen = set()
    for case in dc.CASES + STREAMS:
        prev, mh = None, Head()
        for f in case.feeds:
            ev = {t: (p, s) for (t, p, s) in f.events}
            for t in range(f.n_ticks):
                p, s = ev.get(t, (None, None))
                before = mh
                tick, mh = dm.plan(mh, p, s, case.spt, case.n_frames)
                lo, hi = -dm.MARGIN * ONE, (case.n_frames + dm.MARGIN) * ONE
                raw = s if s is not None else before.pos
                seen |= {"clamp low"} if raw < lo and tick.pos == lo else set()
                seen |= {"clamp high"} if raw > hi and tick.pos == hi else set()
                looping = bool(tick.flags & dm.T_LOOPING)
                if tick.flags & dm.T_PLAY and tick.dstep:
                    seen.add("slewing")
                if prev is not None and prev.dstep and tick.flags & dm.T_PLAY and not tick.dstep and tick.step == mh.params.step and p is None:
                    seen.add("slew snaps to its target")
                if looping and not before.last_looping:
                    seen.add("loop catches")
                if before.last_looping and not looping:
                    seen.add("loop releases")
                if s is not None and looping and p is None and not (tick.loop_in * ONE <= tick.pos < (tick.loop_in + tick.loop_len) * ONE):
                    seen.add("seek out of a loop that holds")
                if s is not None and looping and not before.last_looping:
                    seen.add("seek into a loop")
                if s is not None and p is not None and p.flags & LOOP and looping and not before.last_looping and not (p.loop_in * ONE <= before.pos < p.loop_out * ONE):
                    seen.add("seek applied before params")
                if tick.flags & dm.T_BEFORE:
                    seen.add("before")
                if tick.flags & dm.T_PAST:
                    seen.add("past")
                prev = tick
    assert seen >= {"clamp low", "clamp high", "slewing", "slew snaps to its target", "loop catches", "loop releases", "seek out of a loop that holds", "seek into a loop",
                    "seek applied before params", "before", "past"}, seen


def test_plan_refuses_what_the_header_says_it_refuses():
    from mixlab_amd import abi, deck
    h = c_head(Head())
    deck.deck_plan(h, 1, 1)
    deck.deck_plan(h, dm.MAX_SPT, dm.MAX_FRAMES)
    for spt, n in ((0, 10), (dm.MAX_SPT + 1, 10), (10, 0), (10, dm.MAX_FRAMES + 1)):
        with pytest.raises(abi.MxError):
            deck.deck_plan(h, spt, n)
    with pytest.raises(abi.MxError):
        deck.deck_plan(c_head(Head(step=4 * ONE + 1)), 10, 10)
    with pytest.raises(abi.MxError):
        deck.deck_plan(h, 10, 10, c_params(Params(step=4 * ONE + 1)))


# ---- the parameter rules and the step helper, at their boundaries ----
CHECKS = [(Params(4 * ONE), 1, True), (Params(-4 * ONE), 1, True), (Params(4 * ONE + 1), 1, False), (Params(-4 * ONE - 1), 1, False),
          (Params(0, 0), 1 << 30, True), (Params(0, 0), (1 << 30) + 1, False), (Params(0, 0), 0, False),
          (Params(0, 1 << 24), 5, True), (Params(0, (1 << 24) + 1), 5, False), (Params(0, -1), 5, False),
          (Params(0, 0, 0, 0, PLAY | LOOP | 4), 5, False), (Params(0, 0, 0, 0, 4), 5, False), (Params(0, 0, 9, 2, PLAY), 5, True),   # loop points are not looked at without LOOP
          (Params(0, 0, 0, 5, LOOP), 5, True), (Params(0, 0, 0, 6, LOOP), 5, False), (Params(0, 0, 4, 5, LOOP), 5, True), (Params(0, 0, 5, 5, LOOP), 5, False),
          (Params(0, 0, 3, 2, LOOP), 5, False), (Params(0, 0, -1, 2, LOOP), 5, False), (Params(0, 0, 0, 1, LOOP | PLAY), 1, True)]


@pytest.mark.parametrize("p,n,ok", CHECKS)
def test_check_at_the_boundaries(p, n, ok):
    from mixlab_amd import abi, deck
    assert (dm.check(p, n) is None) == ok
    if ok:
        deck.deck_check(c_params(p), n)
    else:
        with pytest.raises(abi.MxError) as e:
            deck.deck_check(c_params(p), n)
        assert e.value.code == abi.MX_ERR_INVALID
    bad_pad = c_params(Params())
    bad_pad._pad = 1
    with pytest.raises(abi.MxError):
        deck.deck_check(bad_pad, 5)


def exact_step(tr, gr, speed):
    return round(Fraction(speed) * tr * ONE / gr)   # Fraction's round: to nearest, ties to even


def test_step_is_the_nearest_q32_exactly():
    from mixlab_amd import abi, deck
    assert deck.deck_step(44100, 48000, 1.0) == 3946001203 == exact_step(44100, 48000, 1.0)
    assert deck.deck_step(48000, 48000, 1.0) == ONE and deck.deck_step(48000, 48000, -1.0) == -ONE and deck.deck_step(48000, 48000, 0.0) == 0
    rng = np.random.default_rng(5)
    for _ in range(2000):
        tr, gr = (int(v) for v in rng.choice([8000, 11025, 22050, 32000, 44100, 48000, 88200, 96000, 192000, 1, 4294967295], 2))
        speed = float(rng.choice([1.0, -1.0])) * float(rng.choice([rng.uniform(0, 4), 2.0 ** (1 / 12), 2.0 ** -40, 5e-324, 126.4 / 128.0]))
        want = exact_step(tr, gr, speed)
        if abs(want) <= 4 * ONE:
            assert deck.deck_step(tr, gr, speed) == want, (tr, gr, speed)
        else:
            with pytest.raises(abi.MxError):
                deck.deck_step(tr, gr, speed)
    # ties go to even: 2^-33 is half a unit, 3 * 2^-33 one and a half
    assert deck.deck_step(1, 1, 2.0 ** -33) == 0 and deck.deck_step(1, 1, 3 * 2.0 ** -33) == 2 and deck.deck_step(1, 1, -3 * 2.0 ** -33) == -2
    # the range ends at 4 * 2^32 exactly
    assert deck.deck_step(1, 1, 4.0) == 4 * ONE and deck.deck_step(1, 1, -4.0) == -4 * ONE and deck.deck_step(4, 1, 1.0) == 4 * ONE
    assert deck.deck_step(1, 1, math.nextafter(4.0, 5.0)) == 4 * ONE and deck.deck_step(1, 1, 4.0 + 2.0 ** -33) == 4 * ONE   # the RESULT is what is bounded; the tie goes to even
    for args in ((1, 1, 4.0 + 2.0 ** -33 + 2.0 ** -50), (1, 1, -(4.0 + 2.0 ** -33 + 2.0 ** -50)), (0, 1, 1.0), (1, 0, 1.0), (1, 1, math.inf), (1, 1, math.nan), (1, 1, 1e300), (4294967295, 1, 1.0)):
        with pytest.raises(abi.MxError):
            deck.deck_step(*args)


# ---- what the header promises ----
def test_unity_from_an_integer_position_is_the_track_bit_for_bit(tables):
    case = dc.BY_NAME["unity from frame 0"]
    (got, recs), = dc.run_model(case, tables)
    assert all(t.bank == 0 for t in recs)
    want = np.zeros((6 * 800, 2), np.float32)
    want[:4097] = dc.track(case).astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32))


def test_before_and_past_ticks_are_zeros_by_the_arithmetic_itself(tables):
    hit = 0
    for case in dc.CASES:
        for got, recs in dc.run_model(case, tables):
            for t, r in enumerate(recs):
                if r.flags & (dm.T_BEFORE | dm.T_PAST):
                    hit += 1
                    assert not got[t * 2 * case.spt:(t + 1) * 2 * case.spt].view(np.uint32).any(), (case.name, t)   # +0.0, bit for bit
    assert hit >= 4


# the error of a 997 Hz tone played at each speed against the f64 ideal of the same tone, in dB relative to the ideal's energy, measured FROM THE MODEL (48 kHz, half
# scale, i16 track, 12 ticks of 800 after 2 of run-in) and recorded in DESIGN.md section 0.15; asserted with 3 dB of margin.  A property of the header's filter and of a
# 16-bit track, not of any device.
TONE_DB = {2.0 ** (1 / 12): -92.2, 0.5: -91.2, 2.0: -94.0, 3.9: -84.1}


@pytest.mark.parametrize("speed", sorted(TONE_DB))
def test_a_tone_played_at_another_speed(tables, speed):
    from mixlab_amd import deck
    rate, spt, f0, amp, n_frames = 48000, 800, 997.0, 0.5, 60000
    tr = np.round(amp * 32768.0 * np.sin(2 * np.pi * f0 * np.arange(n_frames) / rate)).astype(np.int16)
    m = dm.DeckModel(np.stack([tr, tr], axis=1), tables)
    step = deck.deck_step(rate, rate, speed)
    m.schedule(0, Params(step, 0, 0, 0, PLAY), 100 * ONE)
    got, recs = m.feed(14, spt)
    got = got.reshape(-1, 2)[2 * spt:].astype(np.float64)
    u = np.array([100 * ONE + n * step for n in range(2 * spt, 14 * spt)], dtype=object)
    ideal = amp * np.sin(2 * np.pi * f0 / rate * np.array([float(Fraction(int(v), ONE)) for v in u]))
    assert np.array_equal(got[:, 0], got[:, 1])
    spec = np.abs(np.fft.rfft(got[:, 0] * np.hanning(len(ideal))))
    peak_hz = np.argmax(spec) * rate / len(ideal)
    assert abs(peak_hz - f0 * step / ONE) <= rate / len(ideal), (peak_hz, f0 * speed)
    db = 10 * np.log10(np.sum((got[:, 0] - ideal) ** 2) / np.sum(ideal ** 2))
    print(f"speed {speed:.6f}: error {db:.2f} dB")
    assert db <= TONE_DB[speed] + 3.0, db


# ---- the cases tell the model from every misreading ----
@pytest.fixture(scope="module")
def truth(tables):
    return {c.name: dc.run_model(c, tables) for c in dc.CASES}


def test_the_list_of_misreadings_is_the_issues():
    assert len(dm.MISREADINGS) == 12 and len(set(dm.MISREADINGS)) == 12


@pytest.mark.parametrize("mis", dm.MISREADINGS)
def test_a_misreading_changes_some_case(tables, truth, mis):
    changed = []
    for c in dc.CASES:
        for (got, recs), (want, wrecs) in zip(dc.run_model(c, tables, mis=(mis,)), truth[c.name]):
            if recs != wrecs or not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                changed.append(c.name)
                break
    print(mis, "changes", len(changed), "cases")
    assert changed, mis


# ---- the launch plan ----
def test_the_cases_draw_every_form_and_ticks_of_one_to_four_chunks(truth):
    total = dict.fromkeys(("ticks_zero", "ticks_stream", "ticks_gather", "chunks_zero", "chunks_stream", "chunks_gather"), 0)
    chunks_per_tick, looping_stream, shifted = set(), 0, 0
    for c in dc.CASES:
        chunks_per_tick.add(-(-c.spt // dc.CHUNK))
        for _got, recs in truth[c.name]:
            for k, v in dc.launch_counts(recs, c.spt).items():
                total[k] += v
            for t in recs:
                if t.flags & dm.T_LOOPING:
                    forms = [dc.chunk_form(t, n0, min(dc.CHUNK, c.spt - n0)) for n0 in range(0, c.spt, dc.CHUNK)]
                    looping_stream += forms.count("stream")
                    shifted += sum(1 for n0, f in zip(range(0, c.spt, dc.CHUNK), forms) if f == "stream" and (t.pos + n0 * t.step - t.loop_in * ONE) // (t.loop_len * ONE) != 0)
    assert all(v > 0 for v in total.values()), total
    assert chunks_per_tick >= {1, 2, 3, 4}
    assert looping_stream > 0 and shifted > 0   # a loop long enough to stream, also after its first wrap
    # outside a loop a chunk gathers only where the direction turns inside it: the window of 4 x chunk + 32 frames is never what refuses a chunk
    turned = 0
    for c in dc.CASES:
        for _got, recs in truth[c.name]:
            for t in recs:
                for n0 in range(0, c.spt, dc.CHUNK):
                    cnt = min(dc.CHUNK, c.spt - n0)
                    if not t.flags & dm.T_LOOPING and dc.chunk_form(t, n0, cnt) == "gather":
                        s0, s1 = t.step + n0 * t.dstep, t.step + (n0 + cnt - 1) * t.dstep
                        assert s0 * s1 < 0, (c.name, t)
                        turned += 1
    assert turned > 0
