"""The deck's echo without a device (include/mixlab_gpu.h "ECHO"): the header's struct and entry points, the setting rules one refusal a
rule, mx_deck_echo_delay against Python integers, mx_deck_echo_plan against the model's cutter, what the header says follows -- on the model -- and that the shared
cases tell the model from each of a list of misreadings."""
import ctypes as C
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import deck_echo_cases as ec
import deck_echo_model as em
from deck_echo_model import OFF, PINGPONG, Echo, EchoModel
from deck_model import ONE

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_set_echo", "mx_deck_schedule_echo", "mx_deck_echo_check", "mx_deck_echo_delay", "mx_deck_echo_state", "mx_deck_echo_plan", "mx_deck_debug_last_echo"}
ECHO_OFFSETS = {"delay": 0, "flags": 4, "send": 8, "feedback": 12, "wet": 16, "damp": 20}


@pytest.fixture(scope="module")
def tables():
    from mixlab_amd import deck
    return np.stack([deck.deck_tables(b) for b in range(4)])


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    assert lay["mx_deck_echo"]["size"] == 24 and lay["mx_deck_echo"]["offsets"] == ECHO_OFFSETS
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert (consts["MX_DECK_ECHO_PINGPONG"], consts["MX_DECK_ECHO_MIN_DELAY"], consts["MX_DECK_ECHO_MAX_DELAY"]) == (PINGPONG, em.MIN_DELAY, em.MAX_DELAY)
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19   # additions only
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_set_echo") == ["mx_deck*", "const mx_deck_echo*"]
    assert sig("mx_deck_schedule_echo") == ["mx_deck*", "uint32_t", "const mx_deck_echo*"]
    assert sig("mx_deck_echo_delay") == ["const mx_deck_beats*", "int64_t", "uint32_t", "uint32_t", "uint32_t*"]
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | {"mx_deck_echo"}):
        assert re.search(rf"\b{name}\b", note), name
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi
    assert C.sizeof(abi.DeckEcho) == 24 and {n: getattr(abi.DeckEcho, n).offset for n, _t in abi.DeckEcho._fields_} == ECHO_OFFSETS
    assert (abi.DECK_ECHO_PINGPONG, abi.DECK_ECHO_MIN_DELAY, abi.DECK_ECHO_MAX_DELAY) == (PINGPONG, em.MIN_DELAY, em.MAX_DELAY)


# ---- the setting rules: one refusal per rule, and the edges that pass ----
OK_SET = Echo(17089, 1.0, 0.5, 1.0, 0.3, 0)
CHECKS = [(OK_SET, True), (OK_SET._replace(delay=256), True), (OK_SET._replace(delay=255), False), (OK_SET._replace(delay=262144), True), (OK_SET._replace(delay=262145), False),
          (OK_SET._replace(delay=0), False),
          (OK_SET._replace(send=float("nan")), False), (OK_SET._replace(feedback=float("inf")), False), (OK_SET._replace(wet=float("-inf")), False), (OK_SET._replace(damp=float("nan")), False),
          (OK_SET._replace(send=-1.0), True), (OK_SET._replace(send=1.0000001), False), (OK_SET._replace(feedback=-1.0), True), (OK_SET._replace(feedback=-1.0000001), False),
          (OK_SET._replace(wet=-4.0), True), (OK_SET._replace(wet=4.000001), False), (OK_SET._replace(damp=0.0), True), (OK_SET._replace(damp=1.0), True),
          (OK_SET._replace(damp=-1e-6), False), (OK_SET._replace(damp=1.0000001), False),
          (OK_SET._replace(flags=PINGPONG), True), (OK_SET._replace(flags=2), False), (OK_SET._replace(flags=PINGPONG | (1 << 31)), False)]


def c_echo(e: Echo):
    from mixlab_amd import abi
    return abi.DeckEcho(e.delay, e.flags, e.send, e.feedback, e.wet, e.damp)


@pytest.mark.parametrize("e,ok", CHECKS)
def test_echo_check_refuses_what_each_rule_refuses(e, ok):
    from mixlab_amd import abi, deck
    assert (em.check(e) is None) == ok
    if ok:
        deck.echo_check(c_echo(e))
    else:
        with pytest.raises(abi.MxError) as err:
            deck.echo_check(c_echo(e))
        assert err.value.code == abi.MX_ERR_INVALID


# ---- the delay of a beat fraction ----
def lib_delay(period, step, num, den):
    from mixlab_amd import abi, deck
    try:
        return deck.echo_delay(abi.DeckBeats(0, period), step, num, den)
    except abi.MxError as e:
        assert e.code == abi.MX_ERR_INVALID
        return None


def test_three_quarters_of_a_beat_at_126_4_bpm_reads_17089():
    period = round(48000 * 60 / 126.4 * ONE)
    assert lib_delay(period, ONE, 3, 4) == 17089 == em.echo_delay(period, ONE, 3, 4)
    assert lib_delay(period, -ONE, 3, 4) == 17089     # a deck running backwards has the same tempo


def test_echo_delay_equals_python_integers_on_random_grids_and_steps():
    rng = np.random.default_rng(20)
    for trial in range(400):
        period = int(rng.integers(1, 1 << 62)) >> int(rng.integers(0, 40))
        step = int(rng.integers(1, 4 * ONE + 1)) * (1 if trial % 3 else -1)
        num, den = int(rng.integers(1, 17)), int(rng.integers(1, 17))
        if trial % 5 == 0:
            num, den = int(rng.integers(1, 1 << 32)), int(rng.integers(1, 1 << 32))
        assert lib_delay(period, step, num, den) == em.echo_delay(period, step, num, den), (period, step, num, den)


def test_echo_delay_ties_go_to_even_and_the_range_edges_hold():
    # period / step = k + 1/2 exactly: 2 k + 1 halves
    for k, want in ((256, 256), (257, 258), (1000, 1000), (1001, 1002), (262143, 262144)):
        assert lib_delay((2 * k + 1) * ONE, 2 * ONE, 1, 1) == want == em.echo_delay((2 * k + 1) * ONE, 2 * ONE, 1, 1)
    assert lib_delay(511 * ONE, 2 * ONE, 1, 1) == 256           # 255.5 -> 256, the floor itself
    assert lib_delay(511 * ONE - 1, 2 * ONE, 1, 1) is None      # just under the tie: 255
    assert lib_delay(262144 * ONE, ONE, 1, 1) == 262144
    assert lib_delay(524289 * ONE, 2 * ONE, 1, 1) == 262144     # 262144.5 -> 262144, the ceiling itself
    assert lib_delay(524289 * ONE + 1, 2 * ONE, 1, 1) is None   # just over the tie: 262145
    assert lib_delay(262145 * ONE, ONE, 1, 1) is None
    assert lib_delay(1 << 52, -(1 << 63), 1 << 20, 1) == 512 == em.echo_delay(1 << 52, -(1 << 63), 1 << 20, 1)     # the most negative step has a magnitude too
    for bad in ((ONE * 1000, 0, 1, 1), (ONE * 1000, ONE, 0, 1), (ONE * 1000, ONE, 1, 0), (0, ONE, 1, 1), (-ONE * 1000, ONE, 1, 1)):
        assert lib_delay(*bad) is None and em.echo_delay(*bad) is None, bad


# ---- the block cut ----
def lib_cut(spt, delays):
    from mixlab_amd import deck
    return deck.echo_plan(spt, delays)


def test_echo_plan_equals_the_models_cutter_on_the_cases_and_on_random_feeds():
    for c in ec.CASES:
        for delays in ec.delays_of(c):
            assert lib_cut(c.spt, delays) == em.cut(c.spt, delays), c.name
    rng = np.random.default_rng(21)
    pool = [0, 256, 257, 300, 440, 441, 442, 799, 800, 801, 802, 1000, 5000, 262144]
    for trial in range(200):
        spt = int(rng.choice([1, 255, 256, 257, 441, 800, 4099]))
        delays = [int(rng.choice(pool)) for _ in range(int(rng.integers(1, 16)))]
        got = lib_cut(spt, delays)
        assert got == em.cut(spt, delays), (spt, delays)
        # every frame of an echo tick lies in exactly one block, in order, and reads nothing its block writes; no block could have taken one frame more
        covered = [f for first, n in got for f in range(first, first + n)]
        assert covered == [f for f in range(len(delays) * spt) if delays[f // spt]]
        for j, (first, n) in enumerate(got):
            assert all(f - delays[f // spt] + 1 < first for f in range(first, first + n))
            nxt = first + n
            if nxt < len(delays) * spt and delays[nxt // spt] and delays[(nxt - 1) // spt]:
                assert nxt - delays[nxt // spt] + 1 >= first


def test_echo_plan_holds_the_cut_across_a_tick_that_drops_the_delay_from_5000_to_256():
    spt, delays = 800, [5000] * 6 + [256] * 2
    got = lib_cut(spt, delays)
    assert got == em.cut(spt, delays)
    assert got[0] == (0, 4800)                       # 4999 frames would be allowed; tick 6, delay 256, allows none of its own: the block ends where tick 6 begins
    assert got[1] == (4800, 255) and got[2] == (5055, 255)
    assert lib_cut(spt, [5000] * 7) == [(0, 4999), (4999, 601)]
    # ... and a tick without an echo ends a block and belongs to none
    assert lib_cut(800, [1000, 0, 1000]) == [(0, 800), (1600, 800)]
    assert lib_cut(800, [0, 0]) == []


def test_echo_plan_refuses_what_the_header_says_it_refuses():
    from mixlab_amd import abi
    n = C.c_uint32()
    d = (C.c_uint32 * 2)(256, 255)
    assert abi.lib.mx_deck_echo_plan(800, d, 1, None, 0, C.byref(n)) == 0 and n.value == 4
    assert abi.lib.mx_deck_echo_plan(800, d, 2, None, 0, C.byref(n)) == abi.MX_ERR_INVALID            # 255
    assert abi.lib.mx_deck_echo_plan(0, d, 1, None, 0, C.byref(n)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_echo_plan((1 << 20) + 1, d, 1, None, 0, C.byref(n)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_echo_plan(800, None, 1, None, 0, C.byref(n)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_echo_plan(800, d, 1, None, 0, None) == abi.MX_ERR_INVALID


# ---- what the header says follows, on the model ----
def noise(n_ticks, spt, seed, amp=1.0):
    rng = np.random.default_rng(seed)
    return (rng.integers(-32768, 32768, size=n_ticks * spt * 2).astype(np.float32) / np.float32(32768.0) * np.float32(amp)).astype(np.float32)


@pytest.mark.parametrize("name", ("schedules inside a feed", "delay 256, 441 frames a tick", "delay 5000, 800 frames a tick", "echo-out under key-lock"))
def test_the_result_does_not_depend_on_how_ticks_are_grouped_into_feeds(tables, name):
    c = ec.BY_NAME[name]
    total = ec.flatten(c)[0]
    ref, ref_st = ec.run_model(c, tables)
    for split in ([1] * total, [5, total - 5]):
        got, st = ec.run_model(c, tables, split=split)
        assert np.array_equal(bits(np.concatenate(got)), bits(np.concatenate(ref))), split
        assert st[-1] == ref_st[-1]


def test_with_wet_0_the_port_holds_the_decks_own_samples():
    x = noise(6, 441, 1)
    m = EchoModel()
    m.schedule(0, Echo(300, 1.0, 0.9, 0.0, 0.3, PINGPONG))
    assert np.array_equal(bits(m.run(x, 441)), bits(x))
    assert m.hist[:m.t].any()          # ... while the line fills all the same


def test_the_freeze_holds_bit_for_bit_over_20_passes_of_the_line():
    spt, D = 441, 441
    m = EchoModel()
    m.schedule(0, Echo(D, 1.0, 0.5, 1.0, 0.0))
    m.run(noise(3, spt, 2), spt)
    m.schedule(0, Echo(D, 0.0, 1.0, 1.0, 0.0))
    m.run(noise(1, spt, 3), spt)                    # the ramp tick: send and feedback still on their way
    zeros = np.zeros(22 * spt * 2, np.float32)
    y = m.run(zeros, spt).reshape(22, D, 2)         # silence in: the port is the line going round
    assert y[1].any()
    for k in range(2, 22):
        assert np.array_equal(bits(y[k]), bits(y[1])), k


def test_channels_never_meet_without_pingpong_and_alternate_strictly_with_it():
    spt, D = 441, 300
    x = np.zeros((8 * spt, 2), np.float32)
    x[10, 0] = 0.75                                 # one impulse, left only
    for damp in (0.0, 0.3):
        m = EchoModel()
        m.schedule(0, Echo(D, 1.0, 0.8, 1.0, damp))
        y = m.run(x.reshape(-1), spt).reshape(-1, 2)
        assert y[:, 0].any() and not y[:, 1].any()
        m = EchoModel()
        m.schedule(0, Echo(D, 1.0, 0.8, 1.0, damp, PINGPONG))
        y = m.run(x.reshape(-1), spt).reshape(-1, 2)
        for rep in range(1, 8 * spt // D):
            seg = y[10 + rep * D - rep:10 + rep * D + rep + 1]          # damping spreads repeat k over +- k frames
            side = rep % 2                                             # repeat 1 sounds right, 2 left, ...
            assert seg[:, side].any() and not seg[:, 1 - side].any(), (damp, rep)


def test_a_tail_with_feedback_a_half_halves_per_repeat_into_the_subnormals_and_is_not_flushed():
    spt, D = 800, 256
    x = np.zeros((46 * spt, 2), np.float32)
    x[spt] = (1.0, -0.333)                        # in the second tick: the first one ramps send and feedback up from 0
    m = EchoModel()
    m.schedule(0, Echo(D, 1.0, 0.5, 1.0, 0.0))
    y = m.run(x.reshape(-1), spt).reshape(-1, 2)[spt:]
    for k in range(1, 138):                                          # repeat k carries send * fb^(k - 1)
        assert y[k * D, 0] == np.float32(2.0 ** -(k - 1)), k         # exact halving, through 2^-127 .. 2^-136: subnormal
    assert 0 < y[137 * D, 0] < np.finfo(np.float32).tiny
    tiny = y[131 * D, 1]
    assert tiny != 0 and abs(tiny) < np.finfo(np.float32).tiny and y[132 * D, 1] == np.float32(np.float64(tiny) * 0.5)


def test_ramps_start_at_old_and_never_reach_new_inside_the_ramp_tick():
    spt, D = 441, 300
    x = np.full(4 * spt * 2, 0.5, np.float32)
    m = EchoModel()
    m.schedule(0, Echo(D, 1.0, 0.0, 0.0, 0.0))
    m.run(x[:spt * 2], spt)                          # off -> on: send ramps from 0
    r = m.hist[:spt, 0].astype(np.float64)
    assert r[0] == 0.0 and np.all(np.diff(r) > 0) and r[-1] < 0.5
    assert r[-1] == np.float32(np.float32(np.float64(spt - 1) / spt) * np.float64(0.5))
    m.run(x[:spt * 2], spt)                          # the next tick uses `new`
    assert np.all(m.hist[spt:2 * spt, 0] == np.float32(0.5))
    m.schedule(0, Echo(D, 0.25, 0.0, 0.0, 0.0))
    m.run(x[:spt * 2], spt)                          # 1 -> 0.25: starts at old, stops short of new
    r = m.hist[2 * spt:3 * spt, 0]
    assert r[0] == np.float32(0.5) and np.all(np.diff(r.astype(np.float64)) < 0) and r[-1] > np.float32(0.125)
    m.run(x[:spt * 2], spt)
    assert np.all(m.hist[3 * spt:4 * spt, 0] == np.float32(0.125))


def test_off_then_on_starts_clean_and_a_change_of_delay_does_not():
    spt = 441
    x = noise(8, spt, 5)
    m = EchoModel()
    m.schedule(0, Echo(300, 1.0, 0.5, 1.0, 0.0))
    m.schedule(3, OFF)
    m.schedule(5, Echo(300, 1.0, 0.5, 1.0, 0.0))
    y = m.run(x, spt).reshape(8, spt, 2)
    xx = x.reshape(8, spt, 2)
    assert np.array_equal(bits(y[3:5]), bits(xx[3:5]))               # off: the deck's own samples
    assert np.array_equal(bits(y[5, :300]), bits(xx[5, :300]))       # on again: nothing of the old line comes back
    assert m.state()[0] == 3 * spt
    m.schedule(0, Echo(1000, 1.0, 0.5, 1.0, 0.0))
    y = m.run(x[:2 * spt * 2], spt).reshape(2, spt, 2)
    assert not np.array_equal(bits(y[0, :300]), bits(xx[0, :300]))   # the new delay reads the line the old one wrote
    assert m.state()[0] == 5 * spt


# ---- the cases tell the model from every misreading ----
@pytest.fixture(scope="module")
def truth(tables):
    out = {}
    for c in ec.QUICK:
        xs = ec.deck_samples(c, tables, [f.n_ticks for f in c.feeds])
        out[c.name] = (xs, ec.run_model(c, tables, xs=xs))
    return out


def test_the_list_of_misreadings_has_eight_entries():
    assert len(em.MISREADINGS) >= 8 and len(set(em.MISREADINGS)) == len(em.MISREADINGS)


# the case named catches the misreading (others may too)
CAUGHT_BY = {"r_from_y": "delay 256, 441 frames a tick", "ramp_n_plus_1": "delay 802, 800 frames a tick", "ramp_f32": "schedules inside a feed",
             "delay_from_tick_start": "schedules inside a feed", "pingpong_crosses_x": "delay 800, 800 frames a tick", "seek_restarts": "schedules inside a feed",
             "line_kept_off_on": "schedules inside a feed", "block_plus_one": "delay 257, 800 frames a tick"}


@pytest.mark.parametrize("mis", em.MISREADINGS)
def test_a_misreading_changes_a_compared_sample_of_the_case_named(tables, truth, mis):
    c = ec.BY_NAME[CAUGHT_BY[mis]]
    xs, (want, _st) = truth[c.name]
    got, _ = ec.run_model(c, tables, mis=(mis,), xs=xs)
    changed = int(np.count_nonzero(bits(np.concatenate(got)) != bits(np.concatenate(want))))
    print(mis, "changes", changed, "samples of", c.name)
    assert changed, mis


TINY = ("delay 256, 16 frames a tick", "delay 257, 16 frames a tick", "one frame a tick")


@pytest.mark.parametrize("name", TINY)
def test_the_tiny_tick_cases_are_heard_and_their_blocks_span_many_ticks(truth, name):
    """after frame D more than half the frames differ from dry; a block of D - 1 frames spans 16 or 17 ticks of 16 frames, 255 of one"""
    c = ec.BY_NAME[name]
    assert c in ec.QUICK and ec.LONG_FEEDS[c.spt] == ec.flatten(c)[0]
    (x,), ((y,), _st) = truth[name]
    D = c.feeds[0].echo[0][1].delay
    differ = np.any((bits(x) != bits(y)).reshape(-1, 2)[D:], axis=1)
    assert 2 * int(differ.sum()) > differ.size, (int(differ.sum()), differ.size)
    (delays,) = ec.delays_of(c)
    spans = [(first + n - 1) // c.spt - first // c.spt + 1 for first, n in em.cut(c.spt, delays)]
    assert spans[0] == -(-(D - 1) // c.spt) and max(spans) <= spans[0] + 1 + (299 - 255 if c.spt == 1 else 0), spans      # 16 ticks or 255, later ones a tick more


def test_at_one_frame_a_tick_the_ramp_tick_sounds_the_old_gains_whole(tables, truth):
    c = ec.BY_NAME["one frame a tick"]
    (x,), ((y,), _st) = truth[c.name]
    feed = c.feeds[0]
    later = c._replace(feeds=[feed._replace(echo=[(t + 1 if t == 300 else t, e) for t, e in feed.echo])])       # the same gains a tick later
    (z,), _ = ec.run_model(later, tables, xs=[x])
    y, z = bits(y).reshape(-1, 2), bits(z).reshape(-1, 2)
    assert np.array_equal(y[:301], z[:301]) and not np.array_equal(y[301], z[301])
    # ... and the line too: frame 300 + 256 reads what tick 300 wrote with the old send and feedback
    never = c._replace(feeds=[feed._replace(echo=[(t, e) for t, e in feed.echo if t not in (300, 400)])])
    m_y, m_n = EchoModel(), EchoModel()
    for m, case in ((m_y, c), (m_n, never)):
        for t, e in case.feeds[0].echo:
            if t < 400:
                m.schedule(t, e)
        m.run(x[:2 * 400], 1)
    assert np.array_equal(bits(m_y.hist[:301]), bits(m_n.hist[:301])) and not np.array_equal(bits(m_y.hist[301]), bits(m_n.hist[301]))


def test_the_tiny_tick_cases_tell_the_model_from_the_misreadings_a_tick_of_their_length_can_show(tables, truth):
    """at one frame a tick the two roundings of the ramp weight agree (the weight is 0), nothing seeks, and what a frame past 256 writes into the line -- where a
    feedback taken from y, or a block a frame too long, would show -- is first read at tick 557, with the echo off; every other misreading changes a sample.
    The damped case of 16 frames a tick shows those two; it has one setting without ping-pong from tick 0 on, ramped from 0 with weights n / 16 that both roundings hold exactly."""
    for name, blind in (("one frame a tick", {"ramp_f32", "seek_restarts", "r_from_y", "block_plus_one"}), ("delay 256, 16 frames a tick", {"ramp_f32", "seek_restarts", "line_kept_off_on", "delay_from_tick_start", "pingpong_crosses_x"})):
        c = ec.BY_NAME[name]
        xs, (want, _st) = truth[name]
        caught = {mis for mis in em.MISREADINGS if np.any(bits(np.concatenate(ec.run_model(c, tables, mis=(mis,), xs=xs)[0])) != bits(np.concatenate(want)))}
        assert caught == set(em.MISREADINGS) - blind, (name, sorted(set(em.MISREADINGS) - caught))


def test_the_cases_reach_both_forms_and_a_block_across_a_tick_boundary():
    one = seq = crossing = 0
    for c in ec.CASES:     # as given and tick by tick, the two groupings the device suite plays
        for delays in ec.delays_of(c) + ec.delays_of(c, [1] * ec.flatten(c)[0]):
            blocks = em.cut(c.spt, delays)
            if len(blocks) <= 1:
                one += bool(blocks)
                continue
            seq += 1
            crossing += sum(1 for first, n in blocks if first // c.spt != (first + n - 1) // c.spt)
    assert one and seq and crossing, (one, seq, crossing)
