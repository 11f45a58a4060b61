"""The deck's sweep filter on the device (include/mixlab_gpu.h "FILTER"): every sample of a SOURCE_STEREO node's port after mx_deck_feed, bit
for bit against the Python models (tests/deck_filter_model.py, and tests/deck_echo_model.py behind it) applied to what DeckModel / KeylockModel say the deck wrote,
over the shared cases (tests/deck_filter_cases.py), with the four carried state values, the setting and the four counters; the same ticks under three groupings
into feeds; three decks in one feed, one of them with neither filter nor echo; a filter switched off; the refusals, which leave everything where it stood; one deck
and one model carried across graphs, tick lengths, a load and key-lock; and the device against mx_deck_filter_host on the device's own input."""
import copy

import numpy as np
import pytest

import deck_cases as dc
import deck_echo_model as em
import deck_filter_cases as fc
import deck_filter_model as fm
from deck_echo_model import Echo
from deck_filter_model import BP, HP, LP, OFF, Filt
from deck_keylock_model import Keylock, KeylockModel
from deck_model import ONE
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

MAX_TICKS, N_SRC = 16, 3
KEYS = ("decks", "ticks_ramp", "ticks_constant", "blocks")
ZERO = dict.fromkeys(KEYS, 0)


@pytest.fixture(scope="module")
def tables():
    return np.stack([deck.deck_tables(b) for b in range(4)])


_graphs = {}


def graph_for(spt: int):
    """one graph per tick length, shared by the tests: N_SRC stereo sources into a mixer"""
    if spt not in _graphs:
        ws = Workspace(*dc.rate_of(spt))
        srcs = [ws.source_stereo() for _ in range(N_SRC)]
        mix = ws.mixer([(0.0, 1.0, False)] * N_SRC)
        for k, s in enumerate(srcs):
            ws.connect(s, 0, mix, k)
        _graphs[spt] = (ws.build(max_ticks_per_run=max(MAX_TICKS, fc.LONG_FEEDS.get(spt, 0))), srcs, [0])
    return _graphs[spt]


def c_params(p):
    return deck.params(p.step, p.slew, p.loop_in, p.loop_out, p.flags)


def c_filt(f: Filt):
    return abi.DeckFilter(f.kind, f.flags, f.g, f.k, f.wet, f.pad)


def c_echo(e: Echo):
    return abi.DeckEcho(e.delay, e.flags, e.send, e.feedback, e.wet, e.damp)


def state_tuple(d):
    on, f = d.filter_state()
    return on, (f.kind, f.flags, f.g, f.k, f.wet, f._pad)


def model_state(on, f):
    return on, (f.kind, f.flags, *(float(np.float32(v)) for v in (f.g, f.k, f.wet)), f.pad)


def assert_bits(got, want, label):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{label}: {bad.size} of {got.size} samples differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


def assert_state4(got, want, label):
    assert np.array_equal(np.asarray(got, np.float64).view(np.uint64), np.asarray(want, np.float64).view(np.uint64)), f"{label}: state {got!r}, want {want!r}"


def make_deck(case):
    d = deck.Deck(case.n_frames)
    d.load(fc.track(case))
    if case.keylock:
        k = case.keylock
        d.set_keylock(deck.keylock(k.pitch, k.hop, k.overlap, k.radius))
    return d


def play_case(case, split=None):
    """the case on the device, its feeds as given or regrouped by split: ([port per feed], [(filter_state, read_filter_state, debug_last_filter) after each feed])"""
    g, srcs, clock = graph_for(case.spt)
    d = make_deck(case)
    total, deck_ev, filt_ev, echo_ev = fc.flatten(case)
    lengths = split if split is not None else [f.n_ticks for f in case.feeds]
    assert sum(lengths) == total
    ports, states, at = [], [], 0
    for n in lengths:
        for t in range(at, at + n):
            if t in deck_ev:
                p, s = deck_ev[t]
                d.schedule(t - at, c_params(p) if p is not None else None, s)
            if t in filt_ev:
                d.schedule_filter(t - at, None if filt_ev[t] is OFF else c_filt(filt_ev[t]))
            if t in echo_ev:
                d.schedule_echo(t - at, None if echo_ev[t] is em.OFF else c_echo(echo_ev[t]))
        deck.feed([d], [srcs[0]], g, n)
        counts = deck.debug_last_filter()
        g.run_ticks(clock[0], n)
        clock[0] += n
        ports.append(g.read_output(srcs[0], 0, n, True))
        states.append((state_tuple(d), d.read_filter_state(), counts))
        at += n
    d.close()
    return ports, states


def check_case(case, tables, split=None):
    ports, states = play_case(case, split)
    want, want_states, _f, _e = fc.run_model(case, tables, split=split)
    for fi, (w, (on, f, s4, counts)) in enumerate(zip(want, want_states)):
        label = f"{case.name}: feed {fi} of {split or 'the case'}"
        assert_bits(ports[fi], w, label)
        assert states[fi][0] == model_state(on, f), label
        assert_state4(states[fi][1], s4, label)
        assert states[fi][2] == counts, label
    return ports, states


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_ports_state_setting_and_counters_equal_the_model(case, tables):
    check_case(case, tables)


@pytest.mark.parametrize("name", ("schedules inside a feed", "lp sweep 20 kHz to 80 Hz", "63 frames a tick", "64 frames a tick", "65 frames a tick", "ring-out",
                                  "echo-out under a closing low-pass"))
def test_one_feed_of_12_twelve_feeds_of_one_and_5_plus_7_give_identical_ports_and_state(name, tables):
    case = fc.BY_NAME[name]
    (ref,), (ref_state,) = check_case(case, tables)
    for split in ([1] * 12, [5, 7]):
        ports, states = check_case(case, tables, split)
        assert_bits(np.concatenate(ports), ref, f"{name}: {split}")
        assert states[-1][0] == ref_state[0]
        assert_state4(states[-1][1], ref_state[1], f"{name}: {split}")


def test_the_subnormal_ring_out_reaches_the_device_unflushed(tables):
    (port,), _s = check_case(fc.BY_NAME["subnormal ring-out"], tables)
    a = np.abs(port)
    assert np.count_nonzero((a > 0) & (a < np.finfo(np.float32).tiny)) > 100      # subnormals in the port, and (check_case) each the model's bit for bit


def test_three_decks_in_one_feed_filter_alone_filter_and_echo_and_neither(tables):
    spt, n = 800, 4
    g, srcs, clock = graph_for(spt)
    scripts = ((ONE, 0, [(0, Filt(LP, 0.1, 0.1)), (2, Filt(HP, 0.3, 0.5))], []), (dc.frames(1.08), dc.frames(40.5), [(1, Filt(BP, 0.2, 0.2))], [(0, Echo(900, 1.0, 0.5, 1.0, 0.3))]),
               (dc.frames(0.92), dc.frames(10.25), [], []))
    cases = [fc.Case(f"three decks {k}", spt, 4097, [fc.Feed(n, [(0, dc.play(step), seek)], f, e)]) for k, (step, seek, f, e) in enumerate(scripts)]

    def run(with_effects: bool):
        decks = [make_deck(c) for c in cases]
        for d, c in zip(decks, cases):
            (_t, p, s), = c.feeds[0].deck
            d.schedule(0, c_params(p), s)
            for t, f in (c.feeds[0].filt if with_effects else ()):
                d.schedule_filter(t, c_filt(f))
            for t, e in (c.feeds[0].echo if with_effects else ()):
                d.schedule_echo(t, c_echo(e))
        deck.feed(decks, srcs, g, n)
        counts = (deck.debug_last_filter(), deck.debug_last_feed(), deck.debug_last_keylock(), deck.debug_last_echo())
        g.run_ticks(clock[0], n)
        clock[0] += n
        ports = [g.read_output(s, 0, n, True) for s in srcs]
        ticks = [[(t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank) for t in d.read_ticks(0, n)] for d in decks]
        states = [(state_tuple(d), d.read_filter_state()) for d in decks]
        for d in decks:
            d.close()
        return ports, ticks, states, counts

    ports, ticks, states, counts = run(True)
    for k, c in enumerate(cases):
        (want,), ((on, f, s4, _c),), _f, _e = fc.run_model(c, tables)
        assert_bits(ports[k], want, c.name)
        assert states[k][0] == model_state(on, f)
        assert_state4(states[k][1], s4, c.name)
    blocks = -(-n * spt // 64)
    assert counts[0] == {"decks": 2, "ticks_ramp": 3, "ticks_constant": 4, "blocks": 2 * blocks}      # deck 0: ramps at 0 and 2; deck 1: off, ramp, two constant
    plain_ports, plain_ticks, plain_states, plain_counts = run(False)
    assert_bits(ports[2], plain_ports[2], "the deck with neither")
    assert ticks == plain_ticks and counts[1] == plain_counts[1] and counts[2] == plain_counts[2]
    assert plain_counts[0] == ZERO and plain_counts[3] == dict.fromkeys(plain_counts[3], 0) and counts[3]["decks_one_block"] + counts[3]["decks_sequential"] == 1
    assert states[2][0] == plain_states[2][0] == (False, (0, 0, 0.0, 0.0, 0.0, 0)) and not states[2][1].any()


def test_a_filter_switched_off_leaves_all_four_counters_zero_and_the_decks_own_samples(tables):
    case = fc.BY_NAME["lp at rest, 441 frames a tick"]
    g, srcs, clock = graph_for(case.spt)
    d = make_deck(case)
    (_t, p, s), = case.feeds[0].deck
    d.schedule(0, c_params(p), s)
    d.set_filter(c_filt(Filt(LP, 0.05, 0.5)))
    deck.feed([d], [srcs[0]], g, 1)
    assert deck.debug_last_filter() == {"decks": 1, "ticks_ramp": 1, "ticks_constant": 0, "blocks": 7} and d.read_filter_state().any()
    g.run_ticks(clock[0], 1)
    d.set_filter(None)
    deck.feed([d], [srcs[0]], g, 2)
    assert deck.debug_last_filter() == ZERO
    g.run_ticks(clock[0] + 1, 2)
    clock[0] += 3
    assert_bits(g.read_output(srcs[0], 0, 2, True), fc.deck_samples(case, tables)[1:3], "filter off: the deck's own samples")
    on, f = state_tuple(d)
    assert (on, f[0], f[2]) == (False, LP, float(np.float32(0.05))) and not d.read_filter_state().any()
    d.close()


def test_a_schedule_past_the_feed_is_refused_and_deck_filter_echo_and_counters_stand_where_they_stood(tables):
    case = fc.BY_NAME["echo-out under a closing low-pass"]
    g, srcs, clock = graph_for(case.spt)
    d, m_f, m_e = make_deck(case), fm.FilterModel(), em.EchoModel()
    xs = fc.deck_samples(case, tables)                  # (the case's deck plays at unity from 0; its own filter and echo events are not used here)
    f0, e0 = Filt(LP, 0.2, 0.3), Echo(900, 1.0, 0.6, 1.0, 0.3)
    d.schedule(0, c_params(dc.play(ONE)), 0)
    d.set_filter(c_filt(f0))
    d.set_echo(c_echo(e0))
    m_f.schedule(0, f0)
    m_e.schedule(0, e0)

    def feed(at, n, label):
        deck.feed([d], [srcs[0]], g, n)
        g.run_ticks(clock[0], n)
        clock[0] += n
        assert_bits(g.read_output(srcs[0], 0, n, True), m_e.run(m_f.run(xs[at:at + n].reshape(-1), case.spt), case.spt), label)
        assert state_tuple(d) == model_state(*m_f.state())
        assert_state4(d.read_filter_state(), m_f.state4(), label)

    feed(0, 2, "the first feed")
    head, st, s4, echo_st, counts, echo_counts = d.state(), state_tuple(d), d.read_filter_state(), d.echo_state()[:2], deck.debug_last_filter(), deck.debug_last_echo()
    d.schedule_filter(3, c_filt(Filt(HP, 0.5, 1.0)))
    d.schedule_echo(1, c_echo(Echo(300)))
    d.schedule(1, c_params(dc.play(2 * ONE)))
    with pytest.raises(abi.MxError) as e:
        deck.feed([d], [srcs[0]], g, 3)
    assert e.value.code == abi.MX_ERR_INVALID and "filter" in str(e.value)
    assert state_tuple(d) == st and d.state().pos_q32 == head.pos_q32 and d.echo_state()[:2] == echo_st
    assert deck.debug_last_filter() == counts and deck.debug_last_echo() == echo_counts
    assert_state4(d.read_filter_state(), s4, "after the refusal")
    feed(2, 2, "the feed after the refusal")           # all three schedules are gone: it plays on as if nothing had been asked
    assert d.state().step_q32 == ONE and d.echo_state()[2].delay == 900
    # settings the check refuses never reach the schedule
    with pytest.raises(abi.MxError):
        d.set_filter(c_filt(Filt(LP, 17.0, 0.3)))
    with pytest.raises(abi.MxError):
        d.schedule_filter(1, c_filt(Filt(4, 0.2, 0.3)))
    feed(4, 2, "after refused settings")
    d.close()


# ---- "nothing else clears them": one deck and one FilterModel carried across every feed ----
class Carried:
    """a filtered deck with its models.  feed() plays n ticks into whatever graph, holds the port, the setting and the four state values to the models, and shows
    that the carried state mattered: the same feed from a state of zeros would have given other samples"""

    def __init__(self, tables, name, n_frames=6000):
        tr = dc.track("filter " + name, n_frames)
        self.d, self.m, self.f, self.at = deck.Deck(n_frames), KeylockModel(tr.copy(), tables), fm.FilterModel(), {}
        self.d.load(tr)

    def play(self, p, seek=None):
        self.d.schedule(0, c_params(p), seek)
        self.m.schedule(0, p, seek)

    def feed(self, g, src, spt, n, label, heard=True):
        deck.feed([self.d], [src], g, n)
        at = self.at.get(id(g), 0)
        g.run_ticks(at, n)
        self.at[id(g)] = at + n
        x = self.m.feed(n, spt)[0]
        cleared = copy.deepcopy(self.f)
        cleared.s[:] = 0.0
        want = self.f.run(x, spt)
        assert_bits(g.read_output(src, 0, n, True), want, label)
        assert state_tuple(self.d) == model_state(*self.f.state()), label
        assert_state4(self.d.read_filter_state(), self.f.state4(), label)
        assert not heard or not np.array_equal(want.view(np.uint32), cleared.run(x, spt).view(np.uint32)), f"{label}: the state is not heard"
        return x, want


def lone_graph(spt):
    ws = Workspace(*dc.rate_of(spt))
    src = ws.source_stereo()
    return ws.build(max_ticks_per_run=MAX_TICKS), src


def ringing_deck(tables, name, g, src, spt):
    c = Carried(tables, name)
    c.play(dc.play(ONE, loop=(0, 6000)), 0)
    f = Filt(BP, 0.03, 0.05)
    c.d.set_filter(c_filt(f))
    c.f.schedule(0, f)
    c.feed(g, src, spt, 3, f"{name}: the first feed", heard=False)
    return c


def test_a_feed_into_a_second_graph_and_back_and_into_another_tick_length_carries_the_state(tables):
    """A, then B of the same tick length with the deck stopped -- what B's port holds is the resonance A left --, then A again, then 441 frames a tick"""
    (ga, sa), (gb, sb), (gc, sc) = lone_graph(800), lone_graph(800), lone_graph(441)
    c = ringing_deck(tables, "two graphs", ga, sa, 800)
    c.play(dc.play(ONE, on=False))
    x, y = c.feed(gb, sb, 800, 2, "into B")
    assert not x.any() and y.any()
    c.play(dc.play(ONE, loop=(0, 6000)))
    c.feed(ga, sa, 800, 2, "into A again")
    c.feed(gc, sc, 441, 3, "into 441 frames a tick")
    c.d.close(); ga.close(); gb.close(); gc.close()


def test_a_load_and_set_keylock_on_and_off_between_feeds_leave_the_state(tables):
    g, src = lone_graph(800)
    c = ringing_deck(tables, "load and key-lock", g, src, 800)
    piece = dc.track("filter load and key-lock, loaded", 2500)             # over the frames the head plays next (it stands at 2400)
    c.d.load(piece, 2000)
    c.m.load(2000, piece)
    c.feed(g, src, 800, 2, "after the load")
    kl = Keylock(ONE, 256, 64, 5)
    c.d.set_keylock(deck.keylock(*kl))
    c.m.set_keylock(kl)
    c.feed(g, src, 800, 2, "key-lock on")
    c.d.set_keylock(None)
    c.m.set_keylock(None)
    c.feed(g, src, 800, 2, "key-lock off")
    c.d.close(); g.close()


def test_the_device_equals_mx_deck_filter_host_on_the_devices_own_input(tables):
    """the port of an unfiltered feed is the device's own input; mx_deck_filter_host over it equals the port of the same feed with the filter -- and both the model"""
    case = fc.BY_NAME["schedules inside a feed"]
    (filtered,), _s = check_case(case, tables)
    (plain,), _s = play_case(case._replace(feeds=[f._replace(filt=[]) for f in case.feeds]))
    host, carry = deck.filter_host(plain, case.spt, [c_filt(f) if f is not None else None for f in fc.settings_per_tick(case)])
    assert_bits(host, filtered, "mx_deck_filter_host on the device's input")
    _p, st, _f, _e = fc.run_model(case, tables)
    assert_state4(np.array(carry.s[:]), st[-1][2], "the carried block")
