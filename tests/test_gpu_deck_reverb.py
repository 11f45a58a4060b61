"""The deck's reverb on the device (include/mixlab_gpu.h "REVERB"): every sample of a SOURCE_STEREO node's port after mx_deck_feed, bit for
bit against the Python models (tests/deck_reverb_model.py, behind tests/deck_filter_model.py and tests/deck_echo_model.py) applied to what DeckModel / KeylockModel
say the deck wrote, over the shared cases (tests/deck_reverb_cases.py), with the specified slots of the twelve rings, the clock, the setting and the four counters;
the same ticks under three groupings into feeds; three decks in one feed, one of them with no effect at all; a schedule past the feed, refused with everything where
it stood; one deck carried into a second graph and into a graph of another tick length; and the device against mx_deck_reverb_host on the device's own input."""
import ctypes as C

import numpy as np
import pytest

import deck_cases as dc
import deck_echo_model as em
import deck_filter_model as fm
import deck_reverb_cases as rc
import deck_reverb_model as rm
from deck_echo_model import Echo
from deck_filter_model import LP, Filt
from deck_model import ONE, DeckModel
from deck_reverb_model import OFF, Reverb, ReverbModel
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

MAX_TICKS, N_SRC = 16, 3
ZERO = dict.fromkeys(("decks", "blocks", "blocks_crossing", "largest_block"), 0)


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
        _graphs[spt] = (ws.build(max_ticks_per_run=max(MAX_TICKS, rc.LONG_FEEDS.get(spt, 0))), srcs, [0])
    return _graphs[spt]


def c_params(p):
    return deck.params(p.step, p.slew, p.loop_in, p.loop_out, p.flags)


def c_rev(r: Reverb):
    return abi.DeckReverb((C.c_uint32 * 8)(*r.delay), (C.c_uint32 * 4)(*r.diff), (C.c_float * 8)(*r.gain), r.send, r.dry, r.wet, r.damp, r.diffusion, r.flags)


def c_filt(f: Filt):
    return abi.DeckFilter(f.kind, f.flags, f.g, f.k, f.wet, f.pad)


def c_echo(e: Echo):
    return abi.DeckEcho(e.delay, e.flags, e.send, e.feedback, e.wet, e.damp)


def state_tuple(d):
    t, on, r = d.reverb_state()
    return t, on, (tuple(r.delay), tuple(r.diff), tuple(r.gain), r.send, r.dry, r.wet, r.damp, r.diffusion, r.flags)


def model_state(t, on, r: Reverb):
    f = lambda v: float(np.float32(v))   # noqa: E731
    return t, on, (tuple(r.delay), tuple(r.diff), tuple(f(v) for v in r.gain), f(r.send), f(r.dry), f(r.wet), f(r.damp), f(r.diffusion), r.flags)


def assert_bits(got, want, label):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{label}: {bad.size} of {got.size} samples differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


def assert_lines(got, want_lines, label):
    want, mask = want_lines
    assert_bits(got[mask], want[mask], label + ": lines")


def make_deck(case):
    d = deck.Deck(case.n_frames)
    d.load(rc.track(case))
    if case.keylock:
        k = case.keylock
        d.set_keylock(deck.keylock(k.pitch, k.hop, k.overlap, k.radius))
    return d


def play_case(case, split=None, with_reverb=True):
    """the case on the device, its feeds as given or regrouped by split: ([port per feed], [(reverb_state, lines, debug_last_reverb) after each feed])"""
    g, srcs, clock = graph_for(case.spt)
    d = make_deck(case)
    total, deck_ev, rev_ev, filt_ev, echo_ev = rc.flatten(case)
    lengths = split if split is not None else [f.n_ticks for f in case.feeds]
    assert sum(lengths) == total
    ports, states, at = [], [], 0
    for n in lengths:
        for t in range(at, at + n):
            if t in deck_ev:
                p, s = deck_ev[t]
                d.schedule(t - at, c_params(p) if p is not None else None, s)
            if t in rev_ev and with_reverb:
                d.schedule_reverb(t - at, None if rev_ev[t] is OFF else c_rev(rev_ev[t]))
            if t in filt_ev:
                d.schedule_filter(t - at, None if filt_ev[t] is fm.OFF else c_filt(filt_ev[t]))
            if t in echo_ev:
                d.schedule_echo(t - at, None if echo_ev[t] is em.OFF else c_echo(echo_ev[t]))
        deck.feed([d], [srcs[0]], g, n)
        counts = deck.debug_last_reverb()
        g.run_ticks(clock[0], n)
        clock[0] += n
        ports.append(g.read_output(srcs[0], 0, n, True))
        states.append((state_tuple(d), d.read_reverb_lines(), counts))
        at += n
    d.close()
    return ports, states


def check_case(case, tables, split=None):
    ports, states = play_case(case, split)
    want, want_states, want_lines, _x = rc.run_model(case, tables, split=split)
    for fi, (w, (t, on, r, counts)) in enumerate(zip(want, want_states)):
        label = f"{case.name}: feed {fi} of {split or 'the case'}"
        assert_bits(ports[fi], w, label)
        assert states[fi][0] == model_state(t, on, r), label
        assert_lines(states[fi][1], want_lines[fi], label)
        assert states[fi][2] == counts, label
    return ports, states


@pytest.mark.parametrize("case", rc.CASES, ids=lambda c: c.name)
def test_ports_lines_state_and_counters_equal_the_model(case, tables):
    check_case(case, tables)


@pytest.mark.parametrize("name", ("schedules inside a feed", "reach lowered mid-feed", "reach raised mid-feed", "63 frames a tick", "64 frames a tick", "65 frames a tick",
                                  "reverb-out", "behind a filter and an echo"))
def test_one_feed_of_12_twelve_feeds_of_one_and_5_plus_7_give_identical_ports_and_lines(name, tables):
    case = rc.BY_NAME[name]
    (ref,), (ref_state,) = check_case(case, tables)
    _p, _s, ((_l, mask),), _x = rc.run_model(case, tables)
    for split in ([1] * 12, [5, 7]):
        ports, states = check_case(case, tables, split)
        assert_bits(np.concatenate(ports), ref, f"{name}: {split}")
        assert states[-1][0] == ref_state[0]
        assert_bits(states[-1][1][mask], ref_state[1][mask], f"{name}: {split}: lines")


def test_the_blocks_of_the_cases_straddle_tick_boundaries_and_the_device_counts_them(tables):
    """the counters of a feed are the model's cut: blocks, those crossing a tick boundary, the largest -- and the cases do cross"""
    for name, crossing in (("designed default, 800 frames a tick", True), ("65 frames a tick", True), ("64 frames a tick", False), ("16 frames a tick", True)):
        case = rc.BY_NAME[name]
        _p, states = play_case(case)
        per_tick = rc.settings_per_tick(case)
        want = rm.counts_of(case.spt, [rm.reach(r) if r is not None else 0 for r in per_tick])
        assert states[0][2] == want and (want["blocks_crossing"] > 0) == crossing, (name, want)
        assert deck.reverb_plan(case.spt, [c_rev(r) if r is not None else None for r in per_tick]) == rm.cut(case.spt, [rm.reach(r) if r is not None else 0 for r in per_tick])


def test_the_subnormal_ring_out_reaches_the_device_unflushed(tables):
    (port,), _s = check_case(rc.BY_NAME["subnormal ring-out"], tables)
    a = np.abs(port)
    assert np.count_nonzero((a > 0) & (a < np.finfo(np.float32).tiny)) > 100      # subnormals in the port, and (check_case) each the model's bit for bit


def test_three_decks_in_one_feed_reverb_alone_filter_echo_and_reverb_and_none(tables):
    spt, n = 800, 4
    g, srcs, clock = graph_for(spt)
    scripts = ((ONE, 0, [(0, rc.DEFAULT), (2, rc.MID)], [], []), (dc.frames(1.08), dc.frames(40.5), [(1, rc.STAGGER)], [(0, Filt(LP, 0.2, 0.2))], [(0, Echo(900, 1.0, 0.5, 1.0, 0.3))]),
               (dc.frames(0.92), dc.frames(10.25), [], [], []))
    cases = [rc.Case(f"three decks {k}", spt, 4097, [rc.Feed(n, [(0, dc.play(step), seek)], r, f, e)]) for k, (step, seek, r, f, e) in enumerate(scripts)]

    def run(with_reverb: bool):
        decks = [make_deck(c) for c in cases]
        for d, c in zip(decks, cases):
            (_t, p, s), = c.feeds[0].deck
            d.schedule(0, c_params(p), s)
            for t, r in (c.feeds[0].rev if with_reverb else ()):
                d.schedule_reverb(t, c_rev(r))
            for t, f in c.feeds[0].filt:
                d.schedule_filter(t, c_filt(f))
            for t, e in c.feeds[0].echo:
                d.schedule_echo(t, c_echo(e))
        deck.feed(decks, srcs, g, n)
        counts = (deck.debug_last_reverb(), deck.debug_last_feed(), deck.debug_last_keylock(), deck.debug_last_echo(), deck.debug_last_filter())
        g.run_ticks(clock[0], n)
        clock[0] += n
        ports = [g.read_output(s, 0, n, True) for s in srcs]
        ticks = [[(t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank) for t in d.read_ticks(0, n)] for d in decks]
        states = [(state_tuple(d), d.read_reverb_lines()) for d in decks]
        for d in decks:
            d.close()
        return ports, ticks, states, counts

    ports, ticks, states, counts = run(True)
    want_counts = dict(ZERO)
    for k, c in enumerate(cases):
        (want,), ((t, on, r, cnt),), (lines,), _x = rc.run_model(c, tables)
        assert_bits(ports[k], want, c.name)
        assert states[k][0] == model_state(t, on, r)
        assert_lines(states[k][1], lines, c.name)
        for key in ("decks", "blocks", "blocks_crossing"):
            want_counts[key] += cnt[key]
        want_counts["largest_block"] = max(want_counts["largest_block"], cnt["largest_block"])
    assert counts[0] == want_counts and want_counts["decks"] == 2
    plain_ports, plain_ticks, plain_states, plain_counts = run(False)                 # the same feed with no reverb anywhere: the filter and the echo stay
    assert_bits(ports[2], plain_ports[2], "the deck with no effect")
    assert ticks == plain_ticks and counts[1:] == plain_counts[1:] and plain_counts[0] == ZERO
    assert counts[3]["decks_one_block"] + counts[3]["decks_sequential"] == 1 and counts[4]["decks"] == 1
    assert not np.array_equal(ports[0], plain_ports[0]) and not np.array_equal(ports[1], plain_ports[1])
    assert states[2][0] == plain_states[2][0] == model_state(0, False, rm.ZERO) and not states[2][1].any()


def test_a_schedule_past_the_feed_is_refused_and_everything_stands_where_it_stood(tables):
    case = rc.BY_NAME["designed default, 800 frames a tick"]
    g, srcs, clock = graph_for(case.spt)
    d, m = make_deck(case), ReverbModel()
    xs = rc.deck_samples(case, tables)
    d.schedule(0, c_params(dc.play(ONE, loop=(0, case.n_frames))), 0)
    d.set_reverb(c_rev(rc.DEFAULT))
    m.schedule(0, rc.DEFAULT)

    def feed(at, n, label):
        deck.feed([d], [srcs[0]], g, n)
        g.run_ticks(clock[0], n)
        clock[0] += n
        assert_bits(g.read_output(srcs[0], 0, n, True), m.run(xs[at:at + n].reshape(-1), case.spt), label)
        assert state_tuple(d) == model_state(*m.state())
        assert_lines(d.read_reverb_lines(), m.lines(), label)

    feed(0, 2, "the first feed")
    head, st, lines, counts = d.state(), state_tuple(d), d.read_reverb_lines(), deck.debug_last_reverb()
    d.schedule_reverb(3, c_rev(rc.MID))
    d.schedule_echo(1, c_echo(Echo(300)))
    d.schedule(1, c_params(dc.play(2 * ONE)))
    with pytest.raises(abi.MxError) as e:
        deck.feed([d], [srcs[0]], g, 3)
    assert e.value.code == abi.MX_ERR_INVALID and "reverb" in str(e.value)
    assert state_tuple(d) == st and d.state().pos_q32 == head.pos_q32 and not d.echo_state()[1]
    assert deck.debug_last_reverb() == counts
    assert_bits(d.read_reverb_lines(), lines, "the lines after the refusal")
    feed(2, 2, "the feed after the refusal")           # all three schedules are gone: it plays on as if nothing had been asked
    assert d.state().step_q32 == ONE and not d.echo_state()[1]
    # settings the check refuses never reach the schedule
    with pytest.raises(abi.MxError):
        d.set_reverb(c_rev(rc.MID._replace(diffusion=0.8)))
    with pytest.raises(abi.MxError):
        d.schedule_reverb(1, c_rev(rc.MID._replace(delay=(100,) * 8)))
    feed(4, 2, "after refused settings")
    d.close()


def lone_graph(spt):
    ws = Workspace(*dc.rate_of(spt))
    src = ws.source_stereo()
    return ws.build(max_ticks_per_run=MAX_TICKS), src


def test_a_deck_carried_into_a_second_graph_and_into_another_tick_length_keeps_its_clock_and_lines(tables):
    """A, then B of the same tick length with the deck stopped -- what B's port holds is the tail A left --, then A again, then 441 frames a tick"""
    (ga, sa), (gb, sb), (gc, sc) = lone_graph(800), lone_graph(800), lone_graph(441)
    tr = dc.track("reverb two graphs", 6000)
    d, dm, m, at = deck.Deck(6000), DeckModel(tr.copy(), tables), ReverbModel(), {}
    d.load(tr)

    def play(p, seek=None):
        d.schedule(0, c_params(p), seek)
        dm.schedule(0, p, seek)

    def feed(g, src, spt, n, label):
        deck.feed([d], [src], g, n)
        a = at.get(id(g), 0)
        g.run_ticks(a, n)
        at[id(g)] = a + n
        x = dm.feed(n, spt)[0]
        want = m.run(x, spt)
        assert_bits(g.read_output(src, 0, n, True), want, label)
        assert state_tuple(d) == model_state(*m.state()), label
        assert_lines(d.read_reverb_lines(), m.lines(), label)
        return x, want

    play(dc.play(ONE, loop=(0, 6000)), 0)
    d.set_reverb(c_rev(rc.DEFAULT))
    m.schedule(0, rc.DEFAULT)
    feed(ga, sa, 800, 3, "the first feed")
    play(dc.play(ONE, on=False))
    x, y = feed(gb, sb, 800, 2, "into B")
    assert not x.any() and y.any() and m.t == 5 * 800
    play(dc.play(ONE, loop=(0, 6000)))
    feed(ga, sa, 800, 2, "into A again")
    feed(gc, sc, 441, 3, "into 441 frames a tick")
    assert d.reverb_state()[0] == 7 * 800 + 3 * 441
    d.close(); ga.close(); gb.close(); gc.close()


def test_the_device_equals_mx_deck_reverb_host_on_the_devices_own_input(tables):
    """the port of a feed without the reverb is the device's own input; mx_deck_reverb_host over it equals the port of the same feed with the reverb -- and both the model"""
    case = rc.BY_NAME["schedules inside a feed"]
    (wet,), ((_st, dev_lines, _c),) = check_case(case, tables)
    (plain,), _s = play_case(case, with_reverb=False)
    host, lines, carry = deck.reverb_host(plain, case.spt, [c_rev(r) if r is not None else None for r in rc.settings_per_tick(case)])
    assert_bits(host, wet, "mx_deck_reverb_host on the device's input")
    _p, st, ((_l, mask),), _x = rc.run_model(case, tables)
    assert_bits(lines[mask], dev_lines[mask], "the host's lines against the device's")
    assert (carry.t, bool(carry.on)) == st[-1][:2]
