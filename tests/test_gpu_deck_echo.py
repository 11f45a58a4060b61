"""The deck's echo on the device (include/mixlab_gpu.h "ECHO"): every sample of a SOURCE_STEREO node's port after mx_deck_feed, bit for bit
against the Python model (tests/deck_echo_model.py) applied to what DeckModel / KeylockModel say the deck wrote, over the shared cases (tests/deck_echo_cases.py):
every delay of the list in one feed of 12 ticks (the sequential form, blocks across tick boundaries) and tick by tick (the one-block form where D > spt), the
schedule inside a feed under three groupings, the echo-out plain, key-locked and looped, the subnormal tail, the ring wrap at the longest delay, several decks in one
feed, the refusals, which leave deck and echo where they stood, the suite's tiny ticks (16 frames and one frame), and what the header's CLOCK paragraph says does
not restart the clock or clear the line: a feed into another graph handle, of the same tick length or another, a graph that adopted the last one's state, a load and
mx_deck_set_keylock."""
import copy

import numpy as np
import pytest

import deck_cases as dc
import deck_echo_cases as ec
import deck_echo_model as em
from deck_echo_model import OFF, PINGPONG, Echo
from deck_keylock_model import Keylock, KeylockModel
from deck_model import ONE
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

MAX_TICKS, N_SRC = 16, 3
KEYS = ("decks_one_block", "decks_sequential", "blocks", "blocks_crossing")


@pytest.fixture(scope="module")
def tables():
    return np.stack([deck.deck_tables(b) for b in range(4)])


_graphs = {}


def graph_for(spt: int):
    """one graph per tick length, shared by the tests: N_SRC stereo sources into a mixer; at the longest tick one source feeding nothing"""
    if spt not in _graphs:
        if spt == ec.LONG_SPT:
            ws = Workspace(spt, 1)
            srcs = [ws.source_stereo()]
            _graphs[spt] = (ws.build(max_ticks_per_run=1), srcs, [0])
        else:
            ws = Workspace(*dc.rate_of(spt))
            srcs = [ws.source_stereo() for _ in range(N_SRC)]
            mix = ws.mixer([(0.0, 1.0, False)] * N_SRC)
            for k, s in enumerate(srcs):
                ws.connect(s, 0, mix, k)
            _graphs[spt] = (ws.build(max_ticks_per_run=max(MAX_TICKS, ec.LONG_FEEDS.get(spt, 0))), srcs, [0])
    return _graphs[spt]


def c_params(p):
    return deck.params(p.step, p.slew, p.loop_in, p.loop_out, p.flags)


def c_echo(e: Echo):
    return abi.DeckEcho(e.delay, e.flags, e.send, e.feedback, e.wet, e.damp)


def state_tuple(d):
    t, on, e = d.echo_state()
    return t, on, (e.delay, e.flags, e.send, e.feedback, e.wet, e.damp)


def model_state(st):
    t, on, e = st
    return t, on, (e.delay, e.flags, *(float(np.float32(v)) for v in (e.send, e.feedback, e.wet, e.damp)))


def assert_bits(got, want, label):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{label}: {bad.size} of {got.size} samples differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


def make_deck(case):
    d = deck.Deck(case.n_frames)
    d.load(ec.track(case))
    if case.keylock:
        k = case.keylock
        d.set_keylock(deck.keylock(k.pitch, k.hop, k.overlap, k.radius))
    return d


def play_case(case, split=None):
    """the case on the device, its feeds as given or regrouped by split: ([port per feed], [echo_state after each feed], mx_deck_debug_last_echo summed)"""
    g, srcs, clock = graph_for(case.spt)
    d = make_deck(case)
    total, deck_ev, echo_ev = ec.flatten(case)
    lengths = split if split is not None else [f.n_ticks for f in case.feeds]
    assert sum(lengths) == total
    ports, states, counts, at = [], [], dict.fromkeys(KEYS, 0), 0
    for n in lengths:
        for t in range(at, at + n):
            if t in deck_ev:
                p, s = deck_ev[t]
                d.schedule(t - at, c_params(p) if p is not None else None, s)
            if t in echo_ev:
                d.schedule_echo(t - at, None if echo_ev[t] is OFF else c_echo(echo_ev[t]))
        deck.feed([d], [srcs[0]], g, n)
        for k, v in deck.debug_last_echo().items():
            counts[k] += v
        g.run_ticks(clock[0], n)
        clock[0] += n
        ports.append(g.read_output(srcs[0], 0, n, True))
        states.append(state_tuple(d))
        at += n
    d.close()
    return ports, states, counts


def model_counts(case, lengths=None):
    """mx_deck_debug_last_echo summed over the case's feeds, from the model's cutter"""
    c = dict.fromkeys(KEYS, 0)
    for delays in ec.delays_of(case, lengths):
        blocks = em.cut(case.spt, delays)
        if not blocks:
            continue
        if len(blocks) == 1:
            c["decks_one_block"] += 1
            continue
        c["decks_sequential"] += 1
        c["blocks"] += len(blocks)
        c["blocks_crossing"] += sum(1 for first, n in blocks if first // case.spt != (first + n - 1) // case.spt)
    return c


def check_case(case, tables, split=None):
    ports, states, counts = play_case(case, split)
    want, want_states = ec.run_model(case, tables, split=split)
    for fi, w in enumerate(want):
        assert_bits(ports[fi], w, f"{case.name}: feed {fi} of {split or 'the case'}")
    assert states == [model_state(s) for s in want_states], case.name
    assert counts == model_counts(case, split), case.name
    return ports, states, counts


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.name)
def test_ports_state_and_forms_equal_the_model(case, tables):
    check_case(case, tables)


# a tick of spt frames is one block when spt <= D - 1 (the header's BLOCKS)
ONE_BLOCK = [c for c in ec.CASES if c.spt != ec.LONG_SPT and min(d for ds in ec.delays_of(c) for d in ds if d) > c.spt]


@pytest.mark.parametrize("case", ONE_BLOCK, ids=lambda c: c.name)
def test_tick_by_tick_every_feed_takes_the_one_block_form_and_equals_the_model(case, tables):
    total = ec.flatten(case)[0]
    _p, _s, counts = check_case(case, tables, [1] * total)
    # a tick with the echo off launches none: the one case whose echo is off for a while, ticks 500 .. 519 of 600, has 20 feeds fewer
    assert counts["decks_one_block"] == (total - 20 if case.name == "one frame a tick" else total) and counts["decks_sequential"] == 0
    assert counts["decks_one_block"] == sum(1 for (d,) in ec.delays_of(case, [1] * total) if d)


def test_the_list_of_one_block_cases_holds_the_delays_just_above_the_threshold():
    names = {c.name for c in ONE_BLOCK}
    assert {"delay 442, 441 frames a tick", "delay 801, 800 frames a tick", "delay 802, 800 frames a tick", "delay 5000, 800 frames a tick", "echo-out under key-lock"} <= names
    assert "delay 441, 441 frames a tick" not in names and "delay 800, 800 frames a tick" not in names     # D = spt is two blocks: spt - 1 frames and one


@pytest.mark.parametrize("name", ("schedules inside a feed", "delay 256, 441 frames a tick", "delay 801, 800 frames a tick", "delay 257, 16 frames a tick", "one frame a tick"))
def test_any_grouping_of_ticks_into_feeds_gives_the_same_ports_and_echo_state(name, tables):
    case = ec.BY_NAME[name]
    total = ec.flatten(case)[0]
    (ref,), (ref_state,), _ = check_case(case, tables)                       # one feed of 12, 64 or 600
    for split in ([1] * total, [5, total - 5]):
        ports, states, _ = check_case(case, tables, split)
        assert_bits(np.concatenate(ports), ref, f"{name}: {split}")
        assert states[-1] == ref_state


def test_both_forms_ran_and_a_block_crossed_a_tick_boundary(tables):
    case = ec.BY_NAME["delay 5000, 800 frames a tick"]
    _p, _s, seq = play_case(case)
    assert seq == {"decks_one_block": 0, "decks_sequential": 1, "blocks": 2, "blocks_crossing": 2}       # 4999 frames, then the other 4601
    _p, _s, one = play_case(case, [1] * 12)
    assert one == {"decks_one_block": 12, "decks_sequential": 0, "blocks": 0, "blocks_crossing": 0}


def test_the_subnormal_tail_reaches_the_device_unflushed(tables):
    case = ec.BY_NAME["subnormal tail"]
    ports, _s, _c = check_case(case, tables)
    last = np.abs(ports[-1])
    tiny = np.finfo(np.float32).tiny
    assert np.count_nonzero((last > 0) & (last < tiny)) > 100      # subnormals in the port, and (check_case) each the model's bit for bit


def test_the_freeze_recirculates_bit_for_bit_on_the_device(tables):
    case = ec.BY_NAME["freeze"]
    (port,), _s, _c = check_case(case, tables)
    y = port.reshape(-1, 2)
    end = 4097 + 440                                                # the track is over and its last frames have come round once
    first = -(-end // 440) * 440
    for k in range(first + 440, 14 * 441 - 440, 440):
        assert_bits(y[k:k + 440], y[first:first + 440], f"pass at {k}")
    assert y[first:first + 440].any()


def test_a_schedule_past_the_feed_is_refused_and_deck_and_echo_stand_where_they_stood(tables):
    case = ec.BY_NAME["delay 802, 800 frames a tick"]
    g, srcs, clock = graph_for(case.spt)
    d = make_deck(case)
    d.schedule(0, c_params(dc.play(ONE)), 0)
    d.set_echo(c_echo(Echo(802)))
    deck.feed([d], [srcs[0]], g, 2)
    g.run_ticks(clock[0], 2)
    clock[0] += 2
    head, st, counts = d.state(), state_tuple(d), deck.debug_last_echo()
    d.schedule_echo(3, c_echo(Echo(300)))
    d.schedule(1, c_params(dc.play(2 * ONE)))
    with pytest.raises(abi.MxError) as e:
        deck.feed([d], [srcs[0]], g, 3)
    assert e.value.code == abi.MX_ERR_INVALID and "echo" in str(e.value)
    assert state_tuple(d) == st and d.state().pos_q32 == head.pos_q32 and deck.debug_last_echo() == counts
    # ... both schedules are gone: the next feed plays on as if nothing had been asked
    deck.feed([d], [srcs[0]], g, 2)
    g.run_ticks(clock[0], 2)
    clock[0] += 2
    got = g.read_output(srcs[0], 0, 2, True)
    want, states = ec.run_model(case, tables, split=[2, 2, 8])
    assert_bits(got, want[1], "the feed after the refusal")
    assert state_tuple(d) == model_state(states[1]) and d.state().step_q32 == ONE
    # settings the check refuses never reach the schedule
    with pytest.raises(abi.MxError):
        d.set_echo(c_echo(Echo(255)))
    with pytest.raises(abi.MxError):
        d.schedule_echo(1, c_echo(Echo(300, feedback=1.5)))
    deck.feed([d], [srcs[0]], g, 2)
    g.run_ticks(clock[0], 2)
    clock[0] += 2
    assert state_tuple(d)[2][0] == 802
    d.close()


def test_two_decks_with_different_echoes_and_a_third_without_in_one_feed(tables):
    spt, n = 800, 4
    g, srcs, clock = graph_for(spt)
    cases = [ec.Case(f"three decks {k}", spt, 4097, [ec.Feed(n, [(0, dc.play(step), seek)], [(0, e)] if e else [])])
             for k, (step, seek, e) in enumerate(((ONE, 0, Echo(256, 1.0, 0.7, 1.0, 0.3)), (dc.frames(1.08), dc.frames(40.5), Echo(5000, 1.0, 0.5, 2.0, 0.0, PINGPONG)),
                                                  (dc.frames(0.92), dc.frames(10.25), None)))]

    def run(with_echo: bool):
        decks = [make_deck(c) for c in cases]
        for d, c in zip(decks, cases):
            (_t, p, s), = c.feeds[0].deck
            d.schedule(0, c_params(p), s)
            if with_echo and c.feeds[0].echo:
                d.set_echo(c_echo(c.feeds[0].echo[0][1]))
        deck.feed(decks, srcs, g, n)
        counts, last_feed = deck.debug_last_echo(), deck.debug_last_feed()
        g.run_ticks(clock[0], n)
        clock[0] += n
        ports = [g.read_output(s, 0, n, True) for s in srcs]
        ticks = [[(t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank) for t in d.read_ticks(0, n)] for d in decks]
        states = [state_tuple(d) for d in decks]
        for d in decks:
            d.close()
        return ports, ticks, states, counts, last_feed

    ports, ticks, states, counts, last_feed = run(True)
    for k, c in enumerate(cases):
        (want,), (st,) = ec.run_model(c, tables)
        assert_bits(ports[k], want, c.name)
        assert states[k] == model_state(st)
    # deck 0 has 256 < spt + 2: sequential; deck 1's 5000 covers the 3200 frames of the feed: one block
    assert counts == {"decks_one_block": 1, "decks_sequential": 1, "blocks": len(em.cut(spt, [256] * n)), "blocks_crossing": model_counts(cases[0])["blocks_crossing"]}
    plain_ports, plain_ticks, plain_states, plain_counts, plain_last_feed = run(False)
    assert_bits(ports[2], plain_ports[2], "the deck without an echo")
    assert ticks == plain_ticks and last_feed == plain_last_feed
    assert states[2] == plain_states[2] == (0, False, (0, 0, 0.0, 0.0, 0.0, 0.0))
    assert plain_counts == dict.fromkeys(KEYS, 0)             # a feed in which no deck has an echo


def test_a_feed_in_which_the_echo_is_off_in_every_tick_launches_no_echo(tables):
    case = ec.BY_NAME["delay 802, 800 frames a tick"]
    g, srcs, clock = graph_for(case.spt)
    d = make_deck(case)
    d.schedule(0, c_params(dc.play(ONE)), 0)
    d.set_echo(c_echo(Echo(802)))
    deck.feed([d], [srcs[0]], g, 1)
    assert deck.debug_last_echo()["decks_one_block"] == 1
    g.run_ticks(clock[0], 1)
    d.set_echo(None)
    deck.feed([d], [srcs[0]], g, 2)
    assert deck.debug_last_echo() == dict.fromkeys(KEYS, 0)
    g.run_ticks(clock[0] + 1, 2)
    clock[0] += 3
    (x0, x1) = ec.deck_samples(case, tables, [1, 2, 9])[:2]
    assert_bits(g.read_output(srcs[0], 0, 2, True), x1, "echo off: the deck's own samples")
    t, on, e = state_tuple(d)
    assert (t, on, e[0]) == (800, False, 802)
    d.close()


# ---- "nothing else restarts the clock or clears the line": one deck and one EchoModel carried across every feed ----
class Carried:
    """an echoing deck with its models.  feed() plays n ticks into whatever graph, holds the port and the echo state to the models, and shows that the line
    mattered: the same feed over a line of zeros would have given other samples"""

    def __init__(self, tables, name, n_frames=12000):
        tr = dc.track("echo " + name, n_frames)
        self.d, self.m, self.e, self.at = deck.Deck(n_frames), KeylockModel(tr.copy(), tables), em.EchoModel(), {}
        self.d.load(tr)

    def play(self, p, seek=None):
        self.d.schedule(0, c_params(p), seek)
        self.m.schedule(0, p, seek)

    def feed(self, g, src, spt, n, label, ringing=True):
        deck.feed([self.d], [src], g, n)
        at = self.at.get(id(g), 0)
        g.run_ticks(at, n)
        self.at[id(g)] = at + n
        x = self.m.feed(n, spt)[0]
        cleared = copy.deepcopy(self.e)
        cleared.hist[:] = 0
        want = self.e.run(x, spt)
        assert_bits(g.read_output(src, 0, n, True), want, label)
        assert state_tuple(self.d) == model_state(self.e.state()), label
        assert not ringing or not np.array_equal(want.view(np.uint32), cleared.run(x, spt).view(np.uint32)), f"{label}: the line is not heard"
        return x, want


def lone_graph(spt, like=None):
    """(Workspace, graph, node) of one stereo source feeding nothing; like: the Workspace to build once more"""
    ws = like or Workspace(*dc.rate_of(spt))
    src = 0 if like else ws.source_stereo()
    return ws, ws.build(max_ticks_per_run=MAX_TICKS), src


def ringing_deck(tables, name, g, src, spt):
    c = Carried(tables, name)
    c.play(dc.play(ONE), 0)
    e = Echo(900, 1.0, 0.7, 1.0, 0.3, PINGPONG)
    c.d.set_echo(c_echo(e))
    c.e.schedule(0, e)
    c.feed(g, src, spt, 3, f"{name}: the first feed", ringing=False)
    return c


def test_a_feed_into_another_graph_handle_neither_restarts_the_clock_nor_clears_the_line(tables):
    """A, then B of the same tick length with the deck stopped -- what B's port holds is the line A wrote --, then A again"""
    (_wa, ga, sa), (_wb, gb, sb) = lone_graph(800), lone_graph(800)
    c = ringing_deck(tables, "two graphs", ga, sa, 800)
    c.play(dc.play(ONE, on=False))
    x, y = c.feed(gb, sb, 800, 2, "into B")
    assert not x.any() and y.any()
    c.play(dc.play(ONE))
    c.feed(ga, sa, 800, 3, "into A again")
    assert state_tuple(c.d)[0] == 8 * 800
    c.d.close(); ga.close(); gb.close()


def test_a_graph_of_another_tick_length_takes_the_deck_with_clock_and_line_as_they_stand(tables):
    (_wa, ga, sa), (_wb, gb, sb) = lone_graph(800), lone_graph(441)
    c = ringing_deck(tables, "two tick lengths", ga, sa, 800)
    c.feed(gb, sb, 441, 5, "into 441 frames a tick")          # D = 900 covers two ticks of 441: a walk of blocks where A's ticks were one block each
    assert state_tuple(c.d)[0] == 3 * 800 + 5 * 441
    c.feed(ga, sa, 800, 2, "back into 800 frames a tick")
    assert state_tuple(c.d)[0] == 5 * 800 + 5 * 441
    c.d.close(); ga.close(); gb.close()


def test_a_graph_that_adopted_the_state_of_the_one_last_fed_goes_on_with_clock_and_line(tables):
    ws, ga, src = lone_graph(800)
    c = ringing_deck(tables, "adopted", ga, src, 800)
    _ws, gb, _src = lone_graph(800, like=ws)
    gb.adopt_state(ga, [0])
    c.at[id(gb)] = c.at[id(ga)]
    c.feed(gb, src, 800, 4, "into the graph built anew")
    assert state_tuple(c.d)[0] == 7 * 800
    c.d.close(); ga.close(); gb.close()


def test_a_load_and_set_keylock_on_and_off_between_feeds_leave_clock_and_line(tables):
    _ws, g, src = lone_graph(800)
    c = ringing_deck(tables, "load and key-lock", g, src, 800)
    piece = dc.track("echo load and key-lock, loaded", 3000)             # over the frames the head plays next (it stands at 2400)
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
    assert state_tuple(c.d)[0] == 9 * 800
    c.d.close(); g.close()
