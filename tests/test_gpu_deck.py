"""The deck on the device (include/mixlab_gpu.h "the deck"): every sample mx_deck_feed writes into a SOURCE_STEREO node's port, and every
record it keeps, against the Python model (tests/deck_model.py) bit for bit, over the shared cases (tests/deck_cases.py): tick lengths around the kernel's chunk,
tracks shorter than the filter, heads outside the track, every bank edge, slews, loops of a frame, several decks in one feed, any grouping of ticks into feeds,
through fused, unfused and second-stream graphs, and the errors, each of which leaves graph and deck as they were."""
import numpy as np
import pytest

import deck_cases as dc
import deck_model as dm
import oracle
from deck_model import ONE, PLAY, Params
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

MAX_TICKS, N_SRC = 8, 5


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
        _graphs[spt] = (ws.build(max_ticks_per_run=MAX_TICKS), srcs, mix, [0])
    return _graphs[spt]


def c_params(p: Params):
    return deck.params(p.step, p.slew, p.loop_in, p.loop_out, p.flags)


def tick_tuple(t):
    return (t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank)


def assert_bits(got, want, label):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{label}: {bad.size} of {got.size} samples differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


def play_case(case, tables, split=None):
    """the case on the device, its feeds as given or regrouped by split (a list of feed lengths over the same ticks): ([samples per feed], [records], counts summed)"""
    g, srcs, _mix, clock = graph_for(case.spt)
    d = deck.Deck(case.n_frames)
    d.load(dc.track(case))
    events = {}
    t0 = 0
    for f in case.feeds:
        for (t, p, s) in f.events:
            events[t0 + t] = (p, s)
        t0 += f.n_ticks
    lengths = split if split is not None else [f.n_ticks for f in case.feeds]
    assert sum(lengths) == t0
    samples, recs, counts, at = [], [], dict.fromkeys(dc.launch_counts([], case.spt), 0), 0
    for n in lengths:
        for t in range(at, at + n):
            if t in events:
                p, s = events[t]
                d.schedule(t - at, c_params(p) if p is not None else None, s)
        deck.feed([d], [srcs[0]], g, n)
        for k, v in deck.debug_last_feed().items():
            counts[k] += v
        g.run_ticks(clock[0], n)
        clock[0] += n
        samples.append(g.read_output(srcs[0], 0, n, True))
        recs += [tick_tuple(t) for t in d.read_ticks(0, n)]
        at += n
    d.close()
    return samples, recs, counts


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_samples_records_and_launch_counts_equal_the_model(case, tables):
    got, recs, counts = play_case(case, tables)
    want = dc.run_model(case, tables)
    want_counts = dict.fromkeys(counts, 0)
    for fi, (w, wrecs) in enumerate(want):
        assert_bits(got[fi], w, f"{case.name}: feed {fi}")
        for k, v in dc.launch_counts(wrecs, case.spt).items():
            want_counts[k] += v
    assert recs == [tuple(t) for _w, wr in want for t in wr], case.name
    assert counts == want_counts, case.name


def test_every_kernel_form_ran(tables):
    """mx_deck_debug_last_feed over three cases: zeros, streaming chunks, gathered chunks -- in ticks of several chunks"""
    total = dict.fromkeys(dc.launch_counts([], 1), 0)
    for name in ("far past the end", "long loop", "loop of three frames at step 4", "back-spin", "pause and resume"):
        for k, v in play_case(dc.BY_NAME[name], tables)[2].items():
            total[k] += v
    assert all(v > 0 for v in total.values()), total
    assert total["chunks_stream"] > total["ticks_stream"] and total["chunks_gather"] > total["ticks_gather"]


def test_unity_from_frame_0_returns_the_uploaded_track(tables):
    case = dc.BY_NAME["unity from frame 0"]
    (got,), _recs, _counts = play_case(case, tables)
    want = np.zeros((6 * 800, 2), np.float32)
    want[:4097] = dc.track(case).astype(np.float32) / np.float32(32768.0)
    assert_bits(got, want, "transparency")


@pytest.mark.parametrize("spt", (735, dc.CHUNK + 1))
def test_any_grouping_of_ticks_into_feeds_gives_the_same_samples_and_records(spt, tables):
    case = dc.BY_NAME[f"random stream, {spt} frames a tick"]
    total = sum(f.n_ticks for f in case.feeds)
    ref_s, ref_r, _ = play_case(case, tables)
    ref = np.concatenate(ref_s)
    assert_bits(ref, np.concatenate([w for w, _r in dc.run_model(case, tables)]), "as given")
    uneven, left, k = [], total, 0
    while left:
        uneven.append(min((3, 1, MAX_TICKS, 2, 5)[k % 5], left))
        left -= uneven[-1]
        k += 1
    for label, split in (("tick by tick", [1] * total), ("uneven", uneven), ("largest feeds", [MAX_TICKS] * (total // MAX_TICKS) + ([total % MAX_TICKS] if total % MAX_TICKS else []))):
        s, r, _ = play_case(case, tables, split)
        assert_bits(np.concatenate(s), ref, label)
        assert r == ref_r, label


def test_five_decks_of_different_lengths_and_states_in_one_feed(tables):
    spt = dc.CHUNK + 1
    g, srcs, mix, clock = graph_for(spt)
    setups = [(1, dc.play(dc.frames(0.92)), dc.frames(-40.25)), (31, dc.play(-dc.frames(1.08)), dc.frames(61.5)), (33, dc.play(ONE, on=False), 0),
              (4097, dc.play(dc.frames(1.08), loop=(100, 350)), dc.frames(120.5)), (4097, dc.play(4 * ONE, slew=1 << 24), dc.frames(10))]
    decks, models = [], []
    for k, (n, p, s) in enumerate(setups):
        tr = dc.track(f"five decks {k}", n)
        d, m = deck.Deck(n), dm.DeckModel(tr, tables)
        d.load(tr)
        d.set(c_params(p)); d.seek(s); m.schedule(0, p, s)
        d.schedule(2, None, dc.frames(3.25)); m.schedule(2, None, dc.frames(3.25))
        decks.append(d); models.append(m)
    order = [3, 0, 4, 1, 2]   # decks and nodes in no particular order
    for run in range(2):
        deck.feed([decks[i] for i in order], [srcs[i] for i in order], g, 3)
        g.run_ticks(clock[0], 3)
        clock[0] += 3
        want = [m.feed(3, spt) for m in models]
        for i in range(5):
            assert_bits(g.read_output(srcs[i], 0, 3, True), want[i][0], f"deck {i}, run {run}")
            assert [tick_tuple(t) for t in decks[i].read_ticks(0, 3)] == [tuple(t) for t in want[i][1]], i
        # the mixer's master bus is what the oracle makes of the model's samples
        ws = Workspace(*dc.rate_of(spt))
        s2 = [ws.source_stereo() for _ in range(N_SRC)]
        m2 = ws.mixer([(0.0, 1.0, False)] * N_SRC)
        for k, s in enumerate(s2):
            ws.connect(s, 0, m2, k)
        og = oracle.OracleGraph(ws)
        bus = g.read_output(mix, 0, 3, True)
        for t in range(3):
            for i in range(5):
                og.set_source(s2[i], want[i][0][t * 2 * spt:(t + 1) * 2 * spt])
            og.run_tick(t)
            assert_bits(bus[t * 2 * spt:(t + 1) * 2 * spt], og.output(m2, 0), f"master bus, run {run} tick {t}")
    h = decks[2].state()
    assert (h.pos_q32, h.step_q32) == (models[2].head.pos, models[2].head.step)
    for d in decks:
        d.close()


def strip_ws(direct: bool):
    """deck -> SOURCE_STEREO -> splitter -> EqThree -> panner -> Mixer, and (direct) the source into the Mixer as well"""
    ws = Workspace(48000, 60)
    src = ws.source_stereo()
    sp, eq, pan = ws.stereo_splitter(), ws.eq_three(3.0, -2.0, 1.5), ws.stereo_panner()
    mix = ws.mixer([(-3.0, 0.8, False), (0.0, 1.0, True)] if direct else [(-3.0, 0.8, False)])
    ws.connect(src, 0, sp, 0); ws.connect(sp, 0, eq, 0); ws.connect(eq, 0, pan, 0); ws.connect(eq, 0, pan, 1); ws.connect(pan, 0, mix, 0)
    if direct:
        ws.connect(src, 0, mix, 1)
    return ws, src, mix


@pytest.mark.parametrize("flags,direct", [(0, True), (abi.FLAG_NO_FUSE, True), (abi.FLAG_OVERLAP_TAIL, False)], ids=["fused", "no_fuse", "overlap_tail"])
def test_through_the_graph_over_consecutive_runs(flags, direct, tables):
    ws, src, mix = strip_ws(direct)
    spt, n = ws.spt, 4
    g = ws.build(max_ticks_per_run=n, flags=flags | abi.FLAG_EQ_EXACT)
    assert bool(g.tail_stream()) == bool(flags & abi.FLAG_OVERLAP_TAIL)   # the Mixer really runs on the second stream there: the ports it reads alternate
    og = oracle.OracleGraph(ws)
    tr = dc.track("through the graph", 4097)
    d, m = deck.Deck(4097), dm.DeckModel(tr, tables)
    d.load(tr)
    p = dc.play(dc.frames(1.08), loop=(500, 3500))
    d.set(c_params(p)); d.seek(dc.frames(600.5)); m.schedule(0, p, dc.frames(600.5))
    for run in range(4):   # both parities of a double-buffered port are written twice
        if run == 2:
            q = dc.play(-dc.frames(0.92), slew=dc.frames(2.0) // 1000, loop=(500, 3500))
            d.schedule(1, c_params(q)); m.schedule(1, q)
        deck.feed([d], [src], g, n)
        g.run_ticks(run * n, n)
        want, _recs = m.feed(n, spt)
        assert_bits(g.read_output(src, 0, n, True), want, f"source port, run {run}")
        bus = g.read_output(mix, 0, n, True)
        for t in range(n):
            og.set_source(src, want[t * 2 * spt:(t + 1) * 2 * spt])
            og.run_tick(run * n + t)
            assert_bits(bus[t * 2 * spt:(t + 1) * 2 * spt], og.output(mix, 0), f"master bus, run {run} tick {t}")
    d.close(); g.close()


def test_a_load_issued_after_a_feed_is_seen_by_the_next_feed(tables):
    spt = dc.CHUNK
    g, srcs, _mix, clock = graph_for(spt)
    tr = dc.track("load behind a feed", 2000)
    d, m = deck.Deck(2000), dm.DeckModel(np.zeros((2000, 2), np.int16), tables)
    p = dc.play(dc.frames(0.92))
    d.set(c_params(p)); m.schedule(0, p)
    for piece in (None, (0, 700), (700, 2000)):
        if piece:
            d.load(tr[piece[0]:piece[1]], piece[0]); m.load(piece[0], tr[piece[0]:piece[1]])
        deck.feed([d], [srcs[1]], g, 2)
        g.run_ticks(clock[0], 2)
        clock[0] += 2
        want, _ = m.feed(2, spt)
        assert_bits(g.read_output(srcs[1], 0, 2, True), want, f"after loading {piece}")
        assert (want != 0).any() == bool(piece)
    d.close()


def test_errors_leave_graph_and_deck_usable(tables):
    spt = dc.CHUNK + 1
    g, srcs, mix, clock = graph_for(spt)
    ws = Workspace(*dc.rate_of(spt))
    mono = ws.source_mono()
    st = ws.source_stereo()
    g2 = ws.build(max_ticks_per_run=2)
    tr = dc.track("errors", 500)
    d, e, m = deck.Deck(500), deck.Deck(500), dm.DeckModel(tr, tables)
    d.load(tr)
    p = dc.play(dc.frames(1.08))
    d.set(c_params(p)); m.schedule(0, p)

    def refused(fn):
        before = d.state()
        with pytest.raises(abi.MxError) as err:
            fn()
        assert err.value.code == abi.MX_ERR_INVALID, err.value
        after = d.state()
        assert (before.pos_q32, before.step_q32, before.params.flags) == (after.pos_q32, after.step_q32, after.params.flags)

    refused(lambda: deck.feed([d], [mix], g, 1))                       # not a source
    refused(lambda: deck.feed([d], [mono], g2, 1))                     # a mono source
    refused(lambda: deck.feed([d], [99], g, 1))                        # no such node
    refused(lambda: deck.feed([d], [srcs[0]], g, MAX_TICKS + 1))       # more ticks than max_ticks_per_run
    refused(lambda: deck.feed([d], [srcs[0]], g, 0))
    refused(lambda: deck.feed([d, d], [srcs[0], srcs[1]], g, 1))       # a deck twice
    refused(lambda: deck.feed([d, e], [srcs[0], srcs[0]], g, 1))       # a node twice
    ptr, _n = g2.output_device_ptr(mono, 0)
    g2.bind_source_device(st, ptr)
    refused(lambda: deck.feed([d], [st], g2, 1))                       # a bound source
    g2.bind_source_device(st, 0)
    refused(lambda: d.set(c_params(Params(4 * ONE + 1, 0, 0, 0, PLAY))))
    refused(lambda: d.schedule(0, c_params(Params(ONE, 0, 400, 501, PLAY | dm.LOOP))))
    # every refused feed dropped the deck's schedule with it; set it again, and one scheduled beyond the feed is refused too
    d.set(c_params(p))
    d.schedule(3, None, 5 * ONE)
    refused(lambda: deck.feed([d], [srcs[0]], g, 3))
    with pytest.raises(abi.MxError):
        d.read_ticks(0, 1)                                             # no feed yet
    d.set(c_params(p))
    for gg, node in ((g, srcs[0]), (g2, st)):
        deck.feed([d], [node], gg, 2)
        gg.run_ticks(clock[0], 2)
        want, _ = m.feed(2, spt)
        assert_bits(gg.read_output(node, 0, 2, True), want, "after the errors")
    clock[0] += 2
    with pytest.raises(abi.MxError):
        d.read_ticks(1, 2)
    for bad in (lambda: deck.Deck(0), lambda: deck.Deck((1 << 30) + 1), lambda: d.load(np.zeros(4, np.int16), 499)):
        with pytest.raises(abi.MxError):
            bad()
    d.close(); e.close(); g2.close()
