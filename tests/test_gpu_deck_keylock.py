"""Key-lock on the device (include/mixlab_gpu.h "KEY-LOCK"): every sample mx_deck_feed writes for a key-locked deck into a SOURCE_STEREO
node's port, every grain record and the debug counts, against the Python model (tests/deck_keylock_model.py) bit for bit over the shared cases
(tests/deck_keylock_cases.py); any grouping of ticks into feeds; plain and key-locked decks in one feed; the identity with the plain deck; fused and unfused graphs;
and the errors, each of which leaves deck, graph and grain state as they were."""
import numpy as np
import pytest

import deck_cases as dc
import deck_keylock_cases as kc
import deck_keylock_model as km
import deck_model as dm
from deck_keylock_cases import KEEP
from deck_keylock_model import Keylock
from deck_model import ONE, PLAY, Params
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

MAX_TICKS, N_SRC = 8, 3


@pytest.fixture(scope="module")
def tables():
    return np.stack([deck.deck_tables(b) for b in range(4)])


_graphs = {}


def graph_for(spt: int, flags: int = 0):
    """one graph per tick length (and flags), shared by the tests: N_SRC stereo sources into a mixer"""
    if (spt, flags) not in _graphs:
        ws = Workspace(*dc.rate_of(spt))
        srcs = [ws.source_stereo() for _ in range(N_SRC)]
        mix = ws.mixer([(0.0, 1.0, False)] * N_SRC)
        for k, s in enumerate(srcs):
            ws.connect(s, 0, mix, k)
        _graphs[(spt, flags)] = (ws.build(max_ticks_per_run=MAX_TICKS, flags=flags), srcs, mix, [0])
    return _graphs[(spt, flags)]


def c_params(p: Params):
    return deck.params(p.step, p.slew, p.loop_in, p.loop_out, p.flags)


def tick_tuple(t):
    return (t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank)


def grain_tuple(g):
    return (g.a_q32, g.g_q32, g.tick, g.frame, g.delta, g.dist, g.flags)


def assert_bits(got, want, label):
    got, want = np.asarray(got, np.float32).reshape(-1), np.asarray(want, np.float32).reshape(-1)
    if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        raise AssertionError(f"{label}: {bad.size} of {got.size} samples differ, first at {bad[0]}: got {got[bad[0]]!r}, want {want[bad[0]]!r}")


COUNT_KEYS = ("grains_searched", "grains_unsearched", "chunks_fading", "chunks_straddling")


def play_case(case, split=None, flags=0):
    """the case on the device, its feeds as given or regrouped by split: ([samples per feed], [tick records], [grain records with the tick counted over the case],
    the debug counts summed)"""
    g, srcs, _mix, clock = graph_for(case.spt, flags)
    d = deck.Deck(case.n_frames)
    d.load(kc.track(case))
    events, calls, t0 = {}, {}, 0
    for f in case.feeds:
        for (t, p, s) in f.events:
            events[t0 + t] = (p, s)
        if f.keylock != KEEP:
            calls[t0] = f.keylock
        t0 += f.n_ticks
    lengths = split if split is not None else [f.n_ticks for f in case.feeds]
    assert sum(lengths) == t0
    samples, recs, grains, counts, at = [], [], [], dict.fromkeys(COUNT_KEYS, 0), 0
    for n in lengths:
        if at in calls:
            d.set_keylock(deck.keylock(*calls[at]) if calls[at] is not None else None)
        for t in range(at, at + n):
            if t in events:
                p, s = events[t]
                d.schedule(t - at, c_params(p) if p is not None else None, s)
        deck.feed([d], [srcs[0]], g, n)
        for k, v in deck.debug_last_keylock().items():
            counts[k] += v
        g.run_ticks(clock[0], n)
        clock[0] += n
        samples.append(g.read_output(srcs[0], 0, n, True))
        recs += [tick_tuple(t) for t in d.read_ticks(0, n)]
        got = d.read_grains()
        assert len(got) == d.grain_count()
        grains += [(x.a_q32, x.g_q32, at + x.tick, x.frame, x.delta, x.dist, x.flags) for x in got]
        at += n
    d.close()
    return samples, recs, grains, counts


def model_grains(results):
    out, at = [], 0
    for _s, recs, grains in results:
        out += [(g.a, g.g, at + g.tick, g.frame, g.delta, g.dist, g.flags) for g in grains]
        at += len(recs)
    return out


_truth = {}


def truth(case, tables):
    if case.name not in _truth:
        _truth[case.name] = kc.run_model(case, tables)
    return _truth[case.name]


@pytest.mark.parametrize("case", kc.CASES, ids=lambda c: c.name)
def test_samples_grains_and_counts_equal_the_model(case, tables):
    got, recs, grains, counts = play_case(case)
    want = truth(case, tables)
    for fi, (w, _r, _g) in enumerate(want):
        assert_bits(got[fi], w, f"{case.name}: feed {fi}")
    assert recs == [tuple(t) for _w, wr, _g in want for t in wr], case.name
    assert grains == model_grains(want), case.name
    assert counts == kc.keylock_counts(case, want), case.name


def test_every_path_ran(tables):
    """mx_deck_debug_last_keylock over a few cases: searched and unsearched grains, fading chunks, chunks with a grain start inside"""
    total = dict.fromkeys(COUNT_KEYS, 0)
    for name in ("spt 257, hop 256", "radius 0", "spt 800, hop 256, more candidates than lanes"):
        for k, v in play_case(kc.BY_NAME[name])[3].items():
            total[k] += v
    assert all(v > 0 for v in total.values()), total


@pytest.mark.parametrize("name", ("spt 257, hop 256", "seek mid-feed", "pause between playing ticks", "spt 255, hop 256"))
def test_any_grouping_of_ticks_into_feeds_gives_the_same_samples_and_grains(name, tables):
    case = kc.BY_NAME[name]
    total = sum(f.n_ticks for f in case.feeds)
    want = truth(case, tables)
    ref, ref_g = np.concatenate([w for w, _r, _g in want]), model_grains(want)
    splits = [[MAX_TICKS] * (total // MAX_TICKS) + ([total % MAX_TICKS] if total % MAX_TICKS else [])]
    if total <= 40:
        splits.append([1] * total)
    for split in splits:
        s, _r, grains, _c = play_case(case, split)
        assert_bits(np.concatenate(s), ref, f"{name}: {split}")
        assert grains == ref_g, split


def test_three_decks_in_one_feed_one_plain_two_key_locked(tables):
    spt = 257
    g, srcs, _mix, clock = graph_for(spt)
    settings = [None, Keylock(ONE, 256, 64, 40), Keylock(kc.STEP_441, 512, 16, 300)]
    steps = [dc.frames(1.08), dc.frames(0.92), dc.frames(1.08)]
    decks, models, alone = [], [], dm.DeckModel(kc.track("music", 4097, "three decks 0"), tables)
    for k, (kl, step) in enumerate(zip(settings, steps)):
        tr = kc.track("music", 4097, f"three decks {k}")
        d, m = deck.Deck(4097), km.KeylockModel(tr, tables)
        d.load(tr)
        p = dc.play(step)
        d.set(c_params(p)); d.seek(dc.frames(100.5 + k)); m.schedule(0, p, dc.frames(100.5 + k))
        if kl is not None:
            d.set_keylock(deck.keylock(*kl)); m.set_keylock(kl)
        decks.append(d); models.append(m)
    alone.schedule(0, dc.play(steps[0]), dc.frames(100.5))
    order = [1, 0, 2]   # the plain deck between the key-locked ones
    for run in range(3):
        deck.feed([decks[i] for i in order], [srcs[i] for i in order], g, 3)
        plain_counts, kl_counts = deck.debug_last_feed(), deck.debug_last_keylock()
        g.run_ticks(clock[0], 3)
        clock[0] += 3
        want = [m.feed(3, spt) for m in models]
        for i in range(3):
            assert_bits(g.read_output(srcs[i], 0, 3, True), want[i][0], f"deck {i}, run {run}")
            assert [grain_tuple(x) for x in decks[i].read_grains()] == [tuple(x) for x in want[i][2]], (i, run)
        assert_bits(g.read_output(srcs[0], 0, 3, True), alone.feed(3, spt)[0], f"the plain deck as if fed alone, run {run}")
        assert plain_counts == dc.launch_counts(want[0][1], spt)                       # the six counters see the plain deck only
        assert kl_counts["grains_searched"] + kl_counts["grains_unsearched"] == len(want[1][2]) + len(want[2][2])
        assert decks[0].grain_count() == 0
    for d in decks:
        d.close()


@pytest.mark.parametrize("step", (ONE, kc.STEP_441), ids=("unity", "44.1 in 48"))
def test_pitch_equal_to_the_step_is_the_plain_decks_feed_bit_for_bit(step, tables):
    spt = 800
    g, srcs, _mix, clock = graph_for(spt)
    tr = kc.track("noise", 4097, "identity")
    a, b = deck.Deck(4097), deck.Deck(4097)
    a.load(tr); b.load(tr)
    for d in (a, b):
        d.set(c_params(dc.play(step))); d.seek(0 if step == ONE else dc.frames(300.37))
    b.set_keylock(deck.keylock(step, 256, 128, 300))
    deck.feed([a, b], [srcs[0], srcs[1]], g, 6)
    g.run_ticks(clock[0], 6)
    clock[0] += 6
    plain = g.read_output(srcs[0], 0, 6, True)
    assert_bits(g.read_output(srcs[1], 0, 6, True), plain, "key-locked against plain")
    assert all(x.delta == 0 and x.dist == 0 for x in b.read_grains()) and b.grain_count() == 6 * 800 // 256 + 1
    if step == ONE:
        want = np.zeros((6 * spt, 2), np.float32)
        want[:4097] = tr.astype(np.float32) / np.float32(32768.0)
        assert_bits(plain, want, "the track itself")
    a.close(); b.close()


@pytest.mark.parametrize("flags", (0, abi.FLAG_NO_FUSE), ids=("fused", "no_fuse"))
def test_through_a_fused_and_an_unfused_graph(flags, tables):
    case = kc.BY_NAME["recommended setting"]
    got, _recs, grains, _counts = play_case(case, flags=flags)
    want = truth(case, tables)
    for fi, (w, _r, _g) in enumerate(want):
        assert_bits(got[fi], w, f"feed {fi}")
    assert grains == model_grains(want)


def test_errors_leave_deck_graph_and_grain_state_as_they_were(tables):
    spt = 257
    g, srcs, mix, clock = graph_for(spt)
    tr = kc.track("music", 3000, "errors")
    d, e, m = deck.Deck(3000), deck.Deck(3000), km.KeylockModel(tr, tables)
    d.load(tr)
    p, kl = dc.play(dc.frames(1.08)), Keylock(ONE, 256, 64, 40)
    d.set(c_params(p)); m.schedule(0, p)
    d.set_keylock(deck.keylock(*kl)); m.set_keylock(kl)

    def good_feed(n, label):
        deck.feed([d], [srcs[0]], g, n)
        g.run_ticks(clock[0], n)
        clock[0] += n
        want, _recs, grains = m.feed(n, spt)
        assert_bits(g.read_output(srcs[0], 0, n, True), want, label)
        assert [grain_tuple(x) for x in d.read_grains()] == [tuple(x) for x in grains], label

    good_feed(2, "before the errors")   # the clock now stands inside a grain: a feed that moved it, or dropped the grain state, would show

    def refused(fn):
        before, n_grains = d.state(), d.grain_count()
        with pytest.raises(abi.MxError) as err:
            fn()
        assert err.value.code == abi.MX_ERR_INVALID, err.value
        after = d.state()
        assert (before.pos_q32, before.step_q32, before.params.flags, n_grains) == (after.pos_q32, after.step_q32, after.params.flags, d.grain_count())
        good_feed(1, "after a refused call")

    refused(lambda: deck.feed([d], [mix], g, 1))                       # not a source
    refused(lambda: deck.feed([d], [99], g, 1))                        # no such node
    refused(lambda: deck.feed([d], [srcs[0]], g, MAX_TICKS + 1))       # more ticks than max_ticks_per_run
    refused(lambda: deck.feed([d], [srcs[0]], g, 0))
    refused(lambda: deck.feed([d, d], [srcs[0], srcs[1]], g, 1))       # a deck twice
    refused(lambda: deck.feed([d, e], [srcs[0], srcs[0]], g, 1))       # a node twice
    d.schedule(3, None, 5 * ONE)
    refused(lambda: deck.feed([d], [srcs[0]], g, 3))                   # an event beyond the feed
    ws = Workspace(*dc.rate_of(spt))
    mono, st = ws.source_mono(), ws.source_stereo()
    g2 = ws.build(max_ticks_per_run=2)
    refused(lambda: deck.feed([d], [mono], g2, 1))                     # a mono source
    ptr, _n = g2.output_device_ptr(mono, 0)
    g2.bind_source_device(st, ptr)
    refused(lambda: deck.feed([d], [st], g2, 1))                       # a bound source
    g2.bind_source_device(st, 0)
    refused(lambda: d.set_keylock(deck.keylock(ONE, 256, 256, 40)))    # settings the check refuses: the deck keeps what it had, and its clock
    refused(lambda: d.set_keylock(deck.keylock(4 * ONE + 1, 256, 64, 40)))
    with pytest.raises(abi.MxError):
        d.read_grains(0, d.grain_count() + 1)
    with pytest.raises(abi.MxError):
        d.read_grains(d.grain_count() + 1, 0)
    assert d.read_grains(d.grain_count(), 0) == []
    # another graph restarts the clock
    deck.feed([d], [st], g2, 2)
    g2.run_ticks(0, 2)
    want, _recs, grains = m.feed(2, spt, graph=1)
    assert grains[0].flags & km.G_FIRST
    assert_bits(g2.read_output(st, 0, 2, True), want, "on another graph")
    assert [grain_tuple(x) for x in d.read_grains()] == [tuple(x) for x in grains]
    d.close(); e.close(); g2.close()
