"""Random deck sessions on the device (tests/random_decks.py; DESIGN.md sections 0.15 and 0.16): the full random graphs of
tests/test_gpu_random_graphs.py with further stereo sources grafted in and a deck, plain or key-locked, on every stereo source -- fed in shuffled
order in most runs, written by the host in the others, with events, set_keylock calls and loads between and inside the runs.  Every materialised
port, every fed deck's tick and grain records, the debug counts and every deck's state, of the fused, unfused, one-tick and second-stream builds,
against the deck models and the oracle bit for bit.  tests/test_cpu_random_decks.py shows what these seeds cover and that each way the device
could get a session wrong changes something compared here.  The last test keeps more feeds in flight than the feed has staging buffers."""
import numpy as np
import pytest

import deck_cases as dc
import deck_keylock_cases as kc
import deck_keylock_model as km
import random_decks as rd
from deck_keylock_model import Keylock
from deck_model import ONE
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace
from random_taps import SETS
from test_gpu_random_graphs import ALL_SETS_RUNS, run_full_graph

pytestmark = pytest.mark.gpu

SEEDS = ([("44k1", s) for s in range(200, 206)] + [("48k", s) for s in range(300, 306)] + [("44k1_100", 400), ("44k1_100", 401), ("16k_1000", 500),
         ("8k_8000", 600)])
TAP_SEEDS = [("44k1", 201), ("44k1", 204), ("48k", 301), ("48k", 302), ("16k_1000", 500), ("8k_8000", 600)]
BUILDS = ("fused", "unfused", "ticked", "overlap")


@pytest.mark.parametrize("shape_id,seed", SEEDS, ids=[f"{s}-{n}" for s, n in SEEDS])
def test_random_deck_session_matches_the_models(shape_id, seed):
    run_full_graph(shape_id, seed, BUILDS, abi.FLAG_EQ_EXACT, decks=rd.session())


@pytest.mark.parametrize("shape_id,seed", TAP_SEEDS, ids=[f"{s}-{n}" for s, n in TAP_SEEDS])
def test_random_deck_session_every_tap_set(shape_id, seed):
    run_full_graph(shape_id, seed, BUILDS, abi.FLAG_EQ_EXACT, tap_sets=SETS, n_runs=ALL_SETS_RUNS, decks=rd.session())


def test_feeds_after_the_graph_of_the_last_feeds_is_gone():
    """Every staging buffer of the feed is last used on a graph that is then destroyed, its stream with it; the feeds after that reuse each buffer,
    and with it the event that says when it is free.  That event once outlived the stream it was recorded on -- the next feed's wait for it was
    refused by the runtime now and then (the sessions above met it) -- so a graph that goes now takes the events recorded on its stream with it."""
    tables = rd.tables()
    spt, n_ticks = dc.CHUNK + 1, 2
    tr = kc.track("music", 2000, "graph gone")
    d, m = deck.Deck(2000), km.KeylockModel(tr.copy(), tables)
    d.load(tr)
    p = dc.play(dc.frames(1.08), loop=(100, 1900))
    d.set(rd.c_params(p)); m.schedule(0, p)
    for gi in range(3):
        ws = Workspace(*dc.rate_of(spt))
        src = ws.source_stereo()
        g = ws.build(max_ticks_per_run=n_ticks)
        for k in range(5):           # more feeds than staging buffers: every buffer's last use is on this graph
            deck.feed([d], [src], g, n_ticks)
            g.run_ticks(k * n_ticks, n_ticks)
            want, _recs, _grains = m.feed(n_ticks, spt)
            got = np.asarray(g.read_output(src, 0, n_ticks, True), np.float32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"graph {gi}, feed {k}"
        g.close()
    d.close()


def test_more_feeds_in_flight_than_staging_slots():
    """Six graphs of 1, 2, 3, 1, 2, 3 stereo sources into a Mixer, a deck per source, plain and key-locked mixed: all six are fed before anything
    runs or is read, so the fifth feed waits for the first one's staging buffer (mx_deck.cpp kSlots = 4); then all run, then all are read.  Once
    more with the graphs in reverse order: a buffer then meets a larger descriptor block than it last held."""
    tables = rd.tables()
    spt, n_ticks = dc.CHUNK + 1, 3
    settings = (None, Keylock(ONE, 256, 64, 5), Keylock(kc.STEP_441, 512, 16, 300))
    graphs = []
    for gi, n_src in enumerate((1, 2, 3, 1, 2, 3)):
        ws = Workspace(*dc.rate_of(spt))
        srcs = [ws.source_stereo() for _ in range(n_src)]
        mix = ws.mixer([(0.0, 1.0, False)] * n_src)
        for k, s in enumerate(srcs):
            ws.connect(s, 0, mix, k)
        decks = []
        for k, s in enumerate(srcs):
            tr = kc.track("music", 4097, f"staging ring {gi} {k}")
            d, m = deck.Deck(4097), km.KeylockModel(tr.copy(), tables)
            d.load(tr)
            p, at = dc.play(dc.frames((0.92, 1.08, 1.0)[(gi + k) % 3])), dc.frames(100.5 + 40 * gi + k)
            d.set(rd.c_params(p)); d.seek(at); m.schedule(0, p, at)
            kl = settings[(gi + 2 * k) % 3]
            if kl is not None:
                d.set_keylock(deck.keylock(*kl)); m.set_keylock(kl)
            decks.append((s, d, m))
        graphs.append((ws.build(max_ticks_per_run=n_ticks), decks))
    assert len(graphs) > 4
    for rnd, order in enumerate((graphs, graphs[::-1])):
        for g, decks in order:
            deck.feed([d for _s, d, _m in decks][::-1], [s for s, _d, _m in decks][::-1], g, n_ticks)
        for g, _decks in order:
            g.run_ticks(rnd * n_ticks, n_ticks)
        for gi, (g, decks) in enumerate(order):
            for s, d, m in decks:
                want, recs, grains = m.feed(n_ticks, spt)
                got = g.read_output(s, 0, n_ticks, True)
                assert np.array_equal(np.asarray(got, np.float32).view(np.uint32), want.view(np.uint32)), f"round {rnd}, graph {gi}, source {s}: the port differs"
                assert [rd.tick_tuple(t) for t in d.read_ticks(0, n_ticks)] == [tuple(t) for t in recs], (rnd, gi, s)
                assert [(x.a_q32, x.g_q32, x.tick, x.frame, x.delta, x.dist, x.flags) for x in d.read_grains()] == [tuple(x) for x in grains], (rnd, gi, s)
    for g, decks in graphs:
        for _s, d, _m in decks:
            d.close()
        g.close()
