"""Random graph sessions with topology edits (tests/random_edits.py): the full random graphs of tests/test_gpu_random_graphs.py through
4-7 runs of 1-6 ticks with an edit before about half of the runs -- modules go, new ones come, some come back, connections are drawn again,
the node order is permuted -- each edit a new graph that adopts the old one's state (mx_graph_adopt_state).  Every build against the
oracle's graph runner with OracleGraph.adopt_state, bit for bit: every materialised port, the meter records (taps are not carried: set
again, from 0), the OutputDevice hand-offs and records (the module persists), every Plotter's indication of every tick.

What is under test is the state carry: Graph::state_locs finds each state by launch group and slot in two different builds, an Envelope's
in its own group or in the EqThree group that evaluates it inline, a Fir's or Resample's at an offset inside a shared group.  The "mixed"
build alternates between the fused layout and MX_FLAG_NO_FUSE from edit to edit.  tests/test_cpu_random_edits.py shows what these draws
cover, that the expected side's adopt is right, and that each way the device's could be wrong changes the values compared here."""
import numpy as np
import pytest

import oracle
from mixlab_amd import abi
from random_edits import EDIT_SEEDS, SPECIAL, run_edit_session
from tick_shapes import FAR_EPOCHS, by_id, far_first_tick

pytestmark = pytest.mark.gpu

IDS = [f"{s}-{n}" for s, n in EDIT_SEEDS]


@pytest.mark.parametrize("shape_id,seed", EDIT_SEEDS, ids=IDS)
def test_random_edit_sessions_match_the_oracle(shape_id, seed):
    assert len(EDIT_SEEDS) == 16 and {s for s, _ in EDIT_SEEDS} == {"44k1", "48k", "44k1_100", "16k_1000", "8k_8000"}
    run_edit_session(shape_id, seed, ("fused", "unfused", "ticked", "overlap", "mixed"), abi.FLAG_EQ_EXACT, special=SPECIAL.get((shape_id, seed)))


@pytest.mark.parametrize("shape_id,seed", EDIT_SEEDS[::3], ids=IDS[::3])
def test_random_edit_sessions_contracted_match_the_contract_oracle(shape_id, seed):
    with oracle.fp_contract():
        run_edit_session(shape_id, seed, ("fused", "unfused"), abi.FLAG_FP_CONTRACT, special=SPECIAL.get((shape_id, seed)))


FAR_SEEDS = [EDIT_SEEDS[3], EDIT_SEEDS[9], EDIT_SEEDS[13]]


@pytest.mark.parametrize("epoch", FAR_EPOCHS)
@pytest.mark.parametrize("shape_id,seed", FAR_SEEDS, ids=[f"{s}-{n}" for s, n in FAR_SEEDS])
def test_random_edit_sessions_far_from_tick_zero(shape_id, seed, epoch):
    """Both sides start at the epoch: an Envelope's state holds sample times, and the ones taken before sample 2^32 (it lies in the session's
    fifth tick) are carried over the edits behind it; OutputDevice clip / lag times likewise."""
    assert {s for s, _ in FAR_SEEDS} == {"44k1", "48k", "44k1_100"}
    n_ticks = 8 if epoch == "across_2p32" else 7 * 6
    run_edit_session(shape_id, seed, ("fused", "unfused", "mixed"), abi.FLAG_EQ_EXACT, first_tick=far_first_tick(epoch, by_id(shape_id).spt, n_ticks))


def test_decks_do_not_notice_a_topology_edit():
    """A deck lives outside the graph.  Two decks, one plain and one key-locked, are fed into stereo sources of g0 for three ticks and then,
    after the edited g1 has adopted g0's state, into sources of g1 that sit at other node indices, for three more: ports, tick records and
    grain records are those of the models (tests/deck_model.py through tests/deck_keylock_model.py) run without a break."""
    import deck_cases as dc
    import deck_keylock_cases as kc
    import deck_keylock_model as km
    from deck_keylock_model import Keylock
    from deck_model import ONE
    from mixlab_amd import deck
    from mixlab_amd.workspace import Workspace

    spt, n = 257, 3
    tables = np.stack([deck.deck_tables(b) for b in range(4)])

    def workspace(edited):
        ws = Workspace(*dc.rate_of(spt))
        ids = {}
        if edited:                       # new modules in front: every survivor's index shifts, and the sources swap places
            ids["osc"] = ws.oscillator(440.0, abi.WAVE_SINE)
            ids["fir"] = ws.fir(np.linspace(-0.2, 0.3, 7)); ids["s1"] = ws.source_stereo(); ids["s0"] = ws.source_stereo()
        else:
            ids["s0"] = ws.source_stereo(); ids["s1"] = ws.source_stereo(); ids["fir"] = ws.fir(np.linspace(-0.2, 0.3, 7))
        ids["mix"] = ws.mixer([(0.0, 1.0, False)] * 2)
        ws.connect(ids["s0"], 0, ids["fir"], 0); ws.connect(ids["fir"], 0, ids["mix"], 0); ws.connect(ids["s1"], 0, ids["mix"], 1)
        return ws, ids

    settings = [None, Keylock(ONE, 256, 64, 40)]
    steps = [dc.frames(1.08), dc.frames(0.92)]
    decks, models = [], []
    for k, (kl, step) in enumerate(zip(settings, steps)):
        tr = kc.track("music", 4097, f"edit decks {k}")
        d, m = deck.Deck(4097), km.KeylockModel(tr, tables)
        d.load(tr)
        p = dc.play(step)
        d.set(deck.params(p.step, p.slew, p.loop_in, p.loop_out, p.flags)); d.seek(dc.frames(100.5 + k)); m.schedule(0, p, dc.frames(100.5 + k))
        if kl is not None:
            d.set_keylock(deck.keylock(*kl)); m.set_keylock(kl)
        decks.append(d); models.append(m)
    ws0, id0 = workspace(False)
    ws1, id1 = workspace(True)
    assert all(id0[name] != id1[name] for name in id0)
    g0 = ws0.build(max_ticks_per_run=n)
    g1 = ws1.build(max_ticks_per_run=n)
    fir_in, hist = [], np.zeros(12, np.float32)
    for run, (g, ids) in enumerate(((g0, id0), (g1, id1))):
        if run:
            mapping = [-1] * len(ws1.nodes)
            for name in ("s0", "s1", "fir", "mix"):
                mapping[id1[name]] = id0[name]
            g1.adopt_state(g0, mapping)
            g0.close()
        nodes = [ids["s0"], ids["s1"]]
        deck.feed(decks, nodes, g, n)
        g.run_ticks(run * n, n)
        want = [m.feed(n, spt) for m in models]
        for i in range(2):
            got = g.read_output(nodes[i], 0, n, True)
            assert np.array_equal(got.reshape(-1).view(np.uint32), np.asarray(want[i][0], np.float32).reshape(-1).view(np.uint32)), f"deck {i}, run {run}: the port"
            assert [(t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank) for t in decks[i].read_ticks(0, n)] == [tuple(t) for t in want[i][1]], (i, run)
            assert [(x.a_q32, x.g_q32, x.tick, x.frame, x.delta, x.dist, x.flags) for x in decks[i].read_grains()] == [tuple(x) for x in want[i][2]], (i, run)
        assert decks[0].grain_count() == 0 and decks[1].grain_count() > 0
        fir_in.append(np.asarray(want[0][0], np.float32).reshape(-1))
        # the Fir behind the plain deck's source carries its history over the edit: the deck's samples, filtered without a break
        assert np.array_equal(g.read_output(ids["fir"], 0, n, True).view(np.uint32), oracle.fir_run(np.linspace(-0.2, 0.3, 7), hist, fir_in[-1]).view(np.uint32)), f"Fir, run {run}"
    for d in decks:
        d.close()
    g1.close()
