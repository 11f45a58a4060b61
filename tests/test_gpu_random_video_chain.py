"""The chain family of the random video graphs on the device (random_video.scenario(seed, chain=True)) against the composed model: sources whose transform is a drawn
subset of GRADE, KEY, MATTE, PLACE -- set in a drawn call order, set again, removed and put back at run boundaries, over rings and queues of two sizes that mix
yuv420p and yuva420p frames -- with everything the first family has around them: every video port, RGBA sink, Monitor tick, scope record and multiview canvas of
every run, bit for bit.  The four done-lists, the four pools, the retained lattice and the placer's tap tables of the engine's SourceTransform meet here.  The
scenarios are those of tests/test_cpu_random_video_chain.py (same seeds, same digest), where each fault of the source transform is shown to change what is compared
here.  In the batched "ports" variant a frame read from a chain source's port is held by the test across the re-sets that follow.  Then two directed cases that
chance does not draw at these sizes."""
import numpy as np
import pytest

import oracle_video as ov
import random_video as rv
import video_grade_model as gm
import video_key_model as km
import video_matte_model as mt
import video_scope_model as sm
from mixlab_amd import video
from test_cpu_random_video_chain import CHAIN_DIGEST, CHAIN_SEEDS
from test_gpu_random_video import apply_event, frame_differs, keyed_cascade, planes_differ, run_scenario
from test_gpu_video_place import upload

pytestmark = pytest.mark.gpu


def test_the_chain_scenarios_are_those_of_the_cpu_suite():
    assert rv.digest([rv.scenario(s, chain=True) for s in CHAIN_SEEDS]) == CHAIN_DIGEST


CASES = [(seed,) + c for seed in CHAIN_SEEDS for c in [("batched", "0", "sinks"), ("batched", "1", "ports"), ("single", "0", "ports")]]


@pytest.mark.parametrize("seed,grouping,inline,observe", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_random_chain_graph_every_port_sink_record_and_canvas(seed, grouping, inline, observe, monkeypatch):
    run_scenario(seed, grouping, inline, observe, monkeypatch, chain=True)


# ---- two directed cases chance does not draw at these sizes ----
KEY = dict(mode=km.KEY_CHROMA, key_u=km.GREEN[0], key_v=km.GREEN[1], invert=0, near_q4=8 * 16, far_q4=40 * 16, spill_far_q4=90 * 16, spill_strength=200)   # DEFAULT_CHROMA
MATTE = dict(clean=[30, 220], choke=1, soften=2, mask=[-40, 36, 16 * 30 + 4, 16 * 40], shape=mt.RECT, invert=0, feather=37)   # hangs off both sizes of frame
PLACE = dict(canvas_w=130, canvas_h=74, dst_x=10, dst_y=-6, dst_w=96, dst_h=60, crop_x=0, crop_y=0, crop_w=0, crop_h=0)                                   # the whole frame
GRADE = dict(flags=gm.CURVE | gm.CHROMA | gm.LUT, curve=[0.8, 12, 236], m=[4300, 300, -300, 4300], off=[-700, 900], k=4, lattice="smooth")


def picture(w, h, seed, coverage):
    """a green-screen picture as the model's Pic, with a noisy coverage plane of its own where asked"""
    y, u, v = km.green_screen(w, h, seed=seed)
    a = None
    if coverage:
        rng = np.random.default_rng(0xC0FE + seed)
        a = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
        a[rng.random((h, w)) < 0.4] = 255
    return rv.Pic(0, w, h, [y, u, v], a, uid=("d", seed))


def set_stage(g, node, op, par):
    apply_event(g, dict(first_tick=0), dict(op=op, src=node, params=par), None)


def test_four_stage_ring_longer_than_the_done_list():
    """All four stages on a ring of 40 frames -- more than the 32 entries a done-list keeps, so every frame goes through the whole chain again on every round and all
    four pools recycle -- that alternates 66x38 and 34x18 with every third frame yuva420p: the grade pool has to match on the coverage plane and the tap tables
    are rebuilt per size.  96 ticks in runs of 6 against the composed model per tick: a hop-1 scope tap on the source's port, and the sink, the composite and
    the port after every run."""
    N, T, RUN = 40, 96, 6
    sc = {}
    pics = [picture(*((66, 38) if k % 2 == 0 else (34, 18)), 300 + k, k % 3 == 0) for k in range(N)]
    want = [rv.transformed(sc, pic, KEY, PLACE, None, grade=GRADE, matte=MATTE) for pic in pics]
    assert not want[0].same(rv.transformed(sc, pics[0], KEY, PLACE, None, matte=MATTE)) and not want[0].same(rv.transformed(sc, pics[0], KEY, PLACE, None, grade=GRADE))
    B = ov.HostFrame(130, 74).fill(3, seed=8)
    g, sa, sb, m, rgba = keyed_cascade(RUN)
    ring = [upload(*pic.planes, pic.a) for pic in pics]
    dB = upload(*B.visible())
    for op, par in (("place", PLACE), ("matte", MATTE), ("grade", GRADE), ("key", KEY)):     # not the chain's order
        set_stage(g, sa, op, par)
    video.graph_set_video_source_ring(g, sa, ring)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    g.set_video_scopes([(sa, 0)], 64, True, 1)
    om = ov.OracleVideoMixer(a=0, b=1, fader=0.7)
    records = {}
    for t0 in range(0, T, RUN):
        g.run_ticks(t0, RUN)
        got = g.read_video_scopes()
        assert len(got) == RUN
        for k in range(RUN):
            j = (t0 + k) % N
            w = want[j]
            prog = om.run_tick((t0 + k) * 735, [(w.host(), (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
            if j not in records:
                records[j] = sm.record((w.pixfmt, w.w, w.h, w.planes), 0, 64, True)
            rec = dict(records[j], tick_in_run=k)
            assert sm.same(got[k][0], rec), f"tick {t0 + k} (frame {j}): {sm.first_difference(got[k][0], rec)}"
        assert not planes_differ([video.graph_rgba_output(g, rgba)], [ov.to_rgba(prog, None)]), f"run ending at tick {t0 + RUN - 1}: the sink"
        assert not planes_differ(video.graph_video_output(g, m, 0).download(), prog.visible()), f"run ending at tick {t0 + RUN - 1}: the composite"
        bad = frame_differs(video.graph_video_output(g, sa, 0), want[(t0 + RUN - 1) % N])
        assert not bad, f"run ending at tick {t0 + RUN - 1}: the source's port: {bad}"
    g.close()


def test_lattice_replaced_at_every_run_boundary_under_three_standing_stages():
    """A four-stage source -- a ring of a yuva420p and a yuv420p frame -- whose grade is set again with ANOTHER lattice before each of 8 runs of 2 ticks, 17 and 33 nodes in
    turn, every handle released before the run; the key, the matte and the placement stay put.  Every run's two ticks (a hop-1 scope tap), its port and its
    composite are that run's model: neither the old lattice nor a frame keyed, matted or placed from the old grade is seen again.  A ninth run with the grade
    removed equals a three-stage graph that never had it."""
    sc = {}
    pics = [picture(66, 38, 400, True), picture(66, 38, 401, False)]
    B = ov.HostFrame(130, 74).fill(2, seed=5)
    g, sa, sb, m, rgba = keyed_cascade(2)
    g0, sa0, sb0, m0, rgba0 = keyed_cascade(2)                              # the graph that never had a grade
    ring = [upload(*pic.planes, pic.a) for pic in pics]
    dB = upload(*B.visible())
    for gg, a, b in ((g, sa, sb), (g0, sa0, sb0)):
        for op, par in (("key", KEY), ("place", PLACE), ("matte", MATTE)):
            set_stage(gg, a, op, par)
        video.graph_set_video_source_ring(gg, a, ring)
        video.graph_set_video_source(gg, b, dB, repeat=True)
        gg.set_video_scopes([(a, 0)], 64, True, 1)
    om = ov.OracleVideoMixer(a=0, b=1, fader=0.7)
    seen = []
    for run in range(9):
        grade = None if run == 8 else dict(GRADE, k=4 + run % 2, lattice="smooth" if run == 0 else 70 + run, curve=[0.8 + 0.05 * run, 12, 236], off=[-700 + 100 * run, 900])
        set_stage(g, sa, "grade", grade)
        g.run_ticks(2 * run, 2)
        got = g.read_video_scopes()
        assert len(got) == 2
        for k in range(2):
            w = rv.transformed(sc, pics[k], KEY, PLACE, None, grade=grade, matte=MATTE)
            prog = om.run_tick((2 * run + k) * 735, [(w.host(), (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
            rec = sm.record((w.pixfmt, w.w, w.h, w.planes), k, 64, True)
            assert sm.same(got[k][0], rec), f"run {run}, tick {k}: {sm.first_difference(got[k][0], rec)}"
        port, comp = video.graph_video_output(g, sa, 0), video.graph_video_output(g, m, 0).download()
        assert not frame_differs(port, w), f"run {run}: the source's port: {frame_differs(port, w)}"
        assert not planes_differ(comp, prog.visible()), f"run {run}: the composite: {planes_differ(comp, prog.visible())}"
        assert not planes_differ([video.graph_rgba_output(g, rgba)], [ov.to_rgba(prog, None)]), f"run {run}: the sink"
        assert all(not w.same(x) for x in seen), f"run {run}: the settings are meant to differ"
        seen.append(w)
    g0.run_ticks(16, 2)
    plain = video.graph_video_output(g0, sa0, 0)
    assert not planes_differ(port.download() + [port.download_alpha()], plain.download() + [plain.download_alpha()]), "grade removed: the port of a graph that never had it"
    assert not planes_differ(comp, video.graph_video_output(g0, m0, 0).download()), "grade removed: the composite of a graph that never had it"
    assert not planes_differ([video.graph_rgba_output(g, rgba)], [video.graph_rgba_output(g0, rgba0)]), "grade removed: the sink of a graph that never had it"
    g.close(); g0.close()
