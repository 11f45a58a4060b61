"""Random video graphs on the device against the composed model (tests/random_video.py): every video port, RGBA sink, Monitor tick, scope record and multiview
canvas of every run, bit for bit -- stored frames and their expiry, symbolic cross-fade chains, the deferred RGBA launch, the per-source caches and pools and the
two hop counters meet here.  The scenarios are those of tests/test_cpu_random_video.py (same seeds, same digest), where each of random_video.FAULTS is shown to
change what is compared here.  Then three directed cases that chance does not draw at these sizes."""
import functools

import numpy as np
import pytest

import oracle_video as ov
import random_video as rv
import video_key_model as km
import video_place_model as pm
import video_scope_model as sm
from mixlab_amd import ingest, video
from mixlab_amd.workspace import Workspace
from test_cpu_random_video import DIGEST, SEEDS
from test_cpu_random_video_chain import grade_abi, matte_abi
from test_gpu_video_graph import MATRIX
from test_gpu_video_place import kp, pp, upload

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=2)
def scenario_of(seed, chain=False):
    return rv.scenario(seed, chain=True) if chain else rv.scenario(seed)


@functools.lru_cache(maxsize=2)
def expected(seed, kind, chain=False):
    """shared between the parametrisations of a seed (they follow each other); never modified"""
    sc = scenario_of(seed, chain)
    return rv.expect(sc, rv.groupings(sc, kind))


def test_the_scenarios_are_those_of_the_cpu_suite():
    assert rv.digest([rv.scenario(s) for s in SEEDS]) == DIGEST and rv.MATRIX == MATRIX


def on_device(pic: rv.Pic):
    if pic.fmt == 0:
        return upload(*pic.planes, pic.a)                       # stride padding full of noise
    return video.DFrame(pic.w, pic.h, fmt=pic.fmt).upload(*pic.planes)


def planes_differ(got, want):
    """'' or where two lists of planes differ"""
    if len(got) != len(want):
        return f"{len(got)} planes, want {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        if g.shape != w.shape:
            return f"plane {k} is {g.shape}, want {w.shape}"
        bad = np.argwhere(g != w)
        if bad.size:
            return f"plane {k} differs at {bad[:3].tolist()} ({len(bad)} samples): got {g[tuple(bad[0])]}, want {w[tuple(bad[0])]}"
    return ""


def frame_differs(d, pic):
    """'' or how device frame d differs from the model's Pic"""
    if (d is None) != (pic is None):
        return f"{'a frame' if d is not None else 'None'}, want {'a frame' if pic is not None else 'None'}"
    if d is None:
        return ""
    if (d.fmt, d.width, d.height) != (pic.pixfmt, pic.w, pic.h):
        return f"format {d.fmt} {d.width}x{d.height}, want {pic.pixfmt} {pic.w}x{pic.h}"
    if d.has_alpha() != (pic.a is not None):
        return f"coverage plane: {d.has_alpha()}"
    return planes_differ(d.download() + ([d.download_alpha()] if pic.a is not None else []), pic.planes + ([pic.a] if pic.a is not None else []))


def build(sc):
    return workspace(sc).build(max_ticks_per_run=rv.MAX_RUN)


def workspace(sc):
    ws = Workspace(sc["rate"], 60)
    for _ in sc["sources"]:
        ws.source_video()
    for m in sc["mixers"]:
        p = m["params"]
        node = ws.video_mixer(a=None if p["a"] < 0 else p["a"], b=None if p["b"] < 0 else p["b"], fader=p["fader"])
        assert node == m["node"]
        for i, ref in enumerate(m["inputs"]):
            if ref is not None:
                ws.connect(ref[0], ref[1], node, i)
    for s in sc["sinks"]:
        assert ws.video_to_rgba(MATRIX if s["matrix"] else None) == s["node"]
        ws.connect(s["mixer"] + sc["n_sources"], 0, s["node"], 0)
    if sc["monitor"]:
        mo = sc["monitor"]
        assert ws.monitor(mo["width"], mo["height"]) == mo["node"]
        ws.connect(mo["mixer"] + sc["n_sources"], 0, mo["node"], 0)
    return ws


def apply_event(g, sc, e, dev):
    op, tick0 = e["op"], sc["first_tick"]
    if op == "ring":
        video.graph_set_video_source_ring(g, e["src"], [dev(f) for f in e["frames"]], dur=tuple(e["dur"]), off=tuple(e["off"]))
    elif op in ("repeat", "shot"):
        video.graph_set_video_source(g, e["src"], dev(e["frame"]), dur=tuple(e["dur"]), off=tuple(e["off"]), repeat=op == "repeat")
    elif op == "queue":
        for q in e["entries"]:
            ingest.graph_queue_video_source(g, e["src"], tick0 + q["tick"], dev(q["frame"]), dur=tuple(q["dur"]), off=tuple(q["off"]))
    elif op == "key":
        video.graph_set_video_source_key(g, e["src"], kp(km.KeyP(**e["params"])) if e["params"] else None)
    elif op == "place":
        video.graph_set_video_source_place(g, e["src"], pp(pm.PlaceP(**e["params"])) if e["params"] else None)
    elif op == "grade":
        if e["params"] is None:
            video.graph_set_video_source_grade(g, e["src"], None)
        else:
            p = rv.grade_p(e["params"])
            lut = video.Lut(p.k, p.nodes) if p.nodes is not None else None       # a handle of the caller's own: the graph retains the lattice
            video.graph_set_video_source_grade(g, e["src"], grade_abi(e["params"]), lut)
            if lut is not None:
                lut.release()                                                    # ... so it is let go of straight after the call, before any run
    elif op == "matte":
        video.graph_set_video_source_matte(g, e["src"], matte_abi(e["params"]) if e["params"] is not None else None)   # a wipe: through video.matte_wipe
    elif op == "band":
        b = e["params"] or dict(in_w=0, in_full_h=0, src_row0=0, slice_rows=0, full_w=0, full_h=0, row0=0, band_rows=0)
        video.graph_set_video_source_band(g, e["src"], b["in_w"], b["in_full_h"], b["src_row0"], b["slice_rows"], b["full_w"], b["full_h"], b["row0"], b["band_rows"])
    elif op == "scopes":
        g.set_video_scopes([tuple(p) for p in e["ports"]], e["wave_cols"], bool(e["vectorscope"]), e["hop"])
    elif op == "multiview":
        if not e["ports"]:
            video.graph_set_multiview(g, [], None)
        else:
            p = rv.mv_params(e)
            views = [video.MultiviewView(v.x, v.y, v.w, v.h, v.border, v.colour, v.fit) for v in p.views]
            video.graph_set_multiview(g, [tuple(x) for x in e["ports"]], video.MultiviewParams(p.canvas_w, p.canvas_h, views, bg=p.bg, hop=e["hop"]))
    else:
        raise AssertionError(op)


def run_scenario(seed, grouping, inline, observe, monkeypatch, chain=False):
    """Builds the graph of scenario `seed`, applies it run by run under `grouping` and compares, after every run, what the model expects.  observe "sinks": only
    what a program would read -- the RGBA sinks, the Monitor, the scope records, the multiview canvas and status: symbolic frames stay symbolic; "ports":
    every video port is downloaded as well (which materialises it).  chain: the scenario of the chain family (tests/test_gpu_random_video_chain.py); there, batched
    and with the ports read, the frame read from the first chain source's port is KEPT on every second run: a frame a caller holds is never rewritten, whatever
    re-sets followed."""
    monkeypatch.setenv("MX_SCALE_INLINE", inline)
    sc, want = scenario_of(seed, chain), expected(seed, grouping, chain)
    hold_port = next(((s, 0) for s, d in enumerate(sc["sources"]) if d.get("stages")), None) if (chain and grouping == "batched") else None
    held_frames = []                                                # (run, frame, expected picture): the test, not the graph, holds it
    g = build(sc)
    keep, made = [], {}

    def dev(fid):                                                   # every frame is uploaded once and kept alive
        if fid not in made:
            made[fid] = on_device(rv.source_frame(sc, fid))
            keep.append(made[fid])
        return made[fid]
    held = []                                                       # (run, canvas, expected planes): a canvas the caller holds is never rewritten
    for i, r in enumerate(want):
        where = f"seed {seed} {grouping} inline={inline} {observe}: run {i} (ticks {r['start']} .. {r['start'] + r['n'] - 1})"
        for e in sc["events"].get(r["start"], []):
            apply_event(g, sc, e, dev)
        for k in range(r["n"]):
            for u in sc["mixer_updates"].get(r["start"] + k, []):
                g.schedule_params(u["node"], k, video.VideoMixerParams(u["params"]["a"], u["params"]["b"], u["params"]["fader"]))
        g.run_ticks(sc["first_tick"] + r["start"], r["n"])
        for node, rgba in r["sinks"].items():
            got = video.graph_rgba_output(g, node)
            assert (got is None) == (rgba is None), f"{where}: sink {node}: {'a picture' if got is not None else 'None'}"
            if rgba is not None:
                assert not planes_differ([got], [rgba]), f"{where}: tick {r['start'] + r['n'] - 1}: sink {node}: {planes_differ([got], [rgba])}"
        if r["monitor"] is not None:
            for k, w in enumerate(r["monitor"]):
                ts, vid = ingest.graph_read_monitor_tick(g, sc["monitor"]["node"], k)
                what = f"{where}: tick {r['start'] + k}: Monitor"
                assert ts == w[0], f"{what}: timestamp {ts}, want {w[0]}"
                assert (vid is None) == (len(w) == 2), f"{what}: {'a picture' if vid else 'none'}"
                if vid is not None:
                    assert (vid[1], vid[2]) == (w[1], w[2]), f"{what}: frame timestamp {vid[1]} duration {vid[2]}, want {w[1]} {w[2]}"
                    assert (vid[0].width, vid[0].height) == (sc["monitor"]["width"], sc["monitor"]["height"])
                    assert not planes_differ(vid[0].download(), w[3]), f"{what}: {planes_differ(vid[0].download(), w[3])}"
        if r["scopes"] is not None:
            got = g.read_video_scopes()
            assert len(got) == len(r["scopes"]["records"]), f"{where}: {len(got)} recorded ticks, want {len(r['scopes']['records'])}"
            for row_g, row_w in zip(got, r["scopes"]["records"]):
                for j, (a, b) in enumerate(zip(row_g, row_w)):
                    assert sm.same(a, b), f"{where}: tick {r['start'] + b['tick_in_run']}: scope tap {j}: {sm.first_difference(a, b)}"
        if r["mv"] is not None:
            canvas, st = video.graph_multiview_output(g)
            status = (st.recorded, st.tick_in_run, st.present_mask, st.shown_mask)
            assert status == r["mv"]["status"], f"{where}: multiview status {status}, want {r['mv']['status']}"
            assert (canvas is None) == (r["mv"]["canvas"] is None), f"{where}: multiview canvas"
            if canvas is not None:
                assert canvas.fmt == video.PIXFMT_YUV420P and not canvas.has_alpha()
                assert not planes_differ(canvas.download(), r["mv"]["canvas"]), f"{where}: tick {r['start'] + status[1]}: multiview canvas: {planes_differ(canvas.download(), r['mv']['canvas'])}"
                if grouping == "batched" and i % 2 == 0:
                    held.append((i, canvas, r["mv"]["canvas"]))
        if observe == "ports":
            for (node, port), pic in r["ports"].items():
                d = video.graph_video_output(g, node, port)
                bad = frame_differs(d, pic)
                assert not bad, f"{where}: tick {r['start'] + r['n'] - 1}: port ({node}, {port}): {bad}"
                if (node, port) == hold_port and d is not None and i % 2 == 0:
                    held_frames.append((i, d, pic))
    for i, canvas, planes in held:
        assert not planes_differ(canvas.download(), planes), f"seed {seed}: the canvas of run {i}, held by the caller, was rewritten: {planes_differ(canvas.download(), planes)}"
    for i, d, pic in held_frames:
        assert not frame_differs(d, pic), f"seed {seed}: the frame of run {i} on port {hold_port}, held by the caller, was rewritten: {frame_differs(d, pic)}"
    g.close()


CASES = [(seed,) + c for n, seed in enumerate(SEEDS)
         for c in [("batched", "0", "sinks"), ("batched", "1", "ports"), ("single", "0", "ports")] + ([("batched", "1", "sinks")] if n % 4 == 0 else [])]


@pytest.mark.parametrize("seed,grouping,inline,observe", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_random_video_graph_every_port_sink_record_and_canvas(seed, grouping, inline, observe, monkeypatch):
    run_scenario(seed, grouping, inline, observe, monkeypatch)


# ---- three directed cases chance does not draw at these sizes ----
KEY = km.DEFAULT_CHROMA


def keyed_cascade(ticks, matrix=None):
    ws = Workspace(44100, 60)
    sa, sb = ws.source_video(), ws.source_video()
    m = ws.video_mixer(a=0, b=1, fader=0.7)
    ws.connect(sa, 0, m, 0); ws.connect(sb, 0, m, 1)
    rgba = ws.video_to_rgba(matrix); ws.connect(m, 0, rgba, 0)
    return ws.build(max_ticks_per_run=ticks), sa, sb, m, rgba


def as_pic(planes):
    y, u, v, a = planes
    return rv.Pic(0, y.shape[1], y.shape[0], [y, u, v], a)


@pytest.mark.parametrize("placed", [False, True], ids=["key", "key-and-place"])
def test_keyed_ring_longer_than_the_done_list(placed):
    """A ring of 40 frames on a keyed (and placed) source: longer than the list of 32 transformed frames a source keeps, and with the pool of 64 behind it every
    frame is transformed again on every round.  96 ticks in runs of 6: the scope tap on the source's port at hop 1 and the composite after every run."""
    N, T, RUN = 40, 96, 6
    place = pm.PlaceP(66, 38, -4, 6, 40, 30, 2, 2, 28, 14)
    pics = [km.green_screen(34, 18, seed=100 + k) for k in range(N)]
    want = []
    for pic in pics:
        planes = km.key_model(*pic, KEY)
        if placed:
            planes = pm.place_model(*planes[:3], place, planes[3])
        want.append(as_pic(planes))
    B = ov.HostFrame(66, 38).fill(3, seed=8)
    g, sa, sb, m, rgba = keyed_cascade(RUN)
    ring = [upload(*pic) for pic in pics]
    dB = upload(*B.visible())
    video.graph_set_video_source_key(g, sa, kp(KEY))
    if placed:
        video.graph_set_video_source_place(g, sa, pp(place))
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
            w = want[(t0 + k) % N]
            prog = om.run_tick((t0 + k) * 735, [(w.host(), (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
            if (t0 + k) % N not in records:
                records[(t0 + k) % N] = sm.record((w.pixfmt, w.w, w.h, w.planes), 0, 64, True)
            assert sm.same(got[k][0], dict(records[(t0 + k) % N], tick_in_run=k)), f"tick {t0 + k}: {sm.first_difference(got[k][0], dict(records[(t0 + k) % N], tick_in_run=k))}"
        assert not planes_differ([video.graph_rgba_output(g, rgba)], [ov.to_rgba(prog, None)]), f"run ending at tick {t0 + RUN - 1}: the sink"
        assert not planes_differ(video.graph_video_output(g, m, 0).download(), prog.visible()), f"run ending at tick {t0 + RUN - 1}: the composite"


def test_whole_frame_place_on_a_ring_of_two_sizes():
    """The ring alternates 66x38 and 34x18 under a whole-frame crop: the tap tables are rebuilt for every frame.  12 ticks, one run of 6 and six runs of 1,
    against place_model per tick through a hop-1 scope tap and the sink."""
    place = pm.PlaceP(130, 74, 10, -6, 96, 60)
    pics = [pm.noise_frame(*((66, 38) if k % 2 == 0 else (34, 18)), 200 + k, k % 3 == 0) for k in range(4)]
    want = [as_pic(pm.place_model(*pic[:3], place, pic[3])) for pic in pics]
    B = ov.HostFrame(130, 74).fill(5, seed=4)
    g, sa, sb, m, rgba = keyed_cascade(6, MATRIX)
    ring = [upload(*pic) for pic in pics]
    dB = upload(*B.visible())
    video.graph_set_video_source_place(g, sa, pp(place))
    video.graph_set_video_source_ring(g, sa, ring)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    g.set_video_scopes([(sa, 0)], 256, False, 1)
    om = ov.OracleVideoMixer(a=0, b=1, fader=0.7)
    tick = 0
    for n in (6, 1, 1, 1, 1, 1, 1):
        g.run_ticks(tick, n)
        got = g.read_video_scopes()
        assert len(got) == n
        for k in range(n):
            w = want[(tick + k) % 4]
            prog = om.run_tick((tick + k) * 735, [(w.host(), (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
            rec = sm.record((w.pixfmt, w.w, w.h, w.planes), k, 256, False)
            assert sm.same(got[k][0], rec), f"tick {tick + k}: {sm.first_difference(got[k][0], rec)}"
        tick += n
        assert not planes_differ([video.graph_rgba_output(g, rgba)], [ov.to_rgba(prog, MATRIX)]), f"run ending at tick {tick - 1}: the sink"
        assert not frame_differs(video.graph_video_output(g, sa, 0), want[(tick - 1) % 4]), f"tick {tick - 1}: the source's port"
