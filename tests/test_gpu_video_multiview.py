"""The multiviewer on the device (mx_video_multiview, mx_graph_set_multiview, mx_graph_multiview_output) against
tests/video_multiview_model.py, every byte of all three planes: integer work.  Every input frame's stride padding holds noise."""
import ctypes as C

import numpy as np
import pytest

import oracle_video as ov
import video_key_model as km
import video_multiview_model as mm
import video_place_model as pm
from mixlab_amd import abi, ingest, video
from mixlab_amd.workspace import Workspace
from test_gpu_video_place import kp, planes_of, upload
from video_multiview_model import MvP, Src, View, multiview_model

pytestmark = pytest.mark.gpu

CASES = mm.cases(abi.MULTIVIEW_TILE_W, abi.MULTIVIEW_TILE_H, abi.MULTIVIEW_TAP_BOUND)
BY_NAME = {c.name: c for c in CASES}


def vp(p: MvP, hop=1):
    return video.MultiviewParams(p.canvas_w, p.canvas_h, [video.MultiviewView(v.x, v.y, v.w, v.h, v.border, v.colour, v.fit) for v in p.views], bg=p.bg, hop=hop)


def on_device(frames, pad_seed=1):
    """the model's frames as device frames (one per distinct Src), stride padding full of noise"""
    made, out = {}, []
    for f in frames:
        if f is None:
            out.append(None)
        elif f.fmt != "yuv420p":
            out.append(video.DFrame(f.w, f.h, fmt=video.PIXFMT_NV12))
        else:
            if id(f) not in made:
                made[id(f)] = upload(f.y, f.u, f.v, f.a, pad_seed=pad_seed)
            out.append(made[id(f)])
    return out


def src_of(d):
    """a device frame read back as the model's Src"""
    if d is None:
        return None
    if d.fmt not in (video.PIXFMT_YUV420P, video.PIXFMT_YUVA420P):
        return Src(d.width, d.height, fmt="other")
    y, u, v = d.download()
    return Src(d.width, d.height, y, u, v, d.download_alpha() if d.has_alpha() else None)


def assert_canvas(out, want, what):
    assert out.fmt == video.PIXFMT_YUV420P and not out.has_alpha()
    for name, g, w in zip("YUV", out.download(), want):
        assert g.shape == w.shape, f"{what}: plane {name} is {g.shape}, want {w.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: plane {name} differs at {bad[:4].tolist()} ({len(bad)} samples), got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


# ---- the pixel call against the model ----
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_multiview_against_the_model_on_all_three_planes(case):
    frames = case.frames()
    out, shown = video.multiview(on_device(frames), vp(case.p))
    assert (out.width, out.height) == (case.p.canvas_w, case.p.canvas_h)
    assert shown == mm.shown_mask(frames, case.p)
    assert_canvas(out, multiview_model(frames, case.p), case.name)


@pytest.mark.parametrize("name", ["grid16", "geo-at-at", "fit0-wide", "geo-above-above", "corners"])
def test_two_padding_noises_give_the_same_canvas(name):
    case = BY_NAME[name]
    frames, want = case.frames(), case.want()
    for seed in (1, 2):
        assert_canvas(video.multiview(on_device(frames, pad_seed=seed), vp(case.p))[0], want, f"{name} padding {seed}")


@pytest.mark.parametrize("canvas", [(2, 2), (66, 38), (130, 74)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_byte_of_the_canvas_planes_is_written_padding_as_a_new_frame_has_it(canvas):
    """The canvas' stride padding is what mx_dframe_create leaves (Y 0, chroma 0x80), whatever the memory held before: frames of the same size are created,
    dirtied, dropped and rendered into again."""
    cw, ch = canvas
    p = MvP(cw, ch, (View(0, 0, cw, ch, 0, mm.RED, 0),)) if cw == 2 else MvP(cw, ch, (View(2, 2, 20, 12, 2, mm.RED, 1), View(cw - 22, ch - 14, 22, 14, 2, mm.GREEN, 0)))
    f = mm.noise_src(34, 18, 12)
    frames = [f] * len(p.views)
    fresh = video.DFrame(cw, ch)
    video.sync()
    dev = on_device(frames)
    for k in range(3):
        dirt = upload(*pm.noise_frame(cw, ch, 20 + k, False)[:3], pad_seed=k)   # its memory may be the next canvas'
        del dirt
        out, _ = video.multiview(dev, vp(p))
        video.sync()
        for (ptr, stride, rows, vis), (fptr, fstride, _r, _v) in zip(planes_of(out), planes_of(fresh)):
            got, ref = np.empty(stride * rows, np.uint8), np.empty(stride * rows, np.uint8)
            abi.check(abi.lib.mx_device_download(got.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), got.size, None))
            abi.check(abi.lib.mx_device_download(ref.ctypes.data_as(C.c_void_p), C.c_void_p(fptr), ref.size, None))
            assert stride == fstride and np.array_equal(got.reshape(rows, stride)[:, vis:], ref.reshape(rows, stride)[:, vis:])
        assert_canvas(out, multiview_model(frames, p), "visible")


# ---- device against device ----
@pytest.mark.parametrize("src", [(66, 38), (20, 40), (130, 20)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fit_1_inner_rectangle_equals_mx_video_scale(src):
    f = mm.noise_src(src[0], src[1], 1, alpha=True)
    d = on_device([f])[0]
    out, shown = video.multiview([d], vp(MvP(130, 74, (View(10, 6, 44, 30, 2, mm.RED, 1),))))
    assert shown == 1
    plain = upload(f.y, f.u, f.v)                    # the scaler would carry the coverage along; the multiviewer ignores it
    scaled = video.DFrame(40, 26)
    video.scale(plain, scaled)
    for k, (g, w) in enumerate(zip(out.download(), scaled.download())):
        c = 1 if k else 0
        assert np.array_equal(g[8 >> c:(8 >> c) + (26 >> c), 12 >> c:(12 >> c) + (40 >> c)], w), k


@pytest.mark.parametrize("src", [(66, 38), (20, 40), (160, 104)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fit_0_picture_equals_mx_video_place(src):
    f = mm.noise_src(src[0], src[1], 2)
    d = on_device([f])[0]
    out, _ = video.multiview([d], vp(MvP(130, 74, (View(10, 6, 44, 30, 2, mm.GREEN, 0),))))
    placed = video.place(d, video.PlaceParams(130, 74, 12, 8, 40, 26))
    for k, (g, w) in enumerate(zip(out.download(), placed.download())):
        c = 1 if k else 0
        sl = (slice(8 >> c, (8 + 26) >> c), slice(12 >> c, (12 + 40) >> c))
        assert np.array_equal(g[sl], w[sl]), k


def test_views_not_shown_keep_their_frame_and_a_blank_inner_rectangle():
    good = mm.noise_src(34, 18, 3)
    thin, wide = mm.noise_src(200, 2, 4), mm.noise_src(66, 18, 5)
    views = (View(2, 2, 24, 14, 2, mm.RED, 1), View(28, 2, 24, 14, 2, mm.GREEN, 1), View(54, 2, 24, 14, 2, mm.WHITE, 1), View(80, 2, 6, 14, 2, mm.RED, 0), View(2, 20, 24, 14, 2, mm.GREEN, 1))
    p = MvP(130, 74, views)
    frames = [None, Src(34, 18, fmt="nv12"), thin, wide, good]
    out, shown = video.multiview(on_device(frames), vp(p))
    assert shown == 0b10000
    assert_canvas(out, multiview_model(frames, p), "not shown")
    y, u, _v = out.download()
    for v in views[:4]:
        assert y[v.y, v.x] == v.colour[0] and y[v.y + v.h - 1, v.x + v.w - 1] == v.colour[0] and u[v.y >> 1, v.x >> 1] == v.colour[1]   # the frame is drawn
        assert not y[v.y + 2:v.y + v.h - 2, v.x + 2:v.x + v.w - 2].any() and (u[(v.y + 2) >> 1:(v.y + v.h - 2) >> 1, (v.x + 2) >> 1:(v.x + v.w - 2) >> 1] == 0x80).all()
    assert y[24:32, 6:22].any()


# ---- in a graph ----
W, H = 160, 90
GRID = MvP(130, 74, tuple(View(2 + 42 * (i % 3), 2 + 36 * (i // 3), 40, 34, 2, (mm.RED, mm.GREEN, mm.WHITE)[i % 3], i % 2) for i in range(5)))


def cascade(ticks, sink=True, monitor=False):
    """two sources -> VideoMixer -> (RGBA sink: the program is a symbolic chain until something needs pixels)(, Monitor)"""
    ws = Workspace(44100, 60)
    sa, sb = ws.source_video(), ws.source_video()
    m = ws.video_mixer(a=0, b=1, fader=0.6)
    ws.connect(sa, 0, m, 0); ws.connect(sb, 0, m, 1)
    rgba = mon = None
    if sink:
        rgba = ws.video_to_rgba(None); ws.connect(m, 0, rgba, 0)
    if monitor:
        mon = ws.monitor(80, 46); ws.connect(m, 0, mon, 0)
    return ws, ws.build(max_ticks_per_run=ticks), sa, sb, m, rgba, mon


def port_frames(g, ports):
    return [src_of(video.graph_video_output(g, n, p)) for n, p in ports]


def test_taps_on_sources_a_keyed_and_placed_one_and_on_a_symbolic_program_with_a_and_b():
    _ws, g, sa, sb, m, rgba, _ = cascade(2)
    pic = km.green_screen(W, H, seed=3)
    B = ov.HostFrame(130, 74).fill(4, seed=5)
    dA, dB = upload(*pic), upload(*B.visible())
    place = pm.PlaceP(130, 74, 20, 10, 64, 36)
    video.graph_set_video_source_key(g, sa, kp(km.DEFAULT_CHROMA))
    video.graph_set_video_source_place(g, sa, video.PlaceParams(130, 74, 20, 10, 64, 36))
    video.graph_set_video_source(g, sa, dA, repeat=True)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    ports = [(sa, 0), (sb, 0), (m, 0), (m, 1), (m, 2)]
    video.graph_set_multiview(g, ports, vp(GRID))
    g.run_ticks(0, 1)
    canvas, st = video.graph_multiview_output(g)
    assert (st.recorded, st.tick_in_run, st.present_mask, st.shown_mask) == (1, 0, 0b11111, 0b11111)
    # what the ports hold: the placed canvas of the keyed picture (the model's), B, and the oracle's composite of the two
    yk, uk, vk, k = km.key_model(*pic, km.DEFAULT_CHROMA)
    py, pu, pv, pa = pm.place_model(yk, uk, vk, place, k)
    A = ov.HostFrame(130, 74)
    for plane, s in zip(A.visible(), (py, pu, pv)):
        plane[:] = s
    A.set_alpha(pa)
    prog = ov.OracleVideoMixer(a=0, b=1, fader=0.6).run_tick(0, [(A, (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
    fA, fB, fP = Src(130, 74, py, pu, pv, pa), Src(130, 74, *B.visible()), Src(130, 74, *prog.visible())
    assert_canvas(canvas, multiview_model([fA, fB, fP, fA, fB], GRID), "graph")
    assert np.array_equal(video.graph_rgba_output(g, rgba), ov.to_rgba(prog, None))


def test_the_sink_and_the_monitor_see_the_same_bytes_with_and_without_the_setting():
    N = 5
    results = []
    for tapped in (False, True):
        _ws, g, sa, sb, m, rgba, mon = cascade(N, monitor=True)
        ring = [upload(*pm.noise_frame(W, H, 30 + k, False)[:3]) for k in range(3)]
        dB = upload(*pm.noise_frame(66, 38, 40, False)[:3])
        video.graph_set_video_source_ring(g, sa, ring)
        video.graph_set_video_source(g, sb, dB, repeat=True)
        if tapped:
            video.graph_set_multiview(g, [(m, 0), (sa, 0), (m, 2), (sb, 0), (m, 0)], vp(GRID, hop=2))
        g.run_ticks(0, N)
        res = {"rgba": video.graph_rgba_output(g, rgba).copy(), "prog": np.concatenate([x.ravel() for x in video.graph_video_output(g, m, 0).download()])}
        for k, planes in enumerate(ingest.graph_read_monitor_video(g, mon, 0, N)):
            res[f"mon{k}"] = np.concatenate([x.ravel() for x in planes])
        if tapped:
            canvas, st = video.graph_multiview_output(g)
            assert (st.recorded, st.tick_in_run) == (3, 4)
            assert_canvas(canvas, multiview_model(port_frames(g, [(m, 0), (sa, 0), (m, 2), (sb, 0), (m, 0)]), GRID), "tapped")
        results.append(res)
    assert results[0].keys() == results[1].keys()
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]), f"{k} differs with the multiview set"


def test_the_hop_rule_the_last_recorded_tick_and_a_held_canvas():
    _ws, g, sa, sb, m, _rgba, _ = cascade(8)
    pics = [mm.noise_src(66, 38, 50 + k) for k in range(5)]
    ring = on_device(pics)
    fb = mm.noise_src(34, 18, 60)
    video.graph_set_video_source_ring(g, sa, ring)
    video.graph_set_video_source(g, sb, on_device([fb])[0], repeat=True)
    one = MvP(66, 38, (View(2, 2, 40, 24, 2, mm.RED, 1), View(44, 2, 20, 12, 2, mm.GREEN, 0)))
    video.graph_set_multiview(g, [(sa, 0), (sb, 0)], vp(one, hop=2))
    with pytest.raises(abi.MxError) as e:
        video.graph_multiview_output(g)                      # no run since the set
    assert e.value.code == abi.MX_ERR_INVALID
    # a 5-tick run at hop 2 over a ring of distinct frames: ticks 0, 2, 4 are recorded, tick 4's frames are shown
    g.run_ticks(0, 5)
    held, st = video.graph_multiview_output(g)
    assert (st.recorded, st.tick_in_run, st.present_mask, st.shown_mask) == (3, 4, 3, 3)
    want4 = multiview_model([pics[4], fb], one)
    assert_canvas(held, want4, "tick 4")
    # one-tick runs: c = 5 (no), 6 (yes), 7 (no), 8 (yes); the ring goes on: tick k shows pics[k % 5]
    for tick, rec in ((5, 0), (6, 1), (7, 0), (8, 1)):
        g.run_ticks(tick, 1)
        canvas, st = video.graph_multiview_output(g)
        assert st.recorded == rec and (canvas is None) == (rec == 0)
        if rec:
            assert st.tick_in_run == 0
            assert_canvas(canvas, multiview_model([pics[tick % 5], fb], one), f"tick {tick}")
            assert canvas.handle != held.handle
    assert_canvas(held, want4, "a canvas the caller holds is not overwritten")
    # c = 9, 10, 11: a 3-tick run records its tick 1 only
    g.run_ticks(9, 3)
    canvas, st = video.graph_multiview_output(g)
    assert (st.recorded, st.tick_in_run) == (1, 1)
    assert_canvas(canvas, multiview_model([pics[10 % 5], fb], one), "tick 10")
    # a source whose frame size changes between runs: the tables are rebuilt
    video.graph_set_video_source_ring(g, sa, [])
    other = mm.noise_src(20, 40, 61)
    video.graph_set_video_source(g, sa, on_device([other])[0], repeat=True)
    g.run_ticks(12, 1)
    canvas, st = video.graph_multiview_output(g)
    assert st.recorded == 1
    assert_canvas(canvas, multiview_model([other, fb], one), "another size")
    # no frame on a port, and a frame of another format: present, not shown
    video.graph_set_video_source(g, sa, video.DFrame(34, 18, fmt=video.PIXFMT_NV12), repeat=True)
    video.graph_set_video_source(g, sb, None)
    g.run_ticks(13, 2)
    canvas, st = video.graph_multiview_output(g)
    assert (st.recorded, st.tick_in_run, st.present_mask, st.shown_mask) == (1, 1, 1, 0)
    assert_canvas(canvas, multiview_model([None, None], one), "nothing shown")
    # removing the setting
    video.graph_set_multiview(g, [], None)
    g.run_ticks(15, 1)
    with pytest.raises(abi.MxError) as e:
        video.graph_multiview_output(g)
    assert e.value.code == abi.MX_ERR_INVALID
    assert_canvas(held, want4, "still the caller's")


def test_errors_and_a_rebuilt_graph_has_no_setting():
    ws, g, sa, sb, m, rgba, _ = cascade(2)
    ws2 = Workspace(44100, 60)
    s2 = ws2.source_video(); au = ws2.source_stereo(); amp = ws2.amplifier(1.0, 0.0); ws2.connect(au, 0, amp, 0)
    m2 = ws2.video_mixer(a=0, b=None, fader=1.0); ws2.connect(s2, 0, m2, 0)
    g2 = ws2.build(max_ticks_per_run=2)
    one = vp(MvP(66, 38, (View(2, 2, 40, 24, 2, mm.RED, 1),)))
    two = vp(MvP(66, 38, (View(2, 2, 20, 12, 2, mm.RED, 1), View(22, 2, 20, 12, 2, mm.RED, 1))))

    def set_raw(graph, ports, params, n=None):
        pa = (abi.PortRef * max(1, len(ports)))(*[abi.PortRef(a, b) for a, b in ports])
        return abi.lib.mx_graph_set_multiview(graph._h, pa, len(ports) if n is None else n, C.byref(params) if params is not None else None)

    assert set_raw(g2, [(amp, 0)], one) == abi.MX_ERR_TYPE and set_raw(g2, [(au, 0)], one) == abi.MX_ERR_TYPE      # audio ports
    assert set_raw(g2, [(999, 0)], one) == abi.MX_ERR_INVALID and set_raw(g2, [(m2, 3)], one) == abi.MX_ERR_INVALID  # node / port out of range
    assert set_raw(g, [(rgba, 0)], one) == abi.MX_ERR_INVALID                                                        # a sink has no output port
    assert set_raw(g2, [(m2, 0)], two) == abi.MX_ERR_INVALID and set_raw(g2, [(m2, 0), (s2, 0)], one) == abi.MX_ERR_INVALID   # n != n_views
    assert set_raw(g2, [(m2, 0)], None) == abi.MX_ERR_INVALID
    bad = vp(MvP(66, 38, (View(2, 2, 40, 24, 2, mm.RED, 1),)), hop=0)
    assert set_raw(g2, [(m2, 0)], bad) == abi.MX_ERR_INVALID and b"hop" in abi.lib.mx_last_error()
    out, st = C.c_void_p(), abi.MultiviewStatus()
    assert abi.lib.mx_graph_multiview_output(g2._h, C.byref(out), C.byref(st)) == abi.MX_ERR_INVALID               # no setting
    assert abi.lib.mx_graph_multiview_output(g2._h, None, C.byref(st)) == abi.MX_ERR_INVALID
    # the same port in two views is allowed; a failed set leaves the setting as it was
    assert set_raw(g2, [(m2, 0), (m2, 0)], two) == abi.MX_OK
    assert set_raw(g2, [(amp, 0)], one) == abi.MX_ERR_TYPE
    f = mm.noise_src(34, 18, 70)
    video.graph_set_video_source(g2, s2, on_device([f])[0], repeat=True)
    g2.run_ticks(0, 1)
    canvas, st = video.graph_multiview_output(g2)
    assert st.shown_mask == 3
    assert_canvas(canvas, multiview_model([f, f], MvP(66, 38, (View(2, 2, 20, 12, 2, mm.RED, 1), View(22, 2, 20, 12, 2, mm.RED, 1)))), "same port twice")
    # mx_graph_adopt_state does not carry the setting
    ws3 = Workspace(44100, 60)
    s3 = ws3.source_video(); a3 = ws3.source_stereo(); p3 = ws3.amplifier(1.0, 0.0); ws3.connect(a3, 0, p3, 0)
    m3 = ws3.video_mixer(a=0, b=None, fader=1.0); ws3.connect(s3, 0, m3, 0)
    g3 = ws3.build(max_ticks_per_run=2)
    g3.adopt_state(g2, list(range(len(ws3.nodes))))
    assert abi.lib.mx_graph_multiview_output(g3._h, C.byref(out), C.byref(st)) == abi.MX_ERR_INVALID
    # the pixel call
    assert abi.lib.mx_video_multiview(None, C.byref(one), C.byref(out), None, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_video_multiview((C.c_void_p * 1)(), None, C.byref(out), None, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_video_multiview((C.c_void_p * 1)(), C.byref(one), None, None, None) == abi.MX_ERR_INVALID
