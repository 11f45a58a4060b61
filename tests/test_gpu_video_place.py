"""The placer on the device (mx_video_place, mx_graph_set_video_source_place) against tests/video_place_model.py, every byte of all four
planes: integer work.  Every input frame's stride padding holds noise.  The composites go through the existing compositor and are compared with the oracle's
alpha cross-fade fed the MODEL's placed planes."""
import ctypes as C

import numpy as np
import pytest

import oracle_video as ov
import video_key_model as km
import video_place_model as pm
from mixlab_amd import abi, ingest, video
from mixlab_amd.workspace import Workspace
from video_key_model import DEFAULT_CHROMA, key_model
from video_place_model import PlaceP, place_model

pytestmark = pytest.mark.gpu

CASES = pm.cases(abi.PLACE_TILE_W, abi.PLACE_TILE_H, abi.PLACE_TAP_BOUND)


def pp(p: PlaceP):
    return video.PlaceParams(p.canvas_w, p.canvas_h, p.dst_x, p.dst_y, p.dst_w, p.dst_h, crop=p.crop())


def kp(p):
    return video.KeyParams(p.mode, p.key_u, p.key_v, bool(p.invert), p.near_q4, p.far_q4, p.spill_far_q4, p.spill_strength)


_hip = None


def hip():
    global _hip
    if _hip is None:
        _hip = C.CDLL(str(abi.LIB_PATH))   # the HIP runtime the library is bound to
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return _hip


def planes_of(d):
    """[(device pointer, stride, rows, visible width)] of Y, U, V(, A)"""
    ptrs, strides = d.device_planes()
    out = [(ptrs[p], strides[p], d.height >> (1 if p else 0), d.width >> (1 if p else 0)) for p in range(3)]
    a, ast = C.c_void_p(), C.c_int32()
    abi.check(abi.lib.mx_dframe_alpha_plane(d._h, C.byref(a), C.byref(ast)))
    if a.value:
        out.append((a.value, ast.value, d.height, d.width))
    return out


def upload(y, u, v, a=None, pad_seed=1):
    """the frame on the device, every byte of its planes -- stride padding included -- set to noise before the visible area is uploaded"""
    d = video.DFrame(y.shape[1], y.shape[0], fmt=video.PIXFMT_YUVA420P if a is not None else video.PIXFMT_YUV420P)
    video.sync()
    rng = np.random.default_rng(0xBAD + pad_seed)
    for ptr, stride, rows, vis in planes_of(d):
        assert stride > vis or vis % 64 == 0
        junk = rng.integers(0, 256, size=stride * rows).astype(np.uint8)
        assert hip().hipMemcpy(ptr, junk.ctypes.data_as(C.c_void_p), junk.size, 1) == 0
    d.upload(y, u, v)
    if a is not None:
        d.upload_alpha(a)
    return d


def assert_planes(out, want, what):
    assert out.fmt == video.PIXFMT_YUVA420P and out.has_alpha()
    got = out.download() + [out.download_alpha()]
    for name, g, w in zip("YUVA", got, want):
        assert g.shape == w.shape, f"{what}: plane {name} is {g.shape}, want {w.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: plane {name} differs at {bad[:4].tolist()} ({len(bad)} samples), got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


# ---- the pixel call against the model ----
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_place_against_the_model_on_all_four_planes(case):
    y, u, v, a = case.frame()
    out = video.place(upload(y, u, v, a), pp(case.p))
    assert (out.width, out.height) == (case.p.canvas_w, case.p.canvas_h)
    assert_planes(out, place_model(y, u, v, case.p, a), case.name)


@pytest.mark.parametrize("crop", [(34, 0, 32, 18), (0, 20, 32, 18), (34, 20, 32, 18), None], ids=["right", "bottom", "corner", "whole"])
def test_padding_bytes_do_not_leak_into_edge_samples(crop):
    """Crops at the frame's right and bottom edge, next to stride padding that holds noise -- two different noises: the outputs are the model's both times."""
    y, u, v, a = pm.noise_frame(66, 38, 11, True)
    for p in (PlaceP(66, 38, 2, 2, 60, 34, *(crop or (0, 0, 0, 0))), PlaceP(66, 38, 10, 4, 16, 10, *(crop or (0, 0, 0, 0))), PlaceP(34, 18, 0, 0, 32, 18, *(crop or (0, 0, 0, 0)))):
        want = place_model(y, u, v, p, a)
        for seed in (1, 2):
            assert_planes(video.place(upload(y, u, v, a, pad_seed=seed), pp(p)), want, f"{p} padding {seed}")


@pytest.mark.parametrize("canvas", [(2, 2), (66, 38), (130, 74)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_byte_of_the_canvas_planes_is_written_padding_as_a_new_frame_has_it(canvas):
    """The canvas' stride padding is what mx_dframe_create_fmt leaves (Y 0, chroma 0x80, coverage 255), whatever the memory held before: frames of the same size
    are created, dirtied, dropped and placed into again."""
    cw, ch = canvas
    y, u, v, a = pm.noise_frame(34, 18, 12, False)
    p = PlaceP(cw, ch, 0, 0, cw, ch)
    fresh = video.DFrame(cw, ch, fmt=video.PIXFMT_YUVA420P)
    video.sync()
    d = upload(y, u, v)
    for k in range(3):
        dirt = upload(*pm.noise_frame(cw, ch, 20 + k, True), pad_seed=k)   # its memory may be the next canvas'
        del dirt
        out = video.place(d, pp(p))
        video.sync()
        for (ptr, stride, rows, vis), (fptr, fstride, _r, _v) in zip(planes_of(out), planes_of(fresh)):
            got, ref = np.empty(stride * rows, np.uint8), np.empty(stride * rows, np.uint8)
            abi.check(abi.lib.mx_device_download(got.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), got.size, None))
            abi.check(abi.lib.mx_device_download(ref.ctypes.data_as(C.c_void_p), C.c_void_p(fptr), ref.size, None))
            assert stride == fstride and np.array_equal(got.reshape(rows, stride)[:, vis:], ref.reshape(rows, stride)[:, vis:])
        assert_planes(out, place_model(y, u, v, p), "visible")


# ---- composites: the existing compositor over the placer's planes ----
def model_layer(planes):
    yo, uo, vo, k = planes
    hf = ov.HostFrame(yo.shape[1], yo.shape[0])
    for plane, src in zip(hf.visible(), (yo, uo, vo)):
        plane[:] = src
    return hf.set_alpha(k)


def assert_frame_equal(d, hf, what):
    for p, (x, y) in enumerate(zip(d.download(), hf.visible())):
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"{what}: plane {p} differs at {bad[:4].tolist()} ({len(bad)} samples)"


W, H = 320, 180
INSET = PlaceP(W, H, 216, 12, 96, 54)


def inset_planes(pic, keyed):
    y, u, v = pic
    if keyed:
        y, u, v, k = key_model(y, u, v, DEFAULT_CHROMA)
        return place_model(y, u, v, INSET, k)
    return place_model(y, u, v, INSET)


@pytest.mark.parametrize("keyed", [False, True], ids=["placed", "keyed-then-placed"])
def test_placed_layer_over_a_background_through_the_crossfade(keyed):
    pic = km.green_screen(160, 90, seed=3)
    planes = inset_planes(pic, keyed)
    A, B = model_layer(planes), ov.HostFrame(W, H).fill(5, seed=2)
    src = upload(*pic)
    dA = video.place(video.key(src, kp(DEFAULT_CHROMA)) if keyed else src, pp(INSET))
    dB = video.DFrame(W, H).upload(*B.visible())
    for fader in (1.0, 0.6, 0.0):
        want = ov.HostFrame(W, H); ov.blank(want); ov.crossfade(want, A, B, fader)
        out = video.DFrame(W, H)
        video.crossfade(out, dA, dB, fader)
        assert_frame_equal(out, want, f"fader {fader}")
        if fader == 1.0:   # a small layer is shown, and the background is intact outside it
            got, bg = out.download(), B.visible()
            mask = np.ones((H, W), bool); mask[12:66, 216:312] = False
            assert np.array_equal(got[0][mask], bg[0][mask]) and np.array_equal(got[1][mask[::2, ::2]], bg[1][mask[::2, ::2]])
            assert not np.array_equal(got[0][~mask], bg[0][~mask])


def mixer_graph(ticks, monitor=None):
    ws = Workspace(44100, 60)
    sa, sb = ws.source_video(), ws.source_video()
    m = ws.video_mixer(a=0, b=1, fader=0.8)
    ws.connect(sa, 0, m, 0); ws.connect(sb, 0, m, 1)
    mon = None
    if monitor:
        mon = ws.monitor(*monitor)
        ws.connect(m, 0, mon, 0)
    return ws.build(max_ticks_per_run=ticks), sa, sb, m, mon


@pytest.mark.parametrize("order", ["place", "key-place", "place-key"])
def test_video_mixer_graph_with_the_source_transform(order):
    """A placed layer A, and a keyed-then-placed one with the two settings made in either order, over B: the same pictures, the oracle's."""
    pic = km.green_screen(160, 90, seed=2)
    planes = inset_planes(pic, order != "place")
    A, B = model_layer(planes), ov.HostFrame(W, H).fill(4, seed=5)
    g, sa, sb, m, _ = mixer_graph(2)
    dA, dB = upload(*pic), video.DFrame(W, H).upload(*B.visible())
    for step in order.split("-"):
        if step == "place":
            video.graph_set_video_source_place(g, sa, pp(INSET))
        else:
            video.graph_set_video_source_key(g, sa, kp(DEFAULT_CHROMA))
    video.graph_set_video_source(g, sa, dA, repeat=True)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    om = ov.OracleVideoMixer(a=0, b=1, fader=0.8)
    for tick in range(2):
        g.run_ticks(tick, 1)
        want = om.run_tick(tick * 735, [(A, (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
        assert_frame_equal(video.graph_video_output(g, m, 0), want, f"tick {tick}")
        placed = video.graph_video_output(g, sa, 0)                      # the source's port carries the placed frame
        assert_planes(placed, planes, "source port")
        if tick == 0:
            first = placed.handle
        else:
            assert placed.handle == first, "a repeated frame is placed once and the result reused"


def test_ring_of_three_frames_over_a_batched_run_keeps_every_ticks_picture():
    """The pool rule: 40 ticks in ONE submission, a Monitor keeping every tick's composite.  First a ring of three frames (three placed frames, reused), then the
    same pictures as 40 frames queued one per tick that the caller lets go of at once -- output frames are recycled, and only once nothing holds them."""
    Wc, Hc, T = 322, 182, 40
    p = PlaceP(Wc, Hc, 200, -10, 140, 80, 10, 6, 120, 60)
    pics = [km.green_screen(160, 90, seed=s) for s in (1, 2, 3)]
    B = ov.HostFrame(Wc, Hc).fill(2, seed=9)
    want = []
    for pic in pics:
        yk, uk, vk, k = key_model(*pic, DEFAULT_CHROMA)
        w = ov.HostFrame(Wc, Hc); ov.blank(w); ov.crossfade(w, model_layer(place_model(yk, uk, vk, p, k)), B, 0.8)
        want.append([x.copy() for x in w.visible()])
    g, sa, sb, m, mon = mixer_graph(T, monitor=(Wc, Hc))
    dB = video.DFrame(Wc, Hc).upload(*B.visible())
    video.graph_set_video_source(g, sb, dB, repeat=True)
    video.graph_set_video_source_key(g, sa, kp(DEFAULT_CHROMA))
    video.graph_set_video_source_place(g, sa, pp(p))
    ring = [upload(*pic) for pic in pics]
    video.graph_set_video_source_ring(g, sa, ring)
    g.run_ticks(0, T)
    for k, planes in enumerate(ingest.graph_read_monitor_video(g, mon, 0, T)):
        assert planes is not None and all(np.array_equal(x, y) for x, y in zip(planes, want[k % 3])), f"ring: tick {k}"
    handles = set()
    for k in range(6):                                                    # two more rounds of the ring, tick by tick: still the same three placed frames
        g.run_ticks(T + k, 1)
        handles.add(video.graph_video_output(g, sa, 0).handle)
    assert len(handles) == 3
    video.graph_set_video_source_ring(g, sa, [])
    del ring
    t0 = T + 6
    for k in range(T):
        d = upload(*pics[k % 3])
        ingest.graph_queue_video_source(g, sa, t0 + k, d, dur=(1, 60), off=(0, 1))
        del d
    g.run_ticks(t0, T)
    for k, planes in enumerate(ingest.graph_read_monitor_video(g, mon, 0, T)):
        assert planes is not None and all(np.array_equal(x, y) for x, y in zip(planes, want[k % 3])), f"queued: tick {k}"


LONG_RING_HANDLES = 32   # distinct placed frames one pass of the 40-frame ring delivers tick by tick.  MEASURED on the commit before the transform left Graph, not derived


def test_ring_longer_than_the_done_list_recycles_placed_frames_within_the_pool_cap():
    """A ring of 40 distinct frames, more than the 32 entries the list of placed frames holds, keyed and placed: every tick keys into one pool (frames no
    list holds) and places into the other.  Two passes in ONE submission with a Monitor (its copies are its own, so the placed frames recycle), then one pass
    tick by tick: every picture is the model's, and the pass hands out a fixed number of distinct frames -- no fewer than the list pins, no more than the
    pool's cap of 64."""
    Wc, Hc, N = 66, 34, 40
    p = PlaceP(Wc, Hc, 20, -4, 40, 24, 2, 2, 60, 30)
    pics = [km.green_screen(Wc, Hc, seed=s) for s in range(1, N + 1)]
    B = ov.HostFrame(Wc, Hc).fill(2, seed=9)
    placed, want = [], []
    for pic in pics:
        yk, uk, vk, k = key_model(*pic, DEFAULT_CHROMA)
        placed.append(place_model(yk, uk, vk, p, k))
        w = ov.HostFrame(Wc, Hc); ov.blank(w); ov.crossfade(w, model_layer(placed[-1]), B, 0.8)
        want.append([x.copy() for x in w.visible()])
    g, sa, sb, m, mon = mixer_graph(2 * N, monitor=(Wc, Hc))
    dB = video.DFrame(Wc, Hc).upload(*B.visible())
    video.graph_set_video_source(g, sb, dB, repeat=True)
    video.graph_set_video_source_key(g, sa, kp(DEFAULT_CHROMA))
    video.graph_set_video_source_place(g, sa, pp(p))
    ring = [upload(*pic, pad_seed=s) for s, pic in enumerate(pics)]
    video.graph_set_video_source_ring(g, sa, ring)
    g.run_ticks(0, 2 * N)
    for k, planes in enumerate(ingest.graph_read_monitor_video(g, mon, 0, 2 * N)):
        assert planes is not None and all(np.array_equal(x, y) for x, y in zip(planes, want[k % N])), f"batched: tick {k}"
    handles = set()
    for k in range(N):
        g.run_ticks(2 * N + k, 1)
        out = video.graph_video_output(g, sa, 0)
        assert_planes(out, placed[k], f"tick by tick: tick {k}")
        handles.add(out.handle)
        del out
    print(f"distinct placed frames in one pass of the ring: {len(handles)}")
    assert 32 <= LONG_RING_HANDLES <= 64
    assert len(handles) == LONG_RING_HANDLES


def test_removing_the_placement_gives_the_pictures_of_a_graph_that_never_had_it():
    pic = km.green_screen(W, H, seed=6)
    B = ov.HostFrame(W, H).fill(1, seed=1)
    outs = []
    for placed_first in (False, True):
        g, sa, sb, m, _ = mixer_graph(2)
        dA, dB = upload(*pic), video.DFrame(W, H).upload(*B.visible())
        video.graph_set_video_source(g, sa, dA, repeat=True)
        video.graph_set_video_source(g, sb, dB, repeat=True)
        if placed_first:
            video.graph_set_video_source_place(g, sa, pp(INSET))
            g.run_ticks(0, 2)
            placed = [x.copy() for x in video.graph_video_output(g, m, 0).download()]
            video.graph_set_video_source_place(g, sa, None)
        g.run_ticks(2, 2)
        outs.append([x.copy() for x in video.graph_video_output(g, m, 0).download()])
        assert not video.graph_video_output(g, sa, 0).has_alpha()
    assert all(np.array_equal(x, y) for x, y in zip(*outs))
    assert any(not np.array_equal(x, y) for x, y in zip(placed, outs[0]))   # and the placement had made a difference


def test_a_new_setting_replaces_the_placed_frames():
    """a frame is transformed once per SETTING: moving the rectangle, or changing the key under it, gives the new picture of the same source frame"""
    pic = km.green_screen(160, 90, seed=4)
    g, sa, sb, m, _ = mixer_graph(1)
    d = upload(*pic)
    video.graph_set_video_source(g, sa, d, repeat=True)
    tick = 0
    for p, key in ((INSET, None), (INSET.but(dst_x=-20, dst_y=100), None), (INSET.but(dst_x=-20, dst_y=100), DEFAULT_CHROMA), (INSET, DEFAULT_CHROMA.but(invert=1)), (INSET, None)):
        video.graph_set_video_source_place(g, sa, pp(p))
        video.graph_set_video_source_key(g, sa, kp(key) if key else None)
        g.run_ticks(tick, 1); tick += 1
        y, u, v = pic
        k = None
        if key:
            y, u, v, k = key_model(y, u, v, key)
        assert_planes(video.graph_video_output(g, sa, 0), place_model(y, u, v, p, k), f"{p} {key}")


BAD = [dict(canvas_w=67), dict(canvas_h=0), dict(canvas_w=16386), dict(crop_x=1, crop_w=8, crop_h=8), dict(crop_w=8, crop_h=0), dict(crop_x=2), dict(crop_w=7, crop_h=8),
       dict(dst_x=1), dict(dst_y=-3), dict(dst_w=0), dict(dst_h=5), dict(dst_w=16386), dict(crop_w=66, crop_h=8, dst_w=2), dict(crop_w=8, crop_h=34, dst_h=0)]


def test_errors_leave_everything_usable():
    pic = pm.noise_frame(66, 38, 1, False)[:3]
    d = upload(*pic)
    base = PlaceP(66, 38, 4, 2, 20, 10)
    good = pp(base)

    def raises(code, fn, *a):
        with pytest.raises(abi.MxError) as e:
            fn(*a)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    def bad_params(bad):
        prm = pp(base)
        for k, val in bad.items():
            setattr(prm, k, val)
        return prm

    for bad in BAD:
        raises(abi.MX_ERR_INVALID, video.place, d, bad_params(bad))
    raises(abi.MX_ERR_INVALID, video.place, d, pp(base.but(crop_x=40, crop_y=0, crop_w=40, crop_h=18)))      # a crop outside the frame
    raises(abi.MX_ERR_INVALID, video.place, d, pp(base.but(crop_x=0, crop_y=30, crop_w=40, crop_h=18)))
    raises(abi.MX_ERR_INVALID, video.place, d, pp(base.but(dst_w=2)))                                        # the whole frame, 66 > 32 * 2
    nv12 = video.DFrame(66, 38, fmt=video.PIXFMT_NV12)
    raises(abi.MX_ERR_INVALID, video.place, nv12, good)
    raises(abi.MX_ERR_INVALID, video.place, video.DFrame(66, 38, fmt=video.PIXFMT_YUV444P), good)
    assert_planes(video.place(d, good), place_model(*pic, base), "after the refused calls")

    ws = Workspace(44100, 60)
    sv, sb = ws.source_video(), ws.source_video()
    au = ws.source_stereo(); amp = ws.amplifier(1.0, 0.0); ws.connect(au, 0, amp, 0)
    m = ws.video_mixer(a=0, b=1, fader=0.8)
    ws.connect(sv, 0, m, 0); ws.connect(sb, 0, m, 1)
    g = ws.build(max_ticks_per_run=2)
    for node in (au, amp, m):
        raises(abi.MX_ERR_TYPE, video.graph_set_video_source_place, g, node, good)
    raises(abi.MX_ERR_INVALID, video.graph_set_video_source_place, g, 99, good)
    for bad in BAD:
        raises(abi.MX_ERR_INVALID, video.graph_set_video_source_place, g, sv, bad_params(bad))
    # place together with band, in either order
    video.graph_set_video_source_band(g, sb, 64, 36, 0, 36, 128, 72, 0, 72)
    assert "band" in raises(abi.MX_ERR_INVALID, video.graph_set_video_source_place, g, sb, good)
    video.graph_set_video_source_band(g, sb, 64, 36, 0, 36, 128, 72, 0, 0)
    video.graph_set_video_source_place(g, sv, good)
    assert "place" in raises(abi.MX_ERR_INVALID, video.graph_set_video_source_band, g, sv, 64, 36, 0, 36, 128, 72, 0, 72)
    # a frame the placer cannot take fails the run, naming the node: another format, and a crop outside the frame that arrives
    video.graph_set_video_source(g, sv, nv12, repeat=True)
    assert f"node {sv}" in raises(abi.MX_ERR_INVALID, g.run_ticks, 0, 1)
    video.graph_set_video_source_place(g, sv, pp(base.but(crop_x=0, crop_y=0, crop_w=64, crop_h=36)))
    small = upload(*pm.noise_frame(34, 18, 2, False)[:3])
    video.graph_set_video_source(g, sv, small, repeat=True)
    assert f"node {sv}" in raises(abi.MX_ERR_INVALID, g.run_ticks, 0, 1)
    ingest.graph_queue_video_source(g, sv, 1, small, dur=(1, 60), off=(0, 1))
    video.graph_set_video_source(g, sv, d, repeat=True)
    assert f"node {sv}" in raises(abi.MX_ERR_INVALID, g.run_ticks, 0, 2)                                      # the queued frame of tick 1
    # ... and the graph goes on: the same node with a frame it can take
    video.graph_set_video_source_place(g, sv, good)
    B = ov.HostFrame(66, 38).fill(3, seed=3)
    dB = video.DFrame(66, 38).upload(*B.visible())
    video.graph_set_video_source(g, sv, d, repeat=True)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    g.run_ticks(2, 2)
    want = ov.OracleVideoMixer(a=0, b=1, fader=0.8)
    w0 = None
    for tick in range(2):
        w0 = want.run_tick(tick * 735, [(model_layer(place_model(*pic, base)), (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
    assert_frame_equal(video.graph_video_output(g, m, 0), w0, "after the refused calls")


def test_scope_tap_on_a_placed_source_sees_the_placed_frame():
    pic = km.green_screen(160, 90, seed=5)
    p = PlaceP(130, 74, 20, 10, 64, 36)
    ws = Workspace(44100, 60)
    sv = ws.source_video()
    m = ws.video_mixer(a=0, b=None, fader=1.0)
    ws.connect(sv, 0, m, 0)
    g = ws.build()
    g.set_video_scopes([(sv, 0)], 0, False, 1)
    video.graph_set_video_source_place(g, sv, pp(p))
    d = upload(*pic)
    video.graph_set_video_source(g, sv, d, repeat=True)
    g.run_ticks(0, 1)
    rec = g.read_video_scopes()[0][0]
    yo, uo, vo, _k = place_model(*pic, p)
    assert rec["pixfmt"] == video.PIXFMT_YUVA420P
    for k, plane in enumerate((yo, uo, vo)):
        assert np.array_equal(rec["hist"][k], np.bincount(plane.ravel(), minlength=256))
    assert not np.array_equal(rec["hist"][0], np.bincount(pic[0].ravel(), minlength=256))
