"""The matte refiner on the device (mx_video_matte, mx_graph_set_video_source_matte) against tests/video_matte_model.py, byte for byte on
all four planes: integer work.  The composites go through the existing compositor and are compared with the oracle's alpha cross-fade fed the MODEL's planes; the
graph form is composed from the existing models -- place_model(matte_model(key_model(grade_model(frame))))."""
import ctypes as C
import functools

import numpy as np
import pytest

import oracle_video as ov
import video_grade_model as gm
import video_key_model as km
import video_matte_model as mm
from mixlab_amd import abi, ingest, video
from mixlab_amd.workspace import Workspace
from video_grade_model import grade_model
from video_key_model import DEFAULT_CHROMA, key_model
from video_matte_model import MatteP, matte_model
from video_place_model import PlaceP, place_model

pytestmark = pytest.mark.gpu

# The issue's sizes (a single chroma sample, one chroma row, one chroma column, frames smaller than every radius, frames of several tiles) and two that straddle the
# kernel's 64 x 32 tile: 68 x 34 is one staged dword and one chroma row past a tile in each axis, 146 x 66 two tiles, a 16-byte word and a part of one past them
SIZES = [(2, 2), (34, 2), (2, 34), (66, 38), (130, 74), (322, 182), (68, 34), (146, 66)]


def mp(p: MatteP):
    return video.MatteParams(clean=p.clean, choke=p.choke, soften=p.soften, mask=p.mask, invert=bool(p.invert), feather_q4=p.feather, shape=p.shape)


def kp(p):
    return video.KeyParams(p.mode, p.key_u, p.key_v, bool(p.invert), p.near_q4, p.far_q4, p.spill_far_q4, p.spill_strength)


@functools.lru_cache(maxsize=None)
def hip():
    h = C.CDLL(str(abi.LIB_PATH))   # the HIP runtime the library is bound to
    h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    return h


def upload(y, u, v, a=None, pad=None):
    """the frame on the device; pad 0x00 / 0xFF: every byte of every plane, stride padding and the coverage plane's included, is set to it before the upload"""
    w, h = y.shape[1], y.shape[0]
    d = video.DFrame(w, h, fmt=video.PIXFMT_YUVA420P if a is not None else video.PIXFMT_YUV420P)
    if pad is not None:
        video.sync()
        ptrs, strides = d.device_planes()
        for p in range(3):
            assert strides[p] > (w if p == 0 else w // 2)
            assert hip().hipMemset(ptrs[p], pad, strides[p] * (h if p == 0 else h // 2)) == 0
        if a is not None:
            ap_, ast = C.c_void_p(), C.c_int32()
            abi.check(abi.lib.mx_dframe_alpha_plane(d._h, C.byref(ap_), C.byref(ast)))
            assert ast.value > w and hip().hipMemset(ap_, pad, ast.value * h) == 0
        assert hip().hipDeviceSynchronize() == 0
    d.upload(y, u, v)
    if a is not None:
        d.upload_alpha(a)
    return d


def assert_planes(out, want, what):
    """want: (Y, U, V, coverage)"""
    assert out.fmt == video.PIXFMT_YUVA420P and out.has_alpha(), what
    got = out.download() + [out.download_alpha()]
    for name, g, w in zip("YUVA", got, want):
        assert g.shape == w.shape, f"{what}: plane {name} is {g.shape}, want {w.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: plane {name} differs at {bad[:4].tolist()} ({len(bad)} samples), got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


def coverages(w, h):
    """the incoming coverage planes: the keyed green screen and the plane of specks, lines, staircase and edge ramps"""
    return {"keyed": mm.keyed_picture(w, h)[3], "speck": mm.speck_plane(w, h)}


# ---- the pixel call against the model ----
@pytest.mark.parametrize("with_alpha", [False, True], ids=["yuv420p", "yuva420p"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_matte_against_the_model_on_all_four_planes(size, with_alpha):
    w, h = size
    y, u, v, _k = mm.keyed_picture(w, h)
    for cname, a in (coverages(w, h).items() if with_alpha else [("none", None)]):
        d = upload(y, u, v, a)
        for name, p in mm.settings(w, h).items():
            assert_planes(video.matte(d, mp(p)), matte_model(y, u, v, p, a_in=a), f"{name}, coverage {cname}")


@pytest.mark.parametrize("with_alpha", [False, True], ids=["yuv420p", "yuva420p"])
def test_matte_full_size(with_alpha):
    """1920 x 1080, three settings: 1020 tiles, the last row of tiles 24 rows tall"""
    w, h = 1920, 1080
    y, u, v, k = mm.keyed_picture(w, h)
    a = k if with_alpha else None
    d = upload(y, u, v, a)
    for name in mm.BIG:
        p = mm.settings(w, h)[name]
        assert_planes(video.matte(d, mp(p)), matte_model(y, u, v, p, a_in=a), name)


PAD_SETTINGS = ("choke+6", "choke-6", "choke+1", "choke-1", "soften6", "choke6-soften6", "grow6-soften6", "all-rect", "clean", "circle-feather")


@pytest.mark.parametrize("pad", [0x00, 0xFF], ids=["pad00", "padff"])
@pytest.mark.parametrize("size", [(34, 2), (2, 34), (66, 38), (130, 74), (68, 34)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_padding_bytes_do_not_leak_into_edge_samples(size, pad):
    """Every byte of the input's planes, the coverage plane's stride padding included, is set to 0x00 (which a minimum would pull in) or to 0xFF (a maximum) on the
    device before the visible area is uploaded: the edge samples are the model's, which clamps the index."""
    w, h = size
    y, u, v, _k = mm.keyed_picture(w, h)
    for cname, a in coverages(w, h).items():
        d = upload(y, u, v, a, pad=pad)
        for name in PAD_SETTINGS:
            p = mm.settings(w, h)[name]
            want = matte_model(y, u, v, p, a_in=a)
            out = video.matte(d, mp(p))
            assert_planes(out, want, f"{name}, coverage {cname}")
            got = out.download_alpha()
            for edge in (np.s_[0, :], np.s_[-1, :], np.s_[:, 0], np.s_[:, -1]):
                assert np.array_equal(got[edge], want[3][edge])
    d = upload(y, u, v, None, pad=pad)
    assert_planes(video.matte(d, mp(MatteP(choke=2, soften=2))), matte_model(y, u, v, MatteP(choke=2, soften=2)), "no coverage")


# ---- composites: the existing compositor over the refiner's planes ----
def model_layer(planes):
    yo, uo, vo, k = planes
    hf = ov.HostFrame(yo.shape[1], yo.shape[0])
    for plane, src in zip(hf.visible(), (yo, uo, vo)):
        plane[:] = src
    return hf.set_alpha(k) if k is not None else hf


def assert_frame_equal(d, hf, what):
    for p, (x, y) in enumerate(zip(d.download(), hf.visible())):
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"{what}: plane {p} differs at {bad[:4].tolist()} ({len(bad)} samples)"


REFINE = MatteP(clean=(24, 230), choke=1, soften=2)


def test_keyed_then_matted_layer_over_a_background_through_the_crossfade():
    w, h = 320, 180
    pic = km.green_screen(w, h, seed=1)
    keyed = key_model(*pic, DEFAULT_CHROMA)
    A, B = model_layer(matte_model(*keyed[:3], REFINE, a_in=keyed[3])), ov.HostFrame(w, h).fill(5, seed=2)
    dA = video.matte(video.key(upload(*pic), kp(DEFAULT_CHROMA)), mp(REFINE))
    dB = video.DFrame(w, h).upload(*B.visible())
    for fader in (1.0, 0.6, 0.0):
        want = ov.HostFrame(w, h); ov.blank(want); ov.crossfade(want, A, B, fader)
        out = video.DFrame(w, h)
        video.crossfade(out, dA, dB, fader)
        assert_frame_equal(out, want, f"fader {fader}")


@pytest.mark.parametrize("kind", [mm.WIPE_LEFT, mm.WIPE_IRIS], ids=["left", "iris"])
def test_wipe_through_the_crossfade_with_the_fader_at_rest(kind):
    """fader 0: wa = 0, wb = aB, out = (A (255 - aB) + B aB) / 255 -- the shape written into B's coverage is the transition"""
    w, h = 320, 180
    A, Bp = ov.HostFrame(w, h).fill(5, seed=2), ov.HostFrame(w, h).fill(3, seed=7)
    dA, dB = video.DFrame(w, h).upload(*A.visible()), video.DFrame(w, h).upload(*Bp.visible())
    seen = []
    for pos in (9000, 32768, 60000):
        c = video.matte_wipe(kind, pos, 16 * 6 + 3, w, h)
        p = mm.wipe(kind, pos, 16 * 6 + 3, w, h)
        B = model_layer(matte_model(*Bp.visible(), p))
        want = ov.HostFrame(w, h); ov.blank(want); ov.crossfade(want, A, B, 0.0)
        out = video.DFrame(w, h)
        video.crossfade(out, dA, video.matte(dB, c), 0.0)
        assert_frame_equal(out, want, f"pos {pos}")
        seen.append(out.download()[0])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])


# ---- the graph form ----
W, H = 320, 180
INSET = PlaceP(W, H, 216, 12, 96, 54)
GRADE = gm.shared_params(4, gm.CURVE | gm.CHROMA, "smooth")
GMATTE = MatteP(clean=(24, 230), choke=-1, soften=1, mask=(16 * 10 + 4, 16 * 6 + 4, 16 * 150 + 4, 16 * 80 + 12), feather=16 * 3)


def pp(p: PlaceP):
    return video.PlaceParams(p.canvas_w, p.canvas_h, p.dst_x, p.dst_y, p.dst_w, p.dst_h, crop=p.crop())


def transformed(pic, steps, matte=GMATTE):
    """place_model(matte_model(key_model(grade_model(frame)))) for the steps present -> (y, u, v, coverage or None)"""
    y, u, v = pic
    k = None
    if "grade" in steps:
        y, u, v = grade_model(y, u, v, GRADE)
    if "key" in steps:
        y, u, v, k = key_model(y, u, v, DEFAULT_CHROMA)
    if "matte" in steps:
        y, u, v, k = matte_model(y, u, v, matte, a_in=k)
    if "place" in steps:
        y, u, v, k = place_model(y, u, v, INSET, k)
    return y, u, v, k


def set_step(g, node, step, matte=GMATTE):
    if step == "grade":
        video.graph_set_video_source_grade(g, node, video.GradeParams(GRADE.flags, GRADE.curve, GRADE.m, GRADE.off))
    elif step == "key":
        video.graph_set_video_source_key(g, node, kp(DEFAULT_CHROMA))
    elif step == "matte":
        video.graph_set_video_source_matte(g, node, mp(matte))
    else:
        video.graph_set_video_source_place(g, node, pp(INSET))


def mixer_graph(ticks, monitor=None, fader=0.8):
    ws = Workspace(44100, 60)
    sa, sb = ws.source_video(), ws.source_video()
    m = ws.video_mixer(a=0, b=1, fader=fader)
    ws.connect(sa, 0, m, 0); ws.connect(sb, 0, m, 1)
    mon = None
    if monitor:
        mon = ws.monitor(*monitor)
        ws.connect(m, 0, mon, 0)
    return ws.build(max_ticks_per_run=ticks), sa, sb, m, mon


def composite(planes, B, fader=0.8):
    w = ov.HostFrame(B.w, B.h); ov.blank(w); ov.crossfade(w, model_layer(planes), B, fader)
    return [x.copy() for x in w.visible()]


@pytest.mark.parametrize("order", ["matte", "matte-key", "place-matte-key-grade", "matte-grade-place-key", "key-place-grade-matte"])
def test_video_mixer_graph_with_the_source_transform(order):
    """The setters called in orders other than grade, key, matte, place: the source's port carries the models composed in the FIXED order and the program output is
    the oracle's composite of it; a repeated frame is transformed once."""
    steps = order.split("-")
    pic = km.green_screen(160, 90, seed=2) if "place" in steps else km.green_screen(W, H, seed=2)
    matte = GMATTE if "place" not in steps else GMATTE.but(mask=(16 * 5 + 4, 16 * 3 + 4, 16 * 75 + 4, 16 * 40 + 12))
    planes = transformed(pic, steps, matte)
    A, B = model_layer(planes), ov.HostFrame(W, H).fill(4, seed=5)
    g, sa, sb, m, _ = mixer_graph(2)
    dA, dB = upload(*pic), video.DFrame(W, H).upload(*B.visible())
    for step in steps:
        set_step(g, sa, step, matte)
    video.graph_set_video_source(g, sa, dA, repeat=True)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    om = ov.OracleVideoMixer(a=0, b=1, fader=0.8)
    for tick in range(2):
        g.run_ticks(tick, 1)
        want = om.run_tick(tick * 735, [(A, (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
        assert_frame_equal(video.graph_video_output(g, m, 0), want, f"tick {tick}")
        out = video.graph_video_output(g, sa, 0)                         # the source's port carries the transformed frame
        assert_planes(out, planes, "source port")
        if tick == 0:
            first = out.handle
        else:
            assert out.handle == first, "a repeated frame is matted once and the result reused"
    if order == "matte-key":                                             # the matte refines what the key decided: the two do not commute
        assert not np.array_equal(planes[3], key_model(*pic, DEFAULT_CHROMA)[3])


def test_ring_of_three_frames_over_a_batched_run_keeps_every_ticks_picture():
    """The pool rule: 40 ticks in ONE submission, a Monitor keeping every tick's composite.  First a ring of three frames (three matted frames, reused), then the
    same pictures as 40 frames queued one per tick that the caller lets go of at once -- output frames are recycled, and only once nothing holds them."""
    Wr, Hr, T = 322, 182, 40
    pics = [km.green_screen(Wr, Hr, seed=s) for s in (1, 2, 3)]
    B = ov.HostFrame(Wr, Hr).fill(2, seed=9)
    want = [composite(transformed(pic, ["key", "matte"], REFINE), B) for pic in pics]
    g, sa, sb, m, mon = mixer_graph(T, monitor=(Wr, Hr))
    dB = video.DFrame(Wr, Hr).upload(*B.visible())
    video.graph_set_video_source(g, sb, dB, repeat=True)
    video.graph_set_video_source_matte(g, sa, mp(REFINE))
    video.graph_set_video_source_key(g, sa, kp(DEFAULT_CHROMA))
    ring = [upload(*pic) for pic in pics]
    video.graph_set_video_source_ring(g, sa, ring)
    g.run_ticks(0, T)
    for k, planes in enumerate(ingest.graph_read_monitor_video(g, mon, 0, T)):
        assert planes is not None and all(np.array_equal(x, y) for x, y in zip(planes, want[k % 3])), f"ring: tick {k}"
    handles = set()
    for k in range(6):                                                    # two more rounds of the ring, tick by tick: still the same three matted frames
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


def test_a_wipe_moving_every_tick_over_a_repeated_frame_gives_each_tick_its_own_plane():
    """Setting again drops the cached pair: layer B carries the wipe's coverage, the fader rests on 0, and every tick's program is that tick's model plane."""
    Wr, Hr = 130, 74
    A, Bp = ov.HostFrame(Wr, Hr).fill(5, seed=2), ov.HostFrame(Wr, Hr).fill(3, seed=7)
    g, sa, sb, m, _ = mixer_graph(1, fader=0.0)
    dA, dB = video.DFrame(Wr, Hr).upload(*A.visible()), video.DFrame(Wr, Hr).upload(*Bp.visible())
    video.graph_set_video_source(g, sa, dA, repeat=True)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    om = ov.OracleVideoMixer(a=0, b=1, fader=0.0)
    for tick in range(8):
        kind, pos = (mm.WIPE_IRIS if tick & 1 else mm.WIPE_BOX), 6000 + 8000 * tick
        video.graph_set_video_source_matte(g, sb, video.matte_wipe(kind, pos, 40, Wr, Hr))
        g.run_ticks(tick, 1)
        planes = matte_model(*Bp.visible(), mm.wipe(kind, pos, 40, Wr, Hr))
        want = om.run_tick(tick * 735, [(A, (1, 60), (0, 1)), (model_layer(planes), (1, 60), (0, 1)), None, None])
        assert_frame_equal(video.graph_video_output(g, m, 0), want, f"tick {tick}")
        out = video.graph_video_output(g, sb, 0)
        assert_planes(out, planes, f"source port, tick {tick}")
        del out


def test_removing_the_matte_gives_the_pictures_of_a_graph_that_never_had_it():
    Wr, Hr = 130, 74
    pic = km.green_screen(Wr, Hr, seed=6)
    B = ov.HostFrame(Wr, Hr).fill(1, seed=1)
    outs = []
    for matted_first in (False, True):
        g, sa, sb, m, _ = mixer_graph(2)
        dA, dB = upload(*pic), video.DFrame(Wr, Hr).upload(*B.visible())
        video.graph_set_video_source(g, sa, dA, repeat=True)
        video.graph_set_video_source(g, sb, dB, repeat=True)
        video.graph_set_video_source_key(g, sa, kp(DEFAULT_CHROMA))
        if matted_first:
            video.graph_set_video_source_matte(g, sa, mp(REFINE))
            g.run_ticks(0, 2)
            matted = [x.copy() for x in video.graph_video_output(g, m, 0).download()]
            video.graph_set_video_source_matte(g, sa, None)
        g.run_ticks(2, 2)
        outs.append([x.copy() for x in video.graph_video_output(g, m, 0).download()])
        assert_planes(video.graph_video_output(g, sa, 0), key_model(*pic, DEFAULT_CHROMA), "the keyed frame alone")
    assert all(np.array_equal(x, y) for x, y in zip(*outs))
    assert any(not np.array_equal(x, y) for x, y in zip(matted, outs[0]))   # and the matte had made a difference


def test_scope_tap_on_a_matted_source_sees_the_matted_frame():
    Wr, Hr = 130, 74
    pic = km.green_screen(Wr, Hr, seed=5)
    ws = Workspace(44100, 60)
    sv = ws.source_video()
    m = ws.video_mixer(a=0, b=None, fader=1.0)
    ws.connect(sv, 0, m, 0)
    g = ws.build()
    g.set_video_scopes([(sv, 0)], 0, False, 1)
    video.graph_set_video_source_matte(g, sv, mp(REFINE))
    d = upload(*pic)
    video.graph_set_video_source(g, sv, d, repeat=True)
    g.run_ticks(0, 1)
    rec = g.read_video_scopes()[0][0]
    assert rec["pixfmt"] == video.PIXFMT_YUVA420P                         # the matted frame carries a coverage plane; the frame that was set does not
    assert np.array_equal(rec["hist"][0], np.bincount(pic[0].ravel(), minlength=256))
    assert_planes(video.graph_video_output(g, sv, 0), matte_model(*pic, REFINE), "source port")


def test_errors_leave_everything_usable():
    Wr, Hr = 66, 38
    y, u, v, k = mm.keyed_picture(Wr, Hr)
    d = upload(y, u, v, k)
    good = mp(REFINE)

    def raises(code, fn, *a):
        with pytest.raises(abi.MxError) as e:
            fn(*a)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    bad = mp(REFINE); bad.soften = 7
    raises(abi.MX_ERR_INVALID, video.matte, d, bad)
    stray = mp(MatteP()); stray.mask_feather_q4 = 3
    raises(abi.MX_ERR_INVALID, video.matte, d, stray)
    nv12 = video.DFrame(Wr, Hr, fmt=video.PIXFMT_NV12)
    raises(abi.MX_ERR_INVALID, video.matte, nv12, good)
    raises(abi.MX_ERR_INVALID, video.matte, video.DFrame(Wr, Hr, fmt=video.PIXFMT_YUV444P), good)
    assert_planes(video.matte(d, good), matte_model(y, u, v, REFINE, a_in=k), "after the refused calls")

    ws = Workspace(44100, 60)
    sv, sb = ws.source_video(), ws.source_video()
    au = ws.source_stereo(); amp = ws.amplifier(1.0, 0.0); ws.connect(au, 0, amp, 0)
    m = ws.video_mixer(a=0, b=1, fader=0.8)
    ws.connect(sv, 0, m, 0); ws.connect(sb, 0, m, 1)
    g = ws.build(max_ticks_per_run=2)
    for node in (au, amp, m):
        raises(abi.MX_ERR_TYPE, video.graph_set_video_source_matte, g, node, good)
    raises(abi.MX_ERR_INVALID, video.graph_set_video_source_matte, g, 99, good)
    raises(abi.MX_ERR_INVALID, video.graph_set_video_source_matte, g, sv, bad)
    # matte together with band, in either order
    video.graph_set_video_source_band(g, sb, 64, 36, 0, 36, 128, 72, 0, 72)
    assert "band" in raises(abi.MX_ERR_INVALID, video.graph_set_video_source_matte, g, sb, good)
    video.graph_set_video_source_band(g, sb, 64, 36, 0, 36, 128, 72, 0, 0)
    video.graph_set_video_source_matte(g, sv, good)
    assert "matte" in raises(abi.MX_ERR_INVALID, video.graph_set_video_source_band, g, sv, 64, 36, 0, 36, 128, 72, 0, 72)
    # a frame the refiner cannot take fails the run, naming the node
    video.graph_set_video_source(g, sv, nv12, repeat=True)
    msg = raises(abi.MX_ERR_INVALID, g.run_ticks, 0, 1)
    assert f"node {sv}" in msg
    # ... and the graph goes on: the same node with a frame it can take
    B = ov.HostFrame(Wr, Hr).fill(3, seed=3)
    dB = video.DFrame(Wr, Hr).upload(*B.visible())
    video.graph_set_video_source(g, sv, d, repeat=True)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    g.run_ticks(0, 2)
    om = ov.OracleVideoMixer(a=0, b=1, fader=0.8)
    A = model_layer(matte_model(y, u, v, REFINE, a_in=k))
    for tick in range(2):
        w0 = om.run_tick(tick * 735, [(A, (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
    assert_frame_equal(video.graph_video_output(g, m, 0), w0, "after the refused calls")
