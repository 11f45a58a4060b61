"""The colour corrector on the device (mx_video_grade, mx_graph_set_video_source_grade) against tests/video_grade_model.py, byte for byte:
integer work.  Every input frame's stride padding holds noise.  The graph form is composed from the existing models -- place_model(key_model(grade_model(frame)))
-- and goes through the existing compositor, compared with the oracle's cross-fade fed the MODELS' planes."""
import ctypes as C
import functools

import numpy as np
import pytest

import alpha_patterns as ap
import oracle_video as ov
import video_grade_model as gm
import video_scope_model as sm
from mixlab_amd import abi, ingest, video
from mixlab_amd.workspace import Workspace
from video_grade_model import CHROMA, CURVE, LUT, grade_model
from video_key_model import DEFAULT_CHROMA, key_model
from video_place_model import PlaceP, place_model

pytestmark = pytest.mark.gpu

# the smallest sizes at which a chunk edge (8 chroma samples), a single chroma column or row and the row's last word in the padding can go wrong; 258 x 150 is
# 17 chunks x 75 rows = 1275 threads: five tiles of 256, the last one partly filled, rows that end inside a tile
SIZES = [(2, 2), (16, 2), (18, 4), (2, 34), (34, 18), (66, 38), (130, 74), (322, 182), (258, 150)]
FLAG_SETS = [0, CURVE, CHROMA, LUT, CURVE | CHROMA | LUT]


def gp(p: gm.GradeP):
    return video.GradeParams(p.flags, p.curve, p.m, p.off)


@functools.lru_cache(maxsize=None)
def params(k, flags, lattice="random"):
    return gm.shared_params(k, flags, lattice)


@functools.lru_cache(maxsize=None)
def device_lut(k, lattice="random"):
    return video.Lut(k, params(k, LUT, lattice).nodes)


def lut_for(p: gm.GradeP, lattice="random"):
    return device_lut(p.k, lattice) if p.flags & LUT else None


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


def upload(y, u, v, a=None, pad=1):
    """the frame on the device, every byte of its planes -- stride padding included -- set to noise (pad: its seed; "ff": to 0xFF) before the visible area is uploaded"""
    d = video.DFrame(y.shape[1], y.shape[0], fmt=video.PIXFMT_YUVA420P if a is not None else video.PIXFMT_YUV420P)
    video.sync()
    rng = np.random.default_rng(0xBAD + (0 if pad == "ff" else pad))
    for ptr, stride, rows, vis in planes_of(d):
        assert stride > vis or vis % 64 == 0
        junk = np.full(stride * rows, 0xFF, np.uint8) if pad == "ff" else rng.integers(0, 256, size=stride * rows).astype(np.uint8)
        assert hip().hipMemcpy(ptr, junk.ctypes.data_as(C.c_void_p), junk.size, 1) == 0
    d.upload(y, u, v)
    if a is not None:
        d.upload_alpha(a)
    return d


def assert_graded(out, want, a, what):
    """want: the model's (Y', U', V'); a: the coverage plane the input carried, or None -- the output has the input's format"""
    assert out.fmt == (video.PIXFMT_YUVA420P if a is not None else video.PIXFMT_YUV420P) and out.has_alpha() == (a is not None), what
    got, want = out.download(), list(want)
    if a is not None:
        got, want = got + [out.download_alpha()], want + [a]
    for name, g, w in zip("YUVA", got, want):
        assert g.shape == w.shape, f"{what}: plane {name} is {g.shape}, want {w.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: plane {name} differs at {bad[:4].tolist()} ({len(bad)} samples), got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


# ---- the pixel call against the model ----
@pytest.mark.parametrize("with_alpha", [False, True], ids=["yuv420p", "yuva420p"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_grade_against_the_model_on_every_plane(size, with_alpha):
    w, h = size
    y, u, v = gm.noise_picture(w, h, 1)
    a = ap.alpha_plane(w, h, "random", 3) if with_alpha else None
    d = upload(y, u, v, a)
    for k in (4, 5):
        for flags in FLAG_SETS:
            if k == 5 and not flags & LUT:
                continue
            p = params(k, flags)
            assert not flags & LUT or (p.nodes.min() == 0 and p.nodes.max() == 4096)
            assert_graded(video.grade(d, gp(p), lut_for(p)), grade_model(y, u, v, p), a, f"lattice 2^{k} + 1, flags {flags}")


# 1920 x 1080 is 120 chunks x 540 rows = 64 800 threads = 254 tiles: one per workgroup of the LDS gather.  1920 x 1096 is 257 tiles, one more than the 256 staging
# workgroups: the first of them walks a second tile (the smallest frame that wide at which that happens)
BIG = [(1080, 4, CURVE | CHROMA | LUT, True), (1080, 5, CURVE | CHROMA | LUT, False), (1080, 4, CURVE | CHROMA, False), (1096, 4, CURVE | CHROMA | LUT, False)]


@pytest.mark.parametrize("h,k,flags,with_alpha", BIG, ids=["1080-all-17-yuva420p", "1080-all-33", "1080-curve-matrix", "1096-all-17-second-tile"])
def test_grade_full_size(h, k, flags, with_alpha):
    w = 1920
    y, u, v = gm.noise_picture(w, h, 2)
    a = ap.alpha_plane(w, h, "soft-disc", 1) if with_alpha else None
    p = params(k, flags, "smooth")
    assert_graded(video.grade(upload(y, u, v, a), gp(p), lut_for(p, "smooth")), grade_model(y, u, v, p), a, "1080p")


@pytest.mark.parametrize("size", [(66, 38), (322, 182)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_the_cached_gather_of_the_17_lattice_gives_the_same_bytes(size, monkeypatch):
    """MX_GRADE_GATHER=global (read at every launch) sends the 17-lattice down the path the 33-lattice always takes: the form tools/grade_cost.py times against the
    default, the lattice staged in LDS"""
    w, h = size
    y, u, v = gm.noise_picture(w, h, 7)
    p = params(4, CURVE | CHROMA | LUT)
    d = upload(y, u, v)
    want = grade_model(y, u, v, p)
    assert_graded(video.grade(d, gp(p), lut_for(p)), want, None, "staged in LDS")
    monkeypatch.setenv("MX_GRADE_GATHER", "global")
    assert_graded(video.grade(d, gp(p), lut_for(p)), want, None, "through the caches")


@pytest.mark.parametrize("k", [4, 5])
def test_every_uv_pictures(k):
    """the pictures tests/test_cpu_video_grade.py shows to meet every fraction ordering, every tie, the end cells, both clip ends and the negative sums"""
    p = params(k, CURVE | CHROMA | LUT)
    for s in gm.LUMA_SHIFTS:
        y, u, v = gm.every_uv_picture(s)
        assert_graded(video.grade(upload(y, u, v), gp(p), lut_for(p)), grade_model(y, u, v, p), None, f"shift {s}")


@pytest.mark.parametrize("size", [(2, 2), (18, 4), (2, 34), (34, 18), (66, 38), (130, 74)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_padding_bytes_do_not_leak_into_the_visible_area(size):
    """the same frame uploaded over three different paddings gives the same visible bytes, the model's: the sizes whose last chunk is partly padding"""
    w, h = size
    y, u, v = gm.noise_picture(w, h, 3)
    a = ap.alpha_plane(w, h, "random", 1)
    p = params(4, CURVE | CHROMA | LUT)
    want = grade_model(y, u, v, p)
    for pad in (1, 2, "ff"):
        assert_graded(video.grade(upload(y, u, v, a, pad=pad), gp(p), lut_for(p)), want, a, f"padding {pad}")
        assert_graded(video.grade(upload(y, u, v, pad=pad), gp(p.but(flags=CURVE | CHROMA))), grade_model(y, u, v, p.but(flags=CURVE | CHROMA)), None, f"padding {pad}, no LUT")


@pytest.mark.parametrize("size", [(66, 38), (322, 182)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_identity_settings_return_the_input(size):
    w, h = size
    y, u, v = gm.noise_picture(w, h, 4)
    a = ap.alpha_plane(w, h, "random", 2)
    d = upload(y, u, v, a)
    assert_graded(video.grade(d, video.GradeParams(0)), (y, u, v), a, "no flag set")
    ident = video.grade_procamp(0, 255, 1, 1, 0)
    ident.flags |= video.GRADE_LUT
    for k in (4, 5):
        assert_graded(video.grade(d, ident, video.Lut(k, video.lut_identity(k))), (y, u, v), a, f"identity curve, matrix and lattice 2^{k} + 1")


# ---- the graph form ----
W, H = 320, 180
INSET = PlaceP(W, H, 216, 12, 96, 54)
GRADE = params(4, CURVE | CHROMA | LUT, "smooth")


def kp(p):
    return video.KeyParams(p.mode, p.key_u, p.key_v, bool(p.invert), p.near_q4, p.far_q4, p.spill_far_q4, p.spill_strength)


def pp(p: PlaceP):
    return video.PlaceParams(p.canvas_w, p.canvas_h, p.dst_x, p.dst_y, p.dst_w, p.dst_h, crop=p.crop())


def green_picture(w, h, seed):
    import video_key_model as km
    return km.green_screen(w, h, seed=seed)


def transformed(pic, steps, grade=GRADE):
    """place_model(key_model(grade_model(frame))) for the steps present -> (y, u, v, coverage or None)"""
    y, u, v = pic
    k = None
    if "grade" in steps:
        y, u, v = grade_model(y, u, v, grade)
    if "key" in steps:
        y, u, v, k = key_model(y, u, v, DEFAULT_CHROMA)
    if "place" in steps:
        y, u, v, k = place_model(y, u, v, INSET, k)
    return y, u, v, k


def model_layer(planes):
    yo, uo, vo, k = planes
    hf = ov.HostFrame(yo.shape[1], yo.shape[0])
    for plane, src in zip(hf.visible(), (yo, uo, vo)):
        plane[:] = src
    return hf.set_alpha(k) if k is not None else hf


def assert_port(d, planes, what):
    assert_graded(d, planes[:3], planes[3], what)


def assert_frame_equal(d, hf, what):
    for p, (x, y) in enumerate(zip(d.download(), hf.visible())):
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"{what}: plane {p} differs at {bad[:4].tolist()} ({len(bad)} samples)"


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


def set_step(g, node, step, grade=GRADE, lattice="smooth"):
    if step == "grade":
        video.graph_set_video_source_grade(g, node, gp(grade), lut_for(grade, lattice))
    elif step == "key":
        video.graph_set_video_source_key(g, node, kp(DEFAULT_CHROMA))
    else:
        video.graph_set_video_source_place(g, node, pp(INSET))


@pytest.mark.parametrize("order", ["grade", "key-grade", "place-key-grade", "key-place-grade", "grade-place-key"])
def test_video_mixer_graph_with_the_source_transform(order):
    """A graded layer A -- graded and keyed, graded, keyed and placed, the setters called in orders other than grade, key, place -- over B: the source's port carries
    place_model(key_model(grade_model(frame))), and the program output is the oracle's composite of it."""
    steps = order.split("-")
    pic = green_picture(160, 90, 2) if "place" in steps else green_picture(W, H, 2)
    planes = transformed(pic, steps)
    A, B = model_layer(planes), ov.HostFrame(W, H).fill(4, seed=5)
    g, sa, sb, m, _ = mixer_graph(2)
    dA, dB = upload(*pic), video.DFrame(W, H).upload(*B.visible())
    for step in steps:
        set_step(g, sa, step)
    video.graph_set_video_source(g, sa, dA, repeat=True)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    om = ov.OracleVideoMixer(a=0, b=1, fader=0.8)
    for tick in range(2):
        g.run_ticks(tick, 1)
        want = om.run_tick(tick * 735, [(A, (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
        assert_frame_equal(video.graph_video_output(g, m, 0), want, f"tick {tick}")
        out = video.graph_video_output(g, sa, 0)                         # the source's port carries the transformed frame
        assert_port(out, planes, "source port")
        if tick == 0:
            first = out.handle
        else:
            assert out.handle == first, "a repeated frame is transformed once and the result reused"
    if order == "grade":                                                 # the key decides on the corrected colour: grading after the key would give another picture
        y, u, v, k = key_model(*pic, DEFAULT_CHROMA)
        assert not np.array_equal(k, transformed(pic, ["grade", "key"])[3])


def composite(planes, B):
    w = ov.HostFrame(B.w, B.h); ov.blank(w); ov.crossfade(w, model_layer(planes), B, 0.8)
    return [x.copy() for x in w.visible()]


def test_ring_of_three_frames_over_a_batched_run_keeps_every_ticks_picture():
    """The pool rule: 40 ticks in ONE submission, a Monitor keeping every tick's composite.  First a ring of three frames (three graded frames, reused), then the same
    pictures as 40 frames queued one per tick that the caller lets go of at once -- output frames are recycled, and only once nothing holds them."""
    Wr, Hr, T = 322, 182, 40
    pics = [green_picture(Wr, Hr, s) for s in (1, 2, 3)]
    B = ov.HostFrame(Wr, Hr).fill(2, seed=9)
    want = [composite(transformed(pic, ["grade", "key"]), B) for pic in pics]
    g, sa, sb, m, mon = mixer_graph(T, monitor=(Wr, Hr))
    dB = video.DFrame(Wr, Hr).upload(*B.visible())
    video.graph_set_video_source(g, sb, dB, repeat=True)
    set_step(g, sa, "key"); set_step(g, sa, "grade")
    ring = [upload(*pic) for pic in pics]
    video.graph_set_video_source_ring(g, sa, ring)
    g.run_ticks(0, T)
    for k, planes in enumerate(ingest.graph_read_monitor_video(g, mon, 0, T)):
        assert planes is not None and all(np.array_equal(x, y) for x, y in zip(planes, want[k % 3])), f"ring: tick {k}"
    handles = set()
    for k in range(6):                                                    # two more rounds of the ring, tick by tick: still the same three frames
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


def test_ring_longer_than_the_done_list_recycles_graded_frames_within_the_pool_cap():
    """A ring of 40 distinct frames, more than the 32 entries the list of graded frames holds, so every tick grades anew and the output frames come out of the pool.
    Two passes in ONE submission with a Monitor, then one pass tick by tick: every picture is the model's, and the pass hands out no fewer distinct frames than the
    list pins (32) and no more than the pool's cap (64)."""
    Wr, Hr, N = 66, 34, 40
    p = params(4, CURVE | CHROMA | LUT)
    pics = [gm.noise_picture(Wr, Hr, s) for s in range(1, N + 1)]
    graded = [grade_model(*pic, p) for pic in pics]
    B = ov.HostFrame(Wr, Hr).fill(2, seed=9)
    want = [composite(gr + (None,), B) for gr in graded]
    g, sa, sb, m, mon = mixer_graph(2 * N, monitor=(Wr, Hr))
    dB = video.DFrame(Wr, Hr).upload(*B.visible())
    video.graph_set_video_source(g, sb, dB, repeat=True)
    video.graph_set_video_source_grade(g, sa, gp(p), lut_for(p))
    ring = [upload(*pic) for pic in pics]
    video.graph_set_video_source_ring(g, sa, ring)
    g.run_ticks(0, 2 * N)
    for k, planes in enumerate(ingest.graph_read_monitor_video(g, mon, 0, 2 * N)):
        assert planes is not None and all(np.array_equal(x, y) for x, y in zip(planes, want[k % N])), f"batched: tick {k}"
    handles = set()
    for k in range(N):
        g.run_ticks(2 * N + k, 1)
        out = video.graph_video_output(g, sa, 0)
        assert_graded(out, graded[k], None, f"tick by tick: tick {k}")
        handles.add(out.handle)
        del out
    print(f"distinct graded frames in one pass of the ring: {len(handles)}")
    assert 32 <= len(handles) <= 64


def test_setting_again_removing_and_putting_back_leaves_no_stale_picture():
    """Another lattice at a run boundary, then no grade, then the first again, on a frame the source repeats: every run shows its own setting's picture, and without the
    grade the pictures are those of a graph that never had it.  The caller lets go of each lattice right after the set call."""
    Wr, Hr = 130, 74
    pic = gm.noise_picture(Wr, Hr, 6)
    B = ov.HostFrame(Wr, Hr).fill(1, seed=1)
    g, sa, sb, m, _ = mixer_graph(2)
    g0, sa0, sb0, m0, _ = mixer_graph(2)                                  # the graph that never had it
    dA, dB = upload(*pic), video.DFrame(Wr, Hr).upload(*B.visible())
    for gg, a, b in ((g, sa, sb), (g0, sa0, sb0)):
        video.graph_set_video_source(gg, a, dA, repeat=True)
        video.graph_set_video_source(gg, b, dB, repeat=True)
    g0.run_ticks(0, 2)
    plain = [x.copy() for x in video.graph_video_output(g0, m0, 0).download()]
    settings = [params(4, CURVE | CHROMA | LUT), params(5, CURVE | CHROMA | LUT), params(4, LUT, "smooth"), None, params(4, CURVE | CHROMA | LUT), params(4, CHROMA)]
    seen = []
    for i, p in enumerate(settings):
        if p is None:
            video.graph_set_video_source_grade(g, sa, None)
        else:
            lut = video.Lut(p.k, p.nodes) if p.flags & LUT else None      # a handle of the caller's own, released before the run
            video.graph_set_video_source_grade(g, sa, gp(p), lut)
            if lut is not None:
                lut.release()
            del lut
        g.run_ticks(2 * i, 2)
        port = video.graph_video_output(g, sa, 0)
        got = [x.copy() for x in video.graph_video_output(g, m, 0).download()]
        if p is None:
            assert_graded(port, pic, None, "grade removed")
            assert all(np.array_equal(x, y) for x, y in zip(got, plain)), "after removal the pictures are those of a graph that never had the grade"
        else:
            graded = grade_model(*pic, p)
            assert_graded(port, graded, None, f"setting {i}")
            assert all(np.array_equal(x, y) for x, y in zip(got, composite(graded + (None,), B))), f"setting {i}: program output"
        seen.append(got)
    assert not all(np.array_equal(x, y) for x, y in zip(seen[0], seen[1])) and not all(np.array_equal(x, y) for x, y in zip(seen[0], seen[3]))   # the settings differ


def test_scope_tap_on_a_graded_source_sees_the_graded_frame():
    Wr, Hr = 130, 74
    pic = gm.noise_picture(Wr, Hr, 5)
    p = params(5, CURVE | CHROMA | LUT, "smooth")
    ws = Workspace(44100, 60)
    sv = ws.source_video()
    m = ws.video_mixer(a=0, b=None, fader=1.0)
    ws.connect(sv, 0, m, 0)
    g = ws.build()
    g.set_video_scopes([(sv, 0)], 64, True, 1)
    video.graph_set_video_source_grade(g, sv, gp(p), lut_for(p, "smooth"))
    d = upload(*pic)
    video.graph_set_video_source(g, sv, d, repeat=True)
    g.run_ticks(0, 1)
    rec = g.read_video_scopes()[0][0]
    want = sm.record((sm.PIXFMT_YUV420P, Wr, Hr, grade_model(*pic, p)), 0, 64, True)
    assert sm.same(rec, want), sm.first_difference(rec, want)
    assert not sm.same(rec, sm.record((sm.PIXFMT_YUV420P, Wr, Hr, pic), 0, 64, True))


def test_errors_leave_everything_usable():
    Wr, Hr = 66, 38
    pic = gm.noise_picture(Wr, Hr, 1)
    d = upload(*pic)
    p = params(4, CURVE | CHROMA | LUT)
    lut = lut_for(p)

    def raises(code, fn, *a):
        with pytest.raises(abi.MxError) as e:
            fn(*a)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    def bad_params():
        out = []
        for field, val in (("flags", 8 | CURVE), ("flags", 1 << 31), ("m_uu", 32768), ("m_vv", -32768), ("m_uv", 1 << 20), ("off_u", 255 * 4096 + 1), ("off_v", -255 * 4096 - 1)):
            prm = gp(p.but(flags=CURVE | CHROMA))
            setattr(prm, field, val)
            out.append(prm)
        return out

    for prm in bad_params():
        raises(abi.MX_ERR_INVALID, video.grade, d, prm)
    raises(abi.MX_ERR_INVALID, video.grade, d, gp(p))                                   # the LUT bit with no LUT
    raises(abi.MX_ERR_INVALID, video.grade, d, gp(p.but(flags=CURVE | CHROMA)), lut)    # a LUT without the bit
    nv12 = video.DFrame(Wr, Hr, fmt=video.PIXFMT_NV12)
    raises(abi.MX_ERR_INVALID, video.grade, nv12, gp(p), lut)
    raises(abi.MX_ERR_INVALID, video.grade, video.DFrame(Wr, Hr, fmt=video.PIXFMT_YUV444P), gp(p), lut)
    edge = gp(p.but(m=(32767, -32767, -32767, 32767), off=(255 * 4096, -255 * 4096)))   # the ends of the ranges are inside them
    assert_graded(video.grade(d, edge, lut), grade_model(*pic, p.but(m=(32767, -32767, -32767, 32767), off=(255 * 4096, -255 * 4096))), None, "coefficients at the ends of their ranges")
    assert_graded(video.grade(d, gp(p), lut), grade_model(*pic, p), None, "after the refused calls")

    ws = Workspace(44100, 60)
    sv, sb = ws.source_video(), ws.source_video()
    au = ws.source_stereo(); amp = ws.amplifier(1.0, 0.0); ws.connect(au, 0, amp, 0)
    m = ws.video_mixer(a=0, b=1, fader=0.8)
    ws.connect(sv, 0, m, 0); ws.connect(sb, 0, m, 1)
    g = ws.build(max_ticks_per_run=2)
    B = ov.HostFrame(Wr, Hr).fill(3, seed=3)
    dB = video.DFrame(Wr, Hr).upload(*B.visible())
    want = composite(grade_model(*pic, p) + (None,), B)

    def correct_tick(tick, what):
        video.graph_set_video_source_grade(g, sv, gp(p), lut)
        video.graph_set_video_source(g, sv, d, repeat=True)
        video.graph_set_video_source(g, sb, dB, repeat=True)
        g.run_ticks(tick, 1)
        got = video.graph_video_output(g, m, 0).download()
        assert all(np.array_equal(x, y) for x, y in zip(got, want)), what

    correct_tick(0, "before any refused call")
    for node in (au, amp, m):
        raises(abi.MX_ERR_TYPE, video.graph_set_video_source_grade, g, node, gp(p), lut)
    raises(abi.MX_ERR_INVALID, video.graph_set_video_source_grade, g, 99, gp(p), lut)
    correct_tick(1, "after a node that is no SOURCE_VIDEO")
    for prm in bad_params():
        raises(abi.MX_ERR_INVALID, video.graph_set_video_source_grade, g, sv, prm)
    raises(abi.MX_ERR_INVALID, video.graph_set_video_source_grade, g, sv, gp(p))
    raises(abi.MX_ERR_INVALID, video.graph_set_video_source_grade, g, sv, gp(p.but(flags=CURVE)), lut)
    correct_tick(2, "after refused parameters: the setting that stood still stands, and a good one replaces it")
    # grade together with band, in either order
    video.graph_set_video_source_band(g, sb, 64, 36, 0, 36, 128, 72, 0, 72)
    assert "band" in raises(abi.MX_ERR_INVALID, video.graph_set_video_source_grade, g, sb, gp(p), lut)
    video.graph_set_video_source_band(g, sb, 64, 36, 0, 36, 128, 72, 0, 0)
    assert "grade" in raises(abi.MX_ERR_INVALID, video.graph_set_video_source_band, g, sv, 64, 36, 0, 36, 128, 72, 0, 72)
    correct_tick(3, "after grade and band met")
    # a frame the corrector cannot take fails the run before anything is launched, naming the node
    video.graph_set_video_source(g, sv, nv12, repeat=True)
    msg = raises(abi.MX_ERR_INVALID, g.run_ticks, 4, 1)
    assert f"node {sv}" in msg
    correct_tick(4, "after a frame of another format")
