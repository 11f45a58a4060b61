"""The keyer on the device (mx_video_key, mx_graph_set_video_source_key) against tests/video_key_model.py, bit for bit: integer work.
The composites go through the existing compositor and are compared with the oracle's alpha cross-fade fed the MODEL's keyed planes."""
import ctypes as C

import numpy as np
import pytest

import alpha_patterns as ap
import oracle_video as ov
import video_key_model as km
from mixlab_amd import abi, ingest, video
from mixlab_amd.workspace import Workspace
from video_key_model import DEFAULT_CHROMA, DEFAULT_LUMA, KeyP, key_model

pytestmark = pytest.mark.gpu

SIZES = [(2, 2), (34, 2), (2, 34), (66, 38), (130, 74), (322, 182), (1920, 1080)]   # the smallest at which chunking, the halo column / row and the edges can go wrong
PARAMS = {
    "chroma-default": DEFAULT_CHROMA,                                                                    # soft ramp, partial spill
    "chroma-invert-nospill": DEFAULT_CHROMA.but(invert=1, spill_strength=0),
    "chroma-hard-fullspill": DEFAULT_CHROMA.but(near_q4=300, far_q4=300, spill_far_q4=1200, spill_strength=255),
    "chroma-span1": DEFAULT_CHROMA.but(near_q4=400, far_q4=401, spill_far_q4=402, spill_strength=100),
    "chroma-span65535": DEFAULT_CHROMA.but(near_q4=0, far_q4=65535, spill_far_q4=65535, invert=1),
    "chroma-spill-span65535": DEFAULT_CHROMA.but(near_q4=0, far_q4=0, spill_far_q4=65535, spill_strength=255),
    "luma-default": DEFAULT_LUMA,
    "luma-invert-hard": DEFAULT_LUMA.but(near_q4=2048, far_q4=2048, invert=1),
    "luma-span1": DEFAULT_LUMA.but(near_q4=2047, far_q4=2048),
    "luma-span65535": DEFAULT_LUMA.but(near_q4=0, far_q4=65535),
}
BIG = ("chroma-default", "chroma-span1", "luma-default")   # the full-size frame: one soft chroma key with spill, one narrow ramp, the luma key


def kp(p: KeyP):
    return video.KeyParams(p.mode, p.key_u, p.key_v, bool(p.invert), p.near_q4, p.far_q4, p.spill_far_q4, p.spill_strength)


def upload(y, u, v, a=None):
    d = video.DFrame(y.shape[1], y.shape[0], fmt=video.PIXFMT_YUVA420P if a is not None else video.PIXFMT_YUV420P).upload(y, u, v)
    if a is not None:
        d.upload_alpha(a)
    return d


def assert_keyed(out, want, what):
    assert out.fmt == video.PIXFMT_YUVA420P and out.has_alpha()
    got = out.download() + [out.download_alpha()]
    for name, g, w in zip("YUVA", got, want):
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: plane {name} differs at {bad[:4].tolist()} ({len(bad)} samples), got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


def picture(w, h, mode):
    return km.green_screen(w, h, seed=1) if mode == km.KEY_CHROMA else km.luma_wedge(w, h, seed=1)


@pytest.mark.parametrize("with_alpha", [False, True], ids=["yuv420p", "yuva420p"])
@pytest.mark.parametrize("size", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_key_against_the_model_on_all_four_planes(size, with_alpha):
    w, h = size
    pics = {m: picture(w, h, m) for m in (km.KEY_CHROMA, km.KEY_LUMA)}
    a = ap.alpha_plane(w, h, "random", 3) if with_alpha else None
    dev = {m: upload(*pics[m], a) for m in pics}
    for name in (BIG if w * h > 100000 else PARAMS):
        p = PARAMS[name]
        out = video.key(dev[p.mode], kp(p))
        assert_keyed(out, key_model(*pics[p.mode], p, a_in=a), name)


@pytest.mark.parametrize("mode", ["chroma", "luma"])
def test_every_uv_pair(mode):
    """256 x 256 chroma planes enumerating every (U, V): from key (0, 0) every distance the square root can see, among them the 27 at which the f32 root of
    d2 << 8 is one too large (a hard key AT such a distance, 4608, shows an uncorrected root)."""
    y, u, v = km.every_uv()
    d = upload(y, u, v)
    if mode == "chroma":
        ps = [KeyP(km.KEY_CHROMA, 0, 0, 0, 4608, 4608, 0, 0), KeyP(km.KEY_CHROMA, 0, 0, 0, 0, 5769, 5770, 255), DEFAULT_CHROMA, DEFAULT_CHROMA.but(key_u=0, key_v=128)]
    else:
        ps = [DEFAULT_LUMA, DEFAULT_LUMA.but(near_q4=0, far_q4=4080)]
    for p in ps:
        assert_keyed(video.key(d, kp(p)), key_model(y, u, v, p), str(p))


@pytest.mark.parametrize("size", [(34, 2), (2, 34), (66, 38), (130, 74)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_padding_bytes_do_not_leak_into_edge_samples(size):
    """Every byte of the input's planes, stride padding included, is set to 0xFF on the device before the visible area is uploaded; keyed on (255, 255) -- and
    as a luma key that lets 255 through -- a padding byte read as picture would change the right-hand edge."""
    w, h = size
    hip = C.CDLL(str(abi.LIB_PATH))   # the HIP runtime the library is bound to
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    y, u, v = km.green_screen(w, h, seed=4, key=(255, 255))
    a = ap.alpha_plane(w, h, "soft-disc", 1)
    d = video.DFrame(w, h, fmt=video.PIXFMT_YUVA420P)
    video.sync()
    ptrs, strides = d.device_planes()
    for p in range(3):
        assert strides[p] > (w if p == 0 else w // 2)
        assert hip.hipMemset(ptrs[p], 0xFF, strides[p] * (h if p == 0 else h // 2)) == 0
    ap_, ast = C.c_void_p(), C.c_int32()
    abi.check(abi.lib.mx_dframe_alpha_plane(d._h, C.byref(ap_), C.byref(ast)))
    assert hip.hipMemset(ap_, 0xFF, ast.value * h) == 0
    assert hip.hipDeviceSynchronize() == 0
    d.upload(y, u, v); d.upload_alpha(a)
    for p in (KeyP(km.KEY_CHROMA, 255, 255, 0, 8 * 16, 40 * 16, 90 * 16, 255), KeyP(km.KEY_CHROMA, 255, 255, 1, 100, 101, 0, 0), DEFAULT_LUMA.but(invert=1)):
        assert_keyed(video.key(d, kp(p)), key_model(y, u, v, p, a_in=a), str(p))


# ---- composites: the existing compositor over the keyer's planes ----
def model_layer(y, u, v, p, a_in=None):
    """the MODEL's keyed frame as the oracle's layer"""
    yo, uo, vo, k = key_model(y, u, v, p, a_in=a_in)
    hf = ov.HostFrame(y.shape[1], y.shape[0])
    for plane, src in zip(hf.visible(), (yo, uo, vo)):
        plane[:] = src
    return hf.set_alpha(k)


def assert_frame_equal(d, hf, what):
    for p, (x, y) in enumerate(zip(d.download(), hf.visible())):
        bad = np.argwhere(x != y)
        assert bad.size == 0, f"{what}: plane {p} differs at {bad[:4].tolist()} ({len(bad)} samples)"


@pytest.mark.parametrize("name", ["chroma-default", "luma-default"])
def test_keyed_layer_over_a_background_through_the_crossfade(name):
    w, h = 320, 180
    p = PARAMS[name]
    pic = picture(w, h, p.mode)
    A, B = model_layer(*pic, p), ov.HostFrame(w, h).fill(5, seed=2)
    dA, dB = video.key(upload(*pic), kp(p)), video.DFrame(w, h).upload(*B.visible())
    for fader in (1.0, 0.6, 0.0):
        want = ov.HostFrame(w, h); ov.blank(want); ov.crossfade(want, A, B, fader)
        out = video.DFrame(w, h)
        video.crossfade(out, dA, dB, fader)
        assert_frame_equal(out, want, f"fader {fader}")


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


@pytest.mark.parametrize("layer", [(320, 180), (160, 120)], ids=["own-size", "scaled-160x120"])
def test_video_mixer_graph_with_the_source_transform(layer):
    """A keyed layer A (the picture's size, or 160 x 120 pillarboxed into it by the mixer's scaler: the coverage is resampled like luma, bars opaque) over B."""
    W, H = 320, 180
    p = DEFAULT_CHROMA
    pic = km.green_screen(*layer, seed=2)
    A, B = model_layer(*pic, p), ov.HostFrame(W, H).fill(4, seed=5)
    g, sa, sb, m, _ = mixer_graph(2)
    dA, dB = upload(*pic), video.DFrame(W, H).upload(*B.visible())
    video.graph_set_video_source_key(g, sa, kp(p))
    video.graph_set_video_source(g, sa, dA, repeat=True)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    om = ov.OracleVideoMixer(a=0, b=1, fader=0.8)
    for tick in range(2):
        g.run_ticks(tick, 1)
        want = om.run_tick(tick * 735, [(A, (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
        assert_frame_equal(video.graph_video_output(g, m, 0), want, f"tick {tick}")
        keyed = video.graph_video_output(g, sa, 0)                       # the source's port carries the keyed frame
        assert_keyed(keyed, key_model(*pic, p), "source port")
        if tick == 0:
            first = keyed.handle
        else:
            assert keyed.handle == first, "a repeated frame is keyed once and the result reused"


def test_ring_of_three_frames_over_a_batched_run_keeps_every_ticks_picture():
    """The pool rule: 40 ticks in ONE submission at the default MX_VIDEO_BATCH, a Monitor keeping every tick's composite.  First a ring of three frames (three
    keyed frames, reused), then the same pictures as 40 frames queued one per tick that the caller lets go of at once -- output frames are recycled, and only
    once nothing holds them."""
    W, H, T = 322, 182, 40
    p = DEFAULT_CHROMA
    pics = [km.green_screen(W, H, seed=s) for s in (1, 2, 3)]
    B = ov.HostFrame(W, H).fill(2, seed=9)
    want = []
    for pic in pics:
        w = ov.HostFrame(W, H); ov.blank(w); ov.crossfade(w, model_layer(*pic, p), B, 0.8)
        want.append([x.copy() for x in w.visible()])
    g, sa, sb, m, mon = mixer_graph(T, monitor=(W, H))
    dB = video.DFrame(W, H).upload(*B.visible())
    video.graph_set_video_source(g, sb, dB, repeat=True)
    video.graph_set_video_source_key(g, sa, kp(p))
    ring = [upload(*pic) for pic in pics]
    video.graph_set_video_source_ring(g, sa, ring)
    g.run_ticks(0, T)
    for k, planes in enumerate(ingest.graph_read_monitor_video(g, mon, 0, T)):
        assert planes is not None and all(np.array_equal(x, y) for x, y in zip(planes, want[k % 3])), f"ring: tick {k}"
    handles = set()
    for k in range(6):                                                    # two more rounds of the ring, tick by tick: still the same three keyed frames
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


LONG_RING_HANDLES = 32   # distinct keyed frames one pass of the 40-frame ring delivers tick by tick.  MEASURED on the commit before the transform left Graph, not derived


def test_ring_longer_than_the_done_list_recycles_keyed_frames_within_the_pool_cap():
    """A ring of 40 distinct frames, more than the 32 entries the list of keyed frames holds, so every tick keys anew and the output frames come out of
    the pool.  Two passes in ONE submission with a Monitor (its copies are its own, so the keyed frames recycle), then one pass tick by tick: every picture
    is the model's, and the pass hands out a fixed number of distinct frames -- no fewer than the list pins, no more than the pool's cap of 64."""
    W, H, N = 66, 34, 40
    p = DEFAULT_CHROMA
    pics = [km.green_screen(W, H, seed=s) for s in range(1, N + 1)]
    keyed = [key_model(*pic, p) for pic in pics]
    B = ov.HostFrame(W, H).fill(2, seed=9)
    want = []
    for pic in pics:
        w = ov.HostFrame(W, H); ov.blank(w); ov.crossfade(w, model_layer(*pic, p), B, 0.8)
        want.append([x.copy() for x in w.visible()])
    g, sa, sb, m, mon = mixer_graph(2 * N, monitor=(W, H))
    dB = video.DFrame(W, H).upload(*B.visible())
    video.graph_set_video_source(g, sb, dB, repeat=True)
    video.graph_set_video_source_key(g, sa, kp(p))
    ring = [upload(*pic) for pic in pics]
    video.graph_set_video_source_ring(g, sa, ring)
    g.run_ticks(0, 2 * N)
    for k, planes in enumerate(ingest.graph_read_monitor_video(g, mon, 0, 2 * N)):
        assert planes is not None and all(np.array_equal(x, y) for x, y in zip(planes, want[k % N])), f"batched: tick {k}"
    handles = set()
    for k in range(N):
        g.run_ticks(2 * N + k, 1)
        out = video.graph_video_output(g, sa, 0)
        assert_keyed(out, keyed[k], f"tick by tick: tick {k}")
        handles.add(out.handle)
        del out
    print(f"distinct keyed frames in one pass of the ring: {len(handles)}")
    assert 32 <= LONG_RING_HANDLES <= 64
    assert len(handles) == LONG_RING_HANDLES


def test_removing_the_key_gives_the_pictures_of_a_graph_that_never_had_it():
    W, H = 130, 74
    pic = km.green_screen(W, H, seed=6)
    B = ov.HostFrame(W, H).fill(1, seed=1)
    outs = []
    for keyed_first in (False, True):
        g, sa, sb, m, _ = mixer_graph(2)
        dA, dB = upload(*pic), video.DFrame(W, H).upload(*B.visible())
        video.graph_set_video_source(g, sa, dA, repeat=True)
        video.graph_set_video_source(g, sb, dB, repeat=True)
        if keyed_first:
            video.graph_set_video_source_key(g, sa, kp(DEFAULT_CHROMA))
            g.run_ticks(0, 2)
            keyed = [x.copy() for x in video.graph_video_output(g, m, 0).download()]
            video.graph_set_video_source_key(g, sa, None)
        g.run_ticks(2, 2)
        outs.append([x.copy() for x in video.graph_video_output(g, m, 0).download()])
        assert not video.graph_video_output(g, sa, 0).has_alpha()
    assert all(np.array_equal(x, y) for x, y in zip(*outs))
    assert any(not np.array_equal(x, y) for x, y in zip(keyed, outs[0]))   # and the key had made a difference


BAD = [dict(mode=2), dict(near_q4=700, far_q4=600), dict(far_q4=65536), dict(spill_far_q4=65536), dict(spill_strength=256),
       dict(mode=km.KEY_LUMA, spill_strength=1), dict(invert=2)]


def test_errors_leave_everything_usable():
    W, H = 66, 38
    pic = km.green_screen(W, H, seed=1)
    d = upload(*pic)
    good = kp(DEFAULT_CHROMA)

    def raises(code, fn, *a):
        with pytest.raises(abi.MxError) as e:
            fn(*a)
        assert e.value.code == code, str(e.value)
        return str(e.value)

    for bad in BAD:
        prm = kp(DEFAULT_CHROMA.but(spill_strength=0) if "mode" in bad and bad.get("spill_strength") is None else DEFAULT_CHROMA)
        for k, val in bad.items():
            setattr(prm, k, val)
        raises(abi.MX_ERR_INVALID, video.key, d, prm)
    prm = kp(DEFAULT_CHROMA); prm._pad = 1
    raises(abi.MX_ERR_INVALID, video.key, d, prm)
    nv12 = video.DFrame(W, H, fmt=video.PIXFMT_NV12)
    raises(abi.MX_ERR_INVALID, video.key, nv12, good)
    raises(abi.MX_ERR_INVALID, video.key, video.DFrame(W, H, fmt=video.PIXFMT_YUV444P), good)
    assert_keyed(video.key(d, good), key_model(*pic, DEFAULT_CHROMA), "after the refused calls")

    ws = Workspace(44100, 60)
    sv, sb = ws.source_video(), ws.source_video()
    au = ws.source_stereo(); amp = ws.amplifier(1.0, 0.0); ws.connect(au, 0, amp, 0)
    m = ws.video_mixer(a=0, b=1, fader=0.8)
    ws.connect(sv, 0, m, 0); ws.connect(sb, 0, m, 1)
    g = ws.build(max_ticks_per_run=2)
    for node in (au, amp, m):
        raises(abi.MX_ERR_TYPE, video.graph_set_video_source_key, g, node, good)
    raises(abi.MX_ERR_INVALID, video.graph_set_video_source_key, g, 99, good)
    for bad in BAD[1:5]:
        prm = kp(DEFAULT_CHROMA)
        for k, val in bad.items():
            setattr(prm, k, val)
        raises(abi.MX_ERR_INVALID, video.graph_set_video_source_key, g, sv, prm)
    # key together with band, in either order
    video.graph_set_video_source_band(g, sb, 64, 36, 0, 36, 128, 72, 0, 72)
    assert "band" in raises(abi.MX_ERR_INVALID, video.graph_set_video_source_key, g, sb, good)
    video.graph_set_video_source_band(g, sb, 64, 36, 0, 36, 128, 72, 0, 0)
    video.graph_set_video_source_key(g, sv, good)
    assert "key" in raises(abi.MX_ERR_INVALID, video.graph_set_video_source_band, g, sv, 64, 36, 0, 36, 128, 72, 0, 72)
    # a frame the keyer cannot take fails the run, naming the node
    video.graph_set_video_source(g, sv, nv12, repeat=True)
    msg = raises(abi.MX_ERR_INVALID, g.run_ticks, 0, 1)
    assert f"node {sv}" in msg
    # ... and the graph goes on: the same node with a frame it can take
    B = ov.HostFrame(W, H).fill(3, seed=3)
    dB = video.DFrame(W, H).upload(*B.visible())
    video.graph_set_video_source(g, sv, d, repeat=True)
    video.graph_set_video_source(g, sb, dB, repeat=True)
    g.run_ticks(0, 2)
    want = ov.OracleVideoMixer(a=0, b=1, fader=0.8)
    w0 = None
    for tick in range(2):
        w0 = want.run_tick(tick * 735, [(model_layer(*pic, DEFAULT_CHROMA), (1, 60), (0, 1)), (B, (1, 60), (0, 1)), None, None])
    assert_frame_equal(video.graph_video_output(g, m, 0), w0, "after the refused calls")


def test_scope_tap_on_a_keyed_source_sees_the_keyed_frame():
    W, H = 130, 74
    p = DEFAULT_CHROMA.but(spill_far_q4=3000, spill_strength=255)
    pic = km.green_screen(W, H, seed=5)
    ws = Workspace(44100, 60)
    sv = ws.source_video()
    m = ws.video_mixer(a=0, b=None, fader=1.0)
    ws.connect(sv, 0, m, 0)
    g = ws.build()
    g.set_video_scopes([(sv, 0)], 0, False, 1)
    video.graph_set_video_source_key(g, sv, kp(p))
    d = upload(*pic)
    video.graph_set_video_source(g, sv, d, repeat=True)
    g.run_ticks(0, 1)
    rec = g.read_video_scopes()[0][0]
    _y, uo, vo, _k = key_model(*pic, p)
    assert rec["pixfmt"] == video.PIXFMT_YUVA420P
    assert np.array_equal(rec["hist"][1], np.bincount(uo.ravel(), minlength=256)) and np.array_equal(rec["hist"][2], np.bincount(vo.ravel(), minlength=256))
    assert not np.array_equal(rec["hist"][1], np.bincount(pic[1].ravel(), minlength=256))
