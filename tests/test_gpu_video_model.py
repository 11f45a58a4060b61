"""The device's pixel path against the independent numpy model of DESIGN.md sections 6 and 7 (tests/video_model.py) -- NOT against the
oracle, which tests/test_cpu_video_model.py holds to the same model -- and, directly, against the f64 cubic within the bound derived
from the weights.  Small frames; the pictures are those of tests/video_cases.py (flat fields, checkerboards, steps, corner pixels, noise)
that test_cpu_video_model.py shows to tell every listed mis-model apart.

Every route a picture can take: the stateless scale (the tiled 4-tap kernel in each of its four staging variants with several tiles
and partial last tiles, the widened two-pass kernels), every input format, the persistent scaler across re-targets, row bands, the RGBA
chain with layers resampled by the scaler kernel and inside the chain kernel, a VideoMixer tick, YUV -> RGBA with every form of the matrix.

The gather kernel (MX_SCALE_SIMPLE=1, or windows beyond the tiled kernel's staging slots) is read once per process and is left to
test_gpu_video_parity.py (yuv410p / yuv411p inputs at 4x chroma enlargements reach it there) and tools/stress_scaler.py."""
import numpy as np
import pytest

import video_cases as vc
import video_model as vm
from mixlab_amd import shard, video
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

ALL_GEOMETRIES = {**{k: (s, d, "planar420") for k, (s, d) in vc.GEOMETRIES.items()}, **{k: v[:3] for k, v in vc.TILED.items()}}
LAYOUT_FMT = {"planar420": video.PIXFMT_YUV420P, "planar422": video.PIXFMT_YUV422P, "planar444": video.PIXFMT_YUV444P}


def upload(planes, w, h, fmt=video.PIXFMT_YUV420P):
    return video.DFrame(w, h, fmt=fmt).upload(*planes)


def assert_planes_equal(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape, f"{what}: plane {k}: {g.shape} for {w.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: plane {k}: {len(bad)} samples differ, first {bad[:3].tolist()}: device {g[tuple(bad[0])]} model {w[tuple(bad[0])]}"


def assert_within_the_ideal(dev, src, model, noise, what):
    """`dev`: the device's bytes of one resampled plane; `src` the plane they come from"""
    dh, dw = dev.shape
    ideal = np.clip(vm.ideal_scale_plane(src, dw, dh), 0, 255)
    bound = vm.ideal_bound(src.shape[1], dw, src.shape[0], dh)
    dist = np.abs(dev.astype(np.float64) - ideal)
    assert (dist <= bound).all(), f"{what}: {dist.max()} from the f64 cubic at {np.unravel_index(dist.argmax(), dist.shape)}, bound {bound.flat[dist.argmax()]}"
    nearest = np.floor(ideal + 0.5)
    assert np.abs(dev - nearest).max() <= 1, what
    if noise:            # a one-sided bias must not hide inside the +-1: no more than twice the model's own share of bytes off the nearest
        assert (dev != nearest).mean() <= 2 * (model != nearest).mean(), what


# ---- video.scale, stateless ----
@pytest.mark.parametrize("name", list(ALL_GEOMETRIES))
def test_stateless_scale_equals_the_model_and_stays_within_the_ideal(name):
    (iw, ih), (ow, oh), layout = ALL_GEOMETRIES[name]
    geo = video.scale_geometry(iw, ih, ow, oh)
    sw, sh, lx, ly = geo
    for pattern in vc.PATTERNS:
        planes = vc.yuv_planes(iw, ih, layout, pattern, seed=3)
        out = video.DFrame(ow, oh)
        video.scale(upload(planes, iw, ih, LAYOUT_FMT[layout]), out)
        got, want = out.download(), vm.scale_frame(planes, "planar", ow, oh, geo)
        assert_planes_equal(got, want, f"{name} {pattern}")
        for k in range(3):
            c = 1 if k else 0
            rect = (slice(ly >> c, (ly >> c) + (sh >> c)), slice(lx >> c, (lx >> c) + (sw >> c)))
            assert_within_the_ideal(got[k][rect], planes[k], want[k][rect], pattern == "noise", f"{name} {pattern} plane {k}")


def device_input(name, inp, w, h):
    fmt, kind, _detail = vc.format_entry(name, video)
    d = video.DFrame(w, h, fmt=fmt)
    if kind in ("packed422", "gray8", "rgb"):
        d.upload_packed(inp["planes"][0])
    else:
        d.upload(*inp["planes"])
    if inp["alpha"] is not None:
        d.upload_alpha(inp["alpha"])
    return d


@pytest.mark.parametrize("geom", list(vc.FORMAT_GEOMETRIES))
@pytest.mark.parametrize("name", vc.ALL_FORMATS)
def test_every_input_format_equals_the_model(name, geom):
    (iw, ih), (ow, oh) = vc.FORMAT_GEOMETRIES[geom]
    _fmt, kind, detail = vc.format_entry(name, video)
    geo = video.scale_geometry(iw, ih, ow, oh)
    sc = video.Scaler(ow, oh)
    for pattern in ("noise", "checker-1", "full"):
        inp = vc.make_input(kind, detail, iw, ih, pattern, seed=5)
        want = vm.scale_frame(*inp["model"], ow, oh, geo, alpha=inp["alpha"])
        d = device_input(name, inp, iw, ih)
        out = video.DFrame(ow, oh)
        video.scale(d, out)
        assert_planes_equal(out.download(), want[:3], f"{name} {geom} {pattern}")
        res = sc.scale(d)                                  # the persistent scaler carries a coverage plane along
        assert_planes_equal(res.download(), want[:3], f"{name} {geom} {pattern}, persistent scaler")
        assert res.has_alpha() == (len(want) == 4)
        if len(want) == 4:
            assert_planes_equal([res.download_alpha()], want[3:], f"{name} {geom} {pattern}: coverage")
        del res


# ---- video.Scaler, persistent, re-targeted ----
def test_persistent_scaler_retargeted_across_three_input_sizes():
    ow, oh = 134, 76
    sc = video.Scaler(ow, oh)
    for k, (iw, ih) in enumerate([(96, 54), (200, 120), (40, 60), (96, 54)]):   # 4-tap, widened, pillarbox, and back
        geo = video.scale_geometry(iw, ih, ow, oh)
        for pattern in ("noise", "checker-2", "corner-br"):
            planes = vc.yuv_planes(iw, ih, "planar420", pattern, seed=10 + k)
            assert_planes_equal(sc.scale(upload(planes, iw, ih)).download(), vm.scale_frame(planes, "planar", ow, oh, geo), f"call {k} {iw}x{ih} {pattern}")


# ---- video.scale_band ----
@pytest.mark.parametrize("src,full,split", [((96, 54), (134, 76), 38), ((40, 60), (96, 54), 26), ((200, 120), (134, 76), 40)], ids=["4-tap", "pillarbox-widened", "widened"])
def test_two_row_bands_concatenated_are_the_models_full_picture(src, full, split):
    """The band boundary falls inside the tap windows of the rows next to it (every row of a resampled plane reads at least four source
    rows, the slices overlap): the bands, each computed from its own slice of the source, must join into the picture of the whole."""
    (iw, ih), (W, H) = src, full
    geo = video.scale_geometry(iw, ih, W, H)
    for pattern in ("noise", "step-h", "checker-1"):
        planes = vc.yuv_planes(iw, ih, "planar420", pattern, seed=8)
        got = [[], [], []]
        needs = []
        for row0, rows in ((0, split), (split, H - split)):
            need = shard.band_source_rows((row0, rows), iw, ih, W, H)
            needs.append(need)
            sl = [planes[0][need[0]:need[0] + need[1]], planes[1][need[0] // 2:(need[0] + need[1]) // 2], planes[2][need[0] // 2:(need[0] + need[1]) // 2]]
            band = video.DFrame(W, rows)
            video.scale_band(upload(sl, iw, need[1]), ih, need[0], band, W, H, row0)
            for k, a in enumerate(band.download()):
                got[k].append(a)
        assert needs[0][0] + needs[0][1] > needs[1][0], "the two slices share source rows: the boundary is inside a tap window"
        assert_planes_equal([np.concatenate(g) for g in got], vm.scale_frame(planes, "planar", W, H, geo), f"{src}->{full} {pattern}")


# ---- the RGBA chain ----
MATRIX = [3900, 150, 46, 4096, 60, 3980, 56, -2048, 20, 120, 3956, 0]


@pytest.mark.parametrize("inline", ["0", "1"], ids=["scaler-kernel", "resampled-in-chain"])
@pytest.mark.parametrize("small,layout", [((96, 54), "planar420"), ((40, 60), "planar420"), ((96, 54), "planar444")], ids=["4-tap", "pillarbox", "widened-chroma"])
def test_rgba_chain_equals_the_model(small, layout, inline, monkeypatch):
    """A smaller layer A over a layer B of the program's size, through graph VideoMixer -> RGBA sink.  Fader 1.0: the program is A's scaled
    picture, fader 0.0: B; the sink's bytes are the model's RGBA of the model's picture either way.  (A VideoMixer only ever enlarges luma;
    the yuv444p layer's chroma shrinks 96 -> 67, which takes the widened kernels.)"""
    monkeypatch.setenv("MX_SCALE_INLINE", inline)          # read per call: layers resampled by the scaler kernel / inside the chain kernel
    W, H = 134, 76
    geo = video.scale_geometry(*small, W, H)
    for fader in (1.0, 0.0):
        ws = Workspace(44100, 60)
        a, b = ws.source_video(), ws.source_video()
        m = ws.video_mixer(a=0, b=1, fader=fader)
        ws.connect(a, 0, m, 0); ws.connect(b, 0, m, 1)
        rgba = ws.video_to_rgba(MATRIX)
        ws.connect(m, 0, rgba, 0)
        g = ws.build()
        for tick, pattern in enumerate(("noise", "checker-1", "corner-tl")):
            pa, pb = vc.yuv_planes(*small, layout, pattern, seed=20), vc.yuv_planes(W, H, "planar420", "noise", seed=21)
            da, db = upload(pa, *small, LAYOUT_FMT[layout]), upload(pb, W, H)
            video.graph_set_video_source(g, a, da, dur=(1, 60), off=(0, 1), repeat=True)
            video.graph_set_video_source(g, b, db, dur=(1, 60), off=(0, 1), repeat=True)
            g.run_ticks(tick, 1)                       # every tick delivers the sources' new frames
            want = vm.scale_frame(pa, "planar", W, H, geo) if fader == 1.0 else pb
            prog = video.graph_video_output(g, m, 0)
            assert (prog.width, prog.height) == (W, H)
            assert_planes_equal(prog.download(), want, f"program, fader {fader} {pattern}")
            assert np.array_equal(video.graph_rgba_output(g, rgba), vm.yuv420_to_rgba(*want, MATRIX)), f"RGBA sink, fader {fader} {pattern}"


# ---- VideoMixer.run_tick ----
@pytest.mark.parametrize("a,b,fader", [(0, 1, 1.0), (1, 0, 0.0)], ids=["fader-1", "fader-0"])
@pytest.mark.parametrize("small", [(96, 54), (40, 60)], ids=["fill", "pillarbox"])
def test_video_mixer_tick_of_two_sizes_is_one_scaled_layer(small, a, b, fader):
    """Inputs of two sizes: the program takes the larger width and height, the smaller layer is resampled into it.  With the small layer on
    channel A at fader 1.0, or on channel B at fader 0.0, the program is that layer's scaled picture and nothing else."""
    W, H = 134, 76
    geo = video.scale_geometry(*small, W, H)
    for pattern in ("noise", "checker-1", "full"):
        layer, other = vc.yuv_planes(*small, "planar420", pattern, seed=30), vc.yuv_planes(W, H, "planar420", "noise", seed=31)
        m = video.VideoMixer(a=a, b=b, fader=fader)
        prog, _a, _b = m.run_tick(0, [(upload(layer, *small), (1, 30), (0, 1)), (upload(other, W, H), (1, 30), (0, 1)), None, None])
        assert (prog.width, prog.height) == (W, H)
        assert_planes_equal(prog.download(), vm.scale_frame(layer, "planar", W, H, geo), f"a={a} b={b} fader {fader} {pattern}")


# ---- video.to_rgba ----
@pytest.mark.parametrize("matrix", vc.MATRICES, ids=[f"m{k}" for k in range(len(vc.MATRICES))])
@pytest.mark.parametrize("size", vc.RGBA_SIZES)
def test_yuv_to_rgba_equals_the_model(size, matrix):
    w, h = size
    bound = vm.ideal_rgba_bound()
    for pattern, planes in vc.rgba_inputs(w, h):
        got = video.to_rgba(upload(planes, w, h), matrix)
        assert np.array_equal(got, vm.yuv420_to_rgba(*planes, matrix)), pattern
        if matrix is None:                                 # and BT.709 from its primaries in f64, within the bound derived from the coefficients
            assert (got[..., 3] == 255).all()
            dist = np.abs(got[..., :3].astype(np.float64) - np.clip(vm.ideal_rgba(*planes), 0, 255)).max(axis=(0, 1))
            assert (dist <= bound).all(), (pattern, dist, bound)
