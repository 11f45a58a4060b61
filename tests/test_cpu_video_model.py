"""The pixel path's checker is checked: oracle/mixlab_oracle_video.c against an independent numpy model of DESIGN.md sections 6 and 7
(tests/video_model.py), that model against f64 references within bounds derived from its own weights, and the test pictures against
deliberate mis-models.  No GPU.

(a) the oracle's scaler, stand-in conversions and YUV -> RGBA equal the model on every byte, over the geometries and input formats that
    tests/test_gpu_video_model.py then runs on the device;
(b) the model stays within video_model.ideal_bound of the continuous cubic and within ideal_rgba_bound of BT.709 in f64 (the largest
    distances seen are recorded in DESIGN.md sections 6 and 7);
(c) the pictures reach every branch of the integer arithmetic, and each mis-model listed in MIS_MODELS changes at least one byte of at
    least one case -- so a kernel and an oracle that shared that misreading would fail the byte comparisons."""
from fractions import Fraction
from math import floor

import numpy as np
import pytest

import oracle_video as ov
import video_cases as vc
import video_model as vm
from mixlab_amd import video

ALL_GEOMETRIES = {**{k: (s, d, "planar420") for k, (s, d) in vc.GEOMETRIES.items()}, **{k: v[:3] for k, v in vc.TILED.items()}}


def host_frame(planes, w, h, fmt=0, alpha=None):
    f = ov.HostFrame(w, h, fmt)
    for k, p in enumerate(planes):
        f.planes[k][:, : p.shape[1]] = p
    if alpha is not None:
        f.set_alpha(alpha)
    return f


def oracle_input(name, inp, w, h):
    """the oracle's own frame of a scaler input, through the oracle's own stand-in conversions"""
    fmt, kind, detail = vc.format_entry(name, video)
    if kind in ("planar", "planar+alpha"):
        return host_frame(inp["planes"], w, h, 0 if kind == "planar+alpha" else fmt, inp["alpha"])
    if kind == "semi":
        return host_frame(inp["planes"], w, h, fmt)
    if kind == "packed422":
        return ov.yuyv_to_422p(inp["planes"][0], fmt)
    if kind == "gray8":      # the oracle has no entry point for it: tests hand it the yuv444p frame (test_gpu_video_parity.py does the same)
        g = inp["planes"][0]
        return host_frame([g, np.full_like(g, 0x80), np.full_like(g, 0x80)], w, h, video.PIXFMT_YUV444P)
    if kind == "rgb":
        return ov.packed_rgb_to_yuv444(inp["planes"][0], fmt)
    return ov.deep_to_8(inp["planes"], w, h, fmt)


def oracle_scale(src, ow, oh):
    want = ov.HostFrame(ow, oh)
    if hasattr(src, "alpha"):
        want.set_alpha(np.zeros((oh, ow), np.uint8))
    ov.blank(want); ov.dynamic_scale(src, want)
    return [p.copy() for p in want.visible()] + ([want.visible_alpha().copy()] if hasattr(src, "alpha") else [])


def assert_planes_equal(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(g != w)
        assert g.shape == w.shape and bad.size == 0, f"{what}: plane {k}: {len(bad)} samples differ, first {bad[:3].tolist()}: model {g[tuple(bad[0])]} oracle {w[tuple(bad[0])]}"


# ---- (a) the oracle equals the model ----
@pytest.mark.parametrize("name", list(ALL_GEOMETRIES))
def test_oracle_scaler_equals_the_model_on_every_byte(name):
    (iw, ih), (ow, oh), layout = ALL_GEOMETRIES[name]
    geo = ov.scaler_geometry(iw, ih, ow, oh)
    for pattern in vc.PATTERNS:
        planes = vc.yuv_planes(iw, ih, layout, pattern, seed=3)
        want = oracle_scale(host_frame(planes, iw, ih, {"planar420": 0, "planar422": 1}[layout]), ow, oh)
        assert_planes_equal(vm.scale_frame(planes, "planar", ow, oh, geo), want, f"{name} {pattern}")


def test_the_listed_geometries_are_what_their_comments_say():
    geo = {k: ov.scaler_geometry(*s, *d) for k, (s, d) in vc.GEOMETRIES.items()}
    assert geo["pillarbox"][2] % 4 == 2 and geo["pillarbox"][0] < 96           # an odd chroma offset
    assert geo["letterbox"][3] > 0 and geo["pillarbox-down"][2] > 0
    assert geo["same-size"] == (64, 36, 0, 0) and geo["destination-2x2"][:2] == (2, 2)
    assert vm.tap_tables(66, geo["down-just-above-1"][0])[1].shape[1] == 8 and vm.tap_tables(130, 10)[1].shape[1] == 54
    for name, ((iw, ih), (ow, oh), layout, variant) in vc.TILED.items():
        sw, sh, _lx, _ly = ov.scaler_geometry(iw, ih, ow, oh)
        cw, ch = vc.SUBSAMPLING[layout]
        jobs = [(iw, ih, sw, sh)] + [(iw >> cw, ih >> ch, sw >> 1, sh >> 1)] * 2
        assert all(s_w <= d_w and s_h <= d_h for s_w, s_h, d_w, d_h in jobs), name                     # four taps on every axis: the tiled kernel
        assert vc.tile_variant(jobs, lambda s, d: vm.tap_tables(s, d)[0]) == variant, name
        assert sw >= 130 and sh >= 42 and sw % 128 and sh % 32 and sh % 40, name                       # > 1 tile per axis, partial last tiles
    assert {v[3] for v in vc.TILED.values()} == {0, 1, 2, 3}


@pytest.mark.parametrize("geom", list(vc.FORMAT_GEOMETRIES))
@pytest.mark.parametrize("name", vc.ALL_FORMATS)
def test_oracle_equals_the_model_for_every_input_format(name, geom):
    (iw, ih), (ow, oh) = vc.FORMAT_GEOMETRIES[geom]
    _fmt, kind, detail = vc.format_entry(name, video)
    geo = ov.scaler_geometry(iw, ih, ow, oh)
    for pattern in ("noise", "checker-1", "full"):
        inp = vc.make_input(kind, detail, iw, ih, pattern, seed=5)
        src = oracle_input(name, inp, iw, ih)
        y, u, v, a = vm.stand_in(*inp["model"])                                # the stand-in frame itself, before any resampling
        if kind != "semi":                                                     # (the oracle keeps nv12 interleaved: nothing to compare before the scale)
            assert_planes_equal([y, u, v], src.visible(), f"{name} {pattern}: stand-in frame")
        if a is not None:
            assert np.array_equal(a, src.visible_alpha())
        got = vm.scale_frame(*inp["model"], ow, oh, geo, alpha=inp["alpha"])
        assert len(got) == (4 if kind == "planar+alpha" or (kind == "rgb" and "a" in detail) else 3)
        assert_planes_equal(got, oracle_scale(src, ow, oh), f"{name} {geom} {pattern}")


def test_the_format_lists_cover_what_the_scaler_accepts():
    ids = sorted(vc.format_entry(n, video)[0] for n in vc.ALL_FORMATS)
    assert ids == list(range(28))                                               # every mx_pixfmt, 0 .. PIXFMT_YUVA420P
    assert sorted(getattr(video, n) for n in vc.DEEP_NAMES) == sorted(video.DEEP)


@pytest.mark.parametrize("matrix", vc.MATRICES, ids=[f"m{k}" for k in range(len(vc.MATRICES))])
@pytest.mark.parametrize("size", vc.RGBA_SIZES)
def test_oracle_yuv_to_rgba_equals_the_model(size, matrix):
    w, h = size
    for pattern, planes in vc.rgba_inputs(w, h):
        assert np.array_equal(vm.yuv420_to_rgba(*planes, matrix), ov.to_rgba(host_frame(planes, w, h), matrix)), pattern


# ---- (b) the model against the ideal ----
def plane_jobs(name):
    """(source plane size, destination plane size) of the planes of a geometry"""
    (iw, ih), (ow, oh), layout = ALL_GEOMETRIES[name]
    sw, sh, _lx, _ly = ov.scaler_geometry(iw, ih, ow, oh)
    cw, ch = vc.SUBSAMPLING[layout]
    return [((iw, ih), (sw, sh)), ((iw >> cw, ih >> ch), (sw >> 1, sh >> 1))]


@pytest.mark.parametrize("name", list(ALL_GEOMETRIES))
def test_model_is_within_the_derived_bound_of_the_f64_cubic(name):
    for (w, h), (dw, dh) in plane_jobs(name):
        bound = vm.ideal_bound(w, dw, h, dh)
        assert bound.shape == (dh, dw) and bound.min() > 0.5
        worst, off = 0.0, 0.0
        for pattern in vc.PATTERNS:
            p = vc.plane(h, w, pattern, seed=3)
            got = vm.scale_plane(p, dw, dh).astype(np.float64)
            ideal = np.clip(vm.ideal_scale_plane(p, dw, dh), 0, 255)
            dist = np.abs(got - ideal)
            assert (dist <= bound).all(), f"{name} {w}x{h}->{dw}x{dh} {pattern}: {dist.max()} at {np.unravel_index(dist.argmax(), dist.shape)}, bound {bound.flat[dist.argmax()]}"
            assert np.abs(got - np.floor(ideal + 0.5)).max() <= 1
            worst = max(worst, dist.max())
            if pattern == "noise":
                off = (got != np.floor(ideal + 0.5)).mean()
            if (w, h) == (dw, dh):
                assert np.array_equal(got, p), "1:1 is the input"
        print(f"{name} {w}x{h}->{dw}x{dh}: max |model - ideal| {worst:.4f} (bound {bound.min():.4f} .. {bound.max():.4f}), noise: {100 * off:.2f} % of bytes != floor(ideal + 1/2)")


def test_same_size_picture_is_the_input():
    planes = vc.yuv_planes(64, 36, "planar420", "noise", seed=1)
    assert_planes_equal(vm.scale_frame(planes, "planar", 64, 36, (64, 36, 0, 0)), planes, "1:1")


def test_model_rgba_is_within_the_derived_bound_of_bt709_in_f64():
    bound = vm.ideal_rgba_bound()
    assert bound.shape == (3,) and (bound < 1.0).all()
    worst = np.zeros(3)
    yy, uu = np.mgrid[0:256, 0:256]
    cases = [p for _n, p in vc.rgba_inputs(130, 70)]
    for vv in (0, 1, 16, 127, 128, 129, 240, 255):                              # every (Y, U) pair at a few V, then every (Y, V) pair at a few U
        cases.append([np.repeat(np.repeat(yy, 2, 0), 2, 1), uu, np.full_like(uu, vv)])
        cases.append([np.repeat(np.repeat(yy, 2, 0), 2, 1), np.full_like(uu, vv), uu])
    for y, u, v in cases:
        dist = np.abs(vm.yuv420_to_rgba(y, u, v)[..., :3].astype(np.float64) - np.clip(vm.ideal_rgba(y, u, v), 0, 255)).max(axis=(0, 1))
        assert (dist <= bound).all(), (dist, bound)
        worst = np.maximum(worst, dist)
    print("max |model - ideal| R G B", worst, "bound", bound)


# ---- (c) the inputs can fail ----
def scale_cases():
    """every (geometry, input) pair test_gpu_video_model.py sends through video.scale: -> (label, model planes, model fmt, alpha, out size, geometry)"""
    for name, ((iw, ih), (ow, oh), layout) in ALL_GEOMETRIES.items():
        geo = ov.scaler_geometry(iw, ih, ow, oh)
        for pattern in vc.PATTERNS:
            yield f"{name} {pattern}", vc.yuv_planes(iw, ih, layout, pattern, seed=3), "planar", None, (ow, oh), geo
    for geom, ((iw, ih), (ow, oh)) in vc.FORMAT_GEOMETRIES.items():
        geo = ov.scaler_geometry(iw, ih, ow, oh)
        for name in vc.ALL_FORMATS:
            _fmt, kind, detail = vc.format_entry(name, video)
            for pattern in ("noise", "checker-1", "full"):
                inp = vc.make_input(kind, detail, iw, ih, pattern, seed=5)
                yield f"{name} {geom} {pattern}", *inp["model"], inp["alpha"], (ow, oh), geo


def test_the_pictures_reach_every_branch_of_the_integer_arithmetic():
    seen = {"negative t": False, "t above 255 * 128": False, "V result below 0 before the clip": False, "V result above 255 before the clip": False}
    for name in ALL_GEOMETRIES:
        for (w, h), (dw, dh) in plane_jobs(name):
            for pattern in vc.PATTERNS:
                _d, t, pre = vm.scale_plane(vc.plane(h, w, pattern, seed=3), dw, dh, intermediates=True)
                seen["negative t"] |= bool((t < 0).any())
                seen["t above 255 * 128"] |= bool((t > 255 * 128).any())
                seen["V result below 0 before the clip"] |= bool((pre < 0).any())
                seen["V result above 255 before the clip"] |= bool((pre > 255).any())
    assert all(seen.values()), seen


def _trunc_shift(x, n):
    x = np.asarray(x, np.int64)
    return np.sign(x) * (np.abs(x) >> n)


def _zero_pad(axis, low):
    def gather(p, idx, ax):
        out = np.take(p, np.clip(idx, 0, p.shape[ax] - 1), axis=ax)
        if ax != axis:
            return out
        outside = (idx < 0) if low else (idx > p.shape[ax] - 1)
        return np.where(outside if ax == 1 else outside[:, :, None], 0, out)
    return gather


def _tables_from(taps_fn):
    def tap_tables(src, dst):
        t = [taps_fn(o, src, dst) for o in range(dst)]
        return np.array([f for f, _c in t], np.int64), np.array([c for _f, c in t], np.int64)
    return tap_tables


def _residual_to_the_other_middle_tap(o, src, dst):
    first, c = vm.taps(o, src, dst)
    if src > dst:
        return first, c
    d = (floor(Fraction((2 * o + 1) * src * 65536, 2 * dst)) - 32768) % 65536
    q14 = vm._taps_mod.q14
    c = [q14(65536 + d), q14(d), q14(65536 - d), q14(131072 - d)]
    c[1 if c[2] > c[1] else 2] += 16384 - sum(c)
    return first, c


def _widened_first_tap_one_later(o, src, dst):
    first, c = vm.taps(o, src, dst)
    return (first + 1 if src > dst else first), c


# name -> (attribute of video_model, its replacement, "scale" or "rgba": which outputs must notice)
MIS_MODELS = {
    "H rounding 64 dropped": ("H_ROUND", 0, "scale"),
    "V rounding 2^20 dropped": ("V_ROUND", 0, "scale"),
    "truncation toward zero for the arithmetic shift": ("asr", _trunc_shift, "scale"),
    "zero padding at the left edge": ("gather", _zero_pad(1, True), "scale"),
    "zero padding at the right edge": ("gather", _zero_pad(1, False), "scale"),
    "zero padding at the top edge": ("gather", _zero_pad(0, True), "scale"),
    "zero padding at the bottom edge": ("gather", _zero_pad(0, False), "scale"),
    "residual given to the other middle tap": ("tap_tables", _tables_from(_residual_to_the_other_middle_tap), "scale"),
    "first tap of the widened kernel one later": ("tap_tables", _tables_from(_widened_first_tap_one_later), "scale"),
    "chroma resampled from the luma size": ("source_size", lambda k, planes: planes[0].shape, "scale"),
    "the other co-sited chroma sample in YUV -> RGBA": ("chroma_index", lambda n: np.minimum((np.arange(n) + 1) >> 1, (n >> 1) - 1), "rgba"),
    "matrix rounding 2048 dropped": ("M_ROUND", 0, "rgba"),
}


@pytest.fixture(scope="module")
def true_pictures():
    scale = [(label, vm.scale_frame(planes, fmt, *out, geo, alpha=alpha)) for label, planes, fmt, alpha, out, geo in scale_cases()]
    rgba = [vm.yuv420_to_rgba(*planes, m) for w, h in vc.RGBA_SIZES for _p, planes in vc.rgba_inputs(w, h) for m in vc.MATRICES]
    return scale, rgba


@pytest.mark.parametrize("mis", list(MIS_MODELS))
def test_each_deliberate_mis_model_changes_a_byte_of_some_case(mis, true_pictures, monkeypatch):
    attr, replacement, which = MIS_MODELS[mis]
    scale, rgba = true_pictures
    monkeypatch.setattr(vm, attr, replacement)
    if which == "scale":
        for (label, want), (_l, planes, fmt, alpha, out, geo) in zip(scale, scale_cases()):
            got = vm.scale_frame(planes, fmt, *out, geo, alpha=alpha)
            if any(not np.array_equal(g, w) for g, w in zip(got, want)):
                print(f"{mis}: first caught by {label}")
                return
    else:
        k = 0
        for w, h in vc.RGBA_SIZES:
            for pattern, planes in vc.rgba_inputs(w, h):
                for m in vc.MATRICES:
                    if not np.array_equal(vm.yuv420_to_rgba(*planes, m), rgba[k]):
                        print(f"{mis}: first caught by {w}x{h} {pattern} matrix {m}")
                        return
                    k += 1
    pytest.fail(f"no case notices the mis-model: {mis}")
