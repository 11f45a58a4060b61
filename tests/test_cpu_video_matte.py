"""The matte refiner without a device (include/mixlab_gpu.h mx_video_matte): the header's struct and the exported entry points, the
properties of the numpy model the GPU suite compares the kernel with (tests/video_matte_model.py), the two host-side helpers, and that the shared pictures can
tell the model from each of a list of plausible mistakes."""
import ctypes as C
import math
import pathlib
import re
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import video_matte_model as mm
from video_matte_model import CIRCLE, MatteP, matte_plane

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

OFFSETS = [("flags", 0), ("clean_black", 4), ("clean_white", 5), ("choke", 6), ("soften", 7), ("mask_shape", 8), ("mask_invert", 12), ("mask_x0", 16),
           ("mask_y0", 20), ("mask_x1", 24), ("mask_y1", 28), ("mask_feather_q4", 32)]
ENTRY_POINTS = {"mx_video_matte", "mx_video_matte_check", "mx_video_matte_wipe", "mx_graph_set_video_source_matte"}


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    h = gen.Header(gen.HEADER.read_text())
    lay = h.layout_json()["mx_video_matte_params"]
    assert lay["size"] == 36 and lay["offsets"] == dict(OFFSETS)
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert [consts[n] for n in ("MX_MATTE_CLEAN", "MX_MATTE_CHOKE", "MX_MATTE_SOFTEN", "MX_MATTE_MASK", "MX_MATTE_MASK_RECT", "MX_MATTE_MASK_CIRCLE")] == [1, 2, 4, 8, 0, 1]
    assert [consts[n] for n in ("MX_WIPE_LEFT", "MX_WIPE_TOP", "MX_WIPE_BOX", "MX_WIPE_IRIS")] == [0, 1, 2, 3]
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # not a module kind, not a profile kind, no new ABI version
    declared = {f[0]: f for f in h.funcs}
    assert [c for _n, c, _a in declared["mx_video_matte"][2]] == ["const mx_dframe*", "const mx_video_matte_params*", "mx_dframe**", "void*"]
    assert [c for _n, c, _a in declared["mx_video_matte_check"][2]] == ["const mx_video_matte_params*"]
    assert [c for _n, c, _a in declared["mx_video_matte_wipe"][2]] == ["uint32_t"] * 5 + ["mx_video_matte_params*"]
    assert [c for _n, c, _a in declared["mx_graph_set_video_source_matte"][2]] == ["mx_graph*", "uint32_t", "const mx_video_matte_params*"]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    exported = {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}
    assert ENTRY_POINTS <= exported


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi
    assert C.sizeof(abi.VideoMatteParams) == 36
    assert [(n, getattr(abi.VideoMatteParams, n).offset) for n, _t in abi.VideoMatteParams._fields_] == OFFSETS
    assert abi.lib.mx_abi_version() == 4


# ---- the model's properties ----
def planes():
    return {"keyed": mm.keyed_picture(66, 38, 1)[3], "speck": mm.speck_plane(66, 38), "speck-tall": mm.speck_plane(18, 50, seed=2)}


@pytest.mark.parametrize("value", [0, 1, 127, 254, 255])
def test_a_constant_plane_passes_choke_and_soften_unchanged(value):
    """the minimum and the maximum of equal samples is the sample, and sum b b v = 4^(2s) v: (v 2^4s + 2^(4s-1)) >> 4s = v"""
    a = np.full((10, 14), value, np.uint8)
    for p in (MatteP(choke=1), MatteP(choke=-6), MatteP(soften=1), MatteP(soften=6), MatteP(choke=6, soften=6), MatteP(clean=(0, 255), choke=-3, soften=4)):
        assert (matte_plane(a, p) == value).all(), p


def test_clean_0_255_is_the_identity_and_black_equal_white_is_a_hard_clip():
    a = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(matte_plane(a, MatteP(clean=(0, 255))), a)      # ((a - 0) 255) / 255 = a between the ends, 0 and 255 at them
    hard = matte_plane(a, MatteP(clean=(128, 128)))
    assert np.array_equal(hard, np.where(a <= 128, 0, 255))               # a <= black is tested first
    soft = matte_plane(a, MatteP(clean=(40, 200))).astype(int)
    assert soft[2, 8] == 0 and soft[12, 8] == 255 and soft[7, 8] == ((120 - 40) * 255) // 160 and (np.diff(soft.ravel()) >= 0).all()


@pytest.mark.parametrize("r", [1, 2, 6])
def test_choke_duality_and_composition(r):
    """max over a window = 255 - min over it of 255 - a; a square of radius r is r squares of radius 1 (Minkowski sum), and the clamp commutes with it because a
    clamped index never leaves the plane"""
    for name, a in planes().items():
        assert np.array_equal(matte_plane(a, MatteP(choke=-r)), 255 - matte_plane(255 - a, MatteP(choke=r))), name
        for sign in (1, -1):
            step = a
            for _ in range(r):
                step = matte_plane(step, MatteP(choke=sign))
            assert np.array_equal(matte_plane(a, MatteP(choke=sign * r)), step), (name, sign)
    a = planes()["speck"]
    assert (matte_plane(a, MatteP(choke=r)) <= a).all() and (matte_plane(a, MatteP(choke=-r)) >= a).all()


@pytest.mark.parametrize("s", [1, 2, 3, 6])
def test_soften_is_the_exact_s_fold_121_filter_rounded_once(s):
    """b_s is the s-fold convolution of [1 2 1]; with the edge clamp applied to the SOURCE index the s-fold filter is NOT s clamped passes, so the rational
    reference extends the plane by clamping, convolves s times in exact fractions on the extended plane, and rounds half up once"""
    a = mm.speck_plane(12, 10, seed=s).astype(int)
    h, w = a.shape
    ext = np.pad(a, s, mode="edge")
    cur = [[Fraction(int(x)) for x in row] for row in ext]
    for _ in range(s):                                                   # one [1 2 1]/4 (x) [1 2 1]/4 pass; each pass eats one sample of the extension per side
        hh, ww = len(cur), len(cur[0])
        rows = [[(cur[y][x - 1] + 2 * cur[y][x] + cur[y][x + 1]) / 4 for x in range(1, ww - 1)] for y in range(hh)]
        cur = [[(rows[y - 1][x] + 2 * rows[y][x] + rows[y + 1][x]) / 4 for x in range(ww - 2)] for y in range(1, hh - 1)]
    assert len(cur) == h and len(cur[0]) == w
    want = np.array([[math.floor(v + Fraction(1, 2)) for v in row] for row in cur])
    assert np.array_equal(matte_plane(a.astype(np.uint8), MatteP(soften=s)), want)
    assert sum(mm.binomial(s)) == 4 ** s and 255 * 4 ** (2 * s) + (1 << (4 * s - 1)) < 2 ** 32


def test_a_hard_integer_pixel_rectangle_covers_its_intersection_with_the_frame():
    w, h = 20, 12
    a = np.full((h, w), 255, np.uint8)
    for (x0, y0, x1, y1) in ((3, 2, 9, 7), (-4, -4, 5, 30), (15, 6, 40, 9), (0, 0, w, h), (25, 3, 30, 5)):
        got = matte_plane(a, MatteP(mask=(16 * x0, 16 * y0, 16 * x1, 16 * y1)))
        want = np.zeros((h, w), np.uint8)
        want[max(0, y0):max(0, min(h, y1)), max(0, x0):max(0, min(w, x1))] = 255
        assert np.array_equal(got, want), (x0, y0, x1, y1)


@pytest.mark.parametrize("n", [1, 3, 8])
def test_a_feather_of_16n_gives_the_stated_ramp(n):
    """inside a rectangle whose left edge is x = 0, sample k is 16k + 8 from the edge: m = ((16k + 8) 255) / (16n) for k < n, 255 from there on"""
    w, h = 4 * n + 8, 2 * (n + 2) + 40
    a = np.full((h, w), 255, np.uint8)
    got = matte_plane(a, MatteP(mask=(0, -(1 << 20), 1 << 20, 1 << 20), feather=16 * n))
    want = [min(255, ((16 * k + 8) * 255) // (16 * n)) if 16 * k + 8 < 16 * n else 255 for k in range(w)]
    assert (got == np.array(want, np.uint8)[None, :]).all()
    assert got[0, 0] == (8 * 255) // (16 * n) and got[0, n] == 255


def test_the_circle_is_the_exact_integer_root():
    """hard circles around (8, 8) -- the centre of sample (0, 0) -- so the distance of sample (x, y) is 16 hypot(x, y): at a radius R the sample is inside iff
    isqrt(256 (x^2 + y^2)) < R.  Radii AT a perfect square's root (16 * 5 for (3, 4), 16 * 13 for (5, 12), 16 * 25 for (7, 24)) and one either side."""
    w, h = 32, 32
    a = np.full((h, w), 255, np.uint8)
    for root in (5, 13, 25):
        for radius in (16 * root - 1, 16 * root, 16 * root + 1):
            got = matte_plane(a, MatteP(mask=(8, 8, radius, 0), shape=CIRCLE))
            want = np.array([[255 if radius - math.isqrt(256 * (x * x + y * y)) > 0 else 0 for x in range(w)] for y in range(h)], np.uint8)
            assert np.array_equal(got, want), radius
    # a feathered circle of the largest radius centred far to the left, its rim crossing the frame: arguments of 2^40, still math.isqrt
    B, f = 1 << 20, 200
    got = matte_plane(a, MatteP(mask=(300 - B, 8, B, 0), shape=CIRCLE, feather=f))
    ds = [[B - math.isqrt((16 * x + 8 - 300 + B) ** 2 + (16 * y) ** 2) for x in range(w)] for y in range(h)]
    want = np.array([[0 if d <= 0 else (255 if d >= f else d * 255 // f) for d in row] for row in ds], np.uint8)
    assert np.array_equal(got, want) and 0 < want[0, 10] < 255 and want[0, 0] == 255 and want[0, 31] == 0
    xs = np.array([0, 1, 2, 3, 4, 15, 16, 17, (1 << 43) - 1, (1 << 42) + 12345, 94906265 ** 2 - 1, 94906265 ** 2], np.int64)
    assert mm.isqrt(xs).tolist() == [math.isqrt(int(x)) for x in xs]


def test_mask_coordinates_at_the_limits_do_not_overflow():
    B = 1 << 20
    a = mm.speck_plane(34, 18)
    assert np.array_equal(matte_plane(a, MatteP(mask=(-B, -B, B, B), feather=65535)), a)                      # d >= 2^20 - 16 w > feather everywhere
    assert not matte_plane(a, MatteP(mask=(B, B, B, B))).any()
    assert np.array_equal(matte_plane(a, MatteP(mask=(B, B, B, B), invert=1)), a)
    assert not matte_plane(a, MatteP(mask=(B, -B, 0, 0), shape=CIRCLE)).any()                                  # radius 0
    assert not matte_plane(a, MatteP(mask=(-B, B, B, 0), shape=CIRCLE)).any()                                  # the centre is about 2^20 sqrt 2 away: outside
    assert np.array_equal(matte_plane(a, MatteP(mask=(-B, B, B, 0), shape=CIRCLE, invert=1, feather=1)), a)


def test_no_stage_is_a_copy_and_an_opaque_plane_without_coverage():
    y, u, v, k = mm.keyed_picture(34, 18)
    yo, uo, vo, a = mm.matte_model(y, u, v, MatteP())
    assert np.array_equal(yo, y) and np.array_equal(uo, u) and np.array_equal(vo, v) and (a == 255).all()
    assert np.array_equal(mm.matte_model(y, u, v, MatteP(), a_in=k)[3], k)
    assert (mm.matte_model(y, u, v, MatteP(choke=3, soften=2))[3] == 255).all()   # without coverage CHOKE and SOFTEN see the constant 255


# ---- the host-side helpers ----
def dev_params(p: MatteP):
    from mixlab_amd import video
    return video.MatteParams(clean=p.clean, choke=p.choke, soften=p.soften, mask=p.mask, invert=bool(p.invert), feather_q4=p.feather, shape=p.shape)


def model_params(c) -> MatteP:
    assert c.flags == mm.MASK
    return MatteP(mask=(c.mask_x0, c.mask_y0, c.mask_x1, c.mask_y1), shape=c.mask_shape, invert=c.mask_invert, feather=c.mask_feather_q4)


WIPE_SIZES = [(34, 18), (130, 74), (1920, 1080)]


@pytest.mark.parametrize("size", WIPE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", [mm.WIPE_LEFT, mm.WIPE_TOP, mm.WIPE_BOX, mm.WIPE_IRIS], ids=["left", "top", "box", "iris"])
def test_wipe_helper_against_the_model(kind, size):
    from mixlab_amd import video
    w, h = size
    for f in (0, 37, 16 * 40, 65535):
        for pos in (0, 1, 777, 32768, 50001, 65535, 65536):
            c = video.matte_wipe(kind, pos, f, w, h)
            video.matte_check(c)
            assert model_params(c) == mm.wipe(kind, pos, f, w, h), (f, pos)
    sw, sh = (w, h) if w <= 130 else (240, 136)                    # the planes of the sweep (the formulas above were checked at full size)
    a = mm.speck_plane(sw, sh) | 1                                       # no sample 0: a covered sample shows
    for f in (0, 16 * 5 + 3):
        assert not matte_plane(a, model_params(video.matte_wipe(kind, 0, f, sw, sh))).any(), "pos 0 covers nothing"
        assert np.array_equal(matte_plane(a, model_params(video.matte_wipe(kind, 65536, f, sw, sh))), a), "pos 65536 gives the plane back"
        full = np.full((sh, sw), 255, np.uint8)
        prev = np.zeros((sh, sw), np.uint8)
        for pos in range(0, 65537, 2048):
            cur = matte_plane(full, model_params(video.matte_wipe(kind, pos, f, sw, sh)))
            assert (cur >= prev).all(), f"coverage fell between pos {pos - 2048} and {pos}"
            prev = cur
        assert (prev == 255).all()


def test_wipe_helper_refuses_what_the_header_excludes():
    from mixlab_amd import abi, video
    for args in ((4, 0, 0, 64, 36), (0, 65537, 0, 64, 36), (0, 0, 65536, 64, 36), (0, 0, 0, 0, 36), (0, 0, 0, 63, 36), (0, 0, 0, 64, 16386)):
        with pytest.raises(abi.MxError) as e:
            video.matte_wipe(*args)
        assert e.value.code == abi.MX_ERR_INVALID, args


GOOD = {"edges": MatteP(clean=(0, 255), choke=-6, soften=6, mask=(-(1 << 20), -(1 << 20), 1 << 20, 1 << 20), feather=65535, invert=1),
        "point-rect": MatteP(mask=(5, 5, 5, 5)), "radius-0": MatteP(mask=(1 << 20, -(1 << 20), 0, 0), shape=CIRCLE), "black-is-white": MatteP(clean=(255, 255))}


def test_check_accepts_every_named_good_setting():
    from mixlab_amd import video
    for size in ((2, 2), (322, 182)):
        for name, p in {**mm.settings(*size), **GOOD}.items():
            c = dev_params(p)
            assert c.flags == p.flags, name
            video.matte_check(c)


RECT_OK = dict(flags=mm.MASK, mask_x0=16, mask_y0=16, mask_x1=160, mask_y1=160)
CIRC_OK = dict(flags=mm.MASK, mask_shape=CIRCLE, mask_x0=16, mask_y0=16, mask_x1=160)
REFUSED = {
    "stray flag bit": dict(flags=16),
    "stray high flag bit": dict(flags=mm.CLEAN | 0x80000000, clean_white=255),
    "black above white": dict(flags=mm.CLEAN, clean_black=200, clean_white=199),
    "choke 0 with the bit": dict(flags=mm.CHOKE),
    "choke 7": dict(flags=mm.CHOKE, choke=7),
    "choke -7": dict(flags=mm.CHOKE, choke=-7),
    "soften 0 with the bit": dict(flags=mm.SOFTEN),
    "soften 7": dict(flags=mm.SOFTEN, soften=7),
    "clean field without the bit": dict(flags=0, clean_white=255),
    "choke without the bit": dict(flags=mm.SOFTEN, soften=1, choke=1),
    "soften without the bit": dict(flags=mm.CHOKE, choke=1, soften=1),
    "feather without the bit": dict(flags=0, mask_feather_q4=1),
    "invert without the bit": dict(flags=mm.CLEAN, clean_white=255, mask_invert=1),
    "mask coordinate without the bit": dict(flags=0, mask_y1=1),
    "shape without the bit": dict(flags=0, mask_shape=1),
    "x0 above x1": dict(RECT_OK, mask_x0=161),
    "y0 above y1": dict(RECT_OK, mask_y0=161),
    "negative radius": dict(CIRC_OK, mask_x1=-1),
    "circle with y1": dict(CIRC_OK, mask_y1=1),
    "shape 2": dict(RECT_OK, mask_shape=2),
    "invert 2": dict(RECT_OK, mask_invert=2),
    "feather 65536": dict(RECT_OK, mask_feather_q4=65536),
    "coordinate beyond 2^20": dict(RECT_OK, mask_x1=(1 << 20) + 1),
    "coordinate below -2^20": dict(RECT_OK, mask_y0=-(1 << 20) - 1),
    "centre beyond 2^20": dict(CIRC_OK, mask_x0=(1 << 20) + 1),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_check_refuses(name):
    from mixlab_amd import abi
    c = abi.VideoMatteParams()
    for k, val in REFUSED[name].items():
        setattr(c, k, val)
    assert abi.lib.mx_video_matte_check(C.byref(c)) == abi.MX_ERR_INVALID, name
    assert b"mx_video_matte" in (abi.lib.mx_last_error() or b"")
    assert abi.lib.mx_video_matte_check(None) == abi.MX_ERR_INVALID


# ---- the pictures can tell ----
def test_the_shared_planes_hold_what_they_are_for():
    a = mm.speck_plane(66, 38).astype(int)
    inner = a[5:-5, 5:-5]
    lone0 = lone255 = 0
    for y in range(1, inner.shape[0] - 1):
        for x in range(1, inner.shape[1] - 1):
            around = inner[y - 1:y + 2, x - 1:x + 2].sum() - inner[y, x]
            lone0 += inner[y, x] == 0 and around == 8 * 255
            lone255 += inner[y, x] == 255 and around == 0
    assert lone0 >= 2 and lone255 >= 2                                    # isolated specks of both kinds
    assert a[0, 0] == 0 and a[-1, -1] == 255 and 0 < a[0, -1] < 255 and 0 < a[-1, 0] < 255   # the ramp reaches every corner
    assert len(np.unique(a[0, :])) > 8 and len(np.unique(a[:, 0])) > 8 and len(np.unique(a[-1, :])) > 8 and len(np.unique(a[:, -1])) > 8
    k = mm.keyed_picture(66, 38)[3]
    n = k.size
    assert (k == 0).sum() >= n // 100 and (k == 255).sum() >= n // 100 and ((k > 0) & (k < 255)).sum() >= n // 100


W0, H0 = 66, 38
SET = mm.settings(W0, H0)
MISTAKES = [   # (mis-model, plane, setting)
    ("edge_zero", "speck", MatteP(choke=2)),                             # a maximum ignores a 0; the minimum does not, and the binomial never does
    ("edge_zero", "keyed", MatteP(soften=2)),
    ("edge_wrap", "speck", MatteP(choke=2)),
    ("edge_wrap", "speck", MatteP(soften=3)),
    ("choke_sign", "speck", MatteP(choke=1)),
    ("choke_sign", "keyed", SET["all-circle"]),
    ("choke_cross", "speck", MatteP(choke=1)),
    ("choke_cross", "keyed", MatteP(choke=-2)),
    ("soften_round_first", "keyed", MatteP(soften=1)),
    ("soften_round_first", "speck", MatteP(soften=6)),
    ("soften_no_round", "keyed", MatteP(soften=2)),
    ("soften_box", "speck", MatteP(soften=1)),
    ("soften_before_choke", "speck", MatteP(choke=1, soften=1)),
    ("soften_before_choke", "keyed", SET["all-circle"]),
    ("clean_last", "keyed", SET["clean-choke2-soften2"]),
    ("clean_last", "speck", MatteP(clean=(100, 110), soften=2)),
    ("clean_round", "keyed", SET["clean"]),
    ("mask_round", "keyed", SET["rect-feather-invert"]),
    ("centre_0", "speck", SET["rect-hard"]),
    ("centre_0", "keyed", SET["circle-feather"]),
    ("sqrt_round", "speck", SET["circle-feather"]),
    ("sqrt_round", "keyed", SET["circle-centred-off-frame"]),
    # a hard edge THROUGH sample centres: d == 0 there, which is outside by the stated order of the tests
    ("feather_order", "speck", MatteP(mask=(16 * 5 + 8, 16 * 3 + 8, 16 * 40 + 8, 16 * 30 + 8))),
    ("feather_order", "keyed", MatteP(mask=(16 * 20 + 8, 16 * 10 + 8, 16 * 5, 0), shape=CIRCLE)),   # (3, 4, 5): samples at distance 80 exactly
    ("invert_after", "keyed", SET["rect-feather-invert"]),
    ("invert_after", "speck", SET["circle-hard-invert"]),
]


@pytest.mark.parametrize("bug,plane,p", MISTAKES, ids=[f"{m[0]}-{m[1]}-{i}" for i, m in enumerate(MISTAKES)])
def test_each_mis_model_differs_from_the_model_on_the_shared_pictures(bug, plane, p):
    assert bug in mm.BUGS
    a = {"keyed": mm.keyed_picture(W0, H0)[3], "speck": mm.speck_plane(W0, H0)}[plane]
    assert not np.array_equal(matte_plane(a, p), matte_plane(a, p, bug=bug)), f"the pictures cannot tell the model from '{bug}'"


def test_every_listed_mistake_is_tried():
    assert {m[0] for m in MISTAKES} == set(mm.BUGS) and len(mm.BUGS) >= 12
