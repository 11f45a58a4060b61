"""The colour corrector without a device (include/mixlab_gpu.h mx_video_grade): the header's struct, constants and exported entry points,
the host-only calls (mx_video_grade_procamp, mx_video_lut_identity, the checks of mx_video_lut_create), the properties of the numpy model the GPU suite compares the
kernel with (tests/video_grade_model.py), and that the shared pictures meet every case of the specification and can tell the model from a list of misreadings."""
import ctypes as C
import math
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import video_grade_model as gm
from video_grade_model import CHROMA, CURVE, LUT, GradeP, grade_model

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

SYMBOLS = {"mx_video_lut_create", "mx_video_lut_retain", "mx_video_lut_release", "mx_video_lut_identity", "mx_video_grade_procamp", "mx_video_grade",
           "mx_graph_set_video_source_grade"}


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()["mx_video_grade_params"]
    assert lay["size"] == 284
    assert lay["offsets"] == {"flags": 0, "curve_y": 4, "m_uu": 260, "m_uv": 264, "m_vu": 268, "m_vv": 272, "off_u": 276, "off_v": 280}
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert (consts["MX_GRADE_CURVE"], consts["MX_GRADE_CHROMA"], consts["MX_GRADE_LUT"]) == (1, 2, 4)
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19          # not a new module kind, no new ABI version
    assert re.search(r"#define\s+MX_PROFILE_KINDS\s+18\b", text)                    # and no new profile kind
    declared = {f[0]: f for f in h.funcs}
    assert SYMBOLS <= set(declared)
    assert [c for _n, c, _a in declared["mx_video_grade"][2]] == ["const mx_dframe*", "const mx_video_grade_params*", "const mx_video_lut*", "mx_dframe**", "void*"]
    assert [c for _n, c, _a in declared["mx_graph_set_video_source_grade"][2]] == ["mx_graph*", "uint32_t", "const mx_video_grade_params*", "mx_video_lut*"]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    exported = {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}
    assert SYMBOLS <= exported


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi
    assert C.sizeof(abi.VideoGradeParams) == 284
    assert [(n, getattr(abi.VideoGradeParams, n).offset) for n, _t in abi.VideoGradeParams._fields_] == \
        [("flags", 0), ("curve_y", 4), ("m_uu", 260), ("m_uv", 264), ("m_vu", 268), ("m_vv", 272), ("off_u", 276), ("off_v", 280)]
    assert (abi.GRADE_CURVE, abi.GRADE_CHROMA, abi.GRADE_LUT) == (CURVE, CHROMA, LUT)
    assert abi.lib.mx_abi_version() == 4


# ---- the lattice: model only ----
@pytest.mark.parametrize("k", [4, 5])
def test_identity_lattice_returns_its_input_for_every_triple(k):
    nodes = gm.identity_lattice(k)
    assert nodes.max() == 4096 and nodes.shape == ((1 << k) + 1,) * 3 + (3,)
    b, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for a in range(256):
        out = gm.lut_eval(nodes, k, np.full_like(b, a), b, c)
        assert np.array_equal(out[..., 0], np.full_like(b, a)) and np.array_equal(out[..., 1], b) and np.array_equal(out[..., 2], c), f"a = {a}"


@pytest.mark.parametrize("k", [4, 5])
def test_equal_fractions_do_not_depend_on_the_axis_order_chosen(k):
    """every triple of fractions with a tie, in cell 0, in a middle cell and in the top cell, on a random lattice: whichever tied axis is walked first, the vertex the two
    walks disagree on has weight 0"""
    S = 1 << (8 - k)
    f = np.array([(x, y, z) for x in range(S) for y in range(S) for z in range(S) if x == y or y == z or x == z])
    nodes = gm.random_lattice(k, 5)
    for cell in (0, 7, (1 << k) - 1):
        a, b, c = (cell * S + f[:, i] for i in range(3))
        first, last = gm.lut_eval(nodes, k, a, b, c, tie="first"), gm.lut_eval(nodes, k, a, b, c, tie="last")
        assert np.array_equal(first, last)
    g = np.array([(x, y, z) for x in range(S) for y in range(S) for z in range(S) if len({x, y, z}) == 3])   # and the tie rule is all the switch changes
    assert np.array_equal(gm.lut_eval(nodes, k, g[:, 0], g[:, 1], g[:, 2], tie="first"), gm.lut_eval(nodes, k, g[:, 0], g[:, 1], g[:, 2], tie="last"))


@pytest.mark.parametrize("k", [4, 5])
def test_a_lattice_sampled_from_an_affine_map_reproduces_it(k):
    """Nodes n = rint(16 g(p)) of an affine g whose values stay inside 0 .. 255.  Inside a tetrahedron the interpolation is the convex combination sum (w_i / S) n_i
    with sum w_i = S, which reproduces an affine map exactly from exact nodes; each node is off by at most 1/2 (Q4 rounding), so acc / S lies within 1/2 of 16 g(x),
    i.e. acc / (16 S) within 1/32 of g(x).  The result floor((acc + 8 S) / (16 S)) = floor(acc / (16 S) + 1/2) is the nearest integer to acc / (16 S), ties up: within
    1/2 of it.  Together |out - g(x)| <= 1/2 + 1/32 = 17/32, and the min(255, .) never bites because g <= 255."""
    A = np.array([[0.55, 0.20, -0.10], [-0.15, 0.70, 0.12], [0.08, -0.22, 0.61]])
    t = np.array([30.0, 40.25, 70.5])
    n, S = (1 << k) + 1, 1 << (8 - k)
    grid = np.arange(n) * S
    P = np.stack(np.meshgrid(grid, grid, grid, indexing="ij"), axis=-1).astype(np.float64)
    G = P @ A.T + t
    assert G.min() >= 0.0 and G.max() <= 255.0
    nodes = np.rint(16.0 * G).astype(np.uint16)
    rng = np.random.default_rng(4)
    x = rng.integers(0, 256, size=(200000, 3))
    x[:3] = [[0, 0, 0], [255, 255, 255], [255, 0, 255]]
    out = gm.lut_eval(nodes, k, x[:, 0], x[:, 1], x[:, 2])
    err = np.abs(out - (x @ A.T + t))
    print(f"affine lattice, k = {k}: largest error {err.max():.4f} (bound {17 / 32})")
    assert err.max() <= 17.0 / 32.0


# ---- the pictures meet every case ----
def _lut_inputs(k):
    pts = [gm.lut_inputs(*gm.every_uv_picture(s), gm.shared_params(k)) for s in gm.LUMA_SHIFTS]
    return np.concatenate(pts, axis=1)


@pytest.mark.parametrize("k", [4, 5])
def test_shared_pictures_cover_the_lut_stage(k):
    S = 1 << (8 - k)
    v = _lut_inputs(k)
    f, cell = v & (S - 1), v >> (8 - k)
    fa, fb, fc = f
    strict = {"a>b>c": (fa > fb) & (fb > fc), "a>c>b": (fa > fc) & (fc > fb), "b>a>c": (fb > fa) & (fa > fc),
              "b>c>a": (fb > fc) & (fc > fa), "c>a>b": (fc > fa) & (fa > fb), "c>b>a": (fc > fb) & (fb > fa)}
    ties = {"a=b>c": (fa == fb) & (fb > fc), "a=b<c": (fa == fb) & (fb < fc), "a=c>b": (fa == fc) & (fc > fb), "a=c<b": (fa == fc) & (fc < fb),
            "b=c>a": (fb == fc) & (fc > fa), "b=c<a": (fb == fc) & (fc < fa), "a=b=c": (fa == fb) & (fb == fc)}
    for name, m in {**strict, **ties}.items():
        assert m.any(), f"no LUT input with fractions {name}"
    for ax in range(3):
        assert (v[ax] == 255).any(), f"axis {ax} never holds 255 (the top cell's last fraction)"
        assert (cell[ax] == (1 << k) - 1).any() and (cell[ax] == 0).any(), f"axis {ax} misses the top cell or cell 0"
    assert ((cell == 0).all(axis=0)).any() and ((cell == (1 << k) - 1).all(axis=0)).any()   # the cube's two end cells themselves


def test_shared_pictures_cover_the_chroma_stage():
    y, u, v = gm.every_uv_picture(0)
    _y1, u1, v1, _ym, raw = gm.stages(y, u, v, gm.shared_params(4))
    su, sv, qu, qv = raw
    for pre, q, out in ((su, qu, u1), (sv, qv, v1)):
        assert (pre < 0).any() and ((pre < 0) & (pre % 4096 != 0)).any()      # a negative pre-shift sum that is no multiple of 4096: floor and truncation differ
        assert (q < 0).any() and (q > 255).any()                                # both clip ends
        assert out.min() == 0 and out.max() == 255
    assert np.abs(su).max() < 2 ** 31 and np.abs(sv).max() < 2 ** 31
    worst = 2 * 32767 * 128 + 255 * 4096 + 2048                                 # the header's "every sum fits an int32"
    assert worst < 2 ** 31


def test_the_luma_pictures_hold_every_code_value_in_every_block_position():
    """37 x + 101 y is even on a block's (0, 0) and (1, 1) samples and odd on the other two: one picture gives each position half the code values, an odd shift the rest"""
    ys = [gm.every_uv_picture(s)[0] for s in gm.LUMA_SHIFTS]
    assert any(s % 2 for s in gm.LUMA_SHIFTS) and not all(s % 2 for s in gm.LUMA_SHIFTS)
    for dy in (0, 1):
        for dx in (0, 1):
            assert len(np.unique(np.concatenate([y[dy::2, dx::2].ravel() for y in ys]))) == 256


# ---- the pictures can tell ----
def _case(variant):
    """(pictures, parameters) on which the misreading must show"""
    if variant == "chroma_trunc_div":
        return [gm.every_uv_picture(0)], gm.shared_params(4, flags=CHROMA)
    if variant == "clamp_4095":
        return [gm.every_uv_picture(s) for s in gm.LUMA_SHIFTS], gm.shared_params(4)
    return [gm.every_uv_picture(0)], gm.shared_params(4)


@pytest.mark.parametrize("variant", gm.VARIANTS)
def test_each_misreading_differs_from_the_model_on_the_shared_pictures(variant):
    pics, p = _case(variant)
    differs = False
    for y, u, v in pics:
        good, bad = grade_model(y, u, v, p), grade_model(y, u, v, p, variant=variant)
        differs = differs or any(not np.array_equal(g, b) for g, b in zip(good, bad))
    assert differs, f"the pictures cannot tell the model from '{variant}'"


@pytest.mark.parametrize("variant", ["trilinear", "ascending", "axes_permuted", "no_lut_rounding", "clamp_4095"])
def test_lut_misreadings_show_on_the_33_lattice_and_the_smooth_lattice_too(variant):
    y, u, v = gm.every_uv_picture(3)
    for p in (gm.shared_params(5), gm.shared_params(4, lattice="smooth")):
        if variant == "clamp_4095" and p.k == 4:
            assert (p.nodes == 4096).any()
            continue                                   # the smooth lattice meets 4096 only where every neighbour does: 4095 rounds to the same byte
        good, bad = grade_model(y, u, v, p), grade_model(y, u, v, p, variant=variant)
        assert any(not np.array_equal(g, b) for g, b in zip(good, bad)), f"k = {p.k}: '{variant}' does not show"


def test_there_are_at_least_ten_misreadings():
    assert len(set(gm.VARIANTS)) >= 10


def test_no_flags_is_a_copy_and_each_stage_alone_does_what_the_header_says():
    y, u, v = gm.noise_picture(66, 38, 1)
    p = gm.shared_params(4)
    yo, uo, vo = grade_model(y, u, v, p.but(flags=0))
    assert np.array_equal(yo, y) and np.array_equal(uo, u) and np.array_equal(vo, v)
    yo, uo, vo = grade_model(y, u, v, p.but(flags=CURVE))
    assert np.array_equal(yo, p.curve[y]) and np.array_equal(uo, u) and np.array_equal(vo, v)
    yo, uo, vo = grade_model(y, u, v, p.but(flags=CHROMA))
    assert np.array_equal(yo, y) and not np.array_equal(uo, u)
    want = [max(0, min(255, 128 + math.floor((p.m[0] * (int(a) - 128) + p.m[1] * (int(b) - 128) + p.off[0] + 2048) / 4096))) for a, b in zip(u.ravel(), v.ravel())]
    assert uo.ravel().tolist() == want                 # Python's own floor division, sample by sample
    ident = p.but(flags=CURVE | CHROMA | LUT, curve=np.arange(256, dtype=np.uint8), m=(4096, 0, 0, 4096), off=(0, 0), nodes=gm.identity_lattice(4))
    yo, uo, vo = grade_model(y, u, v, ident)
    assert np.array_equal(yo, y) and np.array_equal(uo, u) and np.array_equal(vo, v)


# ---- host-only calls of the library ----
def test_procamp_identity_is_exact():
    from mixlab_amd import abi, video
    p = video.grade_procamp(0, 255, 1, 1, 0)
    assert p.flags == abi.GRADE_CURVE | abi.GRADE_CHROMA
    assert list(p.curve_y) == list(range(256))
    assert (p.m_uu, p.m_uv, p.m_vu, p.m_vv, p.off_u, p.off_v) == (4096, 0, 0, 4096, 0, 0)


PROCAMPS = [(16, 235, 1.0, 1.0, 0.0), (0, 255, 2.2, 1.5, 30.0), (10.5, 200.25, 0.45, 0.0, -75.0), (-20, 300, 1.7, 7.9, 180.0), (64, 65, 3.0, 0.31, 12.5), (0, 255, 1.0, 2.0, 90.0)]


@pytest.mark.parametrize("args", PROCAMPS, ids=[str(a) for a in PROCAMPS])
def test_procamp_is_within_one_of_pythons_f64(args):
    """one libm ulp in pow / cos / sin can move a rint by one, no more"""
    from mixlab_amd import video
    black, white, gamma, sat, hue = args
    p = video.grade_procamp(*args)
    for i in range(256):
        t = min(1.0, max(0.0, (i - black) / (white - black)))
        want = max(0, min(255, round(255.0 * t ** (1.0 / gamma))))
        assert abs(p.curve_y[i] - want) <= 1, f"curve_y[{i}] = {p.curve_y[i]}, f64 gives {want}"
    h = math.radians(hue)
    want = [4096 * sat * math.cos(h), 4096 * sat * math.sin(h), -4096 * sat * math.sin(h), 4096 * sat * math.cos(h)]
    for got, w in zip((p.m_uu, p.m_uv, p.m_vu, p.m_vv), want):
        assert abs(got - w) <= 1.5 and abs(got - round(w)) <= 1
    assert (p.off_u, p.off_v) == (0, 0)


def test_procamp_errors():
    from mixlab_amd import abi, video
    for bad in ((100, 100, 1, 1, 0), (200, 100, 1, 1, 0), (0, 255, 0, 1, 0), (0, 255, -1, 1, 0), (0, 255, 1, 8.0, 0), (0, 255, 1, -8.0, 0), (0, 255, float("nan"), 1, 0)):
        with pytest.raises(abi.MxError) as e:
            video.grade_procamp(*bad)
        assert e.value.code == abi.MX_ERR_INVALID, bad
    p = video.grade_procamp(0, 255, 1, 7.99, 0)       # 32727: just inside
    assert p.m_uu == round(4096 * 7.99)


@pytest.mark.parametrize("k", [4, 5])
def test_library_identity_lattice_is_the_models(k):
    from mixlab_amd import video
    assert np.array_equal(video.lut_identity(k), gm.identity_lattice(k))


def test_lut_checks_come_before_any_device_work():
    """a node of 4097 and lattice_log2 of 3 or 6 are refused on a machine without a GPU: the checks run first"""
    from mixlab_amd import abi, video
    for k in (3, 6):
        n = (1 << k) + 1
        with pytest.raises(abi.MxError) as e:
            video.Lut(k, np.zeros((n, n, n, 3), np.uint16))
        assert e.value.code == abi.MX_ERR_INVALID
        with pytest.raises(abi.MxError) as e:
            video.lut_identity(k)
        assert e.value.code == abi.MX_ERR_INVALID
    nodes = gm.identity_lattice(4)
    nodes[16, 3, 9, 1] = 4097
    with pytest.raises(abi.MxError) as e:
        video.Lut(4, nodes)
    assert e.value.code == abi.MX_ERR_INVALID and "4096" in str(e.value)
    h = C.c_void_p()
    assert abi.lib.mx_video_lut_create(4, None, C.byref(h)) == abi.MX_ERR_INVALID and not h.value
