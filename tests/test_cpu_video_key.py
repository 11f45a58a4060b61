"""The keyer without a device (include/mixlab_gpu.h mx_video_key): the header's struct and the two exported entry points, the
properties of the numpy model the GPU suite compares the kernel with (tests/video_key_model.py), and that the shared pictures can tell the model from
each of a list of plausible mistakes."""
import ctypes as C
import math
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import alpha_patterns as ap
import video_key_model as km
from video_key_model import DEFAULT_CHROMA, DEFAULT_LUMA, KeyP, key_model

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402


# ---- the interface ----
def test_header_declares_the_params_struct_and_the_library_exports_both_entry_points():
    h = gen.Header(gen.HEADER.read_text())
    lay = h.layout_json()["mx_video_key_params"]
    assert lay["size"] == 24
    assert lay["offsets"] == {"mode": 0, "key_u": 4, "key_v": 5, "invert": 6, "_pad": 7, "near_q4": 8, "far_q4": 12, "spill_far_q4": 16, "spill_strength": 20}
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_KEY_CHROMA"] == 0 and consts["MX_KEY_LUMA"] == 1
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19          # not a new module kind, no new ABI version
    declared = {f[0]: f for f in h.funcs}
    assert [c for _n, c, _a in declared["mx_video_key"][2]] == ["const mx_dframe*", "const mx_video_key_params*", "mx_dframe**", "void*"]
    assert [c for _n, c, _a in declared["mx_graph_set_video_source_key"][2]] == ["mx_graph*", "uint32_t", "const mx_video_key_params*"]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    exported = {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}
    assert {"mx_video_key", "mx_graph_set_video_source_key"} <= exported


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi
    assert C.sizeof(abi.VideoKeyParams) == 24
    assert [(n, getattr(abi.VideoKeyParams, n).offset) for n, _t in abi.VideoKeyParams._fields_] == \
        [("mode", 0), ("key_u", 4), ("key_v", 5), ("invert", 6), ("_pad", 7), ("near_q4", 8), ("far_q4", 12), ("spill_far_q4", 16), ("spill_strength", 20)]


# ---- the model's properties ----
def flat(w, h, yv, uv, vv):
    return np.full((h, w), yv, np.uint8), np.full((h // 2, w // 2), uv, np.uint8), np.full((h // 2, w // 2), vv, np.uint8)


def test_distance_is_the_exact_integer_root_for_every_du_dv():
    du, dv = np.mgrid[-255:256, -255:256]
    d2 = du * du + dv * dv
    assert d2.max() == 130050 and (d2.max() << 8) == 33292800 > 2 ** 24
    got = km.dist_q4(d2)
    want = np.array([math.isqrt(int(x) << 8) for x in np.unique(d2)])
    lut = dict(zip(np.unique(d2).tolist(), want.tolist()))
    assert got.max() == 5769
    assert np.array_equal(got, np.vectorize(lut.get)(d2))


def test_key_colour_is_transparent_and_far_colours_are_opaque():
    p = DEFAULT_CHROMA
    _y, _u, _v, k = key_model(*flat(8, 6, 90, p.key_u, p.key_v), p)
    assert (k == 0).all()
    y, u, v = km.green_screen(66, 38, 1)
    d = km.dist_q4((u.astype(int) - p.key_u) ** 2 + (v.astype(int) - p.key_v) ** 2)
    _y, _u, _v, k = key_model(y, u, v, p)
    assert (d > p.far_q4).any()
    assert (k[::2, ::2][d > p.far_q4] == 255).all()                     # even (x, y): the chroma sample's own decision
    assert np.array_equal(k[::2, ::2], km.ramp(d, p.near_q4, p.far_q4).astype(np.uint8))


def test_near_equal_far_is_a_hard_key():
    for pic, p in ((km.every_uv(), DEFAULT_CHROMA.but(near_q4=160, far_q4=160, spill_strength=0)), (km.luma_wedge(130, 74), DEFAULT_LUMA.but(near_q4=1600, far_q4=1600))):
        k = key_model(*pic, p)[3]
        assert set(np.unique(k[::2, ::2]).tolist()) == {0, 255}
    y, u, v = km.luma_wedge(130, 74)
    k = key_model(y, u, v, DEFAULT_LUMA.but(near_q4=1600, far_q4=1600))[3]
    assert np.array_equal(k == 0, y.astype(int) * 16 <= 1600)           # d == lo is still 0: the tests are applied in the stated order


def test_invert_and_incoming_coverage():
    y, u, v = km.green_screen(66, 38, 2)
    for p in (DEFAULT_CHROMA, DEFAULT_LUMA):
        k = key_model(y, u, v, p)[3]
        assert np.array_equal(key_model(y, u, v, p.but(invert=1))[3], 255 - k)
        assert np.array_equal(key_model(y, u, v, p, a_in=np.full(y.shape, 255, np.uint8))[3], k)
        assert not key_model(y, u, v, p, a_in=np.zeros(y.shape, np.uint8))[3].any()
        a = ap.alpha_plane(66, 38, "random", 1)
        assert np.array_equal(key_model(y, u, v, p.but(invert=1), a_in=a)[3], ((255 - k.astype(int)) * a) // 255)


def test_spill_suppression_ends():
    y, u, v = km.green_screen(66, 38, 3)
    p = DEFAULT_CHROMA
    # w = 255 everywhere: every distance lies at or below far, full strength
    full = key_model(y, u, v, p.but(near_q4=0, far_q4=6000, spill_far_q4=6001, spill_strength=255))
    assert (full[1] == 128).all() and (full[2] == 128).all()
    off = key_model(y, u, v, p.but(spill_strength=0))
    assert np.array_equal(off[1], u) and np.array_equal(off[2], v)
    assert np.array_equal(key_model(y, u, v, p.but(spill_far_q4=p.far_q4))[1], u)   # spill_far <= far: inactive
    on, inv = key_model(y, u, v, p), key_model(y, u, v, p.but(invert=1))
    assert np.array_equal(on[1], inv[1]) and np.array_equal(on[2], inv[2])          # whatever invert is
    assert np.array_equal(on[0], y) and np.array_equal(off[3], on[3])               # Y copied; spill does not move the coverage


def test_luma_mode_copies_chroma():
    y, u, v = km.luma_wedge(66, 38)
    yo, uo, vo, k = key_model(y, u, v, DEFAULT_LUMA)
    assert np.array_equal(yo, y) and np.array_equal(uo, u) and np.array_equal(vo, v)
    assert np.array_equal(k, km.ramp(y.astype(int) * 16, DEFAULT_LUMA.near_q4, DEFAULT_LUMA.far_q4).astype(np.uint8))


# ---- the pictures can tell ----
@pytest.mark.parametrize("size", [(66, 38), (322, 182), (1920, 1080)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_green_screen_exercises_both_ramps(size):
    y, u, v = km.green_screen(*size, seed=1)
    yo, uo, vo, k = key_model(y, u, v, DEFAULT_CHROMA)
    n = k.size
    assert (k == 0).sum() >= n // 100 and (k == 255).sum() >= n // 100 and ((k > 0) & (k < 255)).sum() >= n // 100
    assert ((uo != u) | (vo != v)).sum() >= u.size // 100


def test_luma_wedge_exercises_the_luma_ramp():
    y, u, v = km.luma_wedge(322, 182)
    k = key_model(y, u, v, DEFAULT_LUMA)[3]
    n = k.size
    assert (k == 0).sum() >= n // 100 and (k == 255).sum() >= n // 100 and ((k > 0) & (k < 255)).sum() >= n // 100
    assert len(np.unique(y)) == 256


def _pictures():
    return {"green": km.green_screen(66, 38, 1), "uv": km.every_uv(), "wedge": km.luma_wedge(130, 74)}


MISTAKES = [   # (mis-model, picture, parameters, with incoming coverage)
    ("sqrt_round", "uv", DEFAULT_CHROMA, False),
    # from key (0, 0) the pair (234, 168) has d2 = 82 980 and d = 4608, where the f32 root of d2 << 8 rounds up to 4609.0: a hard key at 4608 tells them apart
    ("sqrt_f32", "uv", KeyP(km.KEY_CHROMA, 0, 0, 0, 4608, 4608, 0, 0), False),
    ("ramp_round", "green", DEFAULT_CHROMA, False),
    ("ramp_round", "wedge", DEFAULT_LUMA, False),
    ("no_plus2", "green", DEFAULT_CHROMA, False),
    # every_uv keyed on (0, 128): the left edge holds the key colour and the right edge does not, so a wrapped or zero-filled column cx + 1 shows
    ("edge_wrap", "uv", DEFAULT_CHROMA.but(key_u=0, key_v=128), False),
    ("edge_zero", "uv", DEFAULT_CHROMA.but(key_u=0, key_v=128), False),
    ("siting", "green", DEFAULT_CHROMA, False),
    ("spill_floor", "green", DEFAULT_CHROMA, False),
    ("invert_after", "green", DEFAULT_CHROMA.but(invert=1), True),
    ("ramp_order", "uv", DEFAULT_CHROMA.but(near_q4=160, far_q4=160), False),
    ("ramp_order", "wedge", DEFAULT_LUMA.but(near_q4=1600, far_q4=1600), False),
]


@pytest.mark.parametrize("bug,pic,p,with_alpha", MISTAKES, ids=[f"{m[0]}-{m[1]}" for m in MISTAKES])
def test_each_mis_model_differs_from_the_model_on_the_shared_pictures(bug, pic, p, with_alpha):
    assert bug in km.BUGS
    y, u, v = _pictures()[pic]
    a = ap.alpha_plane(y.shape[1], y.shape[0], "soft-disc", 2) if with_alpha else None
    good, bad = key_model(y, u, v, p, a_in=a), key_model(y, u, v, p, a_in=a, bug=bug)
    assert any(not np.array_equal(g, b) for g, b in zip(good, bad)), f"the pictures cannot tell the model from '{bug}'"


def test_every_listed_mistake_is_tried():
    assert {m[0] for m in MISTAKES} == set(km.BUGS)
