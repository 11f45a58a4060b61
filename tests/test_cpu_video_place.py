"""The placer without a device (include/mixlab_gpu.h mx_video_place): the header's struct and the two exported entry points, the
properties of the numpy model the GPU suite compares the kernel with (tests/video_place_model.py), and that the shared cases can tell the model from each
of a list of plausible misreadings."""
import ctypes as C
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import video_model as vm
import video_place_model as pm
from video_place_model import PlaceP, place_model

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

FIELDS = ["canvas_w", "canvas_h", "crop_x", "crop_y", "crop_w", "crop_h", "dst_x", "dst_y", "dst_w", "dst_h"]


# ---- the interface ----
def test_header_declares_the_params_struct_and_the_library_exports_both_entry_points():
    h = gen.Header(gen.HEADER.read_text())
    lay = h.layout_json()["mx_video_place_params"]
    assert lay["size"] == 40
    assert lay["offsets"] == {n: 4 * i for i, n in enumerate(FIELDS)}
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # not a module kind, no new ABI version
    declared = {f[0]: f for f in h.funcs}
    assert [c for _n, c, _a in declared["mx_video_place"][2]] == ["const mx_dframe*", "const mx_video_place_params*", "mx_dframe**", "void*"]
    assert [c for _n, c, _a in declared["mx_graph_set_video_source_place"][2]] == ["mx_graph*", "uint32_t", "const mx_video_place_params*"]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    exported = {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}
    assert {"mx_video_place", "mx_graph_set_video_source_place"} <= exported


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi, video
    assert C.sizeof(abi.VideoPlaceParams) == 40
    assert [(n, getattr(abi.VideoPlaceParams, n).offset) for n, _t in abi.VideoPlaceParams._fields_] == [(n, 4 * i) for i, n in enumerate(FIELDS)]
    assert abi.VideoPlaceParams.dst_x.size == 4 and dict(abi.VideoPlaceParams._fields_)["dst_x"] is C.c_int32 and dict(abi.VideoPlaceParams._fields_)["dst_y"] is C.c_int32
    p = video.PlaceParams(66, 38, -4, 6, 20, 10, crop=(2, 4, 8, 12))
    assert [getattr(p, n) for n in FIELDS] == [66, 38, 2, 4, 8, 12, -4, 6, 20, 10]
    assert [getattr(video.PlaceParams(66, 38, 0, 0, 2, 2), n) for n in FIELDS[2:6]] == [0, 0, 0, 0]
    assert abi.lib.mx_abi_version() == 4


def test_exported_tile_and_tap_bound_match_the_kernels():
    from mixlab_amd import abi
    src = (ROOT / "mixlab_amd" / "csrc" / "mx_video.hpp").read_text()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"(MX_PLACE_\w+) = (\d+)", src)}
    assert got == {"MX_PLACE_TILE_W": abi.PLACE_TILE_W, "MX_PLACE_TILE_H": abi.PLACE_TILE_H, "MX_PLACE_TAP_BOUND": abi.PLACE_TAP_BOUND}
    # the bound is a tap count the scaler can produce, and one step of the downscale ratio above it is another form
    assert abi.lib.mx_video_scaler_tap_count(64, 16) == abi.PLACE_TAP_BOUND < abi.lib.mx_video_scaler_tap_count(66, 16) and abi.lib.mx_video_scaler_tap_count(64, 2) == 130


# ---- the model's properties ----
@pytest.mark.parametrize("alpha", [False, True])
def test_identity_placement_returns_the_input(alpha):
    y, u, v, a = pm.noise_frame(66, 38, 1, alpha)
    oy, ou, ov, oa = place_model(y, u, v, PlaceP(66, 38, 0, 0, 66, 38), a)
    assert np.array_equal(oy, y) and np.array_equal(ou, u) and np.array_equal(ov, v)
    assert np.array_equal(oa, a if alpha else np.full_like(y, 255))


@pytest.mark.parametrize("size", [(34, 18), (130, 74), (16, 10)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("alpha", [False, True])
def test_whole_frame_to_the_full_canvas_is_the_scaler_without_letterbox(size, alpha):
    y, u, v, a = pm.noise_frame(66, 38, 2, alpha)
    w, h = size
    got = place_model(y, u, v, PlaceP(w, h, 0, 0, w, h), a)
    want = vm.scale_frame([y, u, v], "planar", w, h, (w, h, 0, 0), alpha=a)
    for k in range(3):
        assert np.array_equal(got[k], want[k])
    assert np.array_equal(got[3], want[3] if alpha else np.full((h, w), 255, np.uint8))


def test_translating_dst_by_an_even_offset_translates_the_picture():
    y, u, v, a = pm.noise_frame(34, 18, 3, True)
    base = place_model(y, u, v, PlaceP(130, 74, 10, 6, 40, 22), a)
    for dx, dy in ((2, 0), (0, 2), (36, 18), (-8, -4)):
        moved = place_model(y, u, v, PlaceP(130, 74, 10 + dx, 6 + dy, 40, 22), a)
        for k, (b, m) in enumerate(zip(base, moved)):
            c = 1 if k in (1, 2) else 0
            sx, sy = dx >> c, dy >> c
            fill = 0x80 if c else 0
            want = np.full_like(b, fill)
            H, W = b.shape
            want[max(sy, 0):H + min(sy, 0), max(sx, 0):W + min(sx, 0)] = b[max(-sy, 0):H - max(sy, 0), max(-sx, 0):W - max(sx, 0)]
            assert np.array_equal(m, want), (dx, dy, k)


def test_a_rectangle_outside_the_canvas_gives_a_blank_transparent_frame():
    y, u, v, a = pm.noise_frame(34, 18, 4, True)
    for dx, dy in ((66, 0), (-34, 0), (0, 38), (0, -18), (2147483646, -2147483648)):
        oy, ou, ov, oa = place_model(y, u, v, PlaceP(66, 38, dx, dy, 34, 18), a)
        assert not oy.any() and not oa.any() and (ou == 0x80).all() and (ov == 0x80).all()


def test_the_crop_alone_decides_the_picture():
    """samples outside the crop are never read: changing them changes nothing"""
    y, u, v, a = pm.noise_frame(66, 38, 5, True)
    p = PlaceP(66, 38, 4, 2, 20, 30, 10, 6, 40, 20)
    want = place_model(y, u, v, p, a)
    y2, u2, v2, a2 = (255 - q for q in (y, u, v, a))
    for q, q2, c in ((y, y2, 0), (u, u2, 1), (v, v2, 1), (a, a2, 0)):
        q2[6 >> c:26 >> c, 10 >> c:50 >> c] = q[6 >> c:26 >> c, 10 >> c:50 >> c]
    for g, w_ in zip(place_model(y2, u2, v2, p, a2), want):
        assert np.array_equal(g, w_)


def test_the_written_out_passes_agree_with_the_pinned_scaler():
    y, _u, _v, _a = pm.noise_frame(66, 38, 6, False)
    for (x0, y0, cw, ch, dw, dh) in ((10, 6, 40, 20, 12, 30), (0, 0, 66, 38, 20, 10), (34, 20, 32, 18, 32, 18)):
        assert np.array_equal(pm._resample_general(y, x0, y0, cw, ch, dw, dh), vm.scale_plane(y[y0:y0 + ch, x0:x0 + cw], dw, dh))


def test_plane_clamping_changes_the_h_pass_of_a_noise_crop():
    """a 6-of-12-column crop of noise, 6 -> 10: clamping tap indices to the plane instead of the crop changes H-pass values at both ends of every row"""
    rng = np.random.default_rng(7)
    p = rng.integers(0, 256, size=(6, 12)).astype(np.int64)
    hf, hc = vm.tap_tables(6, 10)
    ix = hf[:, None] + np.arange(hc.shape[1])[None, :]
    crop = vm.asr((p[:, np.clip(ix, 0, 5) + 4] * hc[None]).sum(axis=2) + vm.H_ROUND, vm.H_SHIFT)
    plane = vm.asr((p[:, np.clip(ix + 4, 0, 11)] * hc[None]).sum(axis=2) + vm.H_ROUND, vm.H_SHIFT)
    assert crop.shape == (6, 10) and 12 <= (crop != plane).sum() <= 24 and not (crop != plane)[:, 2:8].any()


# ---- the shared cases can tell ----
def _small_cases():
    from mixlab_amd import abi
    return [c for c in pm.cases(abi.PLACE_TILE_W, abi.PLACE_TILE_H, abi.PLACE_TAP_BOUND) if not c.big]


def test_the_cases_cover_both_forms_and_the_sizes_around_the_tile():
    from mixlab_amd import abi
    cs = pm.cases(abi.PLACE_TILE_W, abi.PLACE_TILE_H, abi.PLACE_TAP_BOUND)
    taps = set()
    for c in cs:
        cw, ch = (c.p.crop_w or c.src_w), (c.p.crop_h or c.src_h)
        taps.add(abi.lib.mx_video_scaler_tap_count(cw, c.p.dst_w)); taps.add(abi.lib.mx_video_scaler_tap_count(ch, c.p.dst_h))
    assert {4, abi.PLACE_TAP_BOUND - 2, abi.PLACE_TAP_BOUND, abi.PLACE_TAP_BOUND + 2, 130} <= taps
    canv = {(c.p.canvas_w, c.p.canvas_h) for c in cs}
    assert {(2, 2), (34, 2), (2, 34), (66, 38), (130, 74), (322, 182), (1920, 1080)} <= canv
    assert {(abi.PLACE_TILE_W + d, abi.PLACE_TILE_H + d) for d in (-2, 0, 2)} <= canv
    assert any(c.alpha for c in cs) and any(not c.alpha for c in cs) and sum(c.big for c in cs) == 2


@pytest.mark.parametrize("bug", pm.BUGS)
def test_each_misreading_changes_a_byte_of_a_shared_case(bug):
    hit = []
    for c in _small_cases():
        if bug == "cov_chroma_tables" and not c.alpha:
            continue
        good, bad = c.want(), c.want(bug)
        if any(not np.array_equal(g, b) for g, b in zip(good, bad)):
            hit.append(c.name)
            if len(hit) >= 3:
                break
    assert hit, f"the shared cases cannot tell the model from '{bug}'"


def test_at_least_eight_misreadings_are_listed():
    assert len(set(pm.BUGS)) >= 8
