"""The multiviewer without a device (include/mixlab_gpu.h mx_video_multiview): the header's structs and the three exported entry points,
every parameter error refused through the ABI before a device is touched, the properties of the numpy model the GPU suite compares the kernel with
(tests/video_multiview_model.py), and that the SMALL shared cases can tell the model from each of a list of plausible misreadings."""
import ctypes as C
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import video_model as vm
import video_multiview_model as mm
import video_place_model as pm
from video_multiview_model import MvP, Src, View, multiview_model

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402


# ---- the interface ----
def test_header_declares_the_structs_and_the_library_exports_the_three_entry_points():
    h = gen.Header(gen.HEADER.read_text())
    lay = h.layout_json()
    assert lay["mx_multiview_view"] == {"size": 24, "offsets": {"x": 0, "y": 4, "w": 8, "h": 12, "border": 16, "border_y": 20, "border_u": 21, "border_v": 22, "fit": 23}}
    assert lay["mx_multiview_params"] == {"size": 404, "offsets": {"canvas_w": 0, "canvas_h": 4, "bg_y": 8, "bg_u": 9, "bg_v": 10, "_pad": 11, "n_views": 12, "hop": 16, "view": 20}}
    assert lay["mx_multiview_status"] == {"size": 16, "offsets": {"recorded": 0, "tick_in_run": 4, "present_mask": 8, "shown_mask": 12}}
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_MULTIVIEW_MAX"] == 16
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # not a module kind, no new ABI version
    declared = {f[0]: f for f in h.funcs}
    assert [c for _n, c, _a in declared["mx_video_multiview"][2]] == ["const mx_dframe*const*", "const mx_multiview_params*", "mx_dframe**", "uint32_t*", "void*"]
    assert [c for _n, c, _a in declared["mx_graph_set_multiview"][2]] == ["mx_graph*", "const mx_port_ref*", "size_t", "const mx_multiview_params*"]
    assert [c for _n, c, _a in declared["mx_graph_multiview_output"][2]] == ["mx_graph*", "mx_dframe**", "mx_multiview_status*"]
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    exported = {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}
    assert {"mx_video_multiview", "mx_graph_set_multiview", "mx_graph_multiview_output"} <= exported


def test_ctypes_mirror_has_the_headers_layout():
    from mixlab_amd import abi, video
    assert (C.sizeof(abi.MultiviewView), C.sizeof(abi.MultiviewParams), C.sizeof(abi.MultiviewStatus)) == (24, 404, 16)
    assert abi.MultiviewParams.view.offset == 20 and abi.MultiviewView.fit.offset == 23 and abi.MultiviewParams.hop.offset == 16
    p = video.MultiviewParams(66, 38, [video.MultiviewView(2, 4, 20, 12, 2, (1, 2, 3), 0)], bg=(9, 8, 7), hop=3)
    v = p.view[0]
    assert (p.canvas_w, p.canvas_h, p.bg_y, p.bg_u, p.bg_v, p._pad, p.n_views, p.hop) == (66, 38, 9, 8, 7, 0, 1, 3)
    assert (v.x, v.y, v.w, v.h, v.border, v.border_y, v.border_u, v.border_v, v.fit) == (2, 4, 20, 12, 2, 1, 2, 3, 0)
    assert abi.lib.mx_abi_version() == 4


def test_exported_tile_and_tap_bound_match_the_kernels():
    from mixlab_amd import abi
    src = (ROOT / "mixlab_amd" / "csrc" / "mx_video.hpp").read_text()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"(MX_MULTIVIEW_\w+) = (\d+)", src)}
    assert got == {"MX_MULTIVIEW_TILE_W": abi.MULTIVIEW_TILE_W, "MX_MULTIVIEW_TILE_H": abi.MULTIVIEW_TILE_H, "MX_MULTIVIEW_TAP_BOUND": abi.MULTIVIEW_TAP_BOUND}
    # the bound is a tap count the scaler can produce, and one step of the downscale ratio above it is another form
    at = 4 * (abi.MULTIVIEW_TAP_BOUND - 2)
    assert abi.lib.mx_video_scaler_tap_count(at, 16) == abi.MULTIVIEW_TAP_BOUND < abi.lib.mx_video_scaler_tap_count(at + 2, 16) and abi.lib.mx_video_scaler_tap_count(64, 2) == 130


# ---- parameter errors: refused on the host, before a frame, a graph or a device is looked at ----
def _params(views, canvas=(66, 38), hop=1, pad=0, n=None):
    from mixlab_amd import abi, video
    p = video.MultiviewParams(canvas[0], canvas[1], [video.MultiviewView(*v) for v in views], hop=hop)
    p._pad = pad
    if n is not None:
        p.n_views = n
    return p


GOOD = [(2, 2, 20, 12, 2), (22, 2, 20, 12, 2)]     # touching is allowed
BAD = {
    "overlap": dict(views=[(2, 2, 20, 12, 2), (20, 2, 20, 12, 2)]),
    "overlap-frames-only": dict(views=[(2, 2, 20, 12, 2), (4, 12, 20, 12, 2)]),
    "contained": dict(views=[(2, 2, 40, 30, 2), (10, 10, 6, 6, 0)]),
    "odd-x": dict(views=[(3, 2, 20, 12, 2)]), "odd-y": dict(views=[(2, 1, 20, 12, 2)]), "odd-w": dict(views=[(2, 2, 21, 12, 2)]), "odd-h": dict(views=[(2, 2, 20, 11, 2)]),
    "odd-border": dict(views=[(2, 2, 20, 12, 1)]), "odd-canvas-w": dict(views=GOOD, canvas=(67, 38)), "odd-canvas-h": dict(views=GOOD, canvas=(66, 37)),
    "outside-right": dict(views=[(50, 2, 20, 12, 2)]), "outside-below": dict(views=[(2, 30, 20, 12, 2)]), "outside-far": dict(views=[(4294967294, 2, 4, 4, 0)]),
    "border-thick-w": dict(views=[(2, 2, 8, 12, 4)]), "border-thick-h": dict(views=[(2, 2, 20, 8, 4)]), "border-66": dict(views=[(0, 0, 160, 160, 66)], canvas=(160, 160)),
    "fit-2": dict(views=[(2, 2, 20, 12, 2, (0, 0, 0), 2)]),
    "no-views": dict(views=GOOD, n=0), "17-views": dict(views=GOOD, n=17), "pad": dict(views=GOOD, pad=1),
    "canvas-0": dict(views=GOOD, canvas=(0, 38)), "canvas-huge": dict(views=GOOD, canvas=(16386, 38)),
}


@pytest.mark.parametrize("name", list(BAD))
def test_parameter_errors_are_refused_through_the_abi_without_a_device(name):
    from mixlab_amd import abi
    p = _params(**BAD[name])
    frames = (C.c_void_p * 16)()
    out, shown = C.c_void_p(), C.c_uint32()
    assert abi.lib.mx_video_multiview(frames, C.byref(p), C.byref(out), C.byref(shown), None) == abi.MX_ERR_INVALID and not out.value
    assert b"mx_multiview_params" in abi.lib.mx_last_error()
    n = p.n_views
    ports = (abi.PortRef * 17)()
    if n:   # with n = 0 the call removes the setting and looks at no parameters
        assert abi.lib.mx_graph_set_multiview(None, ports, n, C.byref(p)) == abi.MX_ERR_INVALID
        assert b"mx_multiview_params" in abi.lib.mx_last_error()


def test_the_graph_form_refuses_hop_0_and_a_count_that_is_not_n_views():
    from mixlab_amd import abi
    ports = (abi.PortRef * 4)()
    p = _params(GOOD, hop=0)
    assert abi.lib.mx_graph_set_multiview(None, ports, 2, C.byref(p)) == abi.MX_ERR_INVALID and b"hop" in abi.lib.mx_last_error()
    p = _params(GOOD, hop=1)
    assert abi.lib.mx_graph_set_multiview(None, ports, 3, C.byref(p)) == abi.MX_ERR_INVALID and b"n_views" in abi.lib.mx_last_error()
    # good parameters get as far as the graph, which is not there
    assert abi.lib.mx_graph_set_multiview(None, ports, 2, C.byref(p)) == abi.MX_ERR_INVALID and b"graph is NULL" in abi.lib.mx_last_error()


# ---- the model's properties ----
@pytest.mark.parametrize("src", [(66, 38), (20, 40), (130, 20), (16, 10)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fit_1_inner_rectangle_is_the_scalers_frame(src):
    f = mm.noise_src(src[0], src[1], 1, alpha=True)
    v = View(10, 6, 44, 30, 2, mm.RED, 1)
    got = multiview_model([f], MvP(130, 74, (v,)))
    iw, ih = 40, 26
    want = vm.scale_frame([f.y, f.u, f.v], "planar", iw, ih, mm.scale_geometry(f.w, f.h, iw, ih))
    for k in range(3):
        c = 1 if k else 0
        assert np.array_equal(got[k][(8 >> c):(8 >> c) + (ih >> c), (12 >> c):(12 >> c) + (iw >> c)], want[k]), k


@pytest.mark.parametrize("src", [(66, 38), (20, 40), (34, 18)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fit_0_picture_is_the_placers(src):
    f = mm.noise_src(src[0], src[1], 2)
    v = View(10, 6, 44, 30, 2, mm.GREEN, 0)
    got = multiview_model([f], MvP(130, 74, (v,)))
    want = pm.place_model(f.y, f.u, f.v, pm.PlaceP(130, 74, 12, 8, 40, 26))
    for k in range(3):
        c = 1 if k else 0
        sl = (slice(8 >> c, (8 + 26) >> c), slice(12 >> c, (12 + 40) >> c))
        assert np.array_equal(got[k][sl], want[k][sl]), k


def test_an_identity_size_view_returns_the_source():
    f = mm.noise_src(66, 38, 3, alpha=True)
    for fit in (0, 1):
        got = multiview_model([f], MvP(66, 38, (View(0, 0, 66, 38, 0, mm.RED, fit),)))
        assert all(np.array_equal(g, w) for g, w in zip(got, (f.y, f.u, f.v)))


def test_permuting_the_views_with_their_frames_leaves_the_canvas_unchanged():
    case = next(c for c in mm.cases(64, 16, 20) if c.name == "grid16")
    frames, want = case.frames(), case.want()
    order = np.random.default_rng(4).permutation(16)
    got = multiview_model([frames[i] for i in order], case.p.but(views=tuple(case.p.views[i] for i in order)))
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_frame_blank_and_background_are_where_the_header_puts_them():
    v = View(10, 6, 24, 14, 2, (1, 2, 3), 1)
    y, u, vv = multiview_model([None], MvP(66, 38, (v,), bg=(9, 8, 7)))
    assert y[0, 0] == 9 and u[0, 0] == 8 and vv[0, 0] == 7
    assert y[6, 10] == 1 and y[7, 33] == 1 and y[8, 12] == 0 and y[17, 31] == 0 and y[18, 12] == 1 and y[20, 12] == 9
    assert u[3, 5] == 2 and u[4, 6] == 0x80 and vv[8, 15] == 0x80 and vv[9, 15] == 3 and vv[10, 15] == 7
    assert mm.shown_mask([None], MvP(66, 38, (v,))) == 0


# ---- the shared cases can tell ----
def _cases():
    from mixlab_amd import abi
    return mm.cases(abi.MULTIVIEW_TILE_W, abi.MULTIVIEW_TILE_H, abi.MULTIVIEW_TAP_BOUND)


def test_the_cases_cover_both_forms_the_tile_sizes_and_every_reason_not_to_show():
    from mixlab_amd import abi
    cs = _cases()
    taps = set()
    for c in cs:
        for v, f in zip(c.p.views, c.frames()):
            P = mm.view_geometry(v, f)[1]
            if P:
                taps.add(abi.lib.mx_video_scaler_tap_count(f.w, P[2])); taps.add(abi.lib.mx_video_scaler_tap_count(f.h, P[3]))
    assert {4, abi.MULTIVIEW_TAP_BOUND - 2, abi.MULTIVIEW_TAP_BOUND, abi.MULTIVIEW_TAP_BOUND + 2, 130} <= taps
    canv = {(c.p.canvas_w, c.p.canvas_h) for c in cs}
    assert {(2, 2), (34, 18), (66, 38), (130, 74), (1920, 1080)} <= canv
    assert {(abi.MULTIVIEW_TILE_W + d, abi.MULTIVIEW_TILE_H + d) for d in (-2, 0, 2)} <= canv
    assert {len(c.p.views) for c in cs} >= {1, 2, 4, 16} and sum(c.big for c in cs) == 2
    assert {v.border for c in cs for v in c.p.views} >= {0, 2, 8, 64} and {v.fit for c in cs for v in c.p.views} == {0, 1}
    grid = next(c for c in cs if c.name == "grid16")
    assert len({(f.w, f.h) for f in grid.frames()}) >= 4
    assert any(f is not None and f.a is not None for c in cs for f in c.frames())
    for name in ("notshown-none", "notshown-format", "notshown-thin", "notshown-ratio"):
        c = next(c for c in cs if c.name == name)
        assert mm.shown_mask(c.frames(), c.p) == 2, name
    for c in cs:   # every case is one the ABI accepts: inside the canvas, even, no overlap
        for i, v in enumerate(c.p.views):
            assert not any(n & 1 for n in (v.x, v.y, v.w, v.h, v.border)) and v.x + v.w <= c.p.canvas_w and v.y + v.h <= c.p.canvas_h and min(v.w, v.h) >= 2 * v.border + 2, c.name
            for o in c.p.views[:i]:
                assert not (v.x < o.x + o.w and o.x < v.x + v.w and v.y < o.y + o.h and o.y < v.y + v.h), c.name


@pytest.mark.parametrize("bug", mm.BUGS)
def test_each_misreading_changes_a_byte_of_a_small_shared_case(bug):
    """a condition, not a measurement: the small cases alone must catch every misreading -- the `big` ones are never needed for it"""
    hit = []
    for c in _cases():
        if c.big:
            continue
        good, bad = c.want(), c.want(bug)
        if any(not np.array_equal(g, b) for g, b in zip(good, bad)):
            hit.append(c.name)
            if len(hit) >= 3:
                break
    assert hit, f"the small shared cases cannot tell the model from '{bug}'"


def test_at_least_ten_misreadings_are_listed():
    assert len(set(mm.BUGS)) >= 10
