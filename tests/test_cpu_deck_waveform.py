"""The deck's waveform picture without a device (include/mixlab_gpu.h "WAVEFORM"): the header's structs and entry points, the setting rules at
both edges of each, mx_deck_waveform_view, mx_deck_waveform_host against the model on every byte of every shared case (with strides above the width, the room beyond
the picture left alone), what the specification promises of any picture, and that the shared cases tell the model from each of a list of misreadings."""
import ctypes as C
import pathlib
import re
import subprocess
import sys

import numpy as np
import pytest

import deck_waveform_cases as wc
import deck_waveform_model as wm
from deck_waveform_model import ENVELOPE, Grid, Marker, Range, Wave

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
import gen_rust_ffi as gen  # noqa: E402

ENTRY_POINTS = {"mx_deck_waveform_check", "mx_deck_waveform_view", "mx_deck_render_waveform", "mx_deck_waveform_host", "mx_deck_debug_last_waveform"}
COLOUR_OFFSETS = {"y": 0, "u": 1, "v": 2, "_pad": 3}
GRID_OFFSETS = {"grid": 0, "from_q32": 16, "to_q32": 24, "colour": 32, "inset": 36}
MARKER_OFFSETS = {"frame": 0, "width": 8, "colour": 12}
RANGE_OFFSETS = {"from_frame": 0, "to_frame": 8, "colour": 16, "_pad": 20}
WAVE_OFFSETS = {"w": 0, "h": 4, "first_frame": 8, "frames_per_px": 16, "style": 20, "gain_q16": 24, "bg": 36, "line": 40, "band": 44, "n_grids": 56, "n_markers": 60,
                "n_ranges": 64, "_pad": 68, "grid": 72, "marker": 712, "range": 1224}
Q = 1 << 32


# ---- the interface ----
def test_header_declares_the_interface_and_the_library_exports_it():
    text = gen.HEADER.read_text()
    h = gen.Header(text)
    lay = h.layout_json()
    assert lay["mx_wave_colour"] == {"size": 4, "offsets": COLOUR_OFFSETS}
    assert lay["mx_wave_grid"] == {"size": 40, "offsets": GRID_OFFSETS}
    assert lay["mx_wave_marker"] == {"size": 16, "offsets": MARKER_OFFSETS}
    assert lay["mx_wave_range"] == {"size": 24, "offsets": RANGE_OFFSETS}
    assert lay["mx_deck_waveform"] == {"size": 1416, "offsets": WAVE_OFFSETS}
    consts = {c[0]: int(c[2]) for c in h.consts}
    assert consts["MX_ABI_VERSION"] == 4 and consts["MX_KIND_COUNT"] == 19 and consts["MX_PROFILE_KINDS"] == 18   # additions only
    assert (consts["MX_WAVE_BANDS"], consts["MX_WAVE_ENVELOPE"], consts["MX_WAVE_MAX_GRIDS"], consts["MX_WAVE_MAX_MARKERS"], consts["MX_WAVE_MAX_RANGES"],
            consts["MX_WAVE_STRIP"]) == (0, 1, 16, 32, 8, 64)
    declared = {f[0]: f for f in h.funcs}
    assert ENTRY_POINTS <= set(declared)
    sig = lambda name: [c for _n, c, _a in declared[name][2]]   # noqa: E731
    assert sig("mx_deck_waveform_check") == ["const mx_deck_waveform*"]
    assert sig("mx_deck_waveform_view") == ["int64_t", "uint32_t", "uint32_t", "int64_t*"]
    assert sig("mx_deck_render_waveform") == ["mx_deck*", "const mx_deck_waveform*", "mx_dframe**", "void*"]
    assert sig("mx_deck_waveform_host") == ["const mx_deck_column*", "uint64_t", "uint32_t", "uint64_t", "const mx_deck_waveform*", "uint8_t*", "int32_t", "uint8_t*",
                                            "uint8_t*", "int32_t"]
    assert re.search(r"int mx_deck_debug_last_waveform\(uint32_t out\[4\]\);", text)
    note = text[text.index("later, without a bump"):text.index("status codes")]
    for name in sorted(ENTRY_POINTS | {"mx_wave_colour", "mx_wave_grid", "mx_wave_marker", "mx_wave_range", "mx_deck_waveform"}):
        assert re.search(rf"\b{name}\b", note), name
    block = text[text.index("---- WAVEFORM:"):text.index("int mx_deck_debug_last_waveform")]
    for words in ("SETTINGS", "COLUMN", "HEIGHTS", "LAYERS", "GRID LINE", "PLANES", "ORDER", "Out of scope", "floor division", "no Q32 quantity below leaves int64",
                  "Y 0, chroma 0x80", "exactly once", "never waits for the host"):
        assert words in block, words
    out = subprocess.run(["nm", "-D", "--defined-only", str(ROOT / "mixlab_amd" / "libmixlab_gpu.so")], capture_output=True, text=True, check=True).stdout
    assert ENTRY_POINTS <= {m.group(1) for m in re.finditer(r" T (mx_\w+)$", out, flags=re.M)}


def test_ctypes_mirrors_have_the_headers_layout():
    from mixlab_amd import abi
    for st, size, offs in ((abi.WaveColour, 4, COLOUR_OFFSETS), (abi.WaveGrid, 40, GRID_OFFSETS), (abi.WaveMarker, 16, MARKER_OFFSETS), (abi.WaveRange, 24, RANGE_OFFSETS),
                           (abi.DeckWaveform, 1416, WAVE_OFFSETS)):
        assert C.sizeof(st) == size and {n: getattr(st, n).offset for n, _t in st._fields_} == offs
    assert (abi.WAVE_BANDS, abi.WAVE_ENVELOPE, abi.WAVE_MAX_GRIDS, abi.WAVE_MAX_MARKERS, abi.WAVE_MAX_RANGES, abi.WAVE_STRIP) == (0, 1, 16, 32, 8, wm.STRIP)


# ---- the setting rules, accepted at the bound and refused one past it ----
OK = Wave(64, 16, 0, 10)
G = Grid(0, 50 * Q, wc.WHITE)
CHECKS = [(OK, True),
          (OK._replace(w=2), True), (OK._replace(w=0), False), (OK._replace(w=3), False), (OK._replace(w=8192, fpp=1), True), (OK._replace(w=8194, fpp=1), False),
          (OK._replace(h=4), True), (OK._replace(h=2), False), (OK._replace(h=5), False), (OK._replace(h=4320), True), (OK._replace(h=4322), False),
          (OK._replace(first_frame=1 << 30), True), (OK._replace(first_frame=(1 << 30) + 1), False), (OK._replace(first_frame=-(1 << 30)), True),
          (OK._replace(first_frame=-(1 << 30) - 1), False),
          (OK._replace(fpp=1), True), (OK._replace(fpp=0), False), (OK._replace(w=1024, fpp=1 << 20), True), (OK._replace(w=2, fpp=(1 << 20) + 1), False),
          (OK._replace(w=1026, fpp=1 << 20), False), (OK._replace(w=8192, fpp=1 << 17), True), (OK._replace(w=8192, fpp=(1 << 17) + 1), False),
          (OK._replace(style=ENVELOPE), True), (OK._replace(style=2), False),
          (OK._replace(gain=(1 << 20, 0, 1 << 20)), True), (OK._replace(gain=((1 << 20) + 1, 0, 0)), False), (OK._replace(gain=(0, (1 << 20) + 1, 0)), False),
          (OK._replace(gain=(0, 0, (1 << 20) + 1)), False),
          (OK._replace(grids=(G,) * 16), True), (OK._replace(grids=(G,) * 17), False),
          (OK._replace(markers=(Marker(0, wc.CYAN),) * 32), True), (OK._replace(markers=(Marker(0, wc.CYAN),) * 33), False),
          (OK._replace(ranges=(Range(0, 1, wc.GREY),) * 8), True), (OK._replace(ranges=(Range(0, 1, wc.GREY),) * 9), False),
          (OK._replace(grids=(G._replace(period_q32=Q),)), True), (OK._replace(grids=(G._replace(period_q32=Q - 1),)), False),
          (OK._replace(grids=(G._replace(period_q32=1 << 56),)), True), (OK._replace(grids=(G._replace(period_q32=(1 << 56) + 1),)), False),
          (OK._replace(grids=(G._replace(first_q32=1 << 61),)), True), (OK._replace(grids=(G._replace(first_q32=(1 << 61) + 1),)), False),
          (OK._replace(grids=(G._replace(first_q32=-(1 << 61)),)), True), (OK._replace(grids=(G._replace(first_q32=-(1 << 61) - 1),)), False),
          (OK._replace(grids=(G._replace(from_q32=5, to_q32=5),)), True), (OK._replace(grids=(G._replace(from_q32=6, to_q32=5),)), False),
          (OK._replace(grids=(G._replace(from_q32=-(1 << 63), to_q32=(1 << 63) - 1),)), True),
          (OK._replace(grids=(G._replace(inset=8),)), True), (OK._replace(grids=(G._replace(inset=9),)), False), (OK._replace(grids=(G, G._replace(inset=9))), False),
          (OK._replace(markers=(Marker(0, wc.CYAN, 16),)), True), (OK._replace(markers=(Marker(0, wc.CYAN, 17),)), False), (OK._replace(markers=(Marker(0, wc.CYAN, 0),)), False),
          (OK._replace(markers=(Marker(-(1 << 63), wc.CYAN, 1), Marker((1 << 63) - 1, wc.CYAN, 1))), True),
          (OK._replace(ranges=(Range(7, 7, wc.GREY),)), True), (OK._replace(ranges=(Range(8, 7, wc.GREY),)), False),
          (OK._replace(ranges=(Range(-(1 << 63), (1 << 63) - 1, wc.GREY),)), True)]


def build_unchecked(p: Wave):
    """the struct of settings the Python helper itself would refuse (too many entries: the counts alone are set past the arrays)"""
    from mixlab_amd import deck
    cut = p._replace(grids=p.grids[:16], markers=p.markers[:32], ranges=p.ranges[:8])
    c = wc.abi_wave(cut)
    c.n_grids, c.n_markers, c.n_ranges = len(p.grids), len(p.markers), len(p.ranges)
    return c


@pytest.mark.parametrize("p,ok", CHECKS)
def test_waveform_check_at_the_boundaries(p, ok):
    from mixlab_amd import abi, deck
    rule = wm.check(p)
    assert (rule is None) == ok
    c = build_unchecked(p)
    if ok:
        deck.waveform_check(c)
    else:
        with pytest.raises(abi.MxError) as e:
            deck.waveform_check(c)
        assert e.value.code == abi.MX_ERR_INVALID and "deck waveform" in str(e.value) and rule in str(e.value), (rule, str(e.value))


def test_waveform_check_refuses_every_pad_and_ignores_entries_beyond_the_counts():
    from mixlab_amd import abi, deck
    full = OK._replace(grids=(G,), markers=(Marker(0, wc.CYAN),), ranges=(Range(0, 1, wc.GREY),))

    def pads(c):
        yield c, "_pad"
        for col in (c.bg, c.line, c.band[0], c.band[1], c.band[2], c.grid[0].colour, c.marker[0].colour, c.range[0].colour):
            yield col, "_pad"
        yield c.range[0], "_pad"
    n = len(list(pads(wc.abi_wave(full))))
    for k in range(n):
        c = wc.abi_wave(full)
        obj, field = list(pads(c))[k]
        setattr(obj, field, 1)
        with pytest.raises(abi.MxError) as e:
            deck.waveform_check(c)
        assert e.value.code == abi.MX_ERR_INVALID and "_pad" in str(e.value)
    c = wc.abi_wave(full)   # entries at index n_* and above are not looked at
    c.grid[1].grid.period_q32, c.grid[1].inset, c.grid[1].colour._pad = 0, 1000, 9
    c.marker[1].width, c.marker[1].colour._pad = 99, 9
    c.range[1].from_frame, c.range[1].to_frame, c.range[1]._pad = 5, 1, 9
    deck.waveform_check(c)
    assert abi.lib.mx_deck_waveform_check(None) == abi.MX_ERR_INVALID


def test_waveform_view():
    from mixlab_amd import abi, deck
    for pos, fpp, x in ((0, 1, 0), (5 * Q + 7, 100, 480), (-3 * Q - 1, 10, 2), (-1, 1, 0), ((1 << 30) * Q, 1 << 17, 8191), ((1 << 30) * Q, 1 << 20, 1024)):
        assert deck.waveform_view(pos, fpp, x) == wm.view(pos, fpp, x) == (pos >> 32) - x * fpp
    assert deck.waveform_view(-1, 1, 0) == -1                            # the shift is arithmetic
    assert deck.waveform_view((1 << 30) * Q + Q - 1, 1, 0) == 1 << 30    # at the bound
    for pos, fpp, x in ((0, 0, 0), (0, (1 << 20) + 1, 0), (0, 1, 8192), (((1 << 30) + 1) * Q, 1, 0), (0, 1 << 20, 1025), (-(1 << 62), 1, 1)):
        with pytest.raises(abi.MxError) as e:
            deck.waveform_view(pos, fpp, x)
        assert e.value.code == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_waveform_view(0, 1, 0, None) == abi.MX_ERR_INVALID


# ---- the host restatement against the model ----
@pytest.mark.parametrize("case", wc.CASES, ids=lambda c: c.name)
def test_waveform_host_equals_the_model_on_every_byte_and_leaves_the_room_beyond_alone(case):
    from mixlab_amd import deck
    p = wc.abi_wave(case.wave)
    w, h = case.wave.w, case.wave.h
    n = wc.track(case).shape[0]
    for ys, cs in ((w, w // 2), (w + 7, w // 2 + 3)):
        got = deck.waveform_host(wc.columns(case), case.settings.column, n, p, ys, cs, fill=0xA5)
        for name, g, want, vis in zip("YUV", got, wc.truth(case), (w, w // 2, w // 2)):
            assert np.array_equal(g[:, :vis], want), (case.name, name, np.argwhere(g[:, :vis] != want)[:4].tolist())
            assert (g[:, vis:] == 0xA5).all(), (case.name, name, "beyond the visible area")


def test_waveform_host_refusals():
    from mixlab_amd import abi, deck
    case = wc.BY_NAME["64 x 16"]
    cols, n = wc.columns(case), wc.track(case).shape[0]
    p = wc.abi_wave(case.wave)
    for call in (lambda: deck.waveform_host(cols[:-1], 64, n, p), lambda: deck.waveform_host(cols, 128, n, p), lambda: deck.waveform_host(cols, 96, n, p),
                 lambda: deck.waveform_host(cols, 64, n, p, y_stride=63), lambda: deck.waveform_host(cols, 64, n, p, c_stride=31),
                 lambda: deck.waveform_host(cols, 64, n, wc.abi_wave(case.wave._replace(fpp=0)))):
        with pytest.raises(abi.MxError) as e:
            call()
        assert e.value.code == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_debug_last_waveform(None) == abi.MX_ERR_INVALID


# ---- what the specification promises of any picture ----
def test_shifting_first_frame_by_fpp_shifts_the_picture_by_one_pixel_column():
    for name in ("130 x 34", "all limits at once: 16 grids, 32 markers, 8 ranges", "first_frame negative and no multiple of fpp, a marker left of it"):
        case = wc.BY_NAME[name]
        cols, n, p = wc.columns(case), wc.track(case).shape[0], case.wave
        wide = p._replace(w=p.w + 2)
        a = wm.render(cols, case.settings.column, n, wide)[0]
        b = wm.render(cols, case.settings.column, n, wide._replace(first_frame=p.first_frame + p.fpp))[0]
        assert np.array_equal(a[:, 1:], b[:, :-1]), name     # luma pixel for pixel (chroma pairs the columns anew)
        pix = lambda q: wm.render(cols, case.settings.column, n, q)   # noqa: E731
        two = pix(wide._replace(first_frame=p.first_frame + 2 * p.fpp))
        for k in range(3):
            assert np.array_equal(pix(wide)[k][:, (2 if k == 0 else 1):], two[k][:, :(-2 if k == 0 else -1)]), (name, k)   # by two columns: all three planes


def test_a_bands_picture_is_mirror_symmetric_where_no_grid_has_an_inset():
    seen = 0
    for case in wc.CASES:
        if case.wave.style == ENVELOPE or any(g.inset for g in case.wave.grids):
            continue
        seen += 1
        for plane in wc.truth(case):
            assert np.array_equal(plane, plane[::-1]), case.name
    assert seen >= 10


def test_zero_gain_leaves_background_line_and_overlays():
    case = wc.BY_NAME["gain 0 under grids, markers and ranges"]
    p = case.wave
    Y = wc.truth(case)[0]
    allowed = {p.bg[0], p.line[0]} | {g.colour[0] for g in p.grids} | {m.colour[0] for m in p.markers} | {r.colour[0] for r in p.ranges}
    assert set(np.unique(Y).tolist()) <= allowed and not {b[0] for b in p.band} & set(np.unique(Y).tolist())
    half = p.h // 2
    assert (Y[half - 1] == Y[half]).all() and {p.line[0]} <= set(Y[half].tolist())
    assert set(np.unique(Y[0]).tolist()) == allowed - {p.line[0]}


# ---- misreadings of the header ----
@pytest.mark.parametrize("mis", wm.MISREADINGS)
def test_the_shared_cases_tell_the_model_from_each_misreading(mis):
    hit = [c.name for c in wc.CASES
           if any((a != b).any() for a, b in zip(wm.render(wc.columns(c), c.settings.column, wc.track(c).shape[0], c.wave, (mis,)), wc.truth(c)))]
    assert hit, mis


def test_the_forms_of_the_shared_cases_cover_every_count():
    total = dict.fromkeys(("strips_single", "strips_several", "strips_outside", "max_records"), 0)
    for c in wc.CASES:
        for k, v in wm.forms(c.wave, c.settings.column, wc.track(c).shape[0]).items():
            total[k] += v
    assert all(v > 0 for v in total.values()), total
