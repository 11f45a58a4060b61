"""The multiviewer's specification (include/mixlab_gpu.h mx_video_multiview) restated in numpy, written from the header text and not
from the kernel, plus the cases the CPU and GPU suites share.  The resampling itself is video_model.scale_plane, the pinned statement of section 6, applied to
the whole source planes; this file works out the rectangles, pastes the pictures and fills frames, blanks and background.  It shares nothing with the product:
the geometry rule (encode.rs:354-374) is restated here too.

`bug=` selects a deliberate MIS-model (tests/test_cpu_video_multiview.py shows each one changes a byte of a small shared case: the cases can tell)."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

import video_model as vm

BUGS = ("frame_outside", "geometry_from_rect", "bars_background", "chroma_offset_full", "chroma_border_full", "tables_of_inner", "coverage_applied",
        "letterbox_odd", "notshown_background", "clamp_stride")
MAX_VIEWS = 16


@dataclass(frozen=True)
class View:
    x: int
    y: int
    w: int
    h: int
    border: int = 0
    colour: tuple = (81, 90, 240)     # a red tally
    fit: int = 1

    def but(self, **kw):
        return replace(self, **kw)


@dataclass(frozen=True)
class MvP:
    canvas_w: int
    canvas_h: int
    views: tuple
    bg: tuple = (40, 120, 136)

    def but(self, **kw):
        return replace(self, **kw)


@dataclass
class Src:
    """A frame as the multiviewer meets it.  fmt "yuv420p": y (h, w), u / v (h/2, w/2) uint8 and a coverage plane a (h, w) or None; any other fmt: only the size."""
    w: int
    h: int
    y: np.ndarray = None
    u: np.ndarray = None
    v: np.ndarray = None
    a: np.ndarray = None
    fmt: str = "yuv420p"


def scale_geometry(in_w, in_h, out_w, out_h, even_offset=True):
    """The DynamicScaler's rule (encode.rs:354-374): the smaller of the two ratios, scaled size and letterbox offset rounded DOWN to even"""
    num, den = (out_w, in_w) if out_w * in_h <= out_h * in_w else (out_h, in_h)
    sw, sh = (num * in_w // den) & ~1, (num * in_h // den) & ~1
    lx, ly = (out_w - sw) // 2, (out_h - sh) // 2
    if even_offset:
        lx, ly = lx & ~1, ly & ~1
    return sw, sh, lx, ly


def view_geometry(v: View, f, bug=None):
    """-> (I, P): the inner and the picture rectangle (x, y, w, h) in luma samples; P None: the view is not shown"""
    b = v.border
    I = (v.x, v.y, v.w, v.h) if bug == "frame_outside" else (v.x + b, v.y + b, v.w - 2 * b, v.h - 2 * b)
    if f is None or f.fmt != "yuv420p":
        return I, None
    if v.fit:
        box = (v.x, v.y, v.w, v.h) if bug == "geometry_from_rect" else I
        sw, sh, lx, ly = scale_geometry(f.w, f.h, box[2], box[3], even_offset=bug != "letterbox_odd")
        P = (box[0] + lx, box[1] + ly, sw, sh)
    else:
        P = I
    if P[2] < 2 or P[3] < 2 or f.w > 32 * P[2] or f.h > 32 * P[3]:
        return I, None
    return I, P


def shown_mask(frames, p: MvP):
    return sum(1 << i for i, (v, f) in enumerate(zip(p.views, frames)) if view_geometry(v, f)[1] is not None)


def _fill(canvas, x, y, w, h, value):
    H, W = canvas.shape
    x0, x1, y0, y1 = max(x, 0), min(x + w, W), max(y, 0), min(y + h, H)
    if x0 < x1 and y0 < y1:
        canvas[y0:y1, x0:x1] = value


def _paste(canvas, S, ox, oy):
    H, W = canvas.shape
    h, w = S.shape
    x0, x1, y0, y1 = max(ox, 0), min(ox + w, W), max(oy, 0), min(oy + h, H)
    if x0 < x1 and y0 < y1:
        canvas[y0:y1, x0:x1] = S[y0 - oy:y1 - oy, x0 - ox:x1 - ox]


def _padded(plane, seed):
    """the plane as it lies in memory: rows 64-byte aligned, the padding holding noise"""
    h, w = plane.shape
    stride = (w + 63) & ~63
    out = np.random.default_rng(seed).integers(0, 256, size=(h, stride)).astype(np.uint8)
    out[:, :w] = plane
    return out


def multiview_model(frames, p: MvP, bug=None):
    """(Y, U, V) of the canvas: frames[i] (a Src or None) in view i of p"""
    assert 1 <= len(p.views) <= MAX_VIEWS and len(frames) == len(p.views)
    out = []
    done = {}   # a source shown in several views of one size is resampled once

    def scaled(plane, pw, ph):
        key = (id(plane), pw, ph)
        if key not in done:
            done[key] = vm.scale_plane(plane, pw, ph)                  # "the WHOLE source plane resampled to P.w x P.h", tables of the plane's own size
        return done[key]
    for k in range(3):
        c = 1 if k else 0
        canvas = np.full((p.canvas_h >> c, p.canvas_w >> c), p.bg[k], np.uint8)
        blank = 0x80 if c else 0
        for v, f in zip(p.views, frames):
            I, P = view_geometry(v, f, bug)
            if P is None and bug == "notshown_background":
                continue
            co = 0 if (c and bug == "chroma_offset_full") else c       # the shift of positions
            cb = 0 if (c and bug == "chroma_border_full") else c       # the shift of the frame's thickness
            rx, ry, rw, rh, bt = v.x >> co, v.y >> co, v.w >> c, v.h >> c, v.border >> cb
            if bug == "frame_outside":
                _fill(canvas, rx - bt, ry - bt, rw + 2 * bt, rh + 2 * bt, v.colour[k])
                inner = (rx, ry, rw, rh)
            else:
                _fill(canvas, rx, ry, rw, rh, v.colour[k])
                inner = (rx + bt, ry + bt, rw - 2 * bt, rh - 2 * bt)
            _fill(canvas, *inner, p.bg[k] if (bug == "bars_background" and P is not None) else blank)
            if P is None:
                continue
            plane = (f.y, f.u, f.v)[k]
            pw, ph = P[2] >> c, P[3] >> c
            if bug == "tables_of_inner" and v.fit:
                S = vm.scale_plane(plane, max(I[2] >> c, pw), max(I[3] >> c, ph))[:ph, :pw]
            elif bug == "clamp_stride":
                S = vm.scale_plane(_padded(plane, 5 + k), pw, ph, src_size=plane.shape)
            else:
                S = scaled(plane, pw, ph)
            if bug == "coverage_applied" and f.a is not None:
                Sa = vm.scale_plane(f.a[::2, ::2] if c else f.a, pw, ph).astype(np.int64)
                S = ((S.astype(np.int64) - blank) * Sa // 255 + blank).astype(np.uint8)
            _paste(canvas, S, P[0] >> co, P[1] >> co)
        out.append(canvas)
    return out


# ---- pictures and the shared cases ----
def noise_src(w, h, seed, alpha=False):
    rng = np.random.default_rng(0x3A17 + seed * 7919 + w * 131 + h)
    y = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    u = rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8)
    v = rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8)
    a = rng.integers(0, 256, size=(h, w)).astype(np.uint8) if alpha else None
    return Src(w, h, y, u, v, a)


@dataclass(frozen=True)
class Case:
    name: str
    p: MvP
    sources: tuple        # per view: (w, h, alpha, seed) -- noise; None -- no frame; ("nv12", w, h) -- a frame of another format
    big: bool = False

    def frames(self):
        made = {}
        out = []
        for s in self.sources:
            if s is None:
                out.append(None)
            elif s[0] == "nv12":
                out.append(Src(s[1], s[2], fmt="nv12"))
            else:
                if s not in made:
                    made[s] = noise_src(s[0], s[1], s[3] + sum(map(ord, self.name)) % 97, s[2])
                out.append(made[s])
        return out

    def want(self, bug=None):
        return multiview_model(self.frames(), self.p, bug)


RED, GREEN, WHITE = (81, 90, 240), (145, 54, 34), (235, 128, 128)


def cases(tile_w, tile_h, tap_bound):
    """The cases of both suites, placed around the kernel's exported tile size and tap bound (mixlab_amd.abi.MULTIVIEW_*; the CPU suite passes the same numbers)."""
    out = []
    k = [0]

    def add(name, p, sources, big=False):
        k[0] += 1
        srcs = []
        for i, s in enumerate(sources):
            if s is None or s[0] == "nv12":
                srcs.append(s)
            else:   # (w, h) or (w, h, seed): every other source carries a coverage plane holding noise
                srcs.append((s[0], s[1], (k[0] + i) % 2 == 0, s[2] if len(s) > 2 else i))
        assert len(srcs) == len(p.views)
        out.append(Case(name, p, tuple(srcs), big))

    # canvases: one view with a frame, the picture fitted; the luma tile and the chroma tile (twice the luma numbers)
    add("canvas2x2", MvP(2, 2, (View(0, 0, 2, 2, 0, RED, 0),)), [(6, 4)])
    canvases = [(34, 18), (66, 38), (130, 74)] + [(tile_w + d, tile_h + d) for d in (-2, 0, 2)] + [(2 * tile_w + d, 2 * tile_h + d) for d in (-2, 0, 2)]
    for cw, ch in canvases:
        add(f"canvas{cw}x{ch}-inset", MvP(cw, ch, (View(2, 2, cw - 4, ch - 4, 2, RED, 1),)), [(34, 18)])
        add(f"canvas{cw}x{ch}-full", MvP(cw, ch, (View(0, 0, cw, ch, 0, RED, 0),)), [(cw, ch)])
    # view edges inside one kernel tile (luma tile 0 is columns 0 .. tile_w - 1, rows 0 .. tile_h - 1; the chroma tile covers twice that in luma numbers)
    add("two-h", MvP(130, 74, (View(4, 2, 16, 10, 2, RED, 0), View(20, 2, 30, 10, 2, GREEN, 1))), [(34, 18), (16, 10)])
    add("two-v", MvP(130, 74, (View(4, 0, 40, 6, 0, RED, 0), View(4, 6, 40, 8, 2, GREEN, 0))), [(34, 18), (66, 38)])
    add("four-point", MvP(130, 74, (View(0, 0, 20, 6, 2, RED, 0), View(20, 0, 24, 6, 0, GREEN, 1), View(0, 6, 20, 8, 2, WHITE, 1), View(20, 6, 24, 8, 2, RED, 0))),
        [(34, 18), (16, 10), (66, 38), (20, 40)])
    sizes = [(34, 18), (66, 38), (16, 10), (130, 74), (20, 40)]
    grid = tuple(View(32 * (i % 4), 18 * (i // 4), 32, 18, (0, 2, 4)[i % 3], (RED, GREEN, WHITE)[i % 3], i % 2) for i in range(16))
    add("grid16", MvP(130, 74, grid), [sizes[i % 5] + (i % 7,) for i in range(16)])
    # borders: none, 2, and the most that still leaves a 2 x 2 inner rectangle (of a small view, and the parameter's maximum)
    for b in (0, 2, 8):
        add(f"border{b}", MvP(130, 74, (View(4, 2, 18, 18, b, GREEN, 0),)), [(34, 18)])
    add("border64", MvP(130, 130, (View(0, 0, 130, 130, 64, GREEN, 0),)), [(34, 18)])
    # fit: sources wider and taller than the view's aspect, stretched and fitted; offsets whose half is odd before it is rounded down to even
    for fit in (0, 1):
        add(f"fit{fit}-wide", MvP(130, 74, (View(10, 6, 44, 30, 2, RED, fit),)), [(66, 18)])
        add(f"fit{fit}-tall", MvP(130, 74, (View(10, 6, 44, 30, 2, RED, fit),)), [(20, 40)])
        add(f"fit{fit}-odd", MvP(130, 74, (View(10, 6, 32, 18, 2, GREEN, fit), View(50, 6, 18, 34, 2, RED, fit))), [(16, 10), (34, 18)])
    # geometries per axis (source samples -> picture samples), stretched; taps: 4 | 4 | 2 ceil(2 s / d) + 2
    at = 4 * (tap_bound - 2)                        # s -> 16 is 2 ceil(s / 8) + 2 taps: tap_bound 20: 72 -> 16 is 20 taps, the bound
    below = at - 8                                  # 64 -> 16: 18 taps
    above = at + 2                                  # 74 -> 16: 22 taps: the gather form
    geo = {"one": (34, 34), "up": (6, 34), "mild": (34, 18), "limit": (64, 2), "below": (below, 16), "at": (at, 16), "above": (above, 16)}
    pairs = [("one", "up"), ("up", "mild"), ("mild", "at"), ("at", "up"), ("below", "above"), ("above", "below"), ("at", "at"), ("limit", "mild"), ("mild", "limit"),
             ("limit", "limit"), ("one", "one"), ("above", "above")]
    for hx, vx in pairs:
        (sw, dw), (sh, dh) = geo[hx], geo[vx]
        add(f"geo-{hx}-{vx}", MvP(130, 74, (View(10, 6, dw + 4, dh + 4, 2, RED, 0), View(60, 40, 30, 20, 2, GREEN, 1))), [(sw, sh), (34, 18)])
    # several tiles of a row, every alignment of the window's first column; the inner rectangle's rows are exactly one tile row.  At the bound on both axes a full
    # tile's window (15 x 4.5 + 20 rows) is more than the kernel stages: the per-tile test sends it to the gather form.  The last case is the largest window that is
    # staged: 4.2:1, 20 taps, full tiles
    add("geo-wide-at", MvP(2 * tile_w + 6, 74, (View(2, tile_h - 2, 2 * tile_w, tile_h + 4, 2, RED, 0),)), [((2 * tile_w - 4) * at // 16 & ~1, at)])
    add("geo-wide-below", MvP(2 * tile_w + 6, 74, (View(2, tile_h - 2, 2 * tile_w, tile_h + 4, 2, RED, 0),)), [((2 * tile_w - 4) * 4, 64)])
    add("geo-full-window", MvP(2 * tile_w + 6, 74, (View(2, tile_h - 2, 2 * tile_w + 4, 2 * tile_h + 4, 2, RED, 0),)), [((2 * tile_w * 21 // 5 + 1) & ~1, (2 * tile_h * 21 // 5 + 1) & ~1)])
    # a view made not shown by each of the four conditions, beside one that is shown
    ok = View(60, 40, 30, 20, 2, GREEN, 1)
    add("notshown-none", MvP(130, 74, (View(10, 6, 24, 14, 2, RED, 1), ok)), [None, (34, 18)])
    add("notshown-format", MvP(130, 74, (View(10, 6, 24, 14, 2, RED, 1), ok)), [("nv12", 34, 18), (34, 18)])
    add("notshown-thin", MvP(130, 74, (View(10, 6, 24, 14, 2, RED, 1), ok)), [(200, 2), (34, 18)])           # fitted: 20 x 0
    add("notshown-ratio", MvP(130, 74, (View(10, 6, 6, 14, 2, RED, 0), ok)), [(66, 18), (34, 18)])           # 66 > 32 x 2
    add("notshown-all", MvP(66, 38, (View(10, 6, 24, 14, 2, RED, 1),)), [None])
    # views touching every edge and corner of the canvas
    W, H = 66, 38
    add("corners", MvP(W, H, (View(0, 0, 20, 12, 2, RED, 1), View(W - 20, 0, 20, 12, 2, GREEN, 0), View(0, H - 12, 20, 12, 0, WHITE, 1), View(W - 20, H - 12, 20, 12, 2, RED, 0))),
        [(34, 18), (16, 10), (66, 38), (20, 40)])
    add("edges", MvP(W, H, (View(24, 0, 18, 10, 2, RED, 1), View(24, H - 10, 18, 10, 2, GREEN, 0), View(0, 14, 12, 10, 0, WHITE, 1), View(W - 12, 14, 12, 10, 2, RED, 0))),
        [(34, 18), (16, 10), (66, 38), (20, 40)])
    # full size: a 2 x 2 of four distinct 1080p sources, and the same four repeated as a 4 x 4
    for n in (2, 4):
        vw, vh = 1920 // n, 1080 // n & ~1
        views = tuple(View(vw * (i % n), vh * (i // n), vw, vh, 4, (RED, GREEN, WHITE)[i % 3], 1) for i in range(n * n))
        add(f"full-{n}x{n}", MvP(1920, 1080, views), [(1920, 1080, i % 4) for i in range(n * n)], big=True)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
