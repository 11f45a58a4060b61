"""The placer's specification (include/mixlab_gpu.h mx_video_place) restated in numpy, written from the header text and not
from the kernel, plus the cases the CPU and GPU suites share.  The resampling itself is video_model.scale_plane, the pinned statement of section 6,
applied to the crop planes; this file cuts the crop, pastes the results into the canvas and fills the rest.  It shares nothing with the product.

`bug=` selects a deliberate MIS-model (tests/test_cpu_video_place.py shows each one changes a byte of a shared case: the cases can tell)."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

import video_model as vm

BUGS = ("clamp_plane", "tables_clipped", "chroma_offset_full", "cov_outside_255", "chroma_outside_0", "drop_last", "cov_chroma_tables",
        "neg_half_trunc", "v_before_h")


@dataclass(frozen=True)
class PlaceP:
    canvas_w: int
    canvas_h: int
    dst_x: int
    dst_y: int
    dst_w: int
    dst_h: int
    crop_x: int = 0
    crop_y: int = 0
    crop_w: int = 0      # 0 x 0: the whole frame
    crop_h: int = 0

    def but(self, **kw):
        return replace(self, **kw)

    def crop(self):
        return None if self.crop_w == 0 else (self.crop_x, self.crop_y, self.crop_w, self.crop_h)


def _resample_general(plane, x0, y0, cw, ch, dw, dh, clamp_plane=False, v_first=False):
    """The section-6 passes written out, for the mis-models only: the crop [x0, x0 + cw) x [y0, y0 + ch) of `plane` -> (dh, dw).  clamp_plane: tap indices
    clamp to the whole plane instead of the crop; v_first: the V pass runs first (with the H pass' rounding), then the H pass (with the V pass')."""
    p = np.asarray(plane, np.int64)
    hf, hc = vm.tap_tables(cw, dw)
    vf, vc = vm.tap_tables(ch, dh)
    ix = hf[:, None] + np.arange(hc.shape[1])[None, :]
    iy = vf[:, None] + np.arange(vc.shape[1])[None, :]
    if clamp_plane:
        ix, iy = np.clip(ix + x0, 0, p.shape[1] - 1), np.clip(iy + y0, 0, p.shape[0] - 1)
    else:
        ix, iy = np.clip(ix, 0, cw - 1) + x0, np.clip(iy, 0, ch - 1) + y0
    if not v_first:
        # H pass over every crop row -- and, where indices clamp to the plane, over the rows above and below the crop that the V taps then reach
        all_rows = np.arange(p.shape[0])
        t = vm.asr((p[all_rows][:, ix] * hc[None, :, :]).sum(axis=2) + vm.H_ROUND, vm.H_SHIFT)          # (H, dw)
        pre = vm.asr((t[iy] * vc[:, :, None]).sum(axis=1) + vm.V_ROUND, vm.V_SHIFT)                     # (dh, dw)
        return vm.clip8(pre).astype(np.uint8)
    t = vm.asr((p[iy] * vc[:, :, None]).sum(axis=1) + vm.H_ROUND, vm.H_SHIFT)                           # (dh, W)
    pre = vm.asr((t[:, ix] * hc[None, :, :]).sum(axis=2) + vm.V_ROUND, vm.V_SHIFT)
    return vm.clip8(pre).astype(np.uint8)


def _paste(canvas, S, ox, oy):
    """S into canvas with S's (0, 0) at canvas (ox, oy), clipped to the canvas"""
    H, W = canvas.shape
    h, w = S.shape
    x0, x1, y0, y1 = max(ox, 0), min(ox + w, W), max(oy, 0), min(oy + h, H)
    if x0 < x1 and y0 < y1:
        canvas[y0:y1, x0:x1] = S[y0 - oy:y1 - oy, x0 - ox:x1 - ox]


def place_model(y, u, v, p: PlaceP, a_in=None, bug=None):
    """(Y, U, V, coverage) of the canvas: the frame (y: (H, W), u / v: (H/2, W/2) uint8; a_in: (H, W) uint8 or None) placed under p"""
    y, u, v = (np.asarray(a, np.uint8) for a in (y, u, v))
    H, W = y.shape
    assert u.shape == (H // 2, W // 2) and v.shape == u.shape
    cx, cy, cw, ch = p.crop() or (0, 0, W, H)
    assert cx + cw <= W and cy + ch <= H and not any(n & 1 for n in (cx, cy, cw, ch, p.dst_x, p.dst_y, p.dst_w, p.dst_h, p.canvas_w, p.canvas_h))
    assert cw <= 32 * p.dst_w and ch <= 32 * p.dst_h
    Cw, Ch = p.canvas_w, p.canvas_h
    out_y = np.zeros((Ch, Cw), np.uint8)
    out_a = np.full((Ch, Cw), 255 if bug == "cov_outside_255" else 0, np.uint8)
    out_u = np.full((Ch // 2, Cw // 2), 0 if bug == "chroma_outside_0" else 0x80, np.uint8)
    out_v = out_u.copy()
    dx, dy, dw, dh = p.dst_x, p.dst_y, p.dst_w, p.dst_h
    if bug == "tables_clipped":   # the tables of the visible part of the rectangle
        x0, x1, y0, y1 = max(dx, 0), min(dx + dw, Cw), max(dy, 0), min(dy + dh, Ch)
        if x0 >= x1 or y0 >= y1:
            return out_y, out_u, out_v, out_a
        dx, dy, dw, dh = x0, y0, x1 - x0, y1 - y0

    def resample(plane, c, tables_c=None):
        """crop plane -> rectangle, both at subsampling c"""
        x0, y0, w, h, ow, oh = cx >> c, cy >> c, cw >> c, ch >> c, dw >> c, dh >> c
        if bug == "clamp_plane":
            return _resample_general(plane, x0, y0, w, h, ow, oh, clamp_plane=True)
        if bug == "v_before_h":
            return _resample_general(plane, x0, y0, w, h, ow, oh, v_first=True)
        return vm.scale_plane(plane[y0:y0 + h, x0:x0 + w], ow, oh)      # "exactly as section 6 resamples a frame that consisted of the crop alone"

    Sy, Su, Sv = resample(y, 0), resample(u, 1), resample(v, 1)
    if a_in is None:
        Sa = np.full((dh, dw), 255, np.uint8)
    elif bug == "cov_chroma_tables":   # the coverage taken at chroma resolution through the chroma tables, then doubled
        half = vm.scale_plane(np.asarray(a_in, np.uint8)[cy:cy + ch:2, cx:cx + cw:2], dw >> 1, dh >> 1)
        Sa = np.repeat(np.repeat(half, 2, axis=0), 2, axis=1)
    else:
        Sa = resample(np.asarray(a_in, np.uint8), 0)
    if bug == "drop_last":
        Sy, Sa, Su, Sv = Sy[:-1, :-1], Sa[:-1, :-1], Su[:-1, :-1], Sv[:-1, :-1]
    _paste(out_y, Sy, dx, dy)
    _paste(out_a, Sa, dx, dy)
    if bug == "chroma_offset_full":
        hx, hy = dx, dy
    elif bug == "neg_half_trunc":     # (d + 1) / 2 with C's division: right for d >= 0, one too far right / down for d < 0
        hx, hy = int((dx + 1) / 2), int((dy + 1) / 2)
    else:
        hx, hy = dx // 2, dy // 2     # even numbers: exact
    _paste(out_u, Su, hx, hy)
    _paste(out_v, Sv, hx, hy)
    return out_y, out_u, out_v, out_a


# ---- pictures and the shared cases ----
def noise_frame(w, h, seed, alpha):
    """-> (y, u, v, a or None): noise on every plane, so that a wrong tap, a wrong clamp or a shifted paste shows"""
    rng = np.random.default_rng(0x91AC + seed * 7919 + w * 131 + h)
    y = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    u = rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8)
    v = rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8)
    a = rng.integers(0, 256, size=(h, w)).astype(np.uint8) if alpha else None
    return y, u, v, a


@dataclass(frozen=True)
class Case:
    name: str
    src_w: int
    src_h: int
    alpha: bool
    p: PlaceP
    big: bool = False

    def frame(self):
        return noise_frame(self.src_w, self.src_h, sum(map(ord, self.name)), self.alpha)

    def want(self, bug=None):
        y, u, v, a = self.frame()
        return place_model(y, u, v, self.p, a, bug)


def cases(tile_w, tile_h, tap_bound):
    """The cases of both suites, placed around the kernel's exported tile size and tap bound (mixlab_amd.abi.PLACE_*; the CPU suite passes the same numbers)."""
    out = []
    k = [0]

    def add(name, sw, sh, p, big=False):
        k[0] += 1
        out.append(Case(name, sw, sh, k[0] % 2 == 0, p, big))

    def even(n):
        return max(2, int(n) & ~1)

    # canvases: the listed ones, the luma tile, and the chroma tile (twice the luma numbers): an inset, and a rectangle larger than the canvas clipped on all four sides
    canvases = [(2, 2), (34, 2), (2, 34), (66, 38), (130, 74), (322, 182)]
    canvases += [(tile_w + d, tile_h + d) for d in (-2, 0, 2)] + [(2 * tile_w + d, 2 * tile_h + d) for d in (-2, 0, 2)]
    for cw, ch in canvases:
        add(f"canvas{cw}x{ch}-inset", 34, 18, PlaceP(cw, ch, (cw // 4) & ~1, (ch // 4) & ~1, even(cw * 0.6), even(ch * 0.6)))
        add(f"canvas{cw}x{ch}-over", 34, 18, PlaceP(cw, ch, -4, -2, cw + 10, ch + 6))
        add(f"canvas{cw}x{ch}-full11", cw, ch, PlaceP(cw, ch, 0, 0, cw, ch))
    # geometries per axis (source samples -> rectangle samples), different ratios on the two axes; taps: 4 | 4 | 2 ceil(2 s / d) + 2
    below = (2 * (tap_bound - 2) // 4 - 1) * 8      # tap_bound 18: 56 -> 16 is 16 taps
    at = (tap_bound - 2) // 4 * 16                  # 64 -> 16: 18 taps, the bound
    above = at + 2                                  # 66 -> 16: 20 taps
    geo = {"one": (34, 34), "up": (6, 34), "mild": (34, 18), "down": (64, 16), "limit": (64, 2), "below": (below, 16), "at": (at, 16), "above": (above, 16)}
    pairs = [("one", "up"), ("up", "mild"), ("mild", "down"), ("down", "up"), ("below", "above"), ("above", "below"), ("at", "mild"), ("up", "at"),
             ("limit", "mild"), ("mild", "limit"), ("limit", "limit"), ("one", "one"), ("down", "down"), ("above", "above")]
    for hx, vx in pairs:
        (sw, dw), (sh, dh) = geo[hx], geo[vx]
        add(f"geo-{hx}-{vx}", sw + 6, sh + 8, PlaceP(130, 74, 10, 6, dw, dh, 2, 4, sw, sh))
        add(f"geo-{hx}-{vx}-clip", sw + 6, sh + 8, PlaceP(66, 38, -6, 38 - dh + 4 if dh > 8 else 36, dw, dh, 4, 2, sw, sh))
    # a wide rectangle under the bound: several tiles per row, every alignment of the window's first column
    add("geo-wide-at", 4 * 322 + 4, 40, PlaceP(322, 182, 2, 2, 318, 20, 2, 0, 4 * 318, 40))
    add("geo-wide-mild", 600, 100, PlaceP(322, 182, -20, -10, 340, 60, 6, 2, 590, 96))
    # crops: whole, interior, touching each corner (the right / bottom ones end at the frame's edge, next to the stride padding)
    for name, crop in (("whole", None), ("interior", (10, 6, 40, 20)), ("tl", (0, 0, 32, 18)), ("tr", (34, 0, 32, 18)), ("bl", (0, 20, 32, 18)), ("br", (34, 20, 32, 18))):
        c = crop or (0, 0, 0, 0)
        add(f"crop-{name}-up", 66, 38, PlaceP(66, 38, 8, 6, 48, 28, *c))
        add(f"crop-{name}-down", 66, 38, PlaceP(66, 38, 30, 20, 12, 8, *c))
    # positions of the rectangle on a 66 x 38 canvas, at 1:1 and scaled
    for tag, (dw, dh) in (("11", (34, 18)), ("sc", (40, 22))):
        pos = {"left": (-10, 8), "right": (66 - 20, 8), "top": (12, -6), "bottom": (12, 38 - 10), "touch-br": (66 - dw, 38 - dh), "touch-tl": (0, 0),
               "near-br": (66 - dw - 2, 38 - dh - 2), "near-tl": (2, 2), "out-right": (66, 4), "out-left": (-dw, 4), "out-below": (4, 38), "out-above": (4, -dh),
               "out-far": (2147483646, -2147483648), "corner": (-dw + 2, -dh + 2)}
        for name, (dx, dy) in pos.items():
            add(f"pos-{tag}-{name}", 34, 18, PlaceP(66, 38, dx, dy, dw, dh))
    # full size: the inset of the issue, and a zoom
    add("full-inset", 1920, 1080, PlaceP(1920, 1080, 1376, 64, 480, 270), big=True)
    add("full-zoom", 1920, 1080, PlaceP(1920, 1080, 0, 0, 1920, 1080, 600, 300, 640, 360), big=True)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out
