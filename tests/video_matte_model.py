"""The matte refiner's specification (include/mixlab_gpu.h mx_video_matte) restated in numpy, written from the text and not from the
kernel, plus the pictures and the named settings the CPU and GPU suites share.  Integer arithmetic on int64, `//` of non-negative values (the header's `/`).

`bug=` selects a deliberate MIS-model (tests/test_cpu_video_matte.py shows each one differs from the model on the shared pictures: the pictures can tell).
"Clean after choke" is not among them: CLEAN is a non-decreasing map of the sample, so it commutes with a minimum and with a maximum and the two orders give the
same bytes; cleaning LAST, behind the binomial, does not commute and is listed ("clean_last")."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace

import numpy as np

import video_key_model as km

CLEAN, CHOKE, SOFTEN, MASK = 1, 2, 4, 8
RECT, CIRCLE = 0, 1
WIPE_LEFT, WIPE_TOP, WIPE_BOX, WIPE_IRIS = 0, 1, 2, 3
BUGS = ("edge_zero", "edge_wrap", "choke_sign", "choke_cross", "soften_round_first", "soften_no_round", "soften_box", "soften_before_choke",
        "clean_last", "clean_round", "mask_round", "centre_0", "sqrt_round", "feather_order", "invert_after")


@dataclass(frozen=True)
class MatteP:
    clean: tuple | None = None    # (black, white)
    choke: int = 0                # 0: the stage is off
    soften: int = 0               # 0: the stage is off
    mask: tuple | None = None     # (x0, y0, x1, y1) in Q4: a rectangle's edges, or a circle's centre, radius and 0
    shape: int = RECT
    invert: int = 0
    feather: int = 0

    def but(self, **kw):
        return replace(self, **kw)

    @property
    def flags(self):
        return (CLEAN if self.clean is not None else 0) | (CHOKE if self.choke else 0) | (SOFTEN if self.soften else 0) | (MASK if self.mask is not None else 0)


# ---- the stages ----
def clean(a, black, white, bug=None):
    a = np.asarray(a, np.int64)
    span = max(1, white - black)
    mid = ((a - black) * 255 + (span // 2 if bug == "clean_round" else 0)) // span
    return np.where(a <= black, 0, np.where(a >= white, 255, mid))


def _tap(a, k, axis, bug=None):
    """b[t] = a[cl(t + k, n)] along `axis` (the mis-models: a zero beyond the plane, or the index wrapped)"""
    n = a.shape[axis]
    t = np.arange(n) + k
    if bug == "edge_wrap":
        return np.take(a, t % n, axis=axis)
    b = np.take(a, np.clip(t, 0, n - 1), axis=axis)
    if bug == "edge_zero":
        gone = (t < 0) | (t >= n)
        b = np.where(gone[None, :] if axis == 1 else gone[:, None], 0, b)
    return b


def choke(a, c, bug=None):
    """the minimum (c > 0) or maximum (c < 0) over the square |i|, |j| <= |c|, clamped to the plane: the square separates into a row and a column pass exactly"""
    a = np.asarray(a, np.int64)
    r = abs(c)
    pick = np.minimum if (c > 0) != (bug == "choke_sign") else np.maximum
    if bug == "choke_cross":   # |i| + |j| <= r ... the plus-shaped element: the row's window and the column's, not their product
        rows = functools.reduce(pick, [_tap(a, k, 1) for k in range(-r, r + 1)])
        cols = functools.reduce(pick, [_tap(a, k, 0) for k in range(-r, r + 1)])
        return pick(rows, cols)
    rows = functools.reduce(pick, [_tap(a, k, 1, bug) for k in range(-r, r + 1)])
    return functools.reduce(pick, [_tap(rows, k, 0, bug) for k in range(-r, r + 1)])


def binomial(s):
    return [math.comb(2 * s, k + s) for k in range(-s, s + 1)]


def soften(a, s, bug=None):
    """(sum_j sum_i b[j] b[i] a(cl(x + i), cl(y + j)) + 2^(4s - 1)) >> 4s: the double sum separates exactly (integers, no rounding between the passes)"""
    a = np.asarray(a, np.int64)
    if bug == "soften_box":
        n = 2 * s + 1
        rows = sum(_tap(a, k, 1) for k in range(-s, s + 1))
        return (sum(_tap(rows, k, 0) for k in range(-s, s + 1)) + n * n // 2) // (n * n)
    b = binomial(s)
    rows = sum(w * _tap(a, k, 1, bug) for w, k in zip(b, range(-s, s + 1)))
    if bug == "soften_round_first":
        rows = (rows + (1 << (2 * s - 1))) >> (2 * s)
        return (sum(w * _tap(rows, k, 0) for w, k in zip(b, range(-s, s + 1))) + (1 << (2 * s - 1))) >> (2 * s)
    total = sum(w * _tap(rows, k, 0, bug) for w, k in zip(b, range(-s, s + 1)))
    return (total + (0 if bug == "soften_no_round" else 1 << (4 * s - 1))) >> (4 * s)


def isqrt(x, bug=None):
    """the exact floor of the root of int64 x < 2^53: f64 holds x exactly, the estimate is then corrected in integers"""
    x = np.asarray(x, np.int64)
    if bug == "sqrt_round":
        return np.rint(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > x, r - 1, r)
    return np.where((r + 1) * (r + 1) <= x, r + 1, r)


def mask_plane(w, h, p: MatteP, bug=None):
    """m per luma sample, before the product (the inversion applied)"""
    c = 0 if bug == "centre_0" else 8
    px = (16 * np.arange(w, dtype=np.int64) + c)[None, :]
    py = (16 * np.arange(h, dtype=np.int64) + c)[:, None]
    x0, y0, x1, y1 = (int(t) for t in p.mask)
    if p.shape == RECT:
        d = np.minimum(np.minimum(px - x0, x1 - px), np.minimum(py - y0, y1 - py))
    else:
        d = x1 - isqrt((px - x0) ** 2 + (py - y0) ** 2, bug)
    f = p.feather
    mid = (d * 255) // max(1, f)
    if bug == "feather_order":
        m = np.where(d >= f, 255, np.where(d <= 0, 0, mid))
    else:
        m = np.where(d <= 0, 0, np.where(d >= f, 255, mid))
    return 255 - m if (p.invert and bug != "invert_after") else m


def matte_plane(a_in, p: MatteP, bug=None):
    """the refined coverage plane of the (H, W) plane a_in under p"""
    a = np.asarray(a_in, np.uint8).astype(np.int64)
    h, w = a.shape
    if p.clean is not None and bug != "clean_last":
        a = clean(a, *p.clean, bug=bug)
    if bug == "soften_before_choke" and p.soften:
        a = soften(a, p.soften)
    if p.choke:
        a = choke(a, p.choke, bug)
    if p.soften and bug != "soften_before_choke":
        a = soften(a, p.soften, bug)
    if p.clean is not None and bug == "clean_last":
        a = clean(a, *p.clean)
    if p.mask is not None:
        m = mask_plane(w, h, p, bug)
        a = (a * m + (127 if bug == "mask_round" else 0)) // 255
        if p.invert and bug == "invert_after":
            a = 255 - a
    assert a.min() >= 0 and a.max() <= 255
    return a.astype(np.uint8)


def matte_model(y, u, v, p: MatteP, a_in=None, bug=None):
    """(Y, U, V, coverage) of the frame under p: the picture copied, the coverage refined; a_in None is 255 everywhere"""
    y = np.asarray(y, np.uint8)
    a = np.full(y.shape, 255, np.uint8) if a_in is None else a_in
    return y.copy(), np.asarray(u, np.uint8).copy(), np.asarray(v, np.uint8).copy(), matte_plane(a, p, bug)


def wipe(kind, pos, f, w, h) -> MatteP:
    """mx_video_matte_wipe's formulas on Python integers"""
    B = 1 << 20
    if kind == WIPE_LEFT:
        return MatteP(mask=(-B, -B, (pos * (16 * w + f)) >> 16, B), feather=f)
    if kind == WIPE_TOP:
        return MatteP(mask=(-B, -B, B, (pos * (16 * h + f)) >> 16), feather=f)
    if kind == WIPE_BOX:
        hx, hy = (pos * (8 * w + f)) >> 16, (pos * (8 * h + f)) >> 16
        return MatteP(mask=(8 * w - hx, 8 * h - hy, 8 * w + hx, 8 * h + hy), feather=f)
    return MatteP(mask=(8 * w, 8 * h, (pos * (math.isqrt((8 * w) ** 2 + (8 * h) ** 2) + 1 + f)) >> 16, 0), shape=CIRCLE, feather=f)


# ---- the named settings: every stage alone, the radii's ends, the full halo, all four stages, both shapes hard / feathered / inverted, off-frame shapes ----
def settings(w, h):
    rect = (16 * (w // 4) + 4, 16 * (h // 4) + 4, 16 * (3 * w // 4) + 4, 16 * (3 * h // 4) + 12)   # edges 4 / 12 sixteenths into a sample: its centre decides
    circ = (8 * w + 3, 8 * h - 5, 16 * (min(w, h) // 3) + 7, 0)
    return {
        "none": MatteP(),
        "clean": MatteP(clean=(40, 200)),
        "clean-hard": MatteP(clean=(128, 128)),
        "choke+1": MatteP(choke=1), "choke-1": MatteP(choke=-1), "choke+6": MatteP(choke=6), "choke-6": MatteP(choke=-6),
        "soften1": MatteP(soften=1), "soften6": MatteP(soften=6),
        "choke6-soften6": MatteP(choke=6, soften=6),
        "grow6-soften6": MatteP(choke=-6, soften=6),
        "rect-hard": MatteP(mask=rect),
        "rect-feather-invert": MatteP(mask=rect, feather=16 * 3 + 5, invert=1),
        "circle-hard": MatteP(mask=circ, shape=CIRCLE),
        "circle-feather": MatteP(mask=circ, shape=CIRCLE, feather=16 * 5 + 3),
        "circle-hard-invert": MatteP(mask=circ, shape=CIRCLE, invert=1),
        "rect-outside": MatteP(mask=(16 * w + 160, 16 * h + 160, 16 * w + 320, 16 * h + 320), feather=40),
        "rect-outside-invert": MatteP(mask=(-(1 << 20), -(1 << 20), -100, -100), invert=1),
        "circle-centred-off-frame": MatteP(mask=(-8 * w, -(16 * h) // 3, 16 * w + 9, 0), shape=CIRCLE, feather=16 * 4 + 1),
        "all-circle": MatteP(clean=(30, 220), choke=2, soften=2, mask=circ, shape=CIRCLE, feather=16 * 5 + 3),
        "all-rect": MatteP(clean=(60, 180), choke=-1, soften=3, mask=rect, feather=16 * 2 + 9, invert=1),
        "clean-choke2-soften2": MatteP(clean=(30, 220), choke=2, soften=2),
    }


BIG = ("all-circle", "choke6-soften6", "rect-feather-invert")   # the three settings of the 1920 x 1080 frame: halo 4 with everything on, the full halo, the streaming form


# ---- pictures ----
@functools.lru_cache(maxsize=None)
def _keyed(w, h, seed):
    y, u, v = km.green_screen(w, h, seed=seed)
    k = km.key_model(y, u, v, km.DEFAULT_CHROMA)[3]
    for arr in (y, u, v, k):
        arr.setflags(write=False)
    return y, u, v, k


def keyed_picture(w, h, seed=1):
    """(y, u, v, coverage): video_key_model.green_screen keyed by key_model under DEFAULT_CHROMA -- the realistic plane: a soft-edged disc over a noisy backing"""
    return _keyed(w, h, seed)


def speck_plane(w, h, seed=0):
    """A coverage plane that exists to separate misreadings: a hard 255 | 0 edge that walks right in a staircase, isolated 0 and 255 specks on either side, a
    one-sample row line and a two-sample column line that flip what they cross, and a border whose diagonal ramp reaches all four edges and corners (0 in the
    top-left corner, 255 in the bottom-right)."""
    rng = np.random.default_rng(0x3A77E + seed * 131 + w * 7 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.where(xx < w // 2 + 2 * ((yy // 4) % 4) - 3, 255, 0).astype(np.int64)
    flip = rng.random((h, w)) < 1.0 / 61.0
    a = np.where(flip, 255 - a, a)                                     # specks
    if h >= 8:
        a[h // 3, :] = 255 - a[h // 3, :]                               # a one-sample line
    if w >= 8:
        a[:, w // 4:w // 4 + 2] = 255 - a[:, w // 4:w // 4 + 2]         # a two-sample line
    b = max(1, min(w, h) // 8)
    border = (xx < b) | (xx >= w - b) | (yy < b) | (yy >= h - b)
    ramp = ((xx * 7 + yy * 13) * 255) // max(1, 7 * (w - 1) + 13 * (h - 1))
    return np.where(border, ramp, a).astype(np.uint8)
