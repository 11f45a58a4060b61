"""Numpy model of the colour corrector, written from the text in include/mixlab_gpu.h (mx_video_grade) alone: a luma curve, a Q12 chroma matrix and a tetrahedral
3D LUT over yuv420p planes, integers throughout.  `variant` names a MISREADING of that text (VARIANTS): the tests show that each changes a byte of the shared
pictures, so the pictures can tell the specification from its neighbours."""
from __future__ import annotations

from dataclasses import dataclass, field, replace

import numpy as np

CURVE, CHROMA, LUT = 1, 2, 4
VARIANTS = ("trilinear", "ascending", "axes_permuted", "chroma_cosited", "mean_before_curve", "no_plus2", "no_lut_rounding", "chroma_trunc_div",
            "neighbour_chroma", "clamp_4095", "lut_first")


@dataclass(frozen=True)
class GradeP:
    flags: int = 0
    curve: np.ndarray = field(default_factory=lambda: np.arange(256, dtype=np.uint8))
    m: tuple = (4096, 0, 0, 4096)      # m_uu, m_uv, m_vu, m_vv
    off: tuple = (0, 0)                # off_u, off_v
    k: int = 0                         # lattice_log2 (LUT bit only)
    nodes: np.ndarray | None = None    # [N][N][N][3] uint16, Q4

    def but(self, **kw):
        return replace(self, **kw)


def identity_lattice(k: int) -> np.ndarray:
    n, step = (1 << k) + 1, 16 << (8 - k)
    i = np.arange(n, dtype=np.int64) * step
    out = np.empty((n, n, n, 3), np.uint16)
    out[..., 0] = i[:, None, None]; out[..., 1] = i[None, :, None]; out[..., 2] = i[None, None, :]
    return out


def random_lattice(k: int, seed: int) -> np.ndarray:
    """every value uniform in 0 .. 4096, then an eighth of the nodes' values forced to 0 and an eighth to 4096: both ends are met all over the cube"""
    rng = np.random.default_rng(0x6AADE + 31 * seed + k)
    n = (1 << k) + 1
    out = rng.integers(0, 4097, size=(n, n, n, 3)).astype(np.uint16)
    pick = rng.integers(0, 8, size=out.shape)
    out[pick == 0] = 0
    out[pick == 1] = 4096
    return out


def smooth_lattice(k: int) -> np.ndarray:
    """a lattice a colourist could have made: lifted blacks, a warm tint growing with luma, saturation falling towards the highlights -- and a ceiling of exactly 4096"""
    n, s = (1 << k) + 1, 1 << (8 - k)
    g = np.arange(n, dtype=np.float64) * s
    Y, U, V = np.meshgrid(g, g, g, indexing="ij")
    sat = 1.3 - 0.5 * Y / 256.0
    y2 = 256.0 * (Y / 256.0) ** 0.8 + 6.0
    u2 = 128.0 + (U - 128.0) * sat - 0.06 * Y
    v2 = 128.0 + (V - 128.0) * sat + 0.09 * Y
    out = np.stack([y2, u2, v2], axis=-1)
    return np.clip(np.rint(out * 16.0), 0, 4096).astype(np.uint16)


def lut_eval(nodes: np.ndarray, k: int, a, b, c, variant: str | None = None, tie: str = "first") -> np.ndarray:
    """[..., 3]: (Y', U', V') of the lattice at (a, b, c), arrays of one shape holding 0 .. 255.  tie: which axis goes first among equal fractions ("first": the lower
    axis, "last": the higher) -- the header says it cannot matter."""
    sh = 8 - k; S = 1 << sh
    shape = np.shape(a)
    v = np.stack([np.asarray(x, np.int64).ravel() for x in (a, b, c)])           # [3][n]
    if variant == "axes_permuted":
        v = v[[1, 2, 0]]
    nd = nodes.astype(np.int64)
    if variant == "clamp_4095":
        nd = np.minimum(nd, 4095)
    cell, f = v >> sh, v & (S - 1)
    if variant == "trilinear":
        acc = np.zeros((v.shape[1], 3), np.int64)
        for corner in range(8):
            d = np.array([(corner >> 2) & 1, (corner >> 1) & 1, corner & 1])[:, None]
            wgt = np.prod(np.where(d == 1, f, S - f), axis=0)
            p = cell + d
            acc += wgt[:, None] * nd[p[0], p[1], p[2]]
        return np.minimum(255, (acc + 8 * S * S * S) >> (3 * sh + 4)).reshape(shape + (3,))
    axis = np.arange(3)[:, None]
    key = -f * 4 + (axis if tie == "first" else 2 - axis)                        # descending fraction; ties by axis number
    order = np.argsort(key, axis=0)                                               # order[0]: the axis of f1
    fs = np.take_along_axis(f, order, axis=0)                                     # f1 >= f2 >= f3
    walk = order[::-1] if variant == "ascending" else order
    w = [S - fs[0], fs[0] - fs[1], fs[1] - fs[2], fs[2]]
    cur = cell.copy()
    acc = w[0][:, None] * nd[cur[0], cur[1], cur[2]]
    for step in range(3):
        cur = cur + (axis == walk[step][None, :])
        acc = acc + w[step + 1][:, None] * nd[cur[0], cur[1], cur[2]]
    assert acc.max(initial=0) <= 65536
    r = (acc + (0 if variant == "no_lut_rounding" else 8 * S)) >> (sh + 4)
    return np.minimum(255, r).reshape(shape + (3,))


def _chroma_stage(u, v, p: GradeP, variant):
    if not p.flags & CHROMA:
        return u.astype(np.int64), v.astype(np.int64), None
    du, dv = u.astype(np.int64) - 128, v.astype(np.int64) - 128
    su = p.m[0] * du + p.m[1] * dv + p.off[0] + 2048
    sv = p.m[2] * du + p.m[3] * dv + p.off[1] + 2048
    if variant == "chroma_trunc_div":
        qu, qv = np.trunc(su / 4096.0).astype(np.int64), np.trunc(sv / 4096.0).astype(np.int64)
    else:
        qu, qv = su >> 12, sv >> 12                                               # numpy's >> on int64 is the arithmetic shift
    return np.clip(128 + qu, 0, 255), np.clip(128 + qv, 0, 255), (su, sv, 128 + qu, 128 + qv)


def stages(y, u, v, p: GradeP, variant=None):
    """the intermediate values: y1 [H][W], u1 / v1 [H/2][W/2], the block mean ym, and the chroma stage's pre-shift sums / unclipped values (None without the bit)"""
    y = np.asarray(y); u = np.asarray(u); v = np.asarray(v)
    assert y.shape[0] % 2 == 0 and y.shape[1] % 2 == 0 and u.shape == v.shape == (y.shape[0] // 2, y.shape[1] // 2)
    curve = np.asarray(p.curve, np.uint8).astype(np.int64)
    y1 = curve[y] if p.flags & CURVE else y.astype(np.int64)
    u1, v1, raw = _chroma_stage(u, v, p, variant)
    src = y.astype(np.int64) if variant == "mean_before_curve" else y1
    ym = (src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2] + (0 if variant == "no_plus2" else 2)) >> 2
    if variant == "mean_before_curve" and p.flags & CURVE:
        ym = curve[ym]
    if variant == "chroma_cosited":
        ym = y1[0::2, 0::2]
    return y1, u1, v1, ym, raw


def grade_model(y, u, v, p: GradeP, variant: str | None = None, tie: str = "first"):
    """-> (Y', U', V') uint8 planes.  A coverage plane is not the model's business: it is copied."""
    if variant == "lut_first" and p.flags & LUT:   # the stages in another order: the lattice first, curve and matrix on its output
        yo, uo, vo = grade_model(y, u, v, p.but(flags=LUT), tie=tie)
        return grade_model(yo, uo, vo, p.but(flags=p.flags & ~LUT), tie=tie)
    y1, u1, v1, ym, _ = stages(y, u, v, p, variant)
    if not p.flags & LUT:
        return y1.astype(np.uint8), u1.astype(np.uint8), v1.astype(np.uint8)
    ub, vb = np.repeat(np.repeat(u1, 2, axis=0), 2, axis=1), np.repeat(np.repeat(v1, 2, axis=0), 2, axis=1)   # the chroma of a luma sample's own block
    if variant == "neighbour_chroma":              # ... or, misread, of the block its right-hand neighbour lies in
        xs = np.minimum((np.arange(y1.shape[1]) + 1) >> 1, u1.shape[1] - 1)
        ub, vb = np.repeat(u1, 2, axis=0)[:, xs], np.repeat(v1, 2, axis=0)[:, xs]
    yo = lut_eval(p.nodes, p.k, y1, ub, vb, variant, tie)[..., 0]
    co = lut_eval(p.nodes, p.k, ym, u1, v1, variant, tie)
    return yo.astype(np.uint8), co[..., 1].astype(np.uint8), co[..., 2].astype(np.uint8)


def lut_inputs(y, u, v, p: GradeP):
    """every (a, b, c) the LUT stage is evaluated at: the luma samples' and the chroma samples', as one [3][n] array"""
    y1, u1, v1, ym, _ = stages(y, u, v, p)
    ub, vb = np.repeat(np.repeat(u1, 2, axis=0), 2, axis=1), np.repeat(np.repeat(v1, 2, axis=0), 2, axis=1)
    return np.concatenate([np.stack([y1.ravel(), ub.ravel(), vb.ravel()]), np.stack([ym.ravel(), u1.ravel(), v1.ravel()])], axis=1)


# ---- the pictures the tests share ----
def gamma_curve(gamma=0.8, black=12, white=236):
    """a table that is no identity, meets 0 and 255 and is not monotone-strict: the ends are flat"""
    t = np.clip((np.arange(256) - black) / float(white - black), 0.0, 1.0)
    return np.clip(np.rint(255.0 * t ** (1.0 / gamma)), 0, 255).astype(np.uint8)


MATRIX = (5213, 1397, -1397, 5213)     # saturation 1.32 turned by 15 degrees: both clip ends on the every-(U, V) planes
OFFSETS = (-3 * 4096 - 1234, 2 * 4096 + 777)
LUMA_SHIFTS = (0, 3, 90)


def every_uv_picture(s: int):
    """a 256 x 256 chroma pair enumerating every (U, V) under a 512 x 512 luma of (37 x + 101 y + s) mod 256"""
    cx, cy = np.meshgrid(np.arange(256), np.arange(256))
    x, yy = np.meshgrid(np.arange(512), np.arange(512))
    return ((37 * x + 101 * yy + s) % 256).astype(np.uint8), cx.astype(np.uint8), cy.astype(np.uint8)


def shared_params(k: int, flags=CURVE | CHROMA | LUT, lattice="random") -> GradeP:
    nodes = None
    if flags & LUT:
        nodes = random_lattice(k, 1) if lattice == "random" else (smooth_lattice(k) if lattice == "smooth" else identity_lattice(k))
    return GradeP(flags, gamma_curve(), MATRIX, OFFSETS, k if flags & LUT else 0, nodes)


def noise_picture(w, h, seed):
    """uniform noise with a few rows and columns of the extremes, so that small frames meet 0 and 255 too"""
    rng = np.random.default_rng(0x9AADE + seed * 7919 + w * 31 + h)
    y = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    u = rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8)
    v = rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8)
    y[0, :] = 255; y[-1, :] = 0; u[:, -1] = 255; v[:, 0] = 0; v[-1, :] = 255
    return y, u, v
