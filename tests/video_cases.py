"""Pictures, geometries and matrices shared by tests/test_cpu_video_model.py and tests/test_gpu_video_model.py -- TEST INFRASTRUCTURE.
Plain numpy; nothing here knows the oracle or the product."""
from __future__ import annotations

import numpy as np

# (input size, output size) of a yuv420p -> yuv420p scale.  Small on purpose: the model is numpy and the same cases run on the device.
GEOMETRIES = {
    "up-1.5x": ((64, 36), (96, 54)),              # enlarging, ratio 2/3
    "up-just-below-1": ((62, 34), (64, 36)),      # enlarging, ratio just below 1
    "same-size": ((64, 36), (64, 36)),            # 1:1
    "down-just-above-1": ((66, 38), (64, 36)),    # the widened kernel at its narrowest (8 taps)
    "down-1.5x": ((96, 54), (64, 36)),
    "down-13x": ((130, 70), (10, 6)),             # 54 taps a side: wider than the plane the chroma comes from
    "source-2x2": ((2, 2), (64, 64)),             # every tap but one clamps
    "destination-2x2": ((64, 64), (2, 2)),
    "pillarbox": ((40, 60), (96, 54)),            # letterbox_x = 30: 2 (mod 4), the chroma rectangle starts on an odd column
    "letterbox": ((100, 30), (64, 64)),
    "pillarbox-down": ((48, 72), (70, 40)),       # bars and the widened kernel together
}
# Upscales for the tiled 4-tap kernel of mixlab_amd/csrc/mx_k_video.hip: luma of at least 130 x 42 and no multiple of the 128-column,
# 32- or 40-row tile, so every one has more than one tile per axis and a partial last tile.  plan_scale_tiles takes, over the planes of a job,
#   rows = ceil(32 sh / dh) + 6,   cols = ceil(128 sw / dw) + 25 rounded up to 16
# and picks the staging variant: cols > 128 -> 2; else rows > 32 -> 1; else 0, promoted to 3 (tiles of 40 rows) when the source rows of every
# 40-row tile (first tap of its last row + 4 - first tap of its first row) still fit 32.  tile_variant() below restates that rule so that
# test_cpu_video_model.py can assert the variant each entry names (its last field); the product reports nothing.
TILED = {
    # scaled to 134 x 74.  cols ceil(128 * 96 / 134) + 25 = 117 -> 128, rows ceil(32 * 54 / 74) + 6 = 30 <= 32, but the first 40-row tile
    # spans 33 source rows (first taps -2 .. 27, + 4) -> stays 0
    "tiled-96x54-to-134x76": ((96, 54), (134, 76), "planar420", 0),
    # scaled to 132 x 76: 84/132 = 0.64.  cols 82 + 25 = 107 -> 112, rows 21 + 6 = 27; the 40-row tiles span 29 and 26 source rows -> 3
    "tiled-84x48-to-134x76": ((84, 48), (134, 76), "planar420", 3),
    # 0.5: cols 64 + 25 = 89 -> 96, rows 16 + 6 = 22; 40-row tiles (40 + 40 + 20) span 24 rows -> 3
    "tiled-88x50-to-176x100": ((88, 50), (176, 100), "planar420", 3),
    # yuv422p scaled to 142 x 78: luma 64/142 = 0.45, but the chroma rows go 36 -> 39: rows ceil(32 * 36 / 39) + 6 = 36 > 32 while
    # cols (58 + 25 = 83 -> 96) stay <= 128 -> 1
    "tiled-422-64x36-to-142x80": ((64, 36), (142, 80), "planar422", 1),
    # scaled to 134 x 74: 120/134 = 0.9.  cols 115 + 25 = 140 -> 144 > 128 -> 2
    "tiled-120x68-to-134x76": ((120, 68), (134, 76), "planar420", 2),
}

# the matrices of test_gpu_video_parity.py::test_yuv_to_rgba_bit_exact_vs_build_spec (exact f32 FMAs / 24-bit products / 32-bit products on the device)
MATRICES = [None, [4096, 0, 0, 0, 0, 4096, 0, 0, 0, 0, 4096, 0],
            [3000, 800, 296, 40960, -200, 4500, -204, 0, 100, -300, 4296, -8192],
            [-4096, 0, 0, 1044480, 0, -4096, 0, 1044480, 0, 0, -4096, 1044480],
            [8192, 8192, 8192, -1000000, -3000, -3000, -3000, 4095, 1, 1, 1, 2047],
            [10922, 10922, 10922, 30000, 4096, 0, 0, -2048, 0, 0, 4097, -2049],
            [20000, 20000, 20000, -7000000, 0, 4096, 0, 0, -20000, 0, 0, 2000000],
            [8400000, 0, 0, 0, 0, 4096, 0, 0, 0, 0, -8400000, 0]]

PATTERNS = ["noise", "zeros", "full", "checker-1", "checker-2", "step-v", "step-h", "corner-tl", "corner-tr", "corner-bl", "corner-br"]


def plane(h, w, pattern, seed=0):
    """(h, w) uint8.  Besides seeded noise, the pictures on which a wrong rounding, shift, clamp or tap placement shows: flat fields at both
    ends of the range, 0 / 255 checkerboards of period 1 and 2, hard steps along either axis, one 255 pixel in a corner of a black plane."""
    y, x = np.mgrid[0:h, 0:w]
    if pattern == "noise":
        return np.random.default_rng([seed, h, w]).integers(0, 256, size=(h, w), dtype=np.uint8)
    if pattern == "zeros":
        return np.zeros((h, w), np.uint8)
    if pattern == "full":
        return np.full((h, w), 255, np.uint8)
    if pattern.startswith("checker-"):
        n = int(pattern[-1])
        return ((((x // n) + (y // n)) & 1) * 255).astype(np.uint8)
    if pattern == "step-v":                       # a vertical edge
        return ((x >= w // 2) * 255).astype(np.uint8)
    if pattern == "step-h":
        return ((y >= h // 2) * 255).astype(np.uint8)
    if pattern.startswith("corner-"):
        p = np.zeros((h, w), np.uint8)
        p[-1 if pattern[7] == "b" else 0, -1 if pattern[8] == "r" else 0] = 255
        return p
    raise ValueError(pattern)


SUBSAMPLING = {"planar420": (1, 1), "planar422": (1, 0), "planar444": (0, 0), "planar410": (2, 2), "planar411": (2, 0), "planar440": (0, 1)}   # log2 (chroma w, chroma h)


def yuv_planes(w, h, layout, pattern, seed=0):
    """(Y, U, V) of a planar 8-bit frame, the same pattern on every plane at its own size"""
    cw, ch = SUBSAMPLING[layout]
    return [plane(h, w, pattern, seed), plane(h >> ch, w >> cw, pattern, seed + 1), plane(h >> ch, w >> cw, pattern, seed + 2)]


def tile_variant(jobs, first_taps):
    """The staging variant plan_scale_tiles (mx_k_video.hip) picks for a job of 4-tap planes, restated for the comments of TILED.
    jobs: [(sw, sh, dw, dh)] per plane; first_taps(src, dst) -> the first tap index of every output sample."""
    rows = max(-(-32 * sh // dh) + 6 for _sw, sh, _dw, dh in jobs)
    cols = max(-(-128 * sw // dw) + 25 for sw, _sh, dw, _dh in jobs)
    cols = (cols + 15) // 16 * 16
    assert rows <= 48 and cols <= 256, "this job would take the gather kernel"
    if cols > 128:
        return 2
    if rows > 32:
        return 1
    for _sw, sh, _dw, dh in jobs:
        f = first_taps(sh, dh)
        for o in range(0, dh, 40):
            if f[min(o + 40, dh) - 1] + 4 - f[o] > 32:
                return 0
    return 3


# ---- scaler inputs of every format: name -> (name of the product's format constant, kind, detail) ----
FORMATS = {
    "yuv420p": ("PIXFMT_YUV420P", "planar", "planar420"), "yuv422p": ("PIXFMT_YUV422P", "planar", "planar422"),
    "yuv444p": ("PIXFMT_YUV444P", "planar", "planar444"), "yuv410p": ("PIXFMT_YUV410P", "planar", "planar410"),
    "yuv411p": ("PIXFMT_YUV411P", "planar", "planar411"), "yuv440p": ("PIXFMT_YUV440P", "planar", "planar440"),
    "nv12": ("PIXFMT_NV12", "semi", None),
    "yuyv422": ("PIXFMT_YUYV422", "packed422", "yuyv"), "uyvy422": ("PIXFMT_UYVY422", "packed422", "uyvy"),
    "gray8": ("PIXFMT_GRAY8", "gray8", None),
    "rgb24": ("PIXFMT_RGB24", "rgb", "rgb"), "bgr24": ("PIXFMT_BGR24", "rgb", "bgr"), "bgra": ("PIXFMT_BGRA", "rgb", "bgra"),
    "rgba": ("PIXFMT_RGBA", "rgb", "rgba"), "argb": ("PIXFMT_ARGB", "rgb", "argb"), "abgr": ("PIXFMT_ABGR", "rgb", "abgr"),
    "yuva420p": ("PIXFMT_YUVA420P", "planar+alpha", "planar420"),
}
DEEP_NAMES = ["PIXFMT_YUV420P10", "PIXFMT_YUV422P10", "PIXFMT_YUV444P10", "PIXFMT_P010", "PIXFMT_YUV420P12", "PIXFMT_YUV422P12",
              "PIXFMT_YUV444P12", "PIXFMT_YUV420P16", "PIXFMT_YUV422P16", "PIXFMT_YUV444P16", "PIXFMT_P016"]
ALL_FORMATS = list(FORMATS) + DEEP_NAMES
# two geometries per format: one through the 4-tap kernel, one through the widened one.  Widths are multiples of 4 (yuv410p / yuv411p);
# at 64 x 36 -> 96 x 54 the chroma of yuv422p / yuv440p enlarges along one axis while it shrinks along the other, that of yuv444p shrinks
# under an enlarging luma.
FORMAT_GEOMETRIES = {"up": ((64, 36), (96, 54)), "pillarbox-down": ((48, 72), (70, 40))}


def coverage(h, w, seed=0):
    """a coverage plane that is neither flat nor noise only: a ramp with opaque and transparent corners and a noisy quarter"""
    y, x = np.mgrid[0:h, 0:w]
    a = ((x * 255) // max(1, w - 1)).astype(np.uint8)
    a[: h // 4] = np.random.default_rng([seed, h, w, 7]).integers(0, 256, size=(h // 4, w), dtype=np.uint8)
    a[-1, 0], a[-1, -1] = 255, 0
    return a


def _deep_words(p8, bits, shift, rng):
    """16-bit words whose `bits`-bit samples follow the 8-bit picture `p8` (noise: the whole range, with the values next to every rounding
    and clipping boundary), with garbage in the bits the format ignores"""
    top = (1 << bits) - 1
    v = (p8.astype(np.int64) * top) // 255
    v += rng.integers(0, 1 << (bits - 8), size=p8.shape) * ((p8 > 0) & (p8 < 255))      # the bits below the 8-bit picture
    edge = [0, 1, (1 << (bits - 9)) - 1, 1 << (bits - 9), (1 << (bits - 8)) + 1, 3 << (bits - 9), top - (1 << (bits - 8)), top - (3 << (bits - 9)) + 1, top - (1 << (bits - 9)), top - 1, top]
    if p8.size > 4 * len(edge) and p8.min() != p8.max():
        v.flat[2:2 + len(edge)] = edge
    junk = rng.integers(0, 1 << (16 - bits), size=p8.shape) if bits < 16 else 0
    return (((v << shift) | junk) if shift else (v | (junk << bits))).astype(np.uint16)


def make_input(kind, detail, w, h, pattern, seed=0):
    """One scaler input -> {"planes": what is uploaded, "model": (planes, fmt) as video_model.stand_in takes them, "alpha": a yuva420p
    frame's coverage plane or None}.  kind "deep": detail = (subsampling name, bits, shift, semi-planar?)."""
    rng = np.random.default_rng([seed, w, h, 99])
    if kind in ("planar", "planar+alpha"):
        pl = yuv_planes(w, h, detail, pattern, seed)
        return {"planes": pl, "model": (pl, "planar"), "alpha": coverage(h, w, seed) if kind == "planar+alpha" else None}
    if kind == "semi":
        y, u, v = yuv_planes(w, h, "planar420", pattern, seed)
        uv = np.empty((h >> 1, w), np.uint8); uv[:, 0::2] = u; uv[:, 1::2] = v
        return {"planes": [y, uv], "model": ([y, uv], "nv12"), "alpha": None}
    if kind == "packed422":
        y, u, v = yuv_planes(w, h, "planar422", pattern, seed)
        pix = np.empty((h, 2 * w), np.uint8)
        yo = detail.index("y")
        pix[:, yo::2] = y; pix[:, detail.index("u")::4] = u; pix[:, detail.index("v")::4] = v
        return {"planes": [pix], "model": ([pix], detail), "alpha": None}
    if kind == "gray8":
        g = plane(h, w, pattern, seed)
        return {"planes": [g], "model": ([g], "gray8"), "alpha": None}
    if kind == "rgb":
        pix = np.stack([coverage(h, w, seed) if c == "a" else plane(h, w, pattern, seed + "rgb".index(c)) for c in detail], axis=-1)
        return {"planes": [pix], "model": ([pix], detail), "alpha": None}
    if kind == "deep":
        lay, bits, shift, semi = detail
        words = [_deep_words(p, bits, shift, rng) for p in yuv_planes(w, h, lay, pattern, seed)]
        if semi:
            uv = np.empty((h >> 1, w), np.uint16); uv[:, 0::2] = words[1]; uv[:, 1::2] = words[2]
            words = [words[0], uv]
        return {"planes": words, "model": (words, ("deep", bits, shift, "semi" if semi else "planar")), "alpha": None}
    raise ValueError(kind)


def format_entry(name, video):
    """(format id, kind, detail) of a name of ALL_FORMATS, the deep formats' layout / depth / alignment read off the product's own table"""
    if name in FORMATS:
        const, kind, detail = FORMATS[name]
        return getattr(video, const), kind, detail
    fmt = getattr(video, name)
    lay, bits, shift = video.DEEP[fmt]
    return fmt, "deep", ({0: "planar420", 1: "planar422", 2: "planar444"}[lay], bits, shift, name in ("PIXFMT_P010", "PIXFMT_P016"))


RGBA_SIZES = [(66, 34), (130, 70)]


def rgba_inputs(w, h):
    for pattern in ("noise", "zeros", "full", "checker-1", "step-v"):
        yield pattern, yuv_planes(w, h, "planar420", pattern, seed=6)
    y, u, v = yuv_planes(w, h, "planar420", "noise", seed=7)                 # saturated chroma against both ends of luma: every clip8
    u[: h // 4] = 0; v[: h // 4] = 255; u[h // 4: h // 2, : w // 4] = 255; v[h // 4: h // 2, : w // 4] = 0
    yield "saturated-chroma", [y, u, v]
