"""The pixel path of DESIGN.md sections 6 and 7 as plain numpy, written from the TEXT of those sections -- TEST INFRASTRUCTURE.

Two halves.  The INTEGER MODEL restates the spec one sentence at a time in int64 numpy: tap tables from the exact rationals of
tests/golden/make_bicubic_taps.py, the H and V passes, index clamping, the letterbox, the stand-in conversions of the input formats, the
YUV -> RGBA formulas and the Q12 matrix.  It shares no code with oracle/mixlab_oracle_video.c, tests/oracle_video.py or the product, and
loads no compiled library: the oracle and the device are both held to it byte for byte (tests/test_cpu_video_model.py,
tests/test_gpu_video_model.py).  The IDEAL REFERENCES are the same operations in f64 without any rounding -- a continuous separable cubic,
BT.709 from its primaries -- together with bounds on the model's distance from them that are computed from the weights and coefficients
themselves, never from a measured figure.

The module-level names H_ROUND, V_ROUND, M_ROUND, asr, gather, tap_tables, source_size and chroma_index are the model's single statements of
the details a shared misreading could get wrong; the tests replace them one at a time to show that their inputs can tell (no product code can
reach this file)."""
from __future__ import annotations

import importlib.util
import json
import pathlib

import numpy as np

_GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
_spec = importlib.util.spec_from_file_location("make_bicubic_taps", _GOLDEN / "make_bicubic_taps.py")
_taps_mod = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_taps_mod)
taps = _taps_mod.taps                     # (o, src, dst) -> (first, [coefficients]): exact rationals, DESIGN.md section 6

_RGB = json.loads((_GOLDEN / "rgb_matrix_bt709.json").read_text())   # the committed RGB -> YUV coefficients (make_rgb_matrix.py's output)

Q14 = 1 << 14                             # the taps of one output sample sum to this
H_SHIFT, V_SHIFT, M_SHIFT, C_SHIFT = 7, 21, 12, 8
H_ROUND = 1 << (H_SHIFT - 1)              # "t = (sum hc S + 64) >> 7"
V_ROUND = 1 << (V_SHIFT - 1)              # "D = clip8((sum vc t + 2^20) >> 21)"
M_ROUND = 1 << (M_SHIFT - 1)              # "(m_c0 R + m_c1 G + m_c2 B + m_c3 + 2048) >> 12"
C_ROUND = 1 << (C_SHIFT - 1)              # "+ 128) >> 8" of the colour formulas


def asr(x, n):
    """arithmetic shift right of int64: floor(x / 2^n), also for negative x"""
    return np.asarray(x, np.int64) >> n


def clip8(x):
    return np.clip(x, 0, 255)


def gather(p, idx, axis):
    """samples of `p` at the indices `idx` along `axis`: "indices clamp to the plane" """
    return np.take(p, np.clip(idx, 0, p.shape[axis] - 1), axis=axis)


_tables = {}


def tap_tables(src, dst):
    """-> first[dst], coef[dst][N] (int64) of `dst` output samples from `src`"""
    if (src, dst) not in _tables:
        t = [taps(o, src, dst) for o in range(dst)]
        _tables[(src, dst)] = (np.array([f for f, _c in t], np.int64), np.array([c for _f, c in t], np.int64))
    return _tables[(src, dst)]


def scale_plane(p, dw, dh, src_size=None, intermediates=False):
    """One plane (h, w) -> (dh, dw) uint8: the H pass over every source row, then the V pass over the int rows `t`.  `src_size` (h, w) is
    the size the tables are made for (the plane's own unless stated).  intermediates=True: -> (D, t, pre) with `pre` the V result before clip8."""
    p = np.asarray(p, np.int64)
    sh, sw = src_size if src_size is not None else p.shape
    hf, hc = tap_tables(sw, dw)
    vf, vc = tap_tables(sh, dh)
    n = np.arange(hc.shape[1])
    S = gather(p, hf[:, None] + n[None, :], 1)                                 # (h, dw, N)
    t = asr((S * hc[None, :, :]).sum(axis=2) + H_ROUND, H_SHIFT)               # (h, dw)
    n = np.arange(vc.shape[1])
    T = gather(t, vf[:, None] + n[None, :], 0)                                 # (dh, N, dw)
    pre = asr((T * vc[:, :, None]).sum(axis=1) + V_ROUND, V_SHIFT)             # (dh, dw)
    D = clip8(pre).astype(np.uint8)
    return (D, t, pre) if intermediates else D


# ---- stand-in conversions: the 8-bit planar frame a scaler input of another format stands for ----
def deep_to_8(words, bits, shift):
    """A plane of 16-bit words holding `bits`-bit samples at bit `shift` (0: low-aligned; p010: 6); the other bits of a word are ignored."""
    v = (np.asarray(words).astype(np.int64) >> shift) & ((1 << bits) - 1)
    return np.minimum(255, (v + (1 << (bits - 9))) >> (bits - 8)).astype(np.uint8)


def deinterleave(uv):
    """nv12 / p010 / p016 chroma rows U V U V ... -> (U, V)"""
    uv = np.asarray(uv)
    return uv[:, 0::2], uv[:, 1::2]


def yuyv_to_422p(pix, order):
    """rows of packed 4:2:2 bytes, order "yuyv" or "uyvy" -> (Y, U, V) of the yuv422p frame with the same samples"""
    pix = np.asarray(pix, np.uint8)
    k = {c: order.index(c) for c in "uv"}
    y0 = order.index("y")
    return pix[:, y0::2], pix[:, k["u"]::4], pix[:, k["v"]::4]


def gray8_to_444(gray):
    g = np.asarray(gray, np.uint8)
    return g, np.full_like(g, 0x80), np.full_like(g, 0x80)


def packed_rgb_to_yuv444(pix, order):
    """(h, w, len(order)) bytes in the order named by `order` ("rgb", "bgra", "argb", ...) -> (Y, U, V, A or None): BT.709 limited range,
    integer, coefficients of tests/golden/rgb_matrix_bt709.json; an A byte is the pixel's coverage and passes through."""
    px = np.asarray(pix).astype(np.int64)
    rgb = np.stack([px[..., order.index(c)] for c in "rgb"], axis=-1)
    out = [asr((rgb * np.array(_RGB[k], np.int64)).sum(axis=-1) + C_ROUND, C_SHIFT) + off for k, off in (("y", 16), ("cb", 128), ("cr", 128))]
    a = np.asarray(pix, np.uint8)[..., order.index("a")] if "a" in order else None
    return tuple(clip8(o).astype(np.uint8) for o in out) + (a,)


def source_size(k, planes):
    """the size plane `k` of (Y, U, V) is resampled from: "every plane is resampled from its own size" """
    return planes[k].shape


RGB_ORDERS = ("rgb", "bgr", "bgra", "rgba", "argb", "abgr")


def stand_in(planes, fmt):
    """-> (Y, U, V, A or None): the 8-bit planar frame a scaler input stands for.  `fmt` names how `planes` is laid out: "planar" (Y, U, V of
    any chroma subsampling), "nv12" (Y, interleaved UV), "gray8" (G,), "yuyv" / "uyvy" (packed rows,), one of RGB_ORDERS ((h, w, bpp) bytes,),
    or ("deep", bits, shift, "planar" | "semi") for 16-bit words."""
    if isinstance(fmt, tuple):
        _deep, bits, shift, lay = fmt
        return stand_in([deep_to_8(p, bits, shift) for p in planes], "nv12" if lay == "semi" else "planar")
    if fmt == "planar":
        return tuple(np.asarray(p, np.uint8) for p in planes) + (None,)
    if fmt == "nv12":
        return (np.asarray(planes[0], np.uint8),) + tuple(np.asarray(c, np.uint8) for c in deinterleave(planes[1])) + (None,)
    if fmt == "gray8":
        return gray8_to_444(planes[0]) + (None,)
    if fmt in ("yuyv", "uyvy"):
        return yuyv_to_422p(planes[0], fmt) + (None,)
    if fmt in RGB_ORDERS:
        return packed_rgb_to_yuv444(planes[0], fmt)
    raise ValueError(f"unknown input layout {fmt!r}")


def scale_frame(planes, fmt, out_w, out_h, geometry, alpha=None):
    """A scaler input (`planes`, `fmt` as stand_in takes them; `alpha`: the coverage plane of a yuva420p input, luma size) -> the yuv420p frame
    [Y, U, V(, A)] of out_w x out_h: every plane resampled from its own size into the letterboxed rectangle `geometry` = (scaled_w, scaled_h,
    letterbox_x, letterbox_y); the bars are blank (Y 0, U = V = 0x80), the coverage's bars opaque."""
    sw, sh, lx, ly = geometry
    y, u, v, a = stand_in(planes, fmt)
    yuv = (y, u, v)
    alpha = a if alpha is None else np.asarray(alpha, np.uint8)
    out = [np.zeros((out_h, out_w), np.uint8), np.full((out_h >> 1, out_w >> 1), 0x80, np.uint8), np.full((out_h >> 1, out_w >> 1), 0x80, np.uint8)]
    if alpha is not None:
        out.append(np.full((out_h, out_w), 255, np.uint8))
    if sw == 0 or sh == 0:
        return out
    for k in range(3):
        c = 1 if k else 0
        out[k][ly >> c:(ly >> c) + (sh >> c), lx >> c:(lx >> c) + (sw >> c)] = scale_plane(yuv[k], sw >> c, sh >> c, src_size=source_size(k, yuv))
    if alpha is not None:
        out[3][ly:ly + sh, lx:lx + sw] = scale_plane(alpha, sw, sh)            # "the scaler resamples the plane with the luma taps"
    return out


# ---- section 7: YUV -> RGBA ----
def chroma_index(n):
    """index of the chroma sample of each of `n` luma positions: nearest (co-sited 2x, 2y)"""
    return np.arange(n) >> 1


def yuv420_to_rgba(y, u, v, matrix_q12=None):
    """-> (h, w, 4) uint8"""
    y = np.asarray(y, np.int64)
    h, w = y.shape
    cy, cx = chroma_index(h), chroma_index(w)
    C = y - 16
    D = np.asarray(u, np.int64)[cy][:, cx] - 128
    E = np.asarray(v, np.int64)[cy][:, cx] - 128
    R = clip8(asr(298 * C + 459 * E + C_ROUND, C_SHIFT))
    G = clip8(asr(298 * C - 55 * D - 136 * E + C_ROUND, C_SHIFT))
    B = clip8(asr(298 * C + 541 * D + C_ROUND, C_SHIFT))
    if matrix_q12 is not None:
        m = np.asarray(matrix_q12, np.int64).reshape(3, 4)
        R, G, B = (clip8(asr(m[c, 0] * R + m[c, 1] * G + m[c, 2] * B + m[c, 3] + M_ROUND, M_SHIFT)) for c in range(3))
    return np.stack([R, G, B, np.full_like(R, 255)], axis=-1).astype(np.uint8)


# ---- the ideal references (f64, nothing rounded) ----
def _cubic(x):
    """B = 0, C = 0.6 cubic of a distance x >= 0"""
    x = np.abs(x)
    return np.where(x < 1, (7 * x ** 3 - 12 * x ** 2 + 5) / 5, np.where(x < 2, (-3 * x ** 3 + 15 * x ** 2 - 24 * x + 12) / 5, 0.0))


def ideal_weights(src, dst):
    """-> first[dst] (int64), w[dst][N] (f64): output o is centred at (o + 1/2) src / dst - 1/2; the cubic is stretched by max(1, src / dst);
    4 taps, or 2 ceil(2 src / dst) + 2 when shrinking, around the centre; weights normalised to 1.  floor(centre) is taken in integers."""
    o = np.arange(dst, dtype=np.int64)
    n = 4 if src <= dst else 2 * -(-2 * src // dst) + 2
    first = ((2 * o + 1) * src - dst) // (2 * dst) - n // 2 + 1
    centre = (o + 0.5) * (src / dst) - 0.5
    w = _cubic((first[:, None] + np.arange(n)[None, :] - centre[:, None]) / max(1.0, src / dst))
    return first, w / w.sum(axis=1, keepdims=True)


def ideal_scale_plane(p, dw, dh):
    """the continuous reference: (dh, dw) f64, unrounded and unclipped (an overshoot leaves [0, 255])"""
    p = np.asarray(p, np.float64)
    hf, hw = ideal_weights(p.shape[1], dw)
    vf, vw = ideal_weights(p.shape[0], dh)
    A = (gather(p, hf[:, None] + np.arange(hw.shape[1])[None, :], 1) * hw[None, :, :]).sum(axis=2)
    return (gather(A, vf[:, None] + np.arange(vw.shape[1])[None, :], 0) * vw[:, :, None]).sum(axis=1)


def ideal_bound(src_w, dw, src_h, dh):
    """(dh, dw) f64: a bound on |scale_plane - clip(ideal_scale_plane, 0, 255)| for ANY 8-bit source plane, from the two sets of weights.

    Write hq = hc / 16384, vq = vc / 16384 (the model's weights as fractions; both kinds of table place their taps at the same indices, which
    the function checks), hw, vw the ideal weights, S in [0, 255] the samples, A = sum hq S and Aw = sum hw S the exact H results.
      H pass:  t = floor(128 A + 1/2) = 128 A + e1,  e1 in (-1/2, 1/2].
      V pass:  pre = floor(sum vq t / 128 + 1/2) = sum vq A + sum vq e1 / 128 + e2,  e2 in (-1/2, 1/2],  so
               |pre - sum vq A| <= 1/2 + 2^-8 sum|vq|.
      Weights: sum vq A - sum vw Aw = sum vq (A - Aw) + sum (vq - vw) Aw.  Both sets of weights sum to 1, so sum (hq - hw) = 0 and
               A - Aw = sum (hq - hw)(S - 255/2):  |A - Aw| <= (255/2) sum|hq - hw|.  Likewise Aw lies in an interval of half-width
               (255/2) sum|hw| and sum (vq - vw) = 0:  |sum (vq - vw) Aw| <= (255/2) sum|hw| sum|vq - vw|.
      Clip:    clip8 is 1-Lipschitz, so it may be applied to both sides (the model clips, therefore the ideal is compared clipped).
    Together, per output sample (x, y):
        1/2 + sum_y|vq| (2^-8 + (255/2) sum_x|hq - hw|) + (255/2) sum_x|hw| sum_y|vq - vw| + f64 term.
    This differs from the first-cut expression 1/2 + sum|vq| (2^-8 + 255 max_x sum|hq - hw|) + 255 sum|vq - vw| in three places: the H term
    is taken at the sample's own column instead of the worst one, centring S halves both weight terms (255/2 for 255), and the last term
    carries sum|hw| because the ideal H result of a plane with negative lobes is NOT confined to [0, 255] -- without that factor the
    expression is not a bound.  The f64 term covers the evaluation of the ideal itself (two dot products of n taps and a normalisation per
    axis, each operation within one unit roundoff u: (nh + nv + 4) u 255 sum|hw| sum|vw|, first order) plus the same amount for
    sum w = 1 holding only to roundoff; it is ~1e-12 and is there so that the bound is one, not because a test needs it."""
    hf, hc = tap_tables(src_w, dw)
    vf, vc = tap_tables(src_h, dh)
    ihf, hw = ideal_weights(src_w, dw)
    ivf, vw = ideal_weights(src_h, dh)
    assert np.array_equal(hf, ihf) and np.array_equal(vf, ivf) and hc.shape == hw.shape and vc.shape == vw.shape, "the model and the ideal place their taps differently"
    hq, vq = hc / Q14, vc / Q14
    dh_, dv_ = np.abs(hq - hw).sum(axis=1), np.abs(vq - vw).sum(axis=1)        # per column, per row
    ah, av, aq = np.abs(hw).sum(axis=1), np.abs(vw).sum(axis=1), np.abs(vq).sum(axis=1)
    u = np.finfo(np.float64).eps / 2
    f64 = 2 * (hw.shape[1] + vw.shape[1] + 4) * u * 255 * av[:, None] * ah[None, :]
    return 0.5 + aq[:, None] * (2.0 ** -(H_SHIFT + 1) + 255 / 2 * dh_[None, :]) + 255 / 2 * ah[None, :] * dv_[:, None] + f64


_KR, _KB = 0.2126, 0.0722
_KG = 1.0 - _KR - _KB
# exact BT.709 limited-range coefficients of (C, D, E) = (Y - 16, U - 128, V - 128) per channel
_IDEAL_RGB = np.array([[255 / 219, 0.0, 255 / 224 * 2 * (1 - _KR)],
                       [255 / 219, -255 / 224 * 2 * _KB * (1 - _KB) / _KG, -255 / 224 * 2 * _KR * (1 - _KR) / _KG],
                       [255 / 219, 255 / 224 * 2 * (1 - _KB), 0.0]])
_MODEL_RGB = np.array([[298, 0, 459], [298, -55, -136], [298, 541, 0]]) / (1 << C_SHIFT)


def ideal_rgba(y, u, v):
    """BT.709 limited range in f64, nearest chroma: (h, w, 3) f64 R, G, B, unrounded and unclipped"""
    y = np.asarray(y, np.float64)
    h, w = y.shape
    cy, cx = np.arange(h) >> 1, np.arange(w) >> 1
    cde = np.stack([y - 16, np.asarray(u, np.float64)[cy][:, cx] - 128, np.asarray(v, np.float64)[cy][:, cx] - 128], axis=-1)
    return cde @ _IDEAL_RGB.T


def ideal_rgba_bound():
    """per channel (R, G, B): a bound on |yuv420_to_rgba(None) - clip(ideal_rgba, 0, 255)|.  The integer formula is
    clip8(floor(x + 1/2)) with x the /256 coefficients applied to (C, D, E): within 1/2 of x; x differs from the ideal by at most
    sum_k |coefficient_k / 256 - exact_k| max|operand_k|, C in [-16, 239], D and E in [-128, 127]; clip8 is 1-Lipschitz."""
    operand = np.array([max(abs(0 - 16), abs(255 - 16)), max(abs(0 - 128), abs(255 - 128)), max(abs(0 - 128), abs(255 - 128))], np.float64)
    return 0.5 + np.abs(_MODEL_RGB - _IDEAL_RGB) @ operand
