"""The keyer's specification (include/mixlab_gpu.h mx_video_key) restated in numpy, written from the text and not from the kernel,
plus the pictures the CPU and GPU suites share.  Integer arithmetic on non-negative values, `/` truncating, unless stated.

`bug=` selects a deliberate MIS-model (tests/test_cpu_video_key.py shows each one differs from the model on the shared pictures: the pictures can tell)."""
from __future__ import annotations

from dataclasses import dataclass, replace

import numpy as np

KEY_CHROMA, KEY_LUMA = 0, 1
BUGS = ("sqrt_round", "sqrt_f32", "ramp_round", "no_plus2", "edge_wrap", "edge_zero", "siting", "spill_floor", "invert_after", "ramp_order")


@dataclass(frozen=True)
class KeyP:
    mode: int = KEY_CHROMA
    key_u: int = 128
    key_v: int = 128
    invert: int = 0
    near_q4: int = 0
    far_q4: int = 0
    spill_far_q4: int = 0
    spill_strength: int = 0

    def but(self, **kw):
        return replace(self, **kw)


GREEN = (54, 34)   # a green-screen green as (U, V)
DEFAULT_CHROMA = KeyP(KEY_CHROMA, GREEN[0], GREEN[1], 0, 8 * 16, 40 * 16, 90 * 16, 200)
DEFAULT_LUMA = KeyP(KEY_LUMA, 0, 0, 0, 40 * 16 + 5, 200 * 16 + 3, 0, 0)


def dist_q4(d2, bug=None):
    """floor(sqrt(d2 << 8)): the exact integer square root (f64 holds the argument exactly; the estimate is then corrected in integers)"""
    x = np.asarray(d2, np.int64) << 8
    if bug == "sqrt_round":
        return np.rint(np.sqrt(x.astype(np.float64))).astype(np.int64)
    if bug == "sqrt_f32":
        return np.floor(np.sqrt(x.astype(np.float32), dtype=np.float32)).astype(np.int64)
    r = np.floor(np.sqrt(x.astype(np.float64))).astype(np.int64)
    r = np.where(r * r > x, r - 1, r)
    return np.where((r + 1) * (r + 1) <= x, r + 1, r)


def ramp(d, lo, hi, bug=None):
    d = np.asarray(d, np.int64)
    span = max(1, hi - lo)
    mid = ((d - lo) * 255 + (span // 2 if bug == "ramp_round" else 0)) // span
    if bug == "ramp_order":
        return np.where(d >= hi, 255, np.where(d <= lo, 0, mid))
    return np.where(d <= lo, 0, np.where(d >= hi, 255, mid))


def key_model(y, u, v, p: KeyP, a_in=None, bug=None):
    """(Y, U', V', coverage) of the frame (y: (H, W), u / v: (H/2, W/2) uint8; a_in: (H, W) uint8 or None) keyed under p"""
    y, u, v = (np.asarray(a, np.uint8) for a in (y, u, v))
    H, W = y.shape
    Hc, Wc = H // 2, W // 2
    assert u.shape == (Hc, Wc) and v.shape == (Hc, Wc) and W % 2 == 0 and H % 2 == 0
    uo, vo = u.copy(), v.copy()
    if p.mode == KEY_CHROMA:
        du = u.astype(np.int64) - p.key_u
        dv = v.astype(np.int64) - p.key_v
        d = dist_q4(du * du + dv * dv, bug)
        ac = ramp(d, p.near_q4, p.far_q4, bug)
        xs, ys = np.arange(W), np.arange(H)
        if bug == "siting":
            xs, ys = xs + 1, ys + 1
        cx, cy = np.minimum(xs >> 1, Wc - 1), np.minimum(ys >> 1, Hc - 1)
        cx1, cy1 = np.minimum(cx + (xs & 1), Wc - 1), np.minimum(cy + (ys & 1), Hc - 1)
        acx = ac
        if bug == "edge_wrap":
            cx1 = (cx + (xs & 1)) % Wc
        if bug == "edge_zero":
            acx = np.zeros((Hc, Wc + 1), np.int64); acx[:, :Wc] = ac
            cx1 = cx + (xs & 1)
        k = (acx[np.ix_(cy, cx)] + acx[np.ix_(cy, cx1)] + acx[np.ix_(cy1, cx)] + acx[np.ix_(cy1, cx1)] + (0 if bug == "no_plus2" else 2)) >> 2
        if p.spill_strength > 0 and p.spill_far_q4 > p.far_q4:
            w = ((255 - ramp(d, p.far_q4, p.spill_far_q4, bug)) * p.spill_strength) // 255

            def tdiv(n, den):
                if bug == "spill_floor":
                    return n // den
                return np.sign(n) * (np.abs(n) // den)
            uo = (128 + tdiv((u.astype(np.int64) - 128) * (255 - w), 255)).astype(np.uint8)
            vo = (128 + tdiv((v.astype(np.int64) - 128) * (255 - w), 255)).astype(np.uint8)
    else:
        k = ramp(y.astype(np.int64) * 16, p.near_q4, p.far_q4, bug)
    if p.invert and bug != "invert_after":
        k = 255 - k
    if a_in is not None:
        k = (k * np.asarray(a_in, np.uint8).astype(np.int64)) // 255
    if p.invert and bug == "invert_after":
        k = 255 - k
    return y.copy(), uo, vo, k.astype(np.uint8)


# ---- pictures ----
def green_screen(w, h, seed=0, key=GREEN):
    """A key-coloured background with a few code values of noise, and a foreground of random colours behind a soft-edged disc: the
    distances from the key colour cross both ramps of DEFAULT_CHROMA.  -> (y, u, v)"""
    rng = np.random.default_rng(0x6B65 + seed * 977 + w * 31 + h)
    hc, wc = h // 2, w // 2
    y = rng.integers(16, 236, size=(h, w)).astype(np.uint8)
    bg = [np.clip(key[i] + rng.integers(-3, 4, size=(hc, wc)), 0, 255) for i in range(2)]
    fg = [rng.integers(0, 256, size=(hc, wc)) for _ in range(2)]
    yy, xx = np.mgrid[0:hc, 0:wc]
    r = max(1.0, min(wc, hc) * 0.42)
    dist = np.hypot(xx - wc * 0.48, yy - hc * 0.52)
    m = np.clip((r - dist) / max(1.5, r * 0.45) + 0.5, 0.0, 1.0)   # 1 inside the disc, 0 outside, a wide soft edge
    u, v = (np.rint(bg[i] * (1.0 - m) + fg[i] * m).astype(np.uint8) for i in range(2))
    return y, u, v


def every_uv(seed=0):
    """512 x 512: the 256 x 256 chroma planes enumerate every (U, V) pair; Y random.  Covers every distance the square root sees."""
    rng = np.random.default_rng(0xE7E + seed)
    v, u = np.mgrid[0:256, 0:256]
    return rng.integers(0, 256, size=(512, 512)).astype(np.uint8), u.astype(np.uint8), v.astype(np.uint8)


def luma_wedge(w, h, seed=0):
    """Y runs through every value along a row (a little noise on top, so neighbouring rows differ); chroma random.  -> (y, u, v)"""
    rng = np.random.default_rng(0x1A3 + seed * 131 + w + h * 7)
    ramp_row = (np.arange(w) * 256 // max(1, w)).astype(np.int64)
    y = np.clip(ramp_row[None, :] + rng.integers(-6, 7, size=(h, w)), 0, 255).astype(np.uint8)
    if w * h >= 512:
        y.flat[:256] = np.arange(256)          # every value is there whatever the width
    u = rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8)
    v = rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8)
    return y, u, v
