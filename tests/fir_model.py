"""An independent numpy model of the two build-specified audio modules, written from DESIGN.md section 7 ("FIR / resampler") alone:

    widen f32 to f64, accumulate in f64 in ascending tap index with separate multiply and add, round once to f32
    Fir       y[n] = f32(sum_{k<K} taps[k] * f64(x[n-k]))
    Resample  output M: n = floor(M * down / up), phase = (M * down) mod up, y[M] = f32(sum_{k<P} taps[phase][k] * f64(x[n-k]))

One individually rounded numpy step per tap (a numpy product followed by a numpy sum is never contracted), vectorised over outputs and channels.
x before the run comes from the history passed in; the history passed out is the last K - 1 (P - 1) frames of history ++ input.  A
disconnected input (x = None) reads zeros.  Frames are (left, right) pairs: arrays of shape (..., frames, 2).

The contracted order (acc = fma(h, x, acc), MX_FLAG_FP_CONTRACT) needs a correctly rounded fused multiply-add.  `fma` is math.fma where the
interpreter has one (HAVE_FAST_FMA), else an exact one over fractions.Fraction that only small cases can afford.

`mis` selects one of MISREADINGS: a deliberate misreading of the paragraph.  tests/test_cpu_fir_model.py shows that each changes a bit of a case
of tests/fir_cases.py, so a kernel and an oracle that shared one would fail against this model.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

F32, F64 = np.float32, np.float64
HAVE_FAST_FMA = hasattr(math, "fma")

MISREADINGS = (
    "descending_taps",      # k = K-1 .. 0
    "f32_accumulation",     # taps and accumulator in f32
    "fma_in_exact_order",   # the default order with fused steps
    "round_per_tap",        # the f64 accumulator rounded to f32 after every tap
    "phase_m_mod_up",       # phase = M mod up
    "n_rounded_up",         # n = ceil(M * down / up)
    "history_off_by_one",   # the carried history ends one frame early
    "history_dropped",      # x before the run reads zero
    "table_transposed",     # taps[k][phase] of the same memory
    "out_base_32bit",       # the sample clocks kept in 32 bits: M = (out_base + m) mod 2^32
    "history_lr_swapped",   # left and right exchanged in the carried history
)


def fma(a: float, b: float, c: float) -> float:
    """a * b + c rounded once (finite operands)"""
    if HAVE_FAST_FMA:
        return math.fma(a, b, c)
    r = Fraction(a) * Fraction(b) + Fraction(c)
    return float(r) if r else a * b + c                  # an exact zero: the sign rule of the two-step sum is the fused one's


def _step(acc, h, x, order, mis):
    """one tap: acc <- acc + h * x in the selected arithmetic; h a scalar or an array broadcast against x"""
    if mis == "f32_accumulation":
        return (acc + (np.asarray(h, F64).astype(F32) * x.astype(F32)).astype(F32)).astype(F32)
    if order == "contracted" or mis == "fma_in_exact_order":
        hb = np.broadcast_to(np.asarray(h, F64), x.shape)
        out = np.empty_like(acc)
        of, hf, xf, af = out.reshape(-1), hb.reshape(-1), np.ascontiguousarray(x).reshape(-1), acc.reshape(-1)
        for i in range(of.size):
            of[i] = fma(float(hf[i]), float(xf[i]), float(af[i]))
        return out
    acc = acc + h * x                                    # two numpy operations: a rounded product, then a rounded sum
    if mis == "round_per_tap":
        acc = acc.astype(F32).astype(F64)
    return acc


def _ext(hist, x, H, frames, mis):
    """history ++ input as f64, shape (..., H + frames, 2)"""
    lead = np.asarray(hist, F32).shape[:-2]
    xin = np.zeros(lead + (frames, 2), F32) if x is None else np.asarray(x, F32)
    h = np.asarray(hist, F32).reshape(lead + (H, 2))
    if mis == "history_dropped":
        h = np.zeros_like(h)
    if mis == "history_lr_swapped":
        h = h[..., ::-1]
    return np.concatenate([h, xin], axis=-2), xin


def _new_hist(hist, xin, H, mis):
    full = np.concatenate([np.asarray(hist, F32).reshape(xin.shape[:-2] + (H, 2)), xin], axis=-2)
    n = full.shape[-2]
    if mis == "history_off_by_one":
        return np.ascontiguousarray(np.concatenate([np.zeros_like(full[..., :1, :]), full], axis=-2)[..., n - H:n, :])
    return np.ascontiguousarray(full[..., n - H:, :])


def fir(taps, hist, x, frames=None, order="exact", mis=None, acc64=False):
    """taps (K,) f64; hist (K - 1, 2) f32; x (frames, 2) f32 or None -> (y (frames, 2) f32, new history).
    acc64: return the f64 accumulator instead of y."""
    taps = np.asarray(taps, F64)
    K, H = taps.size, taps.size - 1
    frames = np.asarray(x).shape[-2] if x is not None else frames
    ext32, xin = _ext(hist, x, H, frames, mis)
    ext = ext32.astype(F64)
    acc = np.zeros((frames, 2), F32 if mis == "f32_accumulation" else F64)
    for k in (range(K - 1, -1, -1) if mis == "descending_taps" else range(K)):
        acc = _step(acc, taps[k], ext[H - k:H - k + frames], order, mis)     # x[n - k], n = 0 .. frames - 1
    return (acc if acc64 else acc.astype(F32)), _new_hist(hist, xin, H, mis)


def resample(tables, up, down, hist, in_base, out_base, x, out_frames, in_frames=None, order="exact", mis=None, acc64=False):
    """tables (C, up, P) f64; hist (C, P - 1, 2) f32; x (C, in_frames, 2) f32 or None; in_base / out_base: the absolute index of the run's
    first input / output frame (Python integers) -> (y (C, out_frames, 2) f32, new history)."""
    tables = np.asarray(tables, F64)
    C, _up, P = tables.shape
    assert _up == up
    H = P - 1
    in_frames = np.asarray(x).shape[-2] if x is not None else in_frames
    ext32, xin = _ext(np.asarray(hist, F32).reshape(C, H, 2), x, H, in_frames, mis)
    # (frame, left/right, channel): a gather of frames copies whole rows
    ext = np.ascontiguousarray(ext32.astype(F64).transpose(1, 2, 0))
    ob, ib = int(out_base), int(in_base)
    if mis == "out_base_32bit":
        ob, ib = ob % (1 << 32), ib % (1 << 32)
    M = [ob + m for m in range(out_frames)]              # Python integers: no width to overflow
    if mis == "out_base_32bit":
        M = [v % (1 << 32) for v in M]
    num = [v * down for v in M]
    n_abs = [(-(-v // up) if mis == "n_rounded_up" else v // up) for v in num]
    phase = np.array([(v % up) for v in (M if mis == "phase_m_mod_up" else num)], np.int64)
    n = np.array([v - ib for v in n_abs], np.int64)      # index into this run's input
    if mis is None:
        assert n.min() >= 0 and n.max() < in_frames, "the run's input does not hold every frame its outputs need"
    if mis == "table_transposed":
        tab = np.ascontiguousarray(tables.reshape(C, P, up).transpose(2, 1, 0))      # [phase][k] <- flat[k * up + phase]
    else:
        tab = np.ascontiguousarray(tables.transpose(1, 2, 0))                        # (phase, k, channel)
    acc = np.zeros((out_frames, 2, C), F32 if mis == "f32_accumulation" else F64)
    for k in (range(P - 1, -1, -1) if mis == "descending_taps" else range(P)):
        idx = n + H - k
        ok = (idx >= 0) & (idx < ext.shape[0])            # always, but for a misreading that moves n
        xs = ext[np.clip(idx, 0, ext.shape[0] - 1)]
        if not ok.all():
            xs[~ok] = 0.0
        acc = _step(acc, tab[phase, k][:, None, :], xs, order, mis)
    y = acc.transpose(2, 0, 1)
    return np.ascontiguousarray(y if acc64 else y.astype(F32)), _new_hist(np.asarray(hist, F32).reshape(C, H, 2), xin, H, mis)
