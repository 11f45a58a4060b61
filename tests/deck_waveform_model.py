"""The deck's waveform picture (include/mixlab_gpu.h "WAVEFORM") in numpy int64 and Python integers, written from the header's text: the records of
deck_analysis_model in, the three planes out.  Python integers do not overflow, so the model says nothing about the width of an intermediate; the header's
GRID LINE paragraph does, and tests/test_cpu_deck_waveform.py holds the C++ restatement against this model at the bounds.

MISREADINGS are ways to read the header wrongly; render(..., mis=(name,)) draws the picture under one of them, and the CPU test shows for each that some byte of
some shared case changes.  One of the issue's list is unreachable in part and is narrowed here:

  no_height_clamp   For BANDS a height above half covers exactly what half covers: d(y) < half on every row, so "d < H" is true on every row for every H >= half,
                    and no picture can tell a clamped height from an unclamped one.  For ENVELOPE the same holds of the set of rows [half - UP, half + DOWN) cut to
                    the picture -- as long as half - UP is computed where it can go negative.  The misreading that IS reachable is the unclamped UP in unsigned
                    arithmetic: half - UP wraps to a row far below the picture and the upper half stays empty.  That is what the name stands for here.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

BANDS, ENVELOPE = 0, 1
MAX_GRIDS, MAX_MARKERS, MAX_RANGES = 16, 32, 8
STRIP = 64
PAD_Y, PAD_C = 0, 0x80   # what the frame's stride padding holds: mx_dframe_create's blank

MISREADINGS = ("chroma_top_left", "bands_high_first", "f1_inclusive", "trunc_div", "beat_right_edge", "no_clamp", "d_off_by_one", "drop_short_last",
               "no_height_clamp", "marker_centre_up", "markers_under_grids", "ranges_over_line", "down_unsigned", "inset_on_markers")


class Grid(NamedTuple):
    first_q32: int
    period_q32: int
    colour: tuple
    from_q32: int = -(1 << 62)
    to_q32: int = 1 << 62
    inset: int = 0


class Marker(NamedTuple):
    frame: int
    colour: tuple
    width: int = 1


class Range(NamedTuple):
    from_frame: int
    to_frame: int
    colour: tuple


class Wave(NamedTuple):
    w: int
    h: int
    first_frame: int
    fpp: int
    style: int = BANDS
    gain: tuple = (1 << 16, 1 << 16, 1 << 16)
    bg: tuple = (16, 128, 128)
    line: tuple = (64, 120, 136)
    band: tuple = ((81, 90, 240), (145, 54, 34), (210, 146, 16))
    grids: tuple = ()
    markers: tuple = ()
    ranges: tuple = ()


def check(p: Wave):
    """None when the settings pass the header's rules, else words of the broken rule (the first, in the header's order)"""
    if p.w % 2 or not 2 <= p.w <= 8192:
        return "w is not even"
    if p.h % 2 or not 4 <= p.h <= 4320:
        return "h is not even"
    if abs(p.first_frame) > 1 << 30:
        return "first_frame"
    if not 1 <= p.fpp <= 1 << 20:
        return "frames_per_px outside"
    if p.w * p.fpp > 1 << 30:
        return "w * frames_per_px"
    if p.style not in (BANDS, ENVELOPE):
        return "style"
    for b in range(3):
        if not 0 <= p.gain[b] <= 1 << 20:
            return "gain_q16[%d]" % b
    if len(p.grids) > MAX_GRIDS:
        return "n_grids"
    if len(p.markers) > MAX_MARKERS:
        return "n_markers"
    if len(p.ranges) > MAX_RANGES:
        return "n_ranges"
    for k, g in enumerate(p.grids):
        if not 1 << 32 <= g.period_q32 <= 1 << 56:
            return "grid %d: period_q32" % k
        if abs(g.first_q32) > 1 << 61:
            return "grid %d: first_q32" % k
        if g.from_q32 > g.to_q32:
            return "grid %d: from_q32" % k
        if g.inset > p.h // 2:
            return "grid %d: inset" % k
    for k, m in enumerate(p.markers):
        if not 1 <= m.width <= 16:
            return "marker %d: width" % k
    for k, r in enumerate(p.ranges):
        if r.from_frame > r.to_frame:
            return "range %d: from_frame" % k
    return None


def view(pos_q32: int, fpp: int, playhead_x: int) -> int:
    return (pos_q32 >> 32) - playhead_x * fpp


def _trunc(a: int, b: int) -> int:
    return abs(a) // b * (1 if a >= 0 else -1)


def span(p: Wave, x: int, C: int, N: int, mis=()):
    """(c0, c1) of pixel column x, or None outside the track"""
    F0 = p.first_frame + x * p.fpp
    F1 = F0 + p.fpp
    last = F1 if "f1_inclusive" in mis else F1 - 1
    lo, hi = (_trunc(F0, C), _trunc(last, C)) if "trunc_div" in mis else (F0 // C, last // C)
    c0, c1 = max(0, lo), min(N - 1, hi)
    return (c0, c1) if c0 <= c1 else None


def holds_line(g: Grid, F0: int, F1: int, n_frames: int, mis=()) -> bool:
    if "no_clamp" not in mis:
        F0, F1 = min(max(F0, 0), n_frames), min(max(F1, 0), n_frames)
    A, B = max(F0 << 32, g.from_q32), min(F1 << 32, g.to_q32)
    if not A < B:
        return False
    line = g.first_q32 + -(-(A - g.first_q32) // g.period_q32) * g.period_q32   # the first line at or after A
    return line <= B if "beat_right_edge" in mis else line < B


def render(cols: np.ndarray, C: int, n_frames: int, p: Wave, mis=()):
    """(Y, U, V): uint8 arrays of h x w, h / 2 x w / 2 and again -- the visible area"""
    assert check(p) is None and C & (C - 1) == 0
    N = -(-n_frames // C)
    assert len(cols) == N
    if "drop_short_last" in mis:
        N = n_frames // C
    w, h, half = p.w, p.h, p.h // 2
    rows = np.arange(h)
    top = rows < half
    d = np.where(top, (half if "d_off_by_one" in mis else half - 1) - rows, rows - half)
    pix = np.zeros((h, w, 3), np.int64)
    for x in range(w):
        F0 = p.first_frame + x * p.fpp
        F1 = F0 + p.fpp
        col = np.empty((h, 3), np.int64)
        col[:] = p.bg

        def ranges():
            for r in p.ranges:
                if max(r.from_frame, F0) < min(r.to_frame, F1):
                    col[:] = r.colour

        if "ranges_over_line" not in mis:
            ranges()
        s = span(p, x, C, N, mis)
        if s is not None:
            part = cols[s[0]:s[1] + 1]
            col[d == 0] = p.line
            if "ranges_over_line" in mis:
                ranges()
            if p.style == BANDS:
                order = (2, 1, 0) if "bands_high_first" in mis else (0, 1, 2)
                for b in order:
                    H = min(half, (int(part["peak"][:, b].max()) * p.gain[b] * half) >> 32)
                    col[d < H] = p.band[b]
            else:
                smax, smin = int(part["smax"].max()), int(part["smin"].min())
                up = (max(smax, 0) * p.gain[0] * half) >> 32
                down = min(half, (max(smin if "down_unsigned" in mis else -smin, 0) * p.gain[0] * half) >> 32)
                start = (half - up) % (1 << 32) if "no_height_clamp" in mis else half - min(half, up)
                col[(rows >= start) & (rows < half + down)] = p.band[0]
        elif "ranges_over_line" in mis:
            ranges()

        def grids():
            for g in p.grids:
                if holds_line(g, F0, F1, n_frames, mis):
                    col[(rows >= g.inset) & (rows < h - g.inset)] = g.colour

        def markers():
            inset = max([g.inset for g in p.grids], default=0) if "inset_on_markers" in mis else 0
            for m in p.markers:
                n = m.frame - p.first_frame
                xm = _trunc(n, p.fpp) if "trunc_div" in mis else n // p.fpp
                lo = xm - ((m.width + 1) // 2 if "marker_centre_up" in mis else m.width // 2)
                if lo <= x < lo + m.width:
                    col[(rows >= inset) & (rows < h - inset)] = m.colour

        if "markers_under_grids" in mis:
            markers(); grids()
        else:
            grids(); markers()
        pix[:, x] = col
    Y = pix[:, :, 0].astype(np.uint8)
    if "chroma_top_left" in mis:
        U, V = pix[0::2, 0::2, 1], pix[0::2, 0::2, 2]
    else:
        quad = pix[0::2, 0::2] + pix[0::2, 1::2] + pix[1::2, 0::2] + pix[1::2, 1::2]
        U, V = (quad[:, :, 1] + 2) >> 2, (quad[:, :, 2] + 2) >> 2
    return Y, U.astype(np.uint8), V.astype(np.uint8)


def forms(p: Wave, C: int, n_frames: int) -> dict:
    """what mx_deck_debug_last_waveform says after a render of p, from the header's description of the counts"""
    N = -(-n_frames // C)
    out = dict.fromkeys(("strips_single", "strips_several", "strips_outside", "max_records"), 0)
    for x0 in range(0, p.w, STRIP):
        spans = [s for s in (span(p, x, C, N) for x in range(x0, min(x0 + STRIP, p.w))) if s is not None]
        if not spans:
            out["strips_outside"] += 1
            continue
        out["strips_several" if any(c1 > c0 for c0, c1 in spans) else "strips_single"] += 1
        out["max_records"] = max(out["max_records"], max(c1 for _, c1 in spans) - min(c0 for c0, _ in spans) + 1)
    return out


def stride(width: int) -> int:
    """the row stride of a frame's plane of `width` bytes: rows are 64-byte aligned"""
    return (width + 63) & ~63


def padded(planes, w: int, h: int):
    """the three planes as the device frame holds them, stride padding included"""
    out = []
    for k, a in enumerate(planes):
        pw, ph = (w, h) if k == 0 else (w // 2, h // 2)
        full = np.full((ph, stride(pw)), PAD_Y if k == 0 else PAD_C, np.uint8)
        full[:, :pw] = a
        out.append(full)
    return out
