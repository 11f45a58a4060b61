"""The shared cases of the deck's waveform picture (tests/test_cpu_deck_waveform.py, tests/test_gpu_deck_waveform.py): a track, the analysis settings, the waveform
settings, and the model's records and picture, computed once per case and shared.  Tracks are generated from seeds; nothing is read from disk.  Everything is small:
tracks of 100 to 6 000 frames, pictures of at most 256 x 64 but for one that is taller than one pass of the fill (2 x 130 lane tasks against 256 lanes)."""
from __future__ import annotations

from typing import Callable, NamedTuple

import numpy as np

import deck_analysis_cases as ac
import deck_analysis_model as am
import deck_waveform_model as wm
from deck_waveform_model import BANDS, ENVELOPE, Grid, Marker, Range, Wave

Q = 1 << 32
A64 = ac.BANDS_63._replace(column=64, max_lag=16)        # 200 Hz / 2.5 kHz, K = 63, C = 64
A512 = ac.BANDS_63._replace(max_lag=16)
EXTREME = am.Settings(64, 16, ac.EXTREME_TAPS, ac.EXTREME_TAPS)

RED, GREEN, BLUE, WHITE, GREY = (81, 90, 240), (145, 54, 34), (41, 240, 110), (235, 128, 128), (126, 100, 160)
CYAN, MAGENTA, YELLOW = (170, 166, 16), (106, 202, 222), (210, 16, 146)


def noise6000():
    return ac.noise(6000, "wave 6000", 9000)


def noise100():
    return ac.noise(100, "wave 100", 20000)


def short_last():
    return ac.noise(5 * 64 + 1, "wave short last", 9000)


def positive():
    return np.abs(ac.noise(2000, "wave positive", 9000).astype(np.int32)).astype(np.int16)


def negative():
    return ac.negative_odd(2000, "wave negative")


def extreme():
    return ac.constant(640, -32768)


class Case(NamedTuple):
    name: str
    build: Callable[[], np.ndarray]
    settings: am.Settings
    wave: Wave


G16 = (600000, 400000, 250000)   # gains that put the bands of noise6000 at a few rows each of a 16-row picture
BEATS = Grid(100 * Q, 50 * Q, WHITE)
CASES = [
    Case("2 x 4, the whole track in two pixel columns", noise6000, A64, Wave(2, 4, 0, 3000, gain=G16)),
    Case("62 x 14", noise6000, A64, Wave(62, 14, 0, 90, gain=G16, grids=(Grid(0, 700 * Q + 5, WHITE, inset=2),), markers=(Marker(2000, CYAN, 3),))),
    Case("64 x 16", noise6000, A64, Wave(64, 16, 100, 90, gain=G16, grids=(Grid(33 * Q, 650 * Q, WHITE),), ranges=(Range(1000, 2500, GREY),))),
    Case("66 x 18", noise6000, A64, Wave(66, 18, -200, 90, gain=G16, grids=(Grid(0, 800 * Q, WHITE, inset=1),), markers=(Marker(5700, CYAN, 2),))),
    Case("130 x 34", noise6000, A64, Wave(130, 34, -100, 47, gain=G16, grids=(Grid(5 * Q, 611 * Q + 77, WHITE),), markers=(Marker(3000, CYAN, 5),))),
    Case("70 x 260, taller than one pass of the fill", noise6000, A64, Wave(70, 260, -300, 95, gain=(400000, 200000, 100000), grids=(Grid(0, 900 * Q, WHITE, inset=20),),
                                                                           markers=(Marker(3100, CYAN, 2),), ranges=(Range(4000, 5000, GREY),))),
    Case("first_frame negative and no multiple of fpp, a marker left of it", noise6000, A64,
         Wave(64, 16, -1000, 37, gain=G16, markers=(Marker(-1010, CYAN, 2), Marker(-1, MAGENTA, 1)), grids=(Grid(-3 * Q, 400 * Q, WHITE),))),
    Case("a window wholly left of the track", noise6000, A64, Wave(64, 16, -5000, 10, gain=G16, grids=(BEATS,), markers=(Marker(-4700, CYAN, 4),), ranges=(Range(-4900, -4600, GREY),))),
    Case("a window wholly right of the track", noise6000, A64, Wave(66, 16, 7000, 10, gain=G16, grids=(BEATS,), markers=(Marker(7100, CYAN, 4),))),
    Case("a window over the track's right end", noise6000, A64, Wave(64, 16, 5500, 10, gain=G16, grids=(Grid(0, 30 * Q, WHITE),))),
    Case("fpp = 1: one record serves 64 pixel columns", noise6000, A64, Wave(130, 32, 1000, 1, gain=G16, grids=(Grid(1003 * Q + 1, 16 * Q, WHITE, inset=4),))),
    Case("fpp = C on the columns' boundaries: one record a pixel column", noise6000, A64, Wave(66, 32, 64, 64, gain=G16)),
    Case("fpp = 3 C + 1: boundaries drift across the pixels", noise6000, A64, Wave(32, 32, -50, 193, gain=G16)),
    Case("fpp = 8192: one pixel column holds the whole track", noise6000, A64, Wave(4, 32, -8192, 8192, gain=G16, grids=(Grid(0, 5000 * Q, WHITE),))),
    Case("a last column one frame long", short_last, A64, Wave(130, 16, 300, 1, gain=G16)),
    Case("a track of 100 frames in two columns", noise100, A64, Wave(64, 16, -20, 3, gain=(30000, 60000, 120000), grids=(Grid(0, 25 * Q, WHITE),))),
    Case("peaks that clamp at half", noise6000, A64, Wave(64, 16, 0, 90, gain=(1 << 20, 1 << 20, 1 << 20))),
    Case("an envelope that clamps at half", noise6000, A64, Wave(64, 16, 0, 90, ENVELOPE, gain=(1 << 20, 0, 0))),
    Case("gain 0 under grids, markers and ranges", noise6000, A64, Wave(64, 16, 0, 90, gain=(0, 0, 0), grids=(Grid(0, 1000 * Q, WHITE),), markers=(Marker(4000, CYAN, 2),),
                                                                     ranges=(Range(500, 3000, GREY),))),
    Case("every sample -32768 under 63 positive taps of sum 32767", extreme, EXTREME, Wave(64, 64, -64, 12, gain=(1 << 20, 3, 1 << 20))),
    Case("the same track as an envelope", extreme, EXTREME, Wave(64, 64, -64, 12, ENVELOPE, gain=(30000, 0, 0))),
    Case("envelope of an all-positive track", positive, A64, Wave(64, 32, -100, 35, ENVELOPE, gain=(150000, 0, 0))),
    Case("envelope of an all-negative track", negative, A64, Wave(64, 32, -100, 35, ENVELOPE, gain=(900000, 0, 0))),
    Case("beats exactly on pixels' left edges", noise6000, A64, Wave(64, 16, 0, 10, gain=G16, grids=(BEATS,))),
    Case("a grid with a negative first_q32", noise6000, A64, Wave(64, 16, -40, 10, gain=G16, grids=(Grid(-7 * Q - 12345, 33 * Q + 999, WHITE),))),
    Case("a grid whose [from, to) begins and ends mid-pixel", noise6000, A64, Wave(64, 16, 0, 10, gain=G16, grids=(Grid(0, 3 * Q, WHITE, 205 * Q, 505 * Q),))),
    Case("a period shorter than a pixel, over the track's right end", noise6000, A64, Wave(64, 16, 5000, 40, gain=G16, grids=(Grid(0, 7 * Q, WHITE, inset=2),))),
    Case("inset = half hides a grid", noise6000, A64, Wave(64, 16, 0, 10, gain=G16, grids=(Grid(0, 50 * Q, WHITE, inset=8), Grid(0, 170 * Q, YELLOW, inset=7)))),
    Case("markers of width 1, 2 and 16 at both edges and off both sides", noise6000, A64,
         Wave(64, 16, 1000, 10, gain=G16, markers=(Marker(1000, CYAN, 1), Marker(1635, MAGENTA, 1), Marker(1001, YELLOW, 2), Marker(1639, BLUE, 2), Marker(1030, WHITE, 16),
                                                   Marker(1600, GREY, 16), Marker(900, RED, 16), Marker(1730, RED, 16), Marker(1720, GREEN, 16), Marker(-(1 << 62), RED, 16),
                                                   Marker((1 << 63) - 1, RED, 16), Marker(1300, CYAN, 15)))),
    Case("two markers and a grid line on one pixel", noise6000, A64, Wave(64, 16, 0, 10, gain=G16, grids=(Grid(305 * Q, 1 << 50, WHITE),),
                                                                      markers=(Marker(303, CYAN, 3), Marker(309, MAGENTA, 1)))),
    Case("lines at odd x", noise6000, A64, Wave(64, 16, 0, 10, gain=G16, grids=(Grid(15 * Q, 60 * Q, YELLOW, inset=3),), markers=(Marker(335, BLUE, 1),))),
    Case("overlapping ranges over the centre line", noise6000, A64, Wave(64, 16, 0, 50, gain=(0, 0, 20000), ranges=(Range(500, 2000, GREY), Range(1500, 2500, BLUE),
                                                                                                                   Range(1700, 1700, RED), Range(-(1 << 63), 120, MAGENTA)))),
    Case("a marker beside a grid with an inset", noise6000, A64, Wave(64, 16, 0, 10, gain=G16, grids=(Grid(0, 100 * Q, WHITE, inset=3),), markers=(Marker(255, CYAN, 2),))),
    Case("all limits at once: 16 grids, 32 markers, 8 ranges", noise6000, A64,
         Wave(256, 64, -333, 27, gain=G16,
              grids=tuple(Grid((k * 37 - 90) * Q + k, (211 + 13 * k) * Q + 7 * k, (40 + 12 * k, 30 + 11 * k, 250 - 9 * k), (k * 150 - 400) * Q, (k * 350 + 900) * Q, k * 2)
                          for k in range(16)),
              markers=tuple(Marker(k * 209 - 500, (250 - 5 * k, 20 + 7 * k, 40 + 6 * k), 1 + k % 16) for k in range(32)),
              ranges=tuple(Range(k * 700 - 600, k * 700 + 300 + 90 * k, (30 + 20 * k, 200 - 15 * k, 60 + 22 * k)) for k in range(8)))),
    Case("C = 512", lambda: ac.noise(5000, "wave 512", 9000), A512, Wave(66, 32, -700, 95, gain=G16, grids=(Grid(0, 1000 * Q, WHITE),))),
]
BY_NAME = {c.name: c for c in CASES}

_tracks, _truth = {}, {}


def track(case: Case) -> np.ndarray:
    key = case.build.__name__ if case.build.__name__ != "<lambda>" else case.name
    if key not in _tracks:
        _tracks[key] = case.build()
        _tracks[key].setflags(write=False)
    return _tracks[key]


def columns(case: Case) -> np.ndarray:
    """the analysis model's records of the case's track, computed once per (track, settings)"""
    key = (case.build.__name__ if case.build.__name__ != "<lambda>" else case.name, case.settings)
    if key not in _truth:
        cols, _ = am.analyse(track(case), case.settings)
        cols.setflags(write=False)
        _truth[key] = cols
    return _truth[key]


def truth(case: Case):
    """(Y, U, V) of the model, computed once"""
    if case.name not in _truth:
        planes = wm.render(columns(case), case.settings.column, track(case).shape[0], case.wave)
        for a in planes:
            a.setflags(write=False)
        _truth[case.name] = planes
    return _truth[case.name]


def abi_wave(p: Wave):
    """the model's settings as the library's struct"""
    from mixlab_amd import deck as dk
    return dk.waveform(p.w, p.h, p.first_frame, p.fpp, p.style, p.gain, p.bg, p.line, p.band,
                       grids=[dk.wave_grid(dk.DeckBeats(g.first_q32, g.period_q32), g.colour, g.from_q32, g.to_q32, g.inset) for g in p.grids],
                       markers=[dk.wave_marker(m.frame, m.colour, m.width) for m in p.markers], ranges=[dk.wave_range(r.from_frame, r.to_frame, r.colour) for r in p.ranges])


def abi_analysis(a: am.Settings):
    from mixlab_amd import deck as dk
    return dk.analysis(a.column, a.max_lag, a.lo, a.hi)
