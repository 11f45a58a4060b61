"""The deck (include/mixlab_gpu.h "the deck"): a track in device memory played at variable speed into a SOURCE_STEREO node.

    deck = Deck(len(track) // 2); deck.load(track_i16)
    deck.set(step_q32=deck_step(44100, 48000, 1.08), flags=abi.DECK_PLAY)
    feed([deck], [source_node], graph, n_ticks); graph.run_ticks(first_tick, n_ticks)

Key-lock (the header's KEY-LOCK) keeps the key while the step sets the tempo:

    deck.set_keylock(keylock(pitch_q32=deck_step(44100, 48000, 1.0)))     # hop 1024, overlap 256, radius 512

Analysis (the header's ANALYSIS) looks at the whole track before it sounds -- overview columns, tempo, beat grid:

    deck.analyse(rate=44100.0)                                            # 200 Hz / 2.5 kHz, 63 taps, columns of 512 frames, 256 lags
    cols, R = deck.read_columns(), deck.read_autocorr()
    grid = beatgrid(cols, R, 512, 44100.0, 60.0, 200.0)                   # grid.bpm, grid.first_beat_frame, grid.period_columns

The fine grid (the header's FINE GRID) turns that read-out into beats good to a hop of 64 frames over the whole track, and two grids into a sync:

    beats = deck.refine_grid(grid, 512, 44100.0).grid                     # first_q32, period_q32: beat n lies at first + n * period
    step, seek, _ = deck_sync(leader_beats, leader.state().pos_q32, leader.state().step_q32, beats, deck.state().pos_q32)
    deck.schedule(0, params(step_q32=step, flags=abi.DECK_PLAY), seek)    # the follower's beats now fall on the leader's, and stay there

The echo (the header's ECHO) is a feedback delay behind the deck, timed in beats; stopping the deck under it is the echo-out:

    deck.set_echo(delay=deck.echo_delay(beats, 3, 4), feedback=0.6)       # a 3/4-beat echo from the next feed on
    deck.schedule(k, params(flags=0))                                     # PLAY cleared at tick k: the tail rings over the incoming track

The sweep filter (the header's FILTER) is the one-knob resonant filter of a transition, ahead of the echo; a sweep is one setting a tick, each ramping from the last:

    deck.set_filter(filter_knob(-0.5, 48000.0))                           # a low-pass half closed, faded in over the next feed's first tick; None (the dead zone) turns it off
    deck.schedule_filter(k, kind=abi.DECK_FILTER_HP, g=0.02, k=0.5)       # ... or by the numbers, from tick k on

The reverb (the header's REVERB) is a feedback delay network behind the echo, last of the deck's passes; stopping the deck under it is the reverb-out:

    deck.set_reverb(reverb_design(48000.0, size=1.0, t60_seconds=2.5, wet=1.0))   # the wash, faded in over the next feed's first tick
    deck.schedule(k, params(flags=0))                                     # PLAY cleared at tick k: the tail rings over the incoming track

Bars (the header's BARS) say which beat is a bar's first and which bar a phrase's first; the two grids go where a beat grid goes:

    pick = deck.find_bars(beats, analysis_bands(rate=44100.0))            # pick.bars, pick.phrases: DeckBeats; pick.bar_best / pick.bar_sum the confidence
    step, seek, _ = deck_sync(leader_pick.bars, leader.state().pos_q32, leader.state().step_q32, pick.bars, deck.state().pos_q32)   # "1" on "1"
    _, line = grid_next(pick.phrases, deck.state().pos_q32)               # the coming phrase line, for an echo-out or a loop

The tempo map (the header's TEMPO MAP) follows a track whose tempo drifts: a grid per window of the track, looked up by position:

    segs = deck.map_tempo(deck.refine_grid(grid, 512, 44100.0))           # abi.DECK_TEMPO_SEGMENT_DTYPE, one per window
    beats, _ = tempomap_at(segs, deck.state().pos_q32)                    # the DeckBeats in force here: goes where a beat grid goes, asked again tick by tick
    deck.schedule_warp(segs, out_period_q32, n_ticks, spt)                # before each feed: the drifting track comes out at one constant beat length

The waveform (the header's WAVEFORM) turns the analysis' columns into a picture on the device, once per video frame -- no record is read back, no picture uploaded:

    first = waveform_view(deck.state().pos_q32, 100, 480)                 # the playing position under pixel column 480 at 100 frames a pixel
    p = waveform(1920, 128, first, 100, gain_q16=(6, 12, 24), grids=[wave_grid(beats, (90, 128, 128)), wave_grid(pick.bars, (235, 128, 128))],
                 markers=[wave_marker(deck.state().pos_q32 >> 32, (255, 128, 128), width=2)], ranges=[wave_range(loop_in, loop_out, (60, 110, 140))])
    frame = deck.render_waveform(p)                                       # a video.DFrame: into multiview(), place(), a VideoMixer or a graph's video source
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .abi import (DeckAnalysis, DeckBarPick, DeckBars, DeckBeats, DeckEcho, DeckFilter, DeckFinegrid, DeckFinePick, DeckGrain, DeckGrid, DeckHead, DeckKeylock, DeckLoudness, DeckParams, DeckReverb, DeckSyncResult, DeckTempomap,
                  DeckTick, DeckTonality, DeckWaveform, WaveColour, WaveGrid, WaveMarker, WaveRange, check, lib)

ONE = 1 << 32   # unity step / one track frame in Q32.32


def params(step_q32=0, slew_q32=0, loop_in=0, loop_out=0, flags=0) -> DeckParams:
    return DeckParams(int(step_q32), int(slew_q32), int(loop_in), int(loop_out), int(flags), 0)


def deck_check(p: DeckParams, n_frames: int) -> None:
    """the parameter rules alone (host only); raises MxError"""
    check(lib.mx_deck_check(C.byref(p), int(n_frames)))


def deck_step(track_rate: int, graph_rate: int, speed: float) -> int:
    """the Q32 step nearest to speed * track_rate / graph_rate (host only)"""
    out = C.c_int64()
    check(lib.mx_deck_step(int(track_rate), int(graph_rate), float(speed), C.byref(out)))
    return out.value


def deck_tables(bank: int) -> np.ndarray:
    """float32[257, 32]: coefficient bank `bank` as the kernel reads it (host only)"""
    if not 0 <= bank < abi.DECK_BANKS:   # before any buffer is handed over
        raise abi.MxError(abi.MX_ERR_INVALID, "bank outside 0 .. 3")
    t = np.zeros((abi.DECK_PHASES + 1, abi.DECK_TAPS), np.float32)
    check(lib.mx_deck_tables(bank, t.ctypes.data_as(C.c_void_p)))
    return t


def deck_plan(head: DeckHead, spt: int, n_frames: int, p: DeckParams | None = None, seek: int | None = None):
    """one tick of the host state machine (pure, host only): (DeckTick, DeckHead after it)"""
    tick, out = DeckTick(), DeckHead()
    s = C.c_int64(seek) if seek is not None else None
    check(lib.mx_deck_plan(C.byref(head), C.byref(p) if p is not None else None, C.byref(s) if s is not None else None, int(spt), int(n_frames),
                           C.byref(tick), C.byref(out)))
    return tick, out


def _debug_last(call, keys) -> dict:
    """the counts one mx_deck_debug_last_* call reports, under the names given"""
    out = (C.c_uint32 * len(keys))()
    check(call(out))
    return dict(zip(keys, (int(v) for v in out)))


def debug_last_feed() -> dict:
    return _debug_last(lib.mx_deck_debug_last_feed, ("ticks_zero", "ticks_stream", "ticks_gather", "chunks_zero", "chunks_stream", "chunks_gather"))


def keylock(pitch_q32=ONE, hop=1024, overlap=256, radius=512) -> DeckKeylock:
    """key-lock settings; the defaults are the header's recommendation at 44.1 / 48 kHz"""
    return DeckKeylock(int(pitch_q32), int(hop), int(overlap), int(radius), 0)


def keylock_check(k: DeckKeylock) -> None:
    """the key-lock setting rules alone (host only); raises MxError"""
    check(lib.mx_deck_keylock_check(C.byref(k)))


def keylock_search(interleaved_i16: np.ndarray, C_frame: int, A_frame: int, overlap: int, radius: int):
    """the grain search rule alone (host only, pure): (delta, dist)"""
    a = np.ascontiguousarray(interleaved_i16, dtype=np.int16).reshape(-1)
    delta, dist = C.c_int32(), C.c_uint32()
    check(lib.mx_deck_keylock_search(a.ctypes.data_as(C.c_void_p), a.size // 2, int(C_frame), int(A_frame), int(overlap), int(radius), C.byref(delta), C.byref(dist)))
    return delta.value, dist.value


def debug_last_keylock() -> dict:
    return _debug_last(lib.mx_deck_debug_last_keylock, ("grains_searched", "grains_unsearched", "chunks_fading", "chunks_straddling"))


# mx_deck_column as a numpy record: 56 bytes, the header's layout
COLUMN_DTYPE = np.dtype([("smin", "<i4"), ("smax", "<i4"), ("peak", "<u4", (3,)), ("onset", "<u4"), ("energy", "<u8", (3,)), ("e", "<u8")])


def analysis(column=512, max_lag=256, lo=(16384,), hi=(16384,), taps=None) -> DeckAnalysis:
    """analysis settings from two Q14 tap tables (the header's ANALYSIS); analysis_bands() designs them"""
    a = DeckAnalysis()
    a.column, a.taps, a.max_lag, a._pad = int(column), int(len(lo) if taps is None else taps), int(max_lag), 0
    if len(lo) != len(hi) or len(lo) > abi.DECK_ANALYSIS_MAX_TAPS:
        raise ValueError("lo and hi hold the same number of taps, 127 at the most")
    for k, (l, h) in enumerate(zip(lo, hi)):
        a.lo[k], a.hi[k] = int(l), int(h)
    return a


def analysis_bands(rate=48000.0, f_lo=200.0, f_hi=2500.0, taps=63, column=512, max_lag=256) -> DeckAnalysis:
    """settings with Hann-windowed sinc tables at the two cutoffs (mx_deck_analysis_bands, host only); the defaults are the header's recommendation"""
    a = DeckAnalysis()
    a.column, a.max_lag = int(column), int(max_lag)
    check(lib.mx_deck_analysis_bands(float(rate), float(f_lo), float(f_hi), int(taps), C.byref(a)))
    return a


def analysis_check(a: DeckAnalysis) -> None:
    """the analysis setting rules alone (host only); raises MxError"""
    check(lib.mx_deck_analysis_check(C.byref(a)))


def column_count(n_frames: int, column: int) -> int:
    n = C.c_uint64()
    check(lib.mx_deck_column_count(int(n_frames), int(column), C.byref(n)))
    return n.value


def columns_host(interleaved_i16: np.ndarray, a: DeckAnalysis, first: int = 0, n: int | None = None, autocorr: bool = False):
    """the column and onset rules in plain C++ on the host (pure): COLUMN_DTYPE[n]; with autocorr (all the columns only) also R as uint64[max_lag]"""
    x = np.ascontiguousarray(interleaved_i16, dtype=np.int16).reshape(-1)
    if n is None:
        n = column_count(x.size // 2, a.column) - first
    cols = np.zeros(max(1, n), COLUMN_DTYPE)
    R = np.zeros(a.max_lag, np.uint64) if autocorr else None
    check(lib.mx_deck_columns_host(x.ctypes.data_as(C.c_void_p), x.size // 2, C.byref(a), int(first), int(n), cols.ctypes.data_as(C.c_void_p),
                                   R.ctypes.data_as(C.c_void_p) if autocorr else None))
    return (cols[:n], R) if autocorr else cols[:n]


def beatgrid(cols: np.ndarray, R: np.ndarray, column: int, rate: float, bpm_lo: float, bpm_hi: float) -> DeckGrid:
    """tempo and beat phase from columns and their autocorrelation (mx_deck_beatgrid, host only, pure)"""
    cols = np.ascontiguousarray(cols, dtype=COLUMN_DTYPE)
    R = np.ascontiguousarray(R, dtype=np.uint64)
    g = DeckGrid()
    check(lib.mx_deck_beatgrid(cols.ctypes.data_as(C.c_void_p) if cols.size else None, cols.size, R.ctypes.data_as(C.c_void_p), R.size, int(column),
                               float(rate), float(bpm_lo), float(bpm_hi), C.byref(g)))
    return g


def debug_last_analysis() -> dict:
    return _debug_last(lib.mx_deck_debug_last_analysis, ("wgs_several_columns", "wgs_tiled_column", "short_track", "wgs_one_column"))


def tonality(rate=48000.0, decim=8, hop_frames=512, octaves=5, f_lo_mhz=65406, segment_hops=64) -> DeckTonality:
    """whole-track tonality settings (the header's KEY AND LOUDNESS); the defaults are five octaves from C2 in segments of 64 hops (5.5 s at 48 kHz)"""
    return DeckTonality(float(rate), int(decim), int(hop_frames), int(octaves), int(f_lo_mhz), int(segment_hops), 0)


def tonality_check(t: DeckTonality) -> None:
    """the tonality setting rules alone (host only); raises MxError"""
    check(lib.mx_deck_tonality_check(C.byref(t)))


def tonality_count(n_frames: int, t: DeckTonality) -> int:
    n = C.c_uint64()
    check(lib.mx_deck_tonality_count(int(n_frames), C.byref(t), C.byref(n)))
    return n.value


def tonality_host(interleaved_i16: np.ndarray, t: DeckTonality, first: int = 0, n: int | None = None) -> list:
    """the tonality rules in plain C++ on the host (pure): segments [first, first + n) as abi.parse_tonality_records dicts"""
    x = np.ascontiguousarray(interleaved_i16, dtype=np.int16).reshape(-1)
    if n is None:
        n = tonality_count(x.size // 2, t) - first
    tonality_check(t)   # before a buffer is sized from the settings
    rb = 32 + 96 * t.octaves
    raw = np.zeros(max(1, n) * rb, np.uint8)
    check(lib.mx_deck_tonality_host(x.ctypes.data_as(C.c_void_p), x.size // 2, C.byref(t), int(first), int(n), raw.ctypes.data_as(C.c_void_p)))
    return abi.parse_tonality_records(raw[:n * rb], t.octaves)


def debug_last_tonality() -> dict:
    return _debug_last(lib.mx_deck_debug_last_tonality, ("wgs_decimate", "wgs_cq_full", "wgs_cq_part", "wgs_head"))


def loudness(rate=48000.0, block_frames=4800, momentary_blocks=4, short_blocks=30) -> DeckLoudness:
    """whole-track loudness settings (the header's KEY AND LOUDNESS); the defaults are 100 ms blocks at 48 kHz, 400 ms and 3 s windows"""
    return DeckLoudness(float(rate), int(block_frames), int(momentary_blocks), int(short_blocks), 0)


def loudness_check(l: DeckLoudness) -> None:
    """the loudness setting rules alone (host only); raises MxError"""
    check(lib.mx_deck_loudness_check(C.byref(l)))


def loudness_count(n_frames: int, block_frames: int) -> int:
    n = C.c_uint64()
    check(lib.mx_deck_loudness_count(int(n_frames), int(block_frames), C.byref(n)))
    return n.value


def loudness_host(interleaved_i16: np.ndarray, l: DeckLoudness) -> np.ndarray:
    """the loudness rules in plain C++ on the host (pure), the whole track: abi.LOUDNESS_TICK_DTYPE[n_blocks]"""
    x = np.ascontiguousarray(interleaved_i16, dtype=np.int16).reshape(-1)
    n = loudness_count(x.size // 2, l.block_frames)
    out = np.zeros(n, abi.LOUDNESS_TICK_DTYPE)
    check(lib.mx_deck_loudness_host(x.ctypes.data_as(C.c_void_p), x.size // 2, C.byref(l), out.ctypes.data_as(C.c_void_p), n))
    return out


def debug_last_loudness() -> dict:
    return _debug_last(lib.mx_deck_debug_last_loudness, ("wgs_peak", "wgs_walk", "scan_steps", "wgs_window"))


def loudness_gain(recs: np.ndarray, momentary_blocks: int = 4, hop_blocks: int = 1, target_lufs: float = -14.0, ceiling_dbtp: float = -1.0):
    """(integrated LUFS, true peak in dBTP, gain in dB that reaches the target under the ceiling) from loudness records (mx_deck_loudness_gain, host only)"""
    r = np.ascontiguousarray(recs, dtype=abi.LOUDNESS_TICK_DTYPE)
    lufs, peak, gain = C.c_double(), C.c_double(), C.c_double()
    check(lib.mx_deck_loudness_gain(r.ctypes.data_as(C.c_void_p) if r.size else None, r.size, int(momentary_blocks), int(hop_blocks), float(target_lufs),
                                    float(ceiling_dbtp), C.byref(lufs), C.byref(peak), C.byref(gain)))
    return lufs.value, peak.value, gain.value


def camelot(key: int) -> str:
    """the Camelot wheel position of a key of abi.tonality_key: "8B" is C major, "8A" A minor (mx_tonality_camelot, host only)"""
    number, minor = C.c_uint32(), C.c_uint32()
    check(lib.mx_tonality_camelot(int(key), C.byref(number), C.byref(minor)))
    return f"{number.value}{'A' if minor.value else 'B'}"


def finegrid(hop=64, n_periods=1, period0_q16=4 << 16, dperiod_q16=0, first_hop=0, max_beats=0) -> DeckFinegrid:
    """fine-grid settings (the header's FINE GRID): candidate j has the period period0_q16 + j * dperiod_q16 in hops of `hop` frames, Q16"""
    return DeckFinegrid(int(hop), int(n_periods), int(period0_q16), int(dperiod_q16), int(first_hop), int(max_beats), 0)


def finegrid_check(s: DeckFinegrid, n_frames: int) -> None:
    """the fine-grid setting rules alone for a track of n_frames (host only); raises MxError"""
    check(lib.mx_deck_finegrid_check(C.byref(s), int(n_frames)))


def finegrid_count(n_frames: int, hop: int) -> int:
    n = C.c_uint64()
    check(lib.mx_deck_finegrid_count(int(n_frames), int(hop), C.byref(n)))
    return n.value


def finegrid_span(centre_q16: int, halfwidth_q16: int, beat_limit: int, n_hops: int, hop: int):
    """the settings of one stage of a search round a centre period (mx_deck_finegrid_span, host only, pure): (DeckFinegrid, clipped)"""
    s, clipped = DeckFinegrid(), C.c_uint32()
    check(lib.mx_deck_finegrid_span(int(centre_q16), int(halfwidth_q16), int(beat_limit), int(n_hops), int(hop), C.byref(s), C.byref(clipped)))
    return s, bool(clipped.value)


def finegrid_period(period_columns: float, column: int, hop: int) -> int:
    """a coarse DeckGrid.period_columns in fine hops, Q16 (mx_deck_finegrid_period, host only)"""
    p = C.c_uint64()
    check(lib.mx_deck_finegrid_period(float(period_columns), int(column), int(hop), C.byref(p)))
    return p.value


def finegrid_host(interleaved_i16: np.ndarray, s: DeckFinegrid, onsets: bool = False):
    """the fine-grid rules in plain C++ on the host (pure): abi.DECK_COMB_DTYPE[n_periods]; with onsets also w as uint32[N]"""
    x = np.ascontiguousarray(interleaved_i16, dtype=np.int16).reshape(-1)
    finegrid_check(s, x.size // 2)   # before a buffer is sized from the settings
    recs = np.zeros(s.n_periods, abi.DECK_COMB_DTYPE)
    w = np.zeros(finegrid_count(x.size // 2, s.hop), np.uint32) if onsets else None
    check(lib.mx_deck_finegrid_host(x.ctypes.data_as(C.c_void_p), x.size // 2, C.byref(s), recs.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p) if onsets else None))
    return (recs, w) if onsets else recs


def finegrid_pick(recs: np.ndarray, s: DeckFinegrid, rate: float) -> DeckFinePick:
    """the best candidate of one stage as beats in track frames, Q32.32 (mx_deck_finegrid_pick, host only, pure): .grid, .index, .score, .n_beats, .bpm"""
    r = np.ascontiguousarray(recs, dtype=abi.DECK_COMB_DTYPE)
    if r.size != s.n_periods:
        raise ValueError("one record per candidate period")
    out = DeckFinePick()
    check(lib.mx_deck_finegrid_pick(r.ctypes.data_as(C.c_void_p), C.byref(s), float(rate), C.byref(out)))
    return out


def deck_sync(leader: DeckBeats, leader_pos_q32: int, leader_step_q32: int, follower: DeckBeats, follower_pos_q32: int):
    """(step, seek, delta) that put the follower's beats on the leader's, all Q32.32 and exact (mx_deck_sync, host only, pure); hand step and seek to Deck.schedule"""
    out = DeckSyncResult()
    check(lib.mx_deck_sync(C.byref(leader), int(leader_pos_q32), int(leader_step_q32), C.byref(follower), int(follower_pos_q32), C.byref(out)))
    return out.step_q32, out.seek_q32, out.delta_q32


def debug_last_finegrid() -> dict:
    return _debug_last(lib.mx_deck_debug_last_finegrid, ("wgs_one_pass", "wgs_strided", "wgs_onset", "trip"))


def echo(delay, send=1.0, feedback=0.5, wet=1.0, damp=0.0, pingpong=False) -> DeckEcho:
    """echo settings (the header's ECHO): delay in output frames (echo_delay() turns a beat fraction into one), the three gains, the damping, ping-pong"""
    return DeckEcho(int(delay), abi.DECK_ECHO_PINGPONG if pingpong else 0, float(send), float(feedback), float(wet), float(damp))


def echo_check(e: DeckEcho) -> None:
    """the echo setting rules alone (host only); raises MxError"""
    check(lib.mx_deck_echo_check(C.byref(e)))


def echo_delay(grid: DeckBeats, step_q32: int, num: int, den: int) -> int:
    """the output frames of num / den beats of `grid` at this step, exactly, ties to even (mx_deck_echo_delay, host only, pure)"""
    out = C.c_uint32()
    check(lib.mx_deck_echo_delay(C.byref(grid), int(step_q32), int(num), int(den), C.byref(out)))
    return out.value


def echo_plan(spt: int, delays) -> list:
    """the blocks the echo kernel cuts a feed into, as (first frame, frames) (mx_deck_echo_plan, host only, pure); delays: one per tick, 0 for a tick without an echo"""
    d = np.ascontiguousarray(delays, dtype=np.uint32)
    n = C.c_uint32()
    check(lib.mx_deck_echo_plan(int(spt), d.ctypes.data_as(C.c_void_p) if d.size else None, d.size, None, 0, C.byref(n)))
    out = np.zeros((max(1, n.value), 2), np.uint64)
    check(lib.mx_deck_echo_plan(int(spt), d.ctypes.data_as(C.c_void_p) if d.size else None, d.size, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    return [(int(a), int(b)) for a, b in out[:n.value]]


def debug_last_echo() -> dict:
    return _debug_last(lib.mx_deck_debug_last_echo, ("decks_one_block", "decks_sequential", "blocks", "blocks_crossing"))


def filt(kind=abi.DECK_FILTER_LP, g=1.0, k=1.0, wet=1.0) -> DeckFilter:
    """sweep filter settings (the header's FILTER): the response, g = tan(pi fc / rate), k = 1 / Q, the wet mix; filter_design() and filter_knob() start from Hz"""
    return DeckFilter(int(kind), 0, float(g), float(k), float(wet), 0)


def filter_check(f: DeckFilter) -> None:
    """the filter setting rules alone (host only); raises MxError"""
    check(lib.mx_deck_filter_check(C.byref(f)))


def filter_design(kind: int, cutoff_hz: float, q: float, rate: float, wet: float = 1.0) -> DeckFilter:
    """the settings of a cutoff and a Q at this rate (mx_deck_filter_design, host only; libm, good to 1 f32 ulp)"""
    out = DeckFilter()
    check(lib.mx_deck_filter_design(int(kind), float(cutoff_hz), float(q), float(rate), float(wet), C.byref(out)))
    return out


def filter_knob(knob: float, rate: float, q: float = 2.0) -> DeckFilter | None:
    """the DJ mapping of one knob in -1 .. 1 (mx_deck_filter_knob, host only): None in the dead zone, a low-pass closing to the left, a high-pass opening to the right"""
    out, on = DeckFilter(), C.c_uint32()
    check(lib.mx_deck_filter_knob(float(knob), float(rate), float(q), C.byref(out), C.byref(on)))
    return out if on.value else None


def filter_host(frames: np.ndarray, spt: int, settings, carry: abi.DeckFilterCarry | None = None):
    """(float32 frames after the filter, the carried block) of mx_deck_filter_host (host only, pure): frames float32 [n_ticks * spt * 2], settings one DeckFilter or
    None per tick, carry what the last call returned (None: a deck that never had a filter)"""
    out = np.ascontiguousarray(frames, np.float32).reshape(-1).copy()
    n_ticks = len(settings)
    assert out.size == n_ticks * int(spt) * 2
    carry = abi.DeckFilterCarry.from_buffer_copy(carry) if carry is not None else abi.DeckFilterCarry()
    ptrs = (C.POINTER(DeckFilter) * max(1, n_ticks))(*[C.pointer(f) if f is not None else None for f in settings])
    check(lib.mx_deck_filter_host(out.ctypes.data_as(C.c_void_p) if out.size else None, int(spt), n_ticks, C.cast(ptrs, C.c_void_p) if n_ticks else None, C.byref(carry)))
    return out, carry


def debug_last_filter() -> dict:
    return _debug_last(lib.mx_deck_debug_last_filter, ("decks", "ticks_ramp", "ticks_constant", "blocks"))


def reverb(delay, diff, gain, send=1.0, dry=1.0, wet=0.5, damp=0.0, diffusion=0.5) -> DeckReverb:
    """reverb settings (the header's REVERB) by the numbers: eight tank delays, four diffuser delays, eight gains; reverb_design() starts from a size and a decay time"""
    return DeckReverb((C.c_uint32 * 8)(*[int(v) for v in delay]), (C.c_uint32 * 4)(*[int(v) for v in diff]), (C.c_float * 8)(*[float(v) for v in gain]),
                      float(send), float(dry), float(wet), float(damp), float(diffusion), 0)


def reverb_check(r: DeckReverb) -> None:
    """the reverb setting rules alone (host only); raises MxError"""
    check(lib.mx_deck_reverb_check(C.byref(r)))


def reverb_design(rate: float, size: float = 1.0, t60_seconds: float = 2.0, damp: float = 0.3, diffusion: float = 0.5, send: float = 1.0, dry: float = 1.0,
                  wet: float = 0.5) -> DeckReverb:
    """the setting of a room size (0.25 .. 4) and a decay time at this rate (mx_deck_reverb_design, host only): prime delays, exact; gains good to 1 f32 ulp"""
    out = DeckReverb()
    check(lib.mx_deck_reverb_design(float(rate), float(size), float(t60_seconds), float(damp), float(diffusion), float(send), float(dry), float(wet), C.byref(out)))
    return out


def _reverb_ptrs(settings):
    return (C.POINTER(DeckReverb) * max(1, len(settings)))(*[C.pointer(r) if r is not None else None for r in settings])


def reverb_plan(spt: int, settings) -> list:
    """the blocks the reverb kernel cuts a feed into, as (first frame, frames) (mx_deck_reverb_plan, host only, pure); settings: one DeckReverb or None per tick"""
    ptrs, n_ticks, n = _reverb_ptrs(settings), len(settings), C.c_uint32()
    check(lib.mx_deck_reverb_plan(int(spt), C.cast(ptrs, C.c_void_p) if n_ticks else None, n_ticks, None, 0, C.byref(n)))
    out = np.zeros((max(1, n.value), 2), np.uint64)
    check(lib.mx_deck_reverb_plan(int(spt), C.cast(ptrs, C.c_void_p) if n_ticks else None, n_ticks, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
    return [(int(a), int(b)) for a, b in out[:n.value]]


def reverb_host(frames: np.ndarray, spt: int, settings, lines: np.ndarray | None = None, carry: abi.DeckReverbCarry | None = None):
    """(float32 frames after the reverb, the lines, the carried block) of mx_deck_reverb_host (host only, pure): frames float32 [n_ticks * spt * 2], settings one
    DeckReverb or None per tick, lines and carry what the last call returned (None: a deck that never had a reverb)"""
    out = np.ascontiguousarray(frames, np.float32).reshape(-1).copy()
    n_ticks = len(settings)
    assert out.size == n_ticks * int(spt) * 2
    lines = np.ascontiguousarray(lines, np.float32).copy() if lines is not None else np.zeros(abi.DECK_REVERB_LINE_FLOATS, np.float32)
    assert lines.size == abi.DECK_REVERB_LINE_FLOATS
    carry = abi.DeckReverbCarry.from_buffer_copy(carry) if carry is not None else abi.DeckReverbCarry()
    ptrs = _reverb_ptrs(settings)
    check(lib.mx_deck_reverb_host(out.ctypes.data_as(C.c_void_p) if out.size else None, int(spt), n_ticks, C.cast(ptrs, C.c_void_p) if n_ticks else None,
                                  lines.ctypes.data_as(C.c_void_p), C.byref(carry)))
    return out, lines, carry


def debug_last_reverb() -> dict:
    return _debug_last(lib.mx_deck_debug_last_reverb, ("decks", "blocks", "blocks_crossing", "largest_block"))


def bars(grid: DeckBeats, tables: DeckAnalysis | None = None, lead=128, beats_per_bar=4, bars_per_phrase=4, w_bar=4, w_phrase=8, max_beats=0) -> DeckBars:
    """bars settings (the header's BARS) on a beat grid; the tap tables are those of `tables` (mx_deck_bars_tables), a single unity tap without it"""
    s = DeckBars()
    s.grid = DeckBeats(int(grid.first_q32), int(grid.period_q32))
    s.lead, s.beats_per_bar, s.bars_per_phrase, s.w_bar, s.w_phrase, s.max_beats = int(lead), int(beats_per_bar), int(bars_per_phrase), int(w_bar), int(w_phrase), int(max_beats)
    check(lib.mx_deck_bars_tables(C.byref(tables if tables is not None else analysis()), C.byref(s)))
    return s


def bars_check(s: DeckBars, n_frames: int) -> None:
    """the bars setting rules alone for a track of n_frames (host only); raises MxError"""
    check(lib.mx_deck_bars_check(C.byref(s), int(n_frames)))


def bars_count(s: DeckBars, n_frames: int):
    """(n_beats, n0): the whole beats the grid places in the track, and the grid index of the first (mx_deck_bars_count, host only)"""
    n, n0 = C.c_uint32(), C.c_int64()
    check(lib.mx_deck_bars_count(C.byref(s), int(n_frames), C.byref(n), C.byref(n0)))
    return n.value, n0.value


def bars_host(interleaved_i16: np.ndarray, s: DeckBars):
    """the bars rules in plain C++ on the host (pure): (abi.DECK_BEAT_DTYPE[n_beats], the folds as uint64[M + M Q])"""
    x = np.ascontiguousarray(interleaved_i16, dtype=np.int16).reshape(-1)
    n, _ = bars_count(s, x.size // 2)   # before a buffer is sized from the settings
    recs = np.zeros(n, abi.DECK_BEAT_DTYPE)
    H = np.zeros(s.beats_per_bar * (1 + s.bars_per_phrase), np.uint64)
    check(lib.mx_deck_bars_host(x.ctypes.data_as(C.c_void_p), x.size // 2, C.byref(s), recs.ctypes.data_as(C.c_void_p), H.ctypes.data_as(C.c_void_p)))
    return recs, H


def bars_pick(folds: np.ndarray, s: DeckBars) -> DeckBarPick:
    """the downbeat and the phrase line as two grids (mx_deck_bars_pick, host only, pure): .bars, .phrases, the two phases and the four sums"""
    H = np.zeros(abi.DECK_BARS_MAX_FOLDS, np.uint64)   # room for any M + M Q, whatever the settings say
    f = np.asarray(folds, dtype=np.uint64).reshape(-1)
    H[:min(f.size, H.size)] = f[:H.size]
    out = DeckBarPick()
    check(lib.mx_deck_bars_pick(H.ctypes.data_as(C.c_void_p), C.byref(s), C.byref(out)))
    return out


def grid_next(grid: DeckBeats, pos_q32: int):
    """(n, line): the first line of a beat, bar or phrase grid at or after pos_q32, and its index (mx_deck_grid_next, host only, pure)"""
    n, line = C.c_int64(), C.c_int64()
    check(lib.mx_deck_grid_next(C.byref(grid), int(pos_q32), C.byref(n), C.byref(line)))
    return n.value, line.value


def debug_last_bars() -> dict:
    return _debug_last(lib.mx_deck_debug_last_bars, ("wgs_half_one_tile", "wgs_half_tiled", "wgs_novelty", "novelties_defined"))


def tempomap(hop=64, n_periods=1, period0_q16=4 << 16, dperiod_q16=0, window_hops=16, stride_hops=8) -> DeckTempomap:
    """tempo map settings (the header's TEMPO MAP): candidate periods in hops of `hop` frames, Q16, searched in windows of window_hops every stride_hops"""
    return DeckTempomap(int(hop), int(n_periods), int(period0_q16), int(dperiod_q16), int(window_hops), int(stride_hops), 0)


def tempomap_check(s: DeckTempomap, n_frames: int) -> None:
    """the tempo map setting rules alone for a track of n_frames (host only); raises MxError"""
    check(lib.mx_deck_tempomap_check(C.byref(s), int(n_frames)))


def tempomap_count(s: DeckTempomap, n_frames: int) -> int:
    """V, the windows of a track of n_frames (host only)"""
    n = C.c_uint32()
    check(lib.mx_deck_tempomap_count(C.byref(s), int(n_frames), C.byref(n)))
    return n.value


def tempomap_span(centre_q16: int, halfwidth_q16: int, window_beats: int, stride_beats: int, n_hops: int, hop: int):
    """the settings of a windowed search round a centre period (mx_deck_tempomap_span, host only, pure): (DeckTempomap, clipped)"""
    s, clipped = DeckTempomap(), C.c_uint32()
    check(lib.mx_deck_tempomap_span(int(centre_q16), int(halfwidth_q16), int(window_beats), int(stride_beats), int(n_hops), int(hop), C.byref(s), C.byref(clipped)))
    return s, bool(clipped.value)


def tempomap_host(interleaved_i16: np.ndarray, s: DeckTempomap, onsets: bool = False):
    """the tempo map rules in plain C++ on the host (pure): abi.DECK_COMB_DTYPE[V, n_periods], and with onsets=True (records, w as uint32[N])"""
    x = np.ascontiguousarray(interleaved_i16, dtype=np.int16).reshape(-1)
    V = tempomap_count(s, x.size // 2)   # before a buffer is sized from the settings
    recs = np.zeros((V, s.n_periods), abi.DECK_COMB_DTYPE)
    w = np.zeros(finegrid_count(x.size // 2, s.hop), np.uint32) if onsets else None
    check(lib.mx_deck_tempomap_host(x.ctypes.data_as(C.c_void_p), x.size // 2, C.byref(s), recs.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p) if onsets else None))
    return (recs, w) if onsets else recs


def tempomap_path(recs: np.ndarray, penalty: int) -> np.ndarray:
    """one candidate index per window, uint32[V], through records of shape [V, n_periods] (mx_deck_tempomap_path, host only, pure); penalty 0 is the per-window pick"""
    r = np.ascontiguousarray(recs, dtype=abi.DECK_COMB_DTYPE)
    if r.ndim != 2 or not r.size:
        raise abi.MxError(abi.MX_ERR_INVALID, "recs must have the shape [windows, n_periods], neither 0")
    if not 0 <= int(penalty) < 1 << 64:
        raise abi.MxError(abi.MX_ERR_INVALID, "penalty outside uint64")
    index = np.zeros(r.shape[0], np.uint32)
    check(lib.mx_deck_tempomap_path(r.ctypes.data_as(C.c_void_p), r.shape[0], r.shape[1], int(penalty), index.ctypes.data_as(C.c_void_p)))
    return index


def tempomap_segments(recs: np.ndarray, s: DeckTempomap, n_frames: int, index: np.ndarray) -> np.ndarray:
    """abi.DECK_TEMPO_SEGMENT_DTYPE[V]: the path's grids, starts and flags (mx_deck_tempomap_segments, host only, pure)"""
    V = tempomap_count(s, n_frames)
    r = np.ascontiguousarray(recs, dtype=abi.DECK_COMB_DTYPE).reshape(-1)
    ix = np.ascontiguousarray(index, dtype=np.uint32).reshape(-1)
    if r.size != V * s.n_periods or ix.size != V:
        raise abi.MxError(abi.MX_ERR_INVALID, "recs / index do not have the settings' windows x n_periods / windows")
    segs = np.zeros(V, abi.DECK_TEMPO_SEGMENT_DTYPE)
    check(lib.mx_deck_tempomap_segments(r.ctypes.data_as(C.c_void_p), C.byref(s), int(n_frames), ix.ctypes.data_as(C.c_void_p), segs.ctypes.data_as(C.c_void_p)))
    return segs


def tempomap_at(segs: np.ndarray, pos_q32: int):
    """(DeckBeats, segment): the grid in force at pos_q32 and its segment's index (mx_deck_tempomap_at, host only, pure)"""
    g = np.ascontiguousarray(segs, dtype=abi.DECK_TEMPO_SEGMENT_DTYPE).reshape(-1)
    grid, seg = DeckBeats(), C.c_uint32()
    check(lib.mx_deck_tempomap_at(g.ctypes.data_as(C.c_void_p) if g.size else None, g.size, int(pos_q32), C.byref(grid), C.byref(seg)))
    return grid, seg.value


def tempomap_step(grid: DeckBeats, out_period_q32: int) -> int:
    """the step at which the beats of `grid` come out out_period_q32 / 2^32 output frames apart (mx_deck_tempomap_step, host only, pure, exact)"""
    step = C.c_int64()
    check(lib.mx_deck_tempomap_step(C.byref(grid), int(out_period_q32), C.byref(step)))
    return step.value


def tempomap_beats(segs: np.ndarray, end_q32: int) -> list:
    """[(position, segment)]: the beats of the map in [0, end_q32), in Python integers -- per segment the lines b of its grid with start <= b and b + period / 2 <= the
    next segment's start (the header's SEGMENTS); a segment without a period has none"""
    out = []
    for v, g in enumerate(segs):
        first, period = int(g["first_q32"]), int(g["period_q32"])
        if period <= 0:
            continue
        b = first + -((first - max(int(g["start_q32"]), 0)) // period) * period     # mx_deck_grid_next
        last = v + 1 == len(segs)
        while b < end_q32 and (last or b + period // 2 <= int(segs[v + 1]["start_q32"])):
            out.append((b, v))
            b += period
    return out


def debug_last_tempomap() -> dict:
    return _debug_last(lib.mx_deck_debug_last_tempomap, ("wgs_staged", "wgs_global", "wgs_onset", "trip"))


def _colour(c) -> WaveColour:
    return c if isinstance(c, WaveColour) else WaveColour(int(c[0]), int(c[1]), int(c[2]), 0)


def wave_grid(grid, colour, from_q32: int = -(1 << 62), to_q32: int = 1 << 62, inset: int = 0, which: str = "bars") -> WaveGrid:
    """one grid entry of a waveform from a DeckBeats, a DeckFinePick (its grid) or a DeckBarPick (its bars, or its phrases with which="phrases")"""
    if isinstance(grid, DeckFinePick):
        grid = grid.grid
    elif isinstance(grid, DeckBarPick):
        grid = grid.phrases if which == "phrases" else grid.bars
    return WaveGrid(DeckBeats(int(grid.first_q32), int(grid.period_q32)), int(from_q32), int(to_q32), _colour(colour), int(inset))


def wave_grids_tempomap(segs: np.ndarray, colour, inset: int = 0, end_q32: int = 1 << 62) -> list:
    """one grid entry per tempo-map segment that places beats (tempomap_segments' records), each over [its start, the next one's start); a picture takes 16"""
    out = []
    for v in range(len(segs)):
        if int(segs[v]["period_q32"]) <= 0:
            continue
        start = max(int(segs[v]["start_q32"]), -(1 << 62))
        stop = int(segs[v + 1]["start_q32"]) if v + 1 < len(segs) else int(end_q32)
        if start < stop:
            out.append(WaveGrid(DeckBeats(int(segs[v]["first_q32"]), int(segs[v]["period_q32"])), start, stop, _colour(colour), int(inset)))
    return out


def wave_marker(frame: int, colour, width: int = 1) -> WaveMarker:
    return WaveMarker(int(frame), int(width), _colour(colour))


def wave_range(from_frame: int, to_frame: int, colour) -> WaveRange:
    return WaveRange(int(from_frame), int(to_frame), _colour(colour), 0)


def waveform(w: int, h: int, first_frame: int, frames_per_px: int, style: int = abi.WAVE_BANDS, gain_q16=(1 << 16, 1 << 16, 1 << 16), bg=(16, 128, 128),
             line=(64, 128, 128), band=((81, 90, 240), (145, 54, 34), (210, 146, 16)), grids=(), markers=(), ranges=()) -> DeckWaveform:
    """waveform settings (the header's WAVEFORM); colours are (Y, U, V); grids / markers / ranges from wave_grid(), wave_marker(), wave_range()"""
    if len(grids) > abi.WAVE_MAX_GRIDS or len(markers) > abi.WAVE_MAX_MARKERS or len(ranges) > abi.WAVE_MAX_RANGES:
        raise ValueError("a waveform takes 16 grids, 32 markers and 8 ranges at the most")
    p = DeckWaveform()
    p.w, p.h, p.first_frame, p.frames_per_px, p.style = int(w), int(h), int(first_frame), int(frames_per_px), int(style)
    for b in range(3):
        p.gain_q16[b] = int(gain_q16[b])
        p.band[b] = _colour(band[b])
    p.bg, p.line = _colour(bg), _colour(line)
    p.n_grids, p.n_markers, p.n_ranges = len(grids), len(markers), len(ranges)
    for k, g in enumerate(grids):
        p.grid[k] = g
    for k, m in enumerate(markers):
        p.marker[k] = m
    for k, r in enumerate(ranges):
        p.range[k] = r
    return p


def waveform_check(p: DeckWaveform) -> None:
    """the waveform setting rules alone (host only); raises MxError"""
    check(lib.mx_deck_waveform_check(C.byref(p)))


def waveform_view(pos_q32: int, frames_per_px: int, playhead_x: int) -> int:
    """the first_frame that puts the position pos_q32 in pixel column playhead_x (mx_deck_waveform_view, host only)"""
    f = C.c_int64()
    check(lib.mx_deck_waveform_view(int(pos_q32), int(frames_per_px), int(playhead_x), C.byref(f)))
    return f.value


def waveform_host(cols: np.ndarray, column: int, n_frames: int, p: DeckWaveform, y_stride: int | None = None, c_stride: int | None = None, fill: int = 0):
    """the picture in plain C++ on the host (pure): (y, u, v) uint8 arrays of h x y_stride, h / 2 x c_stride and again, pre-filled with `fill`; the picture is
    their first w (w / 2) columns, and the rest is left alone"""
    cols = np.ascontiguousarray(cols, dtype=COLUMN_DTYPE)
    ys, cs = int(p.w if y_stride is None else y_stride), int(p.w // 2 if c_stride is None else c_stride)
    y = np.full((p.h, max(1, ys)), fill, np.uint8)
    u, v = np.full((p.h // 2, max(1, cs)), fill, np.uint8), np.full((p.h // 2, max(1, cs)), fill, np.uint8)
    check(lib.mx_deck_waveform_host(cols.ctypes.data_as(C.c_void_p) if cols.size else None, cols.size, int(column), int(n_frames), C.byref(p),
                                    y.ctypes.data_as(C.c_void_p), ys, u.ctypes.data_as(C.c_void_p), v.ctypes.data_as(C.c_void_p), cs))
    return y, u, v


def debug_last_waveform() -> dict:
    return _debug_last(lib.mx_deck_debug_last_waveform, ("strips_single", "strips_several", "strips_outside", "max_records"))


_NOT_GIVEN = object()   # Deck.analyse_finegrid: no settings argument at all, as against None


class Deck:
    """Thin RAII wrapper of mx_deck_*."""

    def __init__(self, n_frames: int, device: int = -1):
        self._h = C.c_void_p()
        self.n_frames = int(n_frames)
        # the counts of each analysis' last analyse*() that succeeded (the library has no call that tells them); None: no results
        self._analysis = None    # (columns, max_lag)
        self._tonality = None    # (segments, octaves)
        self._loudness = None    # blocks
        self._finegrid = None    # (n_periods, hops)
        self._bars = None        # (n_beats, M + M Q)
        self._tempomap = None    # (windows * n_periods, hops)
        check(lib.mx_deck_create(self.n_frames, device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            lib.mx_deck_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def load(self, interleaved_i16: np.ndarray, first_frame: int = 0):
        a = np.ascontiguousarray(interleaved_i16, dtype=np.int16).reshape(-1)
        check(lib.mx_deck_load_i16(self._h, int(first_frame), a.ctypes.data_as(C.c_void_p), a.size // 2))

    def set(self, p: DeckParams | None = None, **kw):
        p = p if p is not None else params(**kw)
        check(lib.mx_deck_set(self._h, C.byref(p)))

    def seek(self, pos_q32: int):
        check(lib.mx_deck_seek(self._h, int(pos_q32)))

    def schedule(self, tick_in_feed: int, p: DeckParams | None = None, seek: int | None = None):
        s = C.c_int64(seek) if seek is not None else None
        check(lib.mx_deck_schedule(self._h, int(tick_in_feed), C.byref(p) if p is not None else None, C.byref(s) if s is not None else None))

    def read_ticks(self, first: int, n: int) -> list[DeckTick]:
        arr = (DeckTick * max(1, n))()
        check(lib.mx_deck_read_ticks(self._h, int(first), int(n), arr))
        return list(arr[:n])

    def set_keylock(self, k: DeckKeylock | None = None, **kw):
        """key-lock from the next feed on; set_keylock(None) with no keywords turns it off"""
        k = k if k is not None else (keylock(**kw) if kw else None)
        check(lib.mx_deck_set_keylock(self._h, C.byref(k) if k is not None else None))

    def grain_count(self) -> int:
        n = C.c_uint32()
        check(lib.mx_deck_grain_count(self._h, C.byref(n)))
        return n.value

    def read_grains(self, first: int = 0, n: int | None = None) -> list[DeckGrain]:
        """the grains that started in the last feed; waits for the feed's kernels"""
        n = self.grain_count() - first if n is None else n
        arr = (DeckGrain * max(1, n))()
        check(lib.mx_deck_read_grains(self._h, int(first), int(n), arr))
        return list(arr[:n])

    def set_echo(self, e: DeckEcho | None = None, **kw):
        """the echo from tick 0 of the next feed on; keywords are echo()'s; set_echo(None) with no keywords turns it off"""
        e = e if e is not None else (echo(**kw) if kw else None)
        check(lib.mx_deck_set_echo(self._h, C.byref(e) if e is not None else None))

    def schedule_echo(self, tick_in_feed: int, e: DeckEcho | None = None, **kw):
        """... from that tick of the next feed on (the echo-out lands on a beat inside a long feed); None with no keywords turns it off there"""
        e = e if e is not None else (echo(**kw) if kw else None)
        check(lib.mx_deck_schedule_echo(self._h, int(tick_in_feed), C.byref(e) if e is not None else None))

    def echo_delay(self, grid: DeckBeats, num: int, den: int) -> int:
        """the delay of num / den beats of `grid` at the step the head moves at now (after the last feed)"""
        return echo_delay(grid, self.state().step_q32, num, den)

    def echo_state(self):
        """(clock t, on, DeckEcho in force) after the last feed; host data, no synchronisation"""
        t, on, e = C.c_uint64(), C.c_uint32(), DeckEcho()
        check(lib.mx_deck_echo_state(self._h, C.byref(t), C.byref(on), C.byref(e)))
        return t.value, bool(on.value), e

    def set_filter(self, f: DeckFilter | None = None, **kw):
        """the sweep filter from tick 0 of the next feed on; keywords are filt()'s; set_filter(None) with no keywords turns it off"""
        f = f if f is not None else (filt(**kw) if kw else None)
        check(lib.mx_deck_set_filter(self._h, C.byref(f) if f is not None else None))

    def schedule_filter(self, tick_in_feed: int, f: DeckFilter | None = None, **kw):
        """... from that tick of the next feed on (a sweep is one setting a tick: each ramps from the last); None with no keywords turns it off there"""
        f = f if f is not None else (filt(**kw) if kw else None)
        check(lib.mx_deck_schedule_filter(self._h, int(tick_in_feed), C.byref(f) if f is not None else None))

    def filter_state(self):
        """(on, DeckFilter in force) after the last feed; host data, no synchronisation"""
        on, f = C.c_uint32(), DeckFilter()
        check(lib.mx_deck_filter_state(self._h, C.byref(on), C.byref(f)))
        return bool(on.value), f

    def read_filter_state(self) -> np.ndarray:
        """float64 [4]: s1 s2 of L, s1 s2 of R after the last feed (waits for the device); zeros when the filter is off or was never on"""
        s = (C.c_double * 4)()
        check(lib.mx_deck_read_filter_state(self._h, s))
        return np.array(s[:], np.float64)

    def set_reverb(self, r: DeckReverb | None = None, **kw):
        """the reverb from tick 0 of the next feed on; keywords are reverb()'s; set_reverb(None) with no keywords turns it off"""
        r = r if r is not None else (reverb(**kw) if kw else None)
        check(lib.mx_deck_set_reverb(self._h, C.byref(r) if r is not None else None))

    def schedule_reverb(self, tick_in_feed: int, r: DeckReverb | None = None, **kw):
        """... from that tick of the next feed on (the reverb-out: send the deck into the tail, then clear PLAY); None with no keywords turns it off there"""
        r = r if r is not None else (reverb(**kw) if kw else None)
        check(lib.mx_deck_schedule_reverb(self._h, int(tick_in_feed), C.byref(r) if r is not None else None))

    def reverb_state(self):
        """(clock t, on, DeckReverb in force) after the last feed; host data, no synchronisation"""
        t, on, r = C.c_uint64(), C.c_uint32(), DeckReverb()
        check(lib.mx_deck_reverb_state(self._h, C.byref(t), C.byref(on), C.byref(r)))
        return t.value, bool(on.value), r

    def read_reverb_lines(self) -> np.ndarray:
        """float32 [DECK_REVERB_LINE_FLOATS]: the raw rings after the last feed, tank then diffusers (waits for the device); only the slots of the clocks in
        [max(0, t - ring), t) are specified"""
        out = np.zeros(abi.DECK_REVERB_LINE_FLOATS, np.float32)
        check(lib.mx_deck_read_reverb_lines(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def _analyse(self, call, attr: str, settings, counts) -> None:
        """one analyse*() call and the counts remembered of it: settings of None free the results; refused settings (MX_ERR_INVALID) leave the deck what it
        had; anything else (no memory) leaves it without this analysis"""
        try:
            check(call(self._h, C.byref(settings) if settings is not None else None))
        except abi.MxError as e:
            if e.code != abi.MX_ERR_INVALID:
                setattr(self, attr, None)
            raise
        setattr(self, attr, counts(settings) if settings is not None else None)

    def analyse(self, a: DeckAnalysis | None = None, **kw):
        """analyse the whole track as loaded now, asynchronously on the deck's own stream; keywords are analysis_bands()'s; analyse(None) frees the results"""
        a = a if a is not None else (analysis_bands(**kw) if kw else None)
        self._analyse(lib.mx_deck_analyse, "_analysis", a, lambda a: (column_count(self.n_frames, a.column), a.max_lag))

    def read_columns(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """COLUMN_DTYPE[n] of the analysis; waits for it"""
        n = (self._analysis[0] - first if self._analysis else 0) if n is None else n
        cols = np.zeros(max(1, n), COLUMN_DTYPE)
        check(lib.mx_deck_read_columns(self._h, int(first), int(n), cols.ctypes.data_as(C.c_void_p)))
        return cols[:n]

    def read_autocorr(self, cap: int | None = None) -> np.ndarray:
        """R as uint64[max_lag] of the analysis; waits for it.  cap is the room offered to the library (by default max_lag): the library fills max_lag of it"""
        lag = self._analysis[1] if self._analysis else 0
        cap = lag if cap is None else cap
        R = np.zeros(max(1, cap), np.uint64)
        check(lib.mx_deck_read_autocorr(self._h, R.ctypes.data_as(C.c_void_p), int(cap)))
        return R[:lag]

    def render_waveform(self, p: DeckWaveform, stream=None):
        """the analysis' columns as a picture under p (waveform()): a new opaque yuv420p video.DFrame, asynchronous on `stream` (None: the library's video
        stream), ordered behind the analysis on the device; no analysis, or settings the check refuses: MxError, the deck as it was"""
        from . import video
        h = C.c_void_p()
        check(lib.mx_deck_render_waveform(self._h, C.byref(p), C.byref(h), stream))
        return video.DFrame(handle=h.value, stream=stream)

    def analyse_tonality(self, t: DeckTonality | None = None, **kw):
        """the whole track's constant-Q sums per segment, asynchronously on the deck's own stream; keywords are tonality()'s; analyse_tonality(None) frees them"""
        t = t if t is not None else (tonality(**kw) if kw else None)
        self._analyse(lib.mx_deck_analyse_tonality, "_tonality", t, lambda t: (tonality_count(self.n_frames, t), t.octaves))

    def read_tonality(self, first: int = 0, n: int | None = None) -> list:
        """segments [first, first + n) of the tonality analysis as abi.parse_tonality_records dicts; waits for it"""
        segs, octaves = self._tonality or (0, 2)
        n = segs - first if n is None else n
        rb = 32 + 96 * octaves
        raw = np.zeros(max(1, n) * rb, np.uint8)
        check(lib.mx_deck_read_tonality(self._h, int(first), int(n), raw.ctypes.data_as(C.c_void_p), max(0, n) * rb))
        return abi.parse_tonality_records(raw[:n * rb], octaves)

    def key(self, rate: float):
        """(key, confidence, Camelot position such as "8A") of the whole track from the summed segment records; key -1 (no variance) has position \"\""""
        k, conf = abi.tonality_key(abi.tonality_chroma(self.read_tonality(), rate))
        return k, conf, (camelot(k) if k >= 0 else "")

    def analyse_loudness(self, l: DeckLoudness | None = None, **kw):
        """the whole track's loudness records per block, asynchronously on the deck's own stream; keywords are loudness()'s; analyse_loudness(None) frees them"""
        l = l if l is not None else (loudness(**kw) if kw else None)
        self._analyse(lib.mx_deck_analyse_loudness, "_loudness", l, lambda l: loudness_count(self.n_frames, l.block_frames))

    def read_loudness(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """abi.LOUDNESS_TICK_DTYPE[n] of the loudness analysis; waits for it"""
        n = ((self._loudness or 0) - first) if n is None else n
        out = np.zeros(max(1, n), abi.LOUDNESS_TICK_DTYPE)
        check(lib.mx_deck_read_loudness(self._h, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def analyse_finegrid(self, s: DeckFinegrid | None = _NOT_GIVEN, **kw):
        """score every candidate period of the settings over the whole track, asynchronously on the deck's own stream; keywords are finegrid()'s;
        analyse_finegrid(None) frees the result.  There are no default settings (a search needs a period to search round): a call with neither
        settings nor keywords, or with both, is a TypeError"""
        if (s is _NOT_GIVEN) == (not kw):
            raise TypeError("analyse_finegrid takes settings (None frees the result) or finegrid()'s keywords, one of the two")
        if s is _NOT_GIVEN:
            s = finegrid(**kw)
        self._analyse(lib.mx_deck_analyse_finegrid, "_finegrid", s, lambda s: (s.n_periods, finegrid_count(self.n_frames, s.hop)))

    def read_finegrid(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """abi.DECK_COMB_DTYPE[n] of the fine grid, one record per candidate period; waits for it"""
        n = ((self._finegrid or (0, 0))[0] - first) if n is None else n
        out = np.zeros(max(1, n), abi.DECK_COMB_DTYPE)
        check(lib.mx_deck_read_finegrid(self._h, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def read_fine_onsets(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """the tooth weights w as uint32[n] of the fine grid; waits for it"""
        n = ((self._finegrid or (0, 0))[1] - first) if n is None else n
        w = np.zeros(max(1, n), np.uint32)
        check(lib.mx_deck_read_fine_onsets(self._h, int(first), int(n), w.ctypes.data_as(C.c_void_p)))
        return w[:n]

    def refine_grid(self, grid: DeckGrid, column: int, rate: float, hop: int = 64) -> DeckFinePick:
        """the coarse grid of beatgrid() refined to a fine hop in the header's two stages: +-2 % round the coarse period over the first 64 beats, then
        +- 4 x stage one's spacing round its winner over the whole track.  Waits for the device twice.  A grid without a period, or a stage that finds
        nothing (a silent track), gives the all-zero pick."""
        if not grid.period_columns > 0.0:
            return DeckFinePick()
        n_hops = finegrid_count(self.n_frames, hop)
        centre = finegrid_period(grid.period_columns, column, hop)
        one, _ = finegrid_span(centre, (centre + 49) // 50, 64, n_hops, hop)
        self.analyse_finegrid(one)
        first = finegrid_pick(self.read_finegrid(), one, rate)
        if not first.score:
            return first
        two, _ = finegrid_span(one.period0_q16 + first.index * one.dperiod_q16, 4 * one.dperiod_q16, 0, n_hops, hop)
        self.analyse_finegrid(two)
        return finegrid_pick(self.read_finegrid(), two, rate)

    def analyse_bars(self, s: DeckBars | None):
        """beat vectors, novelties and folds of the whole track on the grid of the settings, asynchronously on the deck's own stream; analyse_bars(None) frees them"""
        self._analyse(lib.mx_deck_analyse_bars, "_bars", s, lambda s: (bars_count(s, self.n_frames)[0], s.beats_per_bar * (1 + s.bars_per_phrase)))

    def read_bars(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """abi.DECK_BEAT_DTYPE[n] of the bars analysis, one record per beat; waits for it"""
        n = ((self._bars or (0, 0))[0] - first) if n is None else n
        out = np.zeros(max(1, n), abi.DECK_BEAT_DTYPE)
        check(lib.mx_deck_read_bars(self._h, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def read_bar_folds(self, cap: int | None = None) -> np.ndarray:
        """H_bar then H_phrase as uint64[M + M Q] of the bars analysis; waits for it.  cap is the room offered to the library (by default M + M Q)"""
        words = (self._bars or (0, 0))[1]
        cap = words if cap is None else cap
        H = np.zeros(max(1, cap), np.uint64)
        check(lib.mx_deck_read_bar_folds(self._h, H.ctypes.data_as(C.c_void_p), int(cap)))
        return H[:words]

    def find_bars(self, pick_or_grid, tables: DeckAnalysis | None = None, **kw) -> DeckBarPick:
        """the downbeats and phrase lines of a beat grid (a DeckBeats, or refine_grid()'s pick): analyse_bars, the folds, bars_pick.  Keywords are bars()'s.  Waits for
        the device once.  A grid without a period (a silent track's pick) gives the all-zero pick."""
        grid = getattr(pick_or_grid, "grid", pick_or_grid)
        if not grid.period_q32 > 0:
            return DeckBarPick()
        s = bars(grid, tables, **kw)
        self.analyse_bars(s)
        return bars_pick(self.read_bar_folds(), s)

    def analyse_tempomap(self, s: DeckTempomap | None):
        """score every candidate period in every window of the track, asynchronously on the deck's own stream; analyse_tempomap(None) frees the result"""
        self._analyse(lib.mx_deck_analyse_tempomap, "_tempomap", s, lambda s: (tempomap_count(s, self.n_frames) * s.n_periods, finegrid_count(self.n_frames, s.hop)))

    def read_tempomap(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """abi.DECK_COMB_DTYPE[n] of the tempo map, record (v, j) at v * n_periods + j; waits for it"""
        n = ((self._tempomap or (0, 0))[0] - first) if n is None else n
        out = np.zeros(max(1, n), abi.DECK_COMB_DTYPE)
        check(lib.mx_deck_read_tempomap(self._h, int(first), int(n), out.ctypes.data_as(C.c_void_p)))
        return out[:n]

    def read_tempomap_onsets(self, first: int = 0, n: int | None = None) -> np.ndarray:
        """the tooth weights w as uint32[n] of the tempo map; waits for it"""
        n = ((self._tempomap or (0, 0))[1] - first) if n is None else n
        w = np.zeros(max(1, n), np.uint32)
        check(lib.mx_deck_read_tempomap_onsets(self._h, int(first), int(n), w.ctypes.data_as(C.c_void_p)))
        return w[:n]

    def map_tempo(self, pick_or_grid, hop: int = 64, window_beats: int = 16, stride_beats: int = 8, width: float = 0.06, penalty: int | None = None) -> np.ndarray:
        """the tempo map round a whole-track grid (a DeckBeats, or refine_grid()'s pick, found at this hop): span (+-width of the period), analyse_tempomap, read, path,
        segments; abi.DECK_TEMPO_SEGMENT_DTYPE[V].  penalty None: floor(the sum of the windows' best scores / (V * n_periods)) -- crossing the whole search range
        costs what one window scores.  Waits for the device once.  A grid without a period (a silent track's pick) gives no segments."""
        grid = getattr(pick_or_grid, "grid", pick_or_grid)
        if not grid.period_q32 > 0:
            return np.zeros(0, abi.DECK_TEMPO_SEGMENT_DTYPE)
        centre = (grid.period_q32 >> 16) // hop
        s, _ = tempomap_span(centre, int(centre * width), window_beats, stride_beats, finegrid_count(self.n_frames, hop), hop)
        self.analyse_tempomap(s)
        recs = self.read_tempomap().reshape(-1, s.n_periods)
        if penalty is None:
            penalty = sum(int(v) for v in recs["score"].max(axis=1)) // recs.size
        return tempomap_segments(recs, s, self.n_frames, tempomap_path(recs, penalty))

    def schedule_warp(self, segs: np.ndarray, out_period_q32: int, n_ticks: int, spt: int, p: DeckParams | None = None, seek: int | None = None) -> list:
        """before a feed of n_ticks ticks of spt frames: walk the head through them as mx_deck_plan says and schedule, at every tick whose head stands in a segment
        that wants another step than the one in force, that segment's mx_deck_tempomap_step -- the rest of the parameters stay.  p and seek, when given, are what the
        host would have handed to set() and seek() for tick 0 (the warp's own event there replaces them, so they go through here); p's step is the map's from the
        start.  [(tick, segment, step)] of the step changes.  Nothing is remembered between calls: the head and its parameters say all there is."""
        head, out = self.state(), []
        for k in range(n_ticks):
            base = p if k == 0 and p is not None else None
            sk = seek if k == 0 else None
            q = base if base is not None else head.params
            grid, seg = tempomap_at(segs, sk if sk is not None else head.pos_q32)
            new = base
            if grid.period_q32 > 0:
                step = tempomap_step(grid, out_period_q32)
                if step != q.step_q32:
                    new = DeckParams(step, q.slew_q32, q.loop_in, q.loop_out, q.flags, 0)
                    out.append((k, seg, step))
            if new is not None or sk is not None:
                self.schedule(k, new, sk)
            _, head = deck_plan(head, spt, self.n_frames, new, sk)
        return out

    def state(self) -> DeckHead:
        h = DeckHead()
        check(lib.mx_deck_state(self._h, C.byref(h)))
        return h


def feed(decks, nodes, graph, n_ticks: int) -> None:
    """write the next n_ticks ticks of every deck into its SOURCE_STEREO node of `graph`: one launch, asynchronous on the graph's stream"""
    n = len(decks)
    if len(nodes) != n:
        raise ValueError("one node per deck")
    hs = (C.c_void_p * max(1, n))(*[d._h.value for d in decks])
    ns = (C.c_uint32 * max(1, n))(*[int(x) for x in nodes])
    check(lib.mx_deck_feed(hs, ns, n, graph._h, int(n_ticks)))
