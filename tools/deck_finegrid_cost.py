#!/usr/bin/env python
"""Cost of the deck's fine beat grid: a 10-minute 48 kHz click track -- 28.8 M frames, 115 MB, a burst every 22 857.3 frames (126.0 BPM) on a
noise floor -- refined at h = 64 in the header's two stages from a coarse period 0.4 % off: +-2 % over the first 64 beats, then +- 4 x stage one's spacing over the whole
track.  Beside two yardsticks: a device-to-device copy of the track's bytes (the roof of a read-once pass) and mx_deck_finegrid_host over the same settings on one
thread (what a host would otherwise do).  The device's records and tooth weights are compared with the host function's, byte for byte, before anything is timed.

Wall times here are host clocks round a synchronising read-out of the records; run it under `rocprofv3 --kernel-trace --stats -- python tools/deck_finegrid_cost.py`
for the kernels' own times (k_fine_onsets, k_fine_comb): --stats averages every launch, the warm-up ones included, so with --trace-csv FILE (the run's kernel trace,
rocprofv3 --output-format csv) this script prints each kernel's mean over the launches after the warm-up instead, stage by stage.

    python tools/deck_finegrid_cost.py --trace-csv out/run/123_kernel_trace.csv     # no device needed

    python tools/deck_finegrid_cost.py [--seconds 600] [--reps 10]"""
import argparse
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mixlab_amd import abi, deck  # noqa: E402

WARMUP = 3
RATE, HOP, COLUMN, PERIOD, T0, COARSE_OFF = 48000.0, 64, 512, 22857.3, 5000.4, 1.004


def trace_means(path):
    """per k_fine_* kernel of a kernel trace: the mean duration over the launches after the comparison runs and the warm-ups.  The tool launches, in this order: the
    comparison (stage one, stage two), then per timed function WARMUP + reps calls -- stage one alone, stage two alone, refine_grid (stage one, stage two each call).
    So launches [2, 2 + W + reps) are stage one, the next W + reps stage two, and the rest alternate."""
    import csv
    runs = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if "k_fine_" in name:
                runs.setdefault(name.split("(")[0].split("::")[-1], []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for name, r in sorted(runs.items()):
        d = [(e - s) / 1e3 for s, e in sorted(r)]
        per = (len(d) - 2) // 4          # W + reps
        for label, part in (("stage one", d[2 + WARMUP:2 + per]), ("stage two", d[2 + per + WARMUP:2 + 2 * per])):
            print(f"{name} {label} launches_after_warmup={len(part)} mean_us={statistics.mean(part):.1f} min_us={min(part):.1f} max_us={max(part):.1f}")


def timed(fn, reps):
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def click_track(n):
    rng = np.random.default_rng(17)
    track = rng.integers(-300, 301, (n, 2), dtype=np.int16)
    k = 0
    while round(T0 + k * PERIOD) + 200 <= n:
        f = round(T0 + k * PERIOD)
        track[f:f + 200] = rng.integers(-20000, 20001, (200, 2), dtype=np.int16)
        k += 1
    return track, k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace-csv")
    args = ap.parse_args()
    if args.trace_csv:
        return trace_means(args.trace_csv)
    n = args.seconds * 48000
    track, n_beats = click_track(n)
    N = deck.finegrid_count(n, HOP)
    coarse = abi.DeckGrid(0.0, PERIOD / COLUMN * COARSE_OFF, 0.0, 0, 0, 0)
    centre = deck.finegrid_period(coarse.period_columns, COLUMN, HOP)
    one, _ = deck.finegrid_span(centre, (centre + 49) // 50, 64, N, HOP)

    t = time.perf_counter()
    host_one, host_w = deck.finegrid_host(track, one, onsets=True)
    t_one = time.perf_counter() - t
    first = deck.finegrid_pick(host_one, one, RATE)
    two, _ = deck.finegrid_span(one.period0_q16 + first.index * one.dperiod_q16, 4 * one.dperiod_q16, 0, N, HOP)
    t = time.perf_counter()
    host_two = deck.finegrid_host(track, two)
    t_two = time.perf_counter() - t
    print(f"finegrid_host one thread: stage one s={t_one:.2f} (periods={one.n_periods} dperiod={one.dperiod_q16} max_beats={one.max_beats})   "
          f"stage two s={t_two:.2f} (periods={two.n_periods} dperiod={two.dperiod_q16})", flush=True)

    d = deck.Deck(n)
    d.load(track)
    d.analyse_finegrid(one)
    assert d.read_finegrid().tobytes() == host_one.tobytes(), "the device's stage-one records differ from mx_deck_finegrid_host's"
    assert d.read_fine_onsets().tobytes() == host_w.tobytes(), "the device's tooth weights differ from mx_deck_finegrid_host's"
    d.analyse_finegrid(two)
    assert d.read_finegrid().tobytes() == host_two.tobytes(), "the device's stage-two records differ from mx_deck_finegrid_host's"
    print(f"records equal: hops={N} stage one periods={one.n_periods} stage two periods={two.n_periods}", flush=True)

    def once(s):
        d.analyse_finegrid(s)
        return d.read_finegrid()   # waits for the analysis: n_periods x 16 bytes back

    for label, s in (("stage one", one), ("stage two", two)):
        med, lo, hi = timed(lambda s=s: once(s), args.reps)
        print(f"analyse_finegrid {label} frames={n} bytes={4 * n} forms={deck.debug_last_finegrid()} ms_wall={med:.3f} min={lo:.3f} max={hi:.3f}", flush=True)
    med, lo, hi = timed(lambda: d.refine_grid(coarse, COLUMN, RATE, HOP), args.reps)
    print(f"refine_grid (both stages, two read-outs, span and pick on the host) ms_wall={med:.3f} min={lo:.3f} max={hi:.3f}", flush=True)

    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    src, dst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), 4 * n) == 0 and hip.hipMalloc(C.byref(dst), 4 * n) == 0
    copies = []
    for k in range(3 + args.reps):
        hip.hipDeviceSynchronize()
        t = time.perf_counter()
        hip.hipMemcpyAsync(dst, src, 4 * n, 3, None)
        hip.hipDeviceSynchronize()
        if k >= 3:
            copies.append((time.perf_counter() - t) * 1e3)
    print(f"copy_d2d bytes={4 * n} ms_wall={statistics.median(copies):.3f} min={min(copies):.3f}", flush=True)
    hip.hipFree(src); hip.hipFree(dst)

    p = d.refine_grid(coarse, COLUMN, RATE, HOP)
    period, first_frame = p.grid.period_q32 / 2.0 ** 32, p.grid.first_q32 / 2.0 ** 32
    print(f"read-out: bpm={p.bpm:.4f} period={period:.4f} frames (true {PERIOD}), first beat at {first_frame:.1f} (true {T0}), {p.n_beats} teeth over {n_beats} bursts; "
          f"the last grid line lies {abs(first_frame + (n_beats - 1) * period - (T0 + (n_beats - 1) * PERIOD)):.1f} frames from the last burst "
          f"(the coarse period alone: {abs(COARSE_OFF - 1.0) * PERIOD * (n_beats - 1):.0f})", flush=True)
    d.close()
    print("deck_finegrid_cost done")


if __name__ == "__main__":
    main()
