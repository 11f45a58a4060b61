#!/usr/bin/env python
"""Cost of the deck's waveform picture: mx_deck_render_waveform over the C = 64 analysis of a 10-minute 48 kHz track (450 000 records,
25 MB), as a scrolling view at 100 frames a pixel and as a whole-track overview, at 1920 x 1080 and at 1920 x 128 -- each beside two yardsticks measured in the same
run: a device-to-device copy of the picture's bytes (the roof of a write-once pass) and the old route, mx_deck_read_columns of the window plus mx_dframe_upload of a
ready-made picture (the CPU's rasterising in between not even counted).  Every picture is compared with mx_deck_waveform_host before anything is timed.

Wall times here are host clocks round the call and a wait for its stream (so they hold the frame's allocation too); run it under
`rocprofv3 --kernel-trace --stats -- python tools/deck_waveform_cost.py` for the kernel's own time, and give the run's kernel trace back with --trace-csv FILE for
the mean per case over the launches after the warm-up.

    python tools/deck_waveform_cost.py [--seconds 600] [--reps 20]
    python tools/deck_waveform_cost.py --trace-csv out/run/123_kernel_trace.csv     # no device needed"""
import argparse
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mixlab_amd import deck, video  # noqa: E402

WARMUP = 3
SIZES = ((1920, 1080), (1920, 128))


def trace_means(path, reps):
    """k_deck_waveform of a kernel trace: per case (the launches come in the order main() makes them: one check, WARMUP and `reps` timed per case) the mean duration"""
    import csv
    with open(path, newline="") as f:
        d = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in csv.DictReader(f) if "k_deck_waveform" in r["Kernel_Name"])
    per = 1 + WARMUP + reps
    for k in range(len(d) // per):
        us = [(e - s) / 1e3 for s, e in d[k * per + 1 + WARMUP:(k + 1) * per]]
        print(f"case {k} k_deck_waveform launches_after_warmup={len(us)} median_us={statistics.median(us):.1f} min_us={min(us):.1f} max_us={max(us):.1f}")


def timed(fn, reps):
    for _ in range(WARMUP):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return f"median_us={statistics.median(t):.1f} min_us={min(t):.1f} max_us={max(t):.1f}", statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace-csv")
    args = ap.parse_args()
    if args.trace_csv:
        return trace_means(args.trace_csv, args.reps)
    n = args.seconds * 48000
    track = np.random.default_rng(17).integers(-32768, 32768, (n, 2), dtype=np.int16)
    a = deck.analysis_bands(column=64, max_lag=16)
    d = deck.Deck(n)
    d.load(track)
    d.analyse(a)
    cols = d.read_columns()
    beats = deck.wave_grid(deck.DeckBeats(12345 << 32, (22050 << 32) + 777), (235, 128, 128), inset=4)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    for w, h in SIZES:
        for what, first, fpp in (("scroll", n // 2, 100), ("overview", 0, -(-n // w))):
            p = deck.waveform(w, h, first, fpp, gain_q16=(40000, 60000, 80000), grids=[beats],
                              markers=[deck.wave_marker(first + fpp * (w // 4), (255, 128, 128), 2)], ranges=[deck.wave_range(first + 10 * fpp, first + 200 * fpp, (60, 110, 140))])
            f = d.render_waveform(p)
            want = deck.waveform_host(cols, 64, n, p)
            assert all(np.array_equal(g, x) for g, x in zip(f.download(), want)), (what, w, h)
            del f

            def render():
                f = d.render_waveform(p)
                video.sync()
                return f
            r_text, r_us = timed(render, args.reps)
            nbytes = w * h * 3 // 2
            src, dst = C.c_void_p(), C.c_void_p()
            assert hip.hipMalloc(C.byref(src), nbytes) == 0 and hip.hipMalloc(C.byref(dst), nbytes) == 0

            def copy():
                hip.hipMemcpyAsync(dst, src, nbytes, 3, None)
                hip.hipDeviceSynchronize()
            c_text, c_us = timed(copy, args.reps)
            hip.hipFree(src); hip.hipFree(dst)
            c0 = max(0, first // 64)
            n_rec = min(len(cols), -(-(first + w * fpp) // 64)) - c0
            ready, target = [np.ascontiguousarray(x) for x in want], video.DFrame(w, h)

            def old_route():
                d.read_columns(c0, n_rec)
                target.upload(*ready)
            o_text, o_us = timed(old_route, args.reps)
            print(f"{what} {w}x{h} fpp={fpp} records_in_window={n_rec} forms={deck.debug_last_waveform()} equal_to_host=True", flush=True)
            print(f"  render_wall {r_text}", flush=True)
            print(f"  copy_d2d bytes={nbytes} {c_text}  render/copy={r_us / c_us:.2f}", flush=True)
            print(f"  old_route read_columns+upload {o_text}  render/old={r_us / o_us:.2f}", flush=True)
    d.close()
    print("deck_waveform_cost done")


if __name__ == "__main__":
    main()
