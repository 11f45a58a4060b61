#!/usr/bin/env python
"""Cost of the deck's track analysis: one analysis of a 10-minute 48 kHz track -- 28.8 M frames, 115 MB, C = 512, K = 63, L = 256 -- beside
two yardsticks: a device-to-device copy of the track's bytes (the roof of a read-once pass) and mx_deck_columns_host over the same track on one thread (what a host
would otherwise do).  The device result is compared with the host's, record for record, before anything is timed.

Wall times here are host clocks round a synchronising read-out; run it under `rocprofv3 --kernel-trace --stats -- python tools/deck_analysis_cost.py` for the
kernels' own times (k_deck_columns, k_deck_onsets, k_deck_autocorr): --stats averages every launch, the 3 warm-up ones included, so with --trace-csv FILE (the
run's kernel trace, rocprofv3 --output-format csv) this script prints each kernel's mean over the launches after the warm-up instead.

    python tools/deck_analysis_cost.py --trace-csv out/run/123_kernel_trace.csv     # no device needed

    python tools/deck_analysis_cost.py [--seconds 600] [--reps 10] [--no-host]"""
import argparse
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from mixlab_amd import deck  # noqa: E402


WARMUP = 3


def trace_means(path):
    """per k_deck_* kernel of a kernel trace: the mean duration over the launches after the first WARMUP, in start order"""
    import csv
    runs = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if "k_deck_" in name:
                runs.setdefault(name.split("(")[0].split("::")[-1], []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for name, r in sorted(runs.items()):
        d = [(e - s) / 1e3 for s, e in sorted(r)][WARMUP:]
        print(f"{name} launches_after_warmup={len(d)} mean_us={statistics.mean(d):.1f} min_us={min(d):.1f} max_us={max(d):.1f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--trace-csv")
    args = ap.parse_args()
    if args.trace_csv:
        return trace_means(args.trace_csv)
    n = args.seconds * 48000
    rng = np.random.default_rng(17)
    track = rng.integers(-32768, 32768, (n, 2), dtype=np.int16)
    a = deck.analysis_bands()   # 200 Hz / 2.5 kHz, K = 63, C = 512, L = 256
    d = deck.Deck(n)
    d.load(track)

    def once():
        d.analyse(a)
        return d.read_autocorr()   # waits for the analysis: 2 KB back

    for _ in range(WARMUP):
        once()
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        once()
        times.append((time.perf_counter() - t) * 1e3)
    print(f"analyse frames={n} bytes={4 * n} columns={deck.column_count(n, a.column)} forms={deck.debug_last_analysis()} "
          f"ms_per_analysis_wall={statistics.median(times):.3f} min={min(times):.3f} max={max(times):.3f}", flush=True)
    cols, R = d.read_columns(), d.read_autocorr()

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

    if not args.no_host:
        t = time.perf_counter()
        hcols, hR = deck.columns_host(track, a, autocorr=True)
        host = time.perf_counter() - t
        print(f"columns_host one thread s={host:.2f} equal_to_device={bool(np.array_equal(hcols, cols) and np.array_equal(hR, R))}", flush=True)
        g = deck.beatgrid(cols, R, a.column, 48000.0, 60.0, 200.0)
        print(f"beatgrid of the noise track: lag={g.lag} phase={g.phase_column} bpm={g.bpm:.3f} confidence={g.confidence:.4f}", flush=True)
    d.close()
    print("deck_analysis_cost done")


if __name__ == "__main__":
    main()
