#!/usr/bin/env python
"""Cost of the deck's bars and phrases: a 10-minute 48 kHz section track -- 28.8 M frames, 115 MB, a kick every 22 857.3 frames (126.0 BPM), a
snare on every bar's third beat, sections of 32 beats that add a high or a mid layer, a pick-up of 6 beats -- analysed on its own grid with the header's recommended
tables (K = 63), M = 4, Q = 8, W = 4 and 16.  Beside two yardsticks: a device-to-device copy of the track's bytes (the roof of a read-once pass) and mx_deck_bars_host
over the same settings on one thread (what a host would otherwise do).  The device's records and folds are compared with the host function's, byte for byte, before
anything is timed.

Wall times here are host clocks round analyse_bars plus the synchronising read of the folds; run it under `rocprofv3 --kernel-trace -- python tools/deck_bars_cost.py`
for the kernels' own times (k_bars_bands, k_bars_novelty, k_bars_fold): with --trace-csv FILE (the run's kernel trace, rocprofv3 --output-format csv) this script
prints each kernel's mean over the launches after the comparison run and the warm-up.

    python tools/deck_bars_cost.py --trace-csv out/run/123_kernel_trace.csv     # no device needed

    python tools/deck_bars_cost.py [--seconds 600] [--reps 10]"""
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
RATE, PERIOD, T0, PICKUP, SECTION = 48000.0, 22857.3, 5000.4, 6, 32


def trace_means(path):
    """per k_bars_* kernel of a kernel trace: the mean duration over the launches after the comparison run (the first) and the warm-ups"""
    import csv
    runs = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if "k_bars_" in name:
                runs.setdefault(name.split("(")[0].split("::")[-1], []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for name, r in sorted(runs.items()):
        d = [(e - s) / 1e3 for s, e in sorted(r)][1 + WARMUP:]
        print(f"{name} launches_after_warmup={len(d)} mean_us={statistics.mean(d):.1f} min_us={min(d):.1f} max_us={max(d):.1f}")


def section_track(n):
    """(track, beats, the constructed bar phase, the constructed phrase phase)"""
    rng = np.random.default_rng(21)
    x = rng.integers(-50, 51, n).astype(np.float64)
    t = np.arange(2000)
    kick = 12000 * np.sin(2 * np.pi * 80 * t / RATE) * np.exp(-t / 600)
    full, half = int(PERIOD), int(PERIOD) // 2
    k = 0
    while round(T0 + (k + 1) * PERIOD) <= n:
        f = round(T0 + k * PERIOD)
        x[f:f + 2000] += kick
        sec = (k - PICKUP) // SECTION if k >= PICKUP else -1
        kind = "ABC"[sec % 3] if sec >= 0 else "A"
        if kind == "B":
            x[f + half:f + full] += rng.integers(-3000, 3001, full - half) * np.where(np.arange(full - half) % 2, 1, -1)
        if kind == "C":
            x[f:f + full] += 4000 * np.sin(2 * np.pi * 1000 * np.arange(full) / RATE)
        if k >= PICKUP and (k - PICKUP) % 4 == 2:
            x[f:f + 1500] += rng.integers(-6000, 6001, 1500)
        k += 1
    x = np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    return np.stack([x, x], axis=1), k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace-csv")
    args = ap.parse_args()
    if args.trace_csv:
        return trace_means(args.trace_csv)
    n = args.seconds * 48000
    track, built = section_track(n)
    s = deck.bars(abi.DeckBeats(round(T0 * 2 ** 32), round(PERIOD * 2 ** 32)), deck.analysis_bands(rate=RATE), bars_per_phrase=SECTION // 4, w_bar=4, w_phrase=SECTION // 2)
    n_beats, n0 = deck.bars_count(s, n)

    t = time.perf_counter()
    host_recs, host_H = deck.bars_host(track, s)
    print(f"bars_host one thread: s={time.perf_counter() - t:.2f} (beats={n_beats} n0={n0} taps={s.taps})", flush=True)

    d = deck.Deck(n)
    d.load(track)
    d.analyse_bars(s)
    assert d.read_bars().tobytes() == host_recs.tobytes(), "the device's records differ from mx_deck_bars_host's"
    assert d.read_bar_folds().tobytes() == host_H.tobytes(), "the device's folds differ from mx_deck_bars_host's"
    print(f"records and folds equal: beats={n_beats} folds={len(host_H)} forms={deck.debug_last_bars()}", flush=True)

    def once():
        d.analyse_bars(s)
        return d.read_bar_folds()   # waits for the analysis: M + M Q words back

    for _ in range(WARMUP):
        once()
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        once()
        times.append((time.perf_counter() - t) * 1e3)
    print(f"analyse_bars + read_bar_folds frames={n} bytes={4 * n} ms_wall={statistics.median(times):.3f} min={min(times):.3f} max={max(times):.3f}", flush=True)

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

    p = deck.bars_pick(host_H, s)
    Hb = sorted(int(v) for v in host_H[:4])
    print(f"read-out: bar phase {p.bar_phase} (constructed {(PICKUP - n0) % 4}), phrase phase {p.phrase_phase} (constructed {(PICKUP - n0) % SECTION}), "
          f"bar winner / runner-up {Hb[-1] / max(1, Hb[-2]):.2f}, bar confidence {p.bar_best / max(1, p.bar_sum):.3f}, phrase confidence {p.phrase_best / max(1, p.phrase_sum):.3f}; "
          f"{built} beats built", flush=True)
    d.close()
    print("deck_bars_cost done")


if __name__ == "__main__":
    main()
