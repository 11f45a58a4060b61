#!/usr/bin/env python
"""Cost of the deck's whole-track tonality and loudness: a 10-minute 48 kHz noise track -- 28.8 M frames, 115 MB -- with tonality
D 8 / Hc 512 / O 5 from C2 / G 64 and loudness F 4800 / M 4 / S 30, beside two yardsticks: a device-to-device copy of the track's bytes (the roof of a read-once
pass) and mx_deck_tonality_host / mx_deck_loudness_host over the same track on one thread (what a host would otherwise do).  The device's records are compared
with the host functions', byte for byte, before anything is timed.

Wall times here are host clocks round a synchronising read-out of one record; run it under `rocprofv3 --kernel-trace --stats -- python tools/deck_loudkey_cost.py`
for the kernels' own times (k_dk_ton_*, k_dk_loud_*): --stats averages every launch, the warm-up ones included, so with --trace-csv FILE (the run's kernel
trace, rocprofv3 --output-format csv) this script prints each kernel's mean over the launches after the warm-up instead.

    python tools/deck_loudkey_cost.py --trace-csv out/run/123_kernel_trace.csv     # no device needed

    python tools/deck_loudkey_cost.py [--seconds 600] [--reps 10]"""
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
FIRST = 1   # the launches of the comparison run come before the warm-up ones


def trace_means(path):
    """per k_dk_* kernel of a kernel trace: the mean duration over the launches after the comparison run and the warm-up, in start order"""
    import csv
    runs = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row["Kernel_Name"]
            if "k_dk_" in name:
                runs.setdefault(name.split("(")[0].split("::")[-1], []).append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    for name, r in sorted(runs.items()):
        per = 2 if "k_dk_loud_walk" in name and "<" not in name else 1   # (both walks under one name where the trace drops template arguments)
        d = [(e - s) / 1e3 for s, e in sorted(r)][(FIRST + WARMUP) * per:]
        print(f"{name} launches_after_warmup={len(d)} mean_us={statistics.mean(d):.1f} min_us={min(d):.1f} max_us={max(d):.1f}")


def timed(fn, reps):
    for _ in range(WARMUP):
        fn()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace-csv")
    args = ap.parse_args()
    if args.trace_csv:
        return trace_means(args.trace_csv)
    n = args.seconds * 48000
    rng = np.random.default_rng(17)
    track = rng.integers(-32768, 32768, (n, 2), dtype=np.int16)
    ton, loud = deck.tonality(48000.0, 8, 512, 5, 65406, 64), deck.loudness(48000.0, 4800, 4, 30)

    t = time.perf_counter()
    host_ton = b"".join(r["raw"] for r in deck.tonality_host(track, ton))
    t_ton = time.perf_counter() - t
    t = time.perf_counter()
    host_loud = deck.loudness_host(track, loud)
    t_loud = time.perf_counter() - t
    print(f"tonality_host one thread s={t_ton:.2f}   loudness_host one thread s={t_loud:.2f}", flush=True)

    d = deck.Deck(n)
    d.load(track)
    d.analyse_tonality(ton); d.analyse_loudness(loud)
    dev_ton, dev_loud = b"".join(r["raw"] for r in d.read_tonality()), d.read_loudness()
    assert dev_ton == host_ton, "the device's tonality records differ from mx_deck_tonality_host's"
    assert dev_loud.tobytes() == host_loud.tobytes(), "the device's loudness records differ from mx_deck_loudness_host's"
    print(f"records equal: tonality segments={deck.tonality_count(n, ton)} loudness blocks={deck.loudness_count(n, loud.block_frames)}", flush=True)

    def once_ton():
        d.analyse_tonality(ton)
        return d.read_tonality(0, 1)   # waits for the analysis: 512 bytes back

    def once_loud():
        d.analyse_loudness(loud)
        return d.read_loudness(0, 1)   # waits for the analysis: 48 bytes back

    med, lo, hi = timed(once_ton, args.reps)
    print(f"analyse_tonality frames={n} bytes={4 * n} forms={deck.debug_last_tonality()} ms_wall={med:.3f} min={lo:.3f} max={hi:.3f}", flush=True)
    med, lo, hi = timed(once_loud, args.reps)
    print(f"analyse_loudness frames={n} bytes={4 * n} forms={deck.debug_last_loudness()} ms_wall={med:.3f} min={lo:.3f} max={hi:.3f}", flush=True)

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

    key, conf, name = d.key(48000.0)
    lufs, peak, gain = deck.loudness_gain(dev_loud, 4, 1, -14.0, -1.0)
    print(f"read-outs of the noise track: key={key} ({name}) confidence={conf:.4f} I={lufs:.2f} LUFS peak={peak:.2f} dBTP gain={gain:.2f} dB "
          f"(chroma sums to {float(abi.tonality_chroma(d.read_tonality(), 48000.0).sum()):.3f})", flush=True)
    d.close()
    print("deck_loudkey_cost done")


if __name__ == "__main__":
    main()
