#!/usr/bin/env python
"""Cost of the deck's tempo map: builds tools/deck_tempomap_forms.cpp against libmixlab_gpu.so (which must have been built) and runs it -- the
two forms of the comb kernel timed alternately in one process over several searches of a ten-minute 48 kHz click track whose tempo ramps, at h = 64, beside
mx_deck_tempomap_host on one thread and one whole-track fine grid launch per window (what a host did before).  Then Deck.map_tempo end to end through the library's own
entry points, wall clock: span, analysis, read-out, path and segments.

    python tools/deck_tempomap_cost.py [--seconds 600] [--reps 20] [--exe PATH | --build-only DIR]

--build-only DIR compiles the program into DIR and stops (no device needed); --exe runs a program built that way instead of compiling one."""
import argparse
import os
import pathlib
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
PKG = ROOT / "mixlab_amd"
sys.path.insert(0, str(ROOT))


def build(build_dir) -> pathlib.Path:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = pathlib.Path(build_dir) / "deck_tempomap_forms"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-O2", "-ffp-contract=off", "-x", "hip", str(ROOT / "tools" / "deck_tempomap_forms.cpp"),
                    f"-L{PKG}", "-lmixlab_gpu", f"-Wl,-rpath,{PKG}", "-o", str(exe)], check=True)
    return exe


def run(exe, seconds, reps) -> None:
    env = {**os.environ, "LD_LIBRARY_PATH": f"{PKG}:{os.environ.get('LD_LIBRARY_PATH', '')}"}
    subprocess.run([str(exe), str(seconds), str(reps)], check=True, env=env)


def end_to_end(seconds, reps) -> None:
    import numpy as np

    from mixlab_amd import abi, deck
    n = seconds * 48000
    rng = np.random.default_rng(17)
    track = rng.integers(-300, 301, (n, 2), dtype=np.int16)
    at = 5000.4
    while at + 200 < n:
        track[int(at):int(at) + 200] = rng.integers(-20000, 20001, (200, 2), dtype=np.int16)
        at += 22000.0 + 1700.0 * at / n
    d = deck.Deck(n)
    d.load(track)
    grid = abi.DeckBeats(0, 22850 << 32)
    times = []
    for k in range(2 + reps):
        t = time.perf_counter()
        segs = d.map_tempo(grid, 64)
        if k >= 2:
            times.append((time.perf_counter() - t) * 1e3)
    periods = segs["period_q32"] / 2.0 ** 32
    print(f"map_tempo end to end (span, analysis, read-out of {d._tempomap[0]} records, path, segments) forms={deck.debug_last_tempomap()} "
          f"ms_wall median={statistics.median(times):.2f} min={min(times):.2f}; segments={len(segs)} periods {periods[0]:.1f} .. {periods[-1]:.1f} frames "
          f"(the track: 22 000 .. 23 700), empty={int((segs['flags'] & abi.DECK_TEMPO_EMPTY).sum())}", flush=True)
    d.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--exe")
    ap.add_argument("--build-only")
    args = ap.parse_args()
    if args.build_only:
        print(build(args.build_only))
        return
    if args.exe:
        run(args.exe, args.seconds, args.reps)
    else:
        with tempfile.TemporaryDirectory() as d:
            run(build(d), args.seconds, args.reps)
    end_to_end(args.seconds, max(3, args.reps // 4))
    print("deck_tempomap_cost done")


if __name__ == "__main__":
    main()
