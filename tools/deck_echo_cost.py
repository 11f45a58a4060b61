#!/usr/bin/env python
"""Cost of the deck's echo: feeds of 2 decks x 1 tick, 2 x 64 ticks and 1024 x 64 ticks at 48 kHz, 800 frames a tick, tempo 1.08, tracks of
60 000 frames in a loop, with an echo at delay 256, 5714 (1/4 beat at 126 BPM) and 100 000 frames, feedback 0.5, damp 0.3 -- and beside each the same feed without an
echo.  Host clock around back-to-back feeds ended by one synchronise (per feed: the whole; enqueue: until the last call returned).

Run it under `rocprofv3 --kernel-trace --output-format csv -- python tools/deck_echo_cost.py` for the kernels' own times, then hand the trace back:

    python tools/deck_echo_cost.py --trace-csv out/run/123_kernel_trace.csv     # no device needed: mean of k_deck_echo_* per configuration, warm-ups left out

    python tools/deck_echo_cost.py [--rounds 3]"""
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
from mixlab_amd.workspace import Workspace  # noqa: E402

WARMUP, SPT, TRACK = 3, 800, 60000
SHAPES = ((2, 1), (2, 64), (1024, 64))
DELAYS = (256, 5714, 100000)


def reps_of(n_decks):
    return 200 if n_decks <= 2 else 20


def trace_means(path):
    """the echo kernels of a one-round run in launch order: per shape and delay WARMUP + reps launches of one of the two kernels"""
    import csv
    runs = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "k_deck_echo_" in row["Kernel_Name"]:
                runs.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"]), row["Kernel_Name"].split("(")[0].split("::")[-1]))
    runs.sort()
    at = 0
    for n_decks, n_ticks in SHAPES:
        for delay in DELAYS:
            part = runs[at + WARMUP:at + WARMUP + reps_of(n_decks)]
            at += WARMUP + reps_of(n_decks)
            d = [(e - s) / 1e3 for s, e, _n in part]
            print(f"decks={n_decks} ticks={n_ticks} delay={delay} kernel={part[0][2]} launches_after_warmup={len(d)} mean_us={statistics.mean(d):.1f} min_us={min(d):.1f} max_us={max(d):.1f}")
    assert at == len(runs), (at, len(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--trace-csv")
    args = ap.parse_args()
    if args.trace_csv:
        return trace_means(args.trace_csv)
    hip = C.CDLL("libamdhip64.so")
    rng = np.random.default_rng(3)
    track = rng.integers(-20000, 20001, (TRACK, 2), dtype=np.int16)
    step = deck.deck_step(48000, 48000, 1.08)
    for n_decks, n_ticks in SHAPES:
        ws = Workspace(48000, 60)
        srcs = [ws.source_stereo() for _ in range(n_decks)]
        g = ws.build(max_ticks_per_run=n_ticks)
        decks = []
        for _ in range(n_decks):
            d = deck.Deck(TRACK)
            d.load(track)
            d.set(step_q32=step, loop_in=0, loop_out=TRACK, flags=abi.DECK_PLAY | abi.DECK_LOOP)
            decks.append(d)
        reps = reps_of(n_decks)

        def timed():
            for _ in range(WARMUP):
                deck.feed(decks, srcs, g, n_ticks)
            hip.hipDeviceSynchronize()
            t = time.perf_counter()
            for _ in range(reps):
                deck.feed(decks, srcs, g, n_ticks)
            t_enq = time.perf_counter() - t
            hip.hipDeviceSynchronize()
            return (time.perf_counter() - t) / reps * 1e6, t_enq / reps * 1e6

        readings = {}
        for _round in range(args.rounds):
            for delay in (0,) + DELAYS:
                for d in decks:
                    d.set_echo(deck.echo(delay, feedback=0.5, damp=0.3) if delay else None)
                readings.setdefault(delay, []).append(timed() + (deck.debug_last_echo(),))
        for delay, r in readings.items():
            whole, enq = statistics.median(x[0] for x in r), statistics.median(x[1] for x in r)
            print(f"decks={n_decks} ticks={n_ticks} {'delay=' + str(delay) if delay else 'no echo'} per_feed_us={whole:.1f} enqueue_us={enq:.1f} "
                  f"all={[round(x[0], 1) for x in r]} forms={r[-1][2]}", flush=True)
        for d in decks:
            d.close()
    print("deck_echo_cost done")


if __name__ == "__main__":
    main()
