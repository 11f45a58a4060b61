#!/usr/bin/env python
"""Cost of the deck's reverb: feeds of 2 decks x 1 tick, 2 x 64 ticks and 1024 x 64 ticks at 48 kHz, 800 frames a tick, tempo 1.08,
tracks of 60 000 frames in a loop, with no reverb and with the designed default setting (mx_deck_reverb_design at size 1, two seconds; set once, so every timed tick
runs without a ramp).  Host clock around back-to-back feeds ended by one synchronise (per feed: the whole; enqueue: until the last call returned).

Run it under `rocprofv3 --kernel-trace --stats --output-format csv -- python tools/deck_reverb_cost.py` for the kernel's own times, then hand the trace back:

    python tools/deck_reverb_cost.py --trace-csv out/run/123_kernel_trace.csv   # no device needed: mean of k_deck_reverb per configuration, warm-ups left out, and the
                                                                                 # cycles a block of the walk at --mhz (the kernel's time over the blocks of ONE deck)
    python tools/deck_reverb_cost.py [--rounds 3] [--plain-only]                # --plain-only: the 1024 x 64 feed with no reverb anywhere, one line, for an A/B"""
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

WARMUP, SPT, TRACK, RATE = 3, 800, 60000, 48000
SHAPES = ((2, 1), (2, 64), (1024, 64))


def reps_of(n_decks):
    return 200 if n_decks <= 2 else 20


def default_setting():
    return deck.reverb_design(float(RATE), 1.0, 2.0, 0.3, 0.5, 1.0, 1.0, 0.5)


def trace_means(path, mhz):
    """the reverb kernels of a one-round run in launch order: per shape the feed that takes the setting in, WARMUP launches, then reps"""
    import csv
    runs = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if "k_deck_reverb" in row["Kernel_Name"]:
                runs.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
    runs.sort()
    r = default_setting()
    at = 0
    for n_decks, n_ticks in SHAPES:
        warm = WARMUP + 1
        part = runs[at + warm:at + warm + reps_of(n_decks)]
        at += warm + reps_of(n_decks)
        d = [(e - s) / 1e3 for s, e in part]
        blocks = len(deck.reverb_plan(SPT, [r] * n_ticks))       # of one deck: the decks run side by side, one workgroup each
        print(f"decks={n_decks} ticks={n_ticks} launches_after_warmup={len(d)} mean_us={statistics.mean(d):.1f} min_us={min(d):.1f} max_us={max(d):.1f} "
              f"blocks_per_deck={blocks} us_per_block={statistics.mean(d) / blocks:.2f} cycles_per_block_at_{mhz:.0f}_MHz={statistics.mean(d) * mhz / blocks:.0f}")
    assert at == len(runs), (at, len(runs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--trace-csv")
    ap.add_argument("--mhz", type=float, default=2400.0)
    ap.add_argument("--plain-only", action="store_true")
    args = ap.parse_args()
    if args.trace_csv:
        return trace_means(args.trace_csv, args.mhz)
    hip = C.CDLL("libamdhip64.so")
    rng = np.random.default_rng(3)
    track = rng.integers(-20000, 20001, (TRACK, 2), dtype=np.int16)
    step = deck.deck_step(RATE, RATE, 1.08)
    has_reverb = hasattr(deck, "reverb_design")       # (--plain-only also runs on a build from before the reverb)
    for n_decks, n_ticks in (SHAPES[-1:] if args.plain_only else SHAPES):
        ws = Workspace(RATE, 60)
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
            for mode in ("none",) + (() if args.plain_only else ("default",)):
                if has_reverb:
                    for d in decks:
                        d.set_reverb(default_setting() if mode == "default" else None)
                    if mode == "default":
                        deck.feed(decks, srcs, g, n_ticks)     # the setting's own ramp tick, out of the way: a launch the trace reader counts among the warm-ups
                readings.setdefault(mode, []).append(timed() + (deck.debug_last_reverb() if has_reverb else {},))
        for mode, r in readings.items():
            whole, enq = statistics.median(x[0] for x in r), statistics.median(x[1] for x in r)
            print(f"decks={n_decks} ticks={n_ticks} reverb={mode} per_feed_us={whole:.1f} enqueue_us={enq:.1f} all={[round(x[0], 1) for x in r]} counters={r[-1][2]}", flush=True)
        for d in decks:
            d.close()
    print("deck_reverb_cost done")


if __name__ == "__main__":
    main()
