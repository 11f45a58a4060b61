#!/usr/bin/env python
"""Cost of level meters on the headline-sized desk: 1024 config-2 strips into one Mixer at 48 kHz, with no taps and
with 1026 taps (every strip's Amplifier port -- stored one float per frame -- plus the Master and the Cue), one-tick runs and 2048-tick runs.
The two cases alternate on the one graph (mx_graph_set_meters between them), three rounds each: a same-box A/B of the wall time per run.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/meter_cost.py` for the kernels' own times (k_meter_reduce / k_meter_hold)."""
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import synth  # noqa: E402
from od_cost import desk  # noqa: E402


def main():
    sr, spt, n_strips = 48000, 800, 1024
    ws, srcs, _ = desk(n_strips, sr, False)
    mix = 0
    amps = [mix + 6 * (k + 1) for k in range(n_strips)]
    taps = [(a, 0) for a in amps] + [(mix, 0), (mix, 1)]
    g = ws.build(max_ticks_per_run=2048)
    x = synth.noise(1, 2048 * spt)
    for s in srcs:
        g.write_source(s, x, 2048)
    tick = 0
    for ticks, reps in ((1, 200), (2048, 10)):
        res = {0: [], 1: []}
        for rnd in range(3):
            for on in (0, 1):
                g.set_meters(taps if on else [])
                for _ in range(3):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                t = time.perf_counter()
                for _ in range(reps):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                res[on].append((time.perf_counter() - t) * 1e3 / reps)
                if on:
                    m = g.read_meters(0, ticks)
                    assert m.shape == (ticks, len(taps)) and int(m["frames"][0, 0]) == spt
        for on in (0, 1):
            print(f"meters={len(taps) if on else 0} ticks={ticks} ms_per_run={statistics.median(res[on]):.3f} "
                  f"rounds={' '.join(f'{v:.3f}' for v in res[on])}", flush=True)
        algo = ticks * (n_strips * spt * 4 + 2 * spt * 8) + ticks * len(taps) * 48
        print(f"ticks={ticks} algorithmic_bytes={algo}", flush=True)
    g.close()
    print("meter_cost done")


if __name__ == "__main__":
    main()
