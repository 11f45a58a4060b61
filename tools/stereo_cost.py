#!/usr/bin/env python
"""Cost of stereo field taps on the headline-sized desk: 1024 config-2 strips into one Mixer at 48 kHz, a window of
180 ticks and a 64 x 64 goniometer, with no taps, with 2 taps (the Master and the Cue, a record every 6 ticks) and with 1026 taps (these and
every strip's Amplifier port, stored one float per frame; a record every 60 ticks, which keeps a 2048-tick run's records at 0.6 GB), one-tick
runs and 2048-tick runs.  The cases alternate on the one graph (mx_graph_set_stereo between them), three rounds each: a same-box A/B of the
wall time per run.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/stereo_cost.py` for the kernels' own times
(k_stereo_emit / k_stereo_reduce / k_stereo_window)."""
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
    buses = [(mix, 0), (mix, 1)]
    cases = {"none": ([], 1), "buses": (buses, 6), "all": ([(mix + 6 * (k + 1), 0) for k in range(n_strips)] + buses, 60)}
    g = ws.build(max_ticks_per_run=2048)
    x = synth.noise(1, 2048 * spt)
    for s in srcs:
        g.write_source(s, x, 2048)
    tick = 0
    for ticks, reps in ((1, 200), (2048, 5)):
        res = {k: [] for k in cases}
        for rnd in range(3):
            for name, (taps, hop) in cases.items():
                g.set_stereo(taps, 180, 64, 0, hop)
                for _ in range(2):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                t = time.perf_counter()
                for _ in range(reps):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                res[name].append((time.perf_counter() - t) * 1e3 / reps)
                if taps:
                    r = g.read_stereo(ticks - 1, 1)
                    assert r.shape == (1, len(taps)) and r["win_ll"][0, -2] > 0
        for name, (taps, hop) in cases.items():
            print(f"stereo={len(taps)} hop={hop} ticks={ticks} ms_per_run={statistics.median(res[name]):.3f} "
                  f"rounds={' '.join(f'{v:.3f}' for v in res[name])}", flush=True)
    g.close()
    print("stereo_cost done")


if __name__ == "__main__":
    main()
