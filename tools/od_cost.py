#!/usr/bin/env python
"""Cost of an OutputDevice on the headline-sized desk (DESIGN.md "OutputDevice"): 1024 config-2 strips into one Mixer, with and without
an OutputDevice (2 channels) on the Master, one-tick runs and 2048-tick runs at 48 kHz.  Prints the wall time per run of each case;
run it under `rocprofv3 --kernel-trace --stats -- python tools/od_cost.py` for the kernels' own times (k_out_route / k_out_scan)."""
import pathlib
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import synth  # noqa: E402
from mixlab_amd.workspace import Workspace  # noqa: E402


def desk(n_strips, sr, with_node):
    ws = Workspace(sr, 60)
    mix = ws.mixer([(-6.0, 0.8, k % 8 == 0) for k in range(n_strips)])
    srcs = []
    for k in range(n_strips):
        trig = ws.trigger(True); env = ws.envelope(); src = ws.source_mono()
        eq = ws.eq_three(2.0, -1.0, 0.5); pan = ws.stereo_panner(); amp = ws.amplifier(1.0, 0.5)
        ws.connect(trig, 0, env, 0); ws.connect(src, 0, eq, 0)
        ws.connect(eq, 0, pan, 0); ws.connect(eq, 0, pan, 1)
        ws.connect(pan, 0, amp, 0); ws.connect(env, 0, amp, 1); ws.connect(amp, 0, mix, k)
        srcs.append(src)
    od = None
    if with_node:
        od = ws.output_device(2, 0, 1)
        ws.connect(mix, 0, od, 0)
    return ws, srcs, od


def main():
    sr, spt, n_strips = 48000, 800, 1024
    for with_node in (False, True):
        ws, srcs, od = desk(n_strips, sr, with_node)
        g = ws.build(max_ticks_per_run=2048)
        x = synth.noise(1, 2048 * spt)
        for s in srcs:
            g.write_source(s, x, 2048)
        for ticks, reps in ((1, 200), (2048, 10)):
            tick = 0
            for _ in range(3):
                g.run_ticks(tick, ticks); tick += ticks
            g.sync()
            t = time.perf_counter()
            for _ in range(reps):
                g.run_ticks(tick, ticks); tick += ticks
            g.sync()
            ms = (time.perf_counter() - t) * 1e3 / reps
            if od is not None:
                out, recs = g.read_audio_out(od, 0, ticks)
                assert out.size == ticks * spt * 2 and recs.size == ticks
            print(f"node={int(with_node)} ticks={ticks} ms_per_run={ms:.3f}", flush=True)
        g.close()
    print("od_cost done")


if __name__ == "__main__":
    main()
