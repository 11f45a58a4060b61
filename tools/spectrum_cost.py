#!/usr/bin/env python
"""Cost of spectrum taps on the headline-sized desk: 1024 config-2 strips into one Mixer at 48 kHz, n_fft 2048 and 31
log bands, with no taps, with 2 taps (the Master and the Cue) and with 1026 taps (these and every strip's Amplifier port, stored one float per
frame), one-tick runs and 2048-tick runs.  The cases alternate on the one graph (mx_graph_set_spectra between them), three rounds each: a
same-box A/B of the wall time per run.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/spectrum_cost.py` for the kernels' own
times (k_spectrum / k_spectrum_history)."""
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import synth  # noqa: E402
from mixlab_amd import abi  # noqa: E402
from od_cost import desk  # noqa: E402


def main():
    sr, spt, n_strips, n_fft, n_bands = 48000, 800, 1024, 2048, 31
    edges = abi.log_band_edges(n_fft, n_bands, 20.0, 20000.0, sr)
    ws, srcs, _ = desk(n_strips, sr, False)
    mix = 0
    buses = [(mix, 0), (mix, 1)]
    cases = {"none": [], "buses": buses, "all": [(mix + 6 * (k + 1), 0) for k in range(n_strips)] + buses}
    g = ws.build(max_ticks_per_run=2048)
    x = synth.noise(1, 2048 * spt)
    for s in srcs:
        g.write_source(s, x, 2048)
    tick = 0
    for ticks, reps in ((1, 200), (2048, 5)):
        res = {k: [] for k in cases}
        for rnd in range(3):
            for name, taps in cases.items():
                g.set_spectra(taps, n_fft, edges)
                for _ in range(2):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                t = time.perf_counter()
                for _ in range(reps):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                res[name].append((time.perf_counter() - t) * 1e3 / reps)
                if taps:
                    r = g.read_spectra(ticks - 1, 1)
                    assert r.shape == (1, len(taps), 2, n_bands) and r[0, -2, 0].max() > 0
        for name, taps in cases.items():
            print(f"spectra={len(taps)} ticks={ticks} n_fft={n_fft} bands={n_bands} ms_per_run={statistics.median(res[name]):.3f} "
                  f"rounds={' '.join(f'{v:.3f}' for v in res[name])}", flush=True)
    g.close()
    print("spectrum_cost done")


if __name__ == "__main__":
    main()
