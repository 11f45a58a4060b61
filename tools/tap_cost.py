#!/usr/bin/env python
"""Cost of one audio tap set on the headline-sized desk (DESIGN.md sections 0.2, 0.3, 0.5, 0.6, 0.8, 0.9, 0.10): 1024 config-2 strips into one Mixer at
48 kHz, with no taps, with 2 taps (the Master and the Cue; not for the meters) and with 1026 taps (these and every strip's Amplifier port,
stored one float per frame), one-tick runs and 2048-tick runs.  The cases alternate on the one graph (the set's mx_graph_set_* between
them), three rounds each: a same-box A/B of the wall time per run.

    python tools/tap_cost.py <meters|spectrum|loudness|stereo|limiter|tempo|tonality>

  meters    hold 0, release 1
  spectrum  n_fft 2048, 31 log bands
  loudness  windows of 24 and 180 ticks
  stereo    a window of 180 ticks and a 64 x 64 goniometer: a record every 6 ticks on the buses, every 60 ticks on 1026 taps, which keeps a
            2048-tick run's records at 0.6 GB
  limiter   ceiling 0.5, lookahead 240 frames (5 ms).  The limited copies of 1026 taps are 6.6 MB per tick of the graph's
            max_ticks_per_run (13.4 GB at 2048), so the three cases alternate on a desk built for runs of LIMITER_LONG = 256 ticks (1.7 GB),
            and the cases without and with 2 taps alternate again on a desk built for 2048-tick runs
  tempo     hops of 128 frames, a window of 2048 hops, 512 lags, a record every 6 ticks; one-tick, 256-tick and 2048-tick runs
  tonality  decimation 8, hops of 512 decimated frames, 5 octaves from C2, a record every 30 ticks; one-tick, 256-tick and 2048-tick runs

Run it under `rocprofv3 --kernel-trace --stats -- python tools/tap_cost.py <set>` for the kernels' own times (k_meter_*, k_spectrum*,
k_loud_*, k_stereo_*, k_limit*, k_tempo_*, k_ton_*)."""
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tools")); sys.path.insert(0, str(ROOT / "tests"))
import synth  # noqa: E402
from mixlab_amd import abi  # noqa: E402
from od_cost import desk  # noqa: E402

SR, SPT, N_STRIPS, N_FFT, N_BANDS = 48000, 800, 1024, 2048, 31
HOPS = {0: 1, 2: 6, N_STRIPS + 2: 60}   # stereo: the goniometer's hop by the number of taps
LIMITER_LONG = 256                       # limiter: ticks of the long runs that 1026 taps take part in


def set_meters(g, taps):
    g.set_meters(taps)


def set_spectrum(g, taps):
    g.set_spectra(taps, N_FFT, abi.log_band_edges(N_FFT, N_BANDS, 20.0, 20000.0, SR))


def set_loudness(g, taps):
    g.set_loudness(taps, 24, 180)


def set_stereo(g, taps):
    g.set_stereo(taps, 180, 64, 0, HOPS[len(taps)])


def set_limiter(g, taps):
    g.set_limiters(taps, 0.5, 240)


def set_tempo(g, taps):
    g.set_tempo(taps, 128, 2048, 512, 6)


def read_tempo(g, taps, ticks):
    rows = g.read_tempo()   # (a one-tick run emits on every sixth run only)
    assert all(len(row) == len(taps) and row[-2]["hop_frames"] == 128 for row in rows) and (ticks < 6 or rows[-1][-2]["acf"][0] > 0)


def set_tonality(g, taps):
    g.set_tonality(taps, 8, 512, 5, 65406, 30)


def read_tonality(g, taps, ticks):
    rows = g.read_tonality()   # (a one-tick run emits on every thirtieth run only)
    assert all(len(row) == len(taps) and row[-2]["hop_frames"] == 512 for row in rows) and (ticks < 30 or rows[-1][-2]["cq"].any())


def read_limiter(g, taps, ticks):
    r = g.read_limiters(ticks - 1, 1)
    y = g.read_limited(len(taps) - 2, ticks - 1, 1)
    assert r.shape == (1, len(taps)) and int(r["frames"][0, 0]) == SPT and y.size == 2 * SPT and float(abs(y).max()) <= 0.5


def read_meters(g, taps, ticks):
    m = g.read_meters(0, ticks)
    assert m.shape == (ticks, len(taps)) and int(m["frames"][0, 0]) == SPT


def read_spectrum(g, taps, ticks):
    r = g.read_spectra(ticks - 1, 1)
    assert r.shape == (1, len(taps), 2, N_BANDS) and r[0, -2, 0].max() > 0


def read_loudness(g, taps, ticks):
    r = g.read_loudness(ticks - 1, 1)
    assert r.shape == (1, len(taps)) and r["momentary_sq"][0, -2] > 0


def read_stereo(g, taps, ticks):
    r = g.read_stereo(ticks - 1, 1)
    assert r.shape == (1, len(taps)) and r["win_ll"][0, -2] > 0


# per set: how a case is set and its read-back checked, the start of its line, the 2-tap case, warm-up runs, repetitions of the long runs
# and the name its closing line carries
SETS = {
    "meters": (set_meters, read_meters, lambda n: f"meters={n}", False, 3, 10, "meter_cost"),
    "spectrum": (set_spectrum, read_spectrum, lambda n: f"spectra={n}", True, 2, 5, "spectrum_cost"),
    "loudness": (set_loudness, read_loudness, lambda n: f"loudness={n}", True, 2, 5, "loudness_cost"),
    "stereo": (set_stereo, read_stereo, lambda n: f"stereo={n} hop={HOPS[n]}", True, 2, 5, "stereo_cost"),
    "limiter": (set_limiter, read_limiter, lambda n: f"limiters={n}", True, 2, 5, "limiter_cost"),
    "tempo": (set_tempo, read_tempo, lambda n: f"tempo={n}", True, 2, 5, "tempo_cost"),
    "tonality": (set_tonality, read_tonality, lambda n: f"tonality={n}", True, 2, 5, "tonality_cost"),
}


def measure(which, max_ticks, cases, lengths):
    """the cases alternating on one desk built for runs of max_ticks ticks: three rounds per run length, the median printed"""
    set_taps, check_read, head, _, warm, _, _ = SETS[which]
    ws, srcs, _ = desk(N_STRIPS, SR, False)
    g = ws.build(max_ticks_per_run=max_ticks)
    x = synth.noise(1, max_ticks * SPT)
    for s in srcs:
        g.write_source(s, x, max_ticks)
    tick = 0
    for ticks, reps in lengths:
        res = [[] for _ in cases]
        for rnd in range(3):
            for k, taps in enumerate(cases):
                set_taps(g, taps)
                for _ in range(warm):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                t = time.perf_counter()
                for _ in range(reps):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                res[k].append((time.perf_counter() - t) * 1e3 / reps)
                if taps:
                    check_read(g, taps, ticks)
        for k, taps in enumerate(cases):
            sizes = f" n_fft={N_FFT} bands={N_BANDS}" if which == "spectrum" else ""
            print(f"{head(len(taps))} ticks={ticks}{sizes} ms_per_run={statistics.median(res[k]):.3f} "
                  f"rounds={' '.join(f'{v:.3f}' for v in res[k])}", flush=True)
        if which == "meters":
            algo = ticks * (N_STRIPS * SPT * 4 + 2 * SPT * 8) + ticks * len(cases[-1]) * 48
            print(f"ticks={ticks} algorithmic_bytes={algo}", flush=True)
    g.close()


def main(which):
    _, _, _, with_buses, _, long_reps, name = SETS[which]
    mix = 0
    buses = [(mix, 0), (mix, 1)]
    cases = [[]] + ([buses] if with_buses else []) + [[(mix + 6 * (k + 1), 0) for k in range(N_STRIPS)] + buses]
    if which == "limiter":
        measure(which, LIMITER_LONG, cases, ((1, 200), (LIMITER_LONG, 3 * long_reps)))
        measure(which, 2048, cases[:2], ((2048, long_reps),))
    elif which in ("tempo", "tonality"):
        measure(which, 2048, cases, ((1, 240), (256, 3 * long_reps), (2048, long_reps)))
    else:
        measure(which, 2048, cases, ((1, 200), (2048, long_reps)))
    print(f"{name} done")


if __name__ == "__main__":
    if len(sys.argv) != 2 or sys.argv[1] not in SETS:
        sys.exit(f"usage: tap_cost.py <{'|'.join(SETS)}>")
    main(sys.argv[1])
