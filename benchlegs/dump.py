"""--dump-outputs DIR: what the timed path handed its caller in its LAST timed step -- the job's Master and Cue buses (N > 1: the exchange's combined
buses, which every rank holds; rank 0 writes them) -- as DIR/master.npy and DIR/cue.npy, float32 [ticks, samples_per_tick, 2 (L, R)].  The inputs are
seeded (tests/synth.py), so two builds run with the same arguments can be compared file for file.  Above CAP_BYTES a fixed, seeded set of whole ticks is
kept, the same for both buses, and DIR/ticks.npy (float64) lists them."""
from __future__ import annotations

import pathlib

import numpy as np

CAP_BYTES = 64 << 20


def collect(job, ex, step):
    """Read the buses of timed step `step` back; call before any later step can overwrite them."""
    if ex is not None:
        m, c = ex.result(step)
    else:
        m, c = (job.g.read_output(job.mix, port, job.T, True) for port in (0, 1))
    return {"master": m.reshape(job.T, job.spt, 2), "cue": c.reshape(job.T, job.spt, 2)}


def write(out_dir, bufs):
    n_ticks = next(iter(bufs.values())).shape[0]
    per_tick = sum(a[0].nbytes for a in bufs.values())
    if per_tick * n_ticks > CAP_BYTES:
        keep = (CAP_BYTES - 8 * n_ticks) // per_tick
        ticks = np.sort(np.random.default_rng(0).choice(n_ticks, size=keep, replace=False))
        bufs = {k: a[ticks] for k, a in bufs.items()}
        bufs["ticks"] = ticks.astype(np.float64)
    out = pathlib.Path(out_dir)
    out.mkdir(parents=True, exist_ok=True)
    for name, a in bufs.items():
        np.save(out / f"{name}.npy", np.ascontiguousarray(a))
    return {name: list(a.shape) for name, a in bufs.items()}
