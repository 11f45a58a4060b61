#!/usr/bin/env python
"""Cost of the keyer.

The graph: the 8-layer 1080p config-4 cascade (7 VideoMixers into the RGBA sink) with and without a key on layer 3 (1080p), whose source is a ring
of 72 distinct frames -- more than the source keeps keyed (32), so with the key set EVERY tick keys a frame it has not seen (a camera: the layer changes
every tick).  A third case keys a ring of two frames: keyed twice, then reused.  The cases alternate on the one graph (mx_graph_set_video_source_key /
_ring between them), three rounds each, median: a same-box A/B of the wall time per tick, one-tick runs and 64-tick runs.

Beside it a device-to-device copy of a frame's 3.1 MB, 256 back to back (what a read-once pass reaches at this size), and mx_video_key alone on the
stream (each call also creates its output frame: an allocation, a blank fill and an opaque fill -- the pixel-path call is not the hot path).

Run it under `rocprofv3 --kernel-trace --stats -- python tools/key_cost.py` for the kernel's own time (k_video_key)."""
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import synth  # noqa: E402
import video_key_model as km  # noqa: E402
from benchlegs.common import VIDEO_SIZES, video_cascade  # noqa: E402
from mixlab_amd import video  # noqa: E402
from mixlab_amd.workspace import Workspace  # noqa: E402

W, H, BATCH, LAYER, RING = 1920, 1080, 256, 3, 72
FRAME_BYTES = W * H * 3 // 2
KEY = km.DEFAULT_CHROMA


def params():
    return video.KeyParams(KEY.mode, KEY.key_u, KEY.key_v, False, KEY.near_q4, KEY.far_q4, KEY.spill_far_q4, KEY.spill_strength)


def main():
    ws = Workspace(44100, 60)
    srcs, _rgba = video_cascade(ws)
    g = ws.build(max_ticks_per_run=64)
    keep = []
    for k, (s, (w, h)) in enumerate(zip(srcs, VIDEO_SIZES)):
        if k == LAYER:
            continue
        ring = [video.DFrame(w, h).upload(*synth.yuv_pattern(w, h, k, j, 0)) for j in range(2)]
        keep.append(ring)
        video.graph_set_video_source_ring(g, s, ring, dur=(1, 60), off=(0, 1))
    y, u, v = km.green_screen(W, H, seed=0)
    long_ring = [video.DFrame(W, H).upload(np.roll(y, 2 * j, axis=0), np.roll(u, j, axis=0), np.roll(v, j, axis=0)) for j in range(RING)]
    cases = {"none": (None, long_ring), "keyed_every_tick": (params(), long_ring), "keyed_ring_of_2": (params(), long_ring[:2])}
    tick = 0
    for ticks, reps in ((1, 128), (64, 4)):
        res = {k: [] for k in cases}
        for _rnd in range(3):
            for name, (prm, ring) in cases.items():
                video.graph_set_video_source_key(g, srcs[LAYER], prm)
                video.graph_set_video_source_ring(g, srcs[LAYER], ring, dur=(1, 60), off=(0, 1))
                for _ in range(2):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                t = time.perf_counter()
                for _ in range(reps):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                res[name].append((time.perf_counter() - t) * 1e6 / (reps * ticks))
        base = statistics.median(res["none"])
        for name in cases:
            m = statistics.median(res[name])
            print(f"graph key={name} ticks_per_run={ticks} us_per_tick={m:.1f} over_none={m - base:+.1f} rounds={' '.join(f'{x:.1f}' for x in res[name])}", flush=True)
    g.close()

    # the yardstick and the pixel-path call
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    src, dst = video.DeviceBuffer(FRAME_BYTES), video.DeviceBuffer(FRAME_BYTES)

    def timed(fn, n):
        for _ in range(8):
            fn()
        hip.hipDeviceSynchronize(); video.sync()
        t = time.perf_counter()
        for _ in range(n):
            fn()
        hip.hipDeviceSynchronize(); video.sync()
        return (time.perf_counter() - t) * 1e6 / n

    copies = [timed(lambda: hip.hipMemcpyAsync(dst.ptr, src.ptr, FRAME_BYTES, 3, None), BATCH) for _ in range(3)]
    copy = statistics.median(copies)
    print(f"copy_d2d bytes={FRAME_BYTES} us_per_frame={copy:.2f} frac_of_8TBs={FRAME_BYTES / (copy * 1e-6) / 8e12:.4f} rounds={' '.join(f'{x:.2f}' for x in copies)}", flush=True)
    prm = params()
    calls = [timed(lambda: video.key(long_ring[0], prm), 64) for _ in range(3)]
    print(f"mx_video_key call (with its output frame's creation) us_per_call={statistics.median(calls):.1f} rounds={' '.join(f'{x:.1f}' for x in calls)}", flush=True)
    moved = 4 * W * H
    print(f"keyer bytes moved per frame (no incoming coverage) = {moved}: the kernel's own time is in the kernel trace (k_video_key)", flush=True)
    print("key_cost done")


if __name__ == "__main__":
    main()
