#!/usr/bin/env python
"""Cost of the placer.

The graph: the 8-layer 1080p config-4 cascade (7 VideoMixers into the RGBA sink) with and without a placement on layer 3 (1080p): the layer shown as a
480 x 270 inset at (1376, 64) of a 1920 x 1080 canvas.  The inset case feeds a ring of 72 distinct frames -- more than the source keeps placed (32), so
EVERY tick places a frame it has not seen (a camera: the layer changes every tick).  The baseline is the same layer, unplaced, as a ring of two frames.
A third case places the ring of two: placed twice, then reused.  The cases alternate on the one graph, three rounds each, median: a same-box A/B of the
wall time per tick, one-tick runs and 64-tick runs.

Beside it, for the kernel trace: a device-to-device copy of a frame's 3.1 MB, 256 back to back, mx_video_key and mx_video_place alone on the stream
(each call also creates its output frame -- the pixel-path calls are not the hot path), and the placer at a zoom (640 x 360 of the frame to the full
canvas: every canvas byte is a resampled one).

Run it under `rocprofv3 --kernel-trace --stats -- python tools/place_cost.py` for the kernels' own times (k_video_place, k_video_key)."""
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


def inset():
    return video.PlaceParams(W, H, 1376, 64, 480, 270)


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
    cases = {"none_ring_of_2": (None, long_ring[:2]), "inset_every_tick": (inset(), long_ring), "inset_ring_of_2": (inset(), long_ring[:2])}
    tick = 0
    for ticks, reps in ((1, 128), (64, 4)):
        res = {k: [] for k in cases}
        for _rnd in range(3):
            for name, (prm, ring) in cases.items():
                video.graph_set_video_source_place(g, srcs[LAYER], prm)
                video.graph_set_video_source_ring(g, srcs[LAYER], ring, dur=(1, 60), off=(0, 1))
                for _ in range(2):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                t = time.perf_counter()
                for _ in range(reps):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                res[name].append((time.perf_counter() - t) * 1e6 / (reps * ticks))
        base = statistics.median(res["none_ring_of_2"])
        for name in cases:
            m = statistics.median(res[name])
            print(f"graph place={name} ticks_per_run={ticks} us_per_tick={m:.1f} over_none={m - base:+.1f} rounds={' '.join(f'{x:.1f}' for x in res[name])}", flush=True)
    g.close()

    # the yardsticks and the pixel-path calls
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
    kprm = video.KeyParams(KEY.mode, KEY.key_u, KEY.key_v, False, KEY.near_q4, KEY.far_q4, KEY.spill_far_q4, KEY.spill_strength)
    calls = [timed(lambda: video.key(long_ring[0], kprm), 64) for _ in range(3)]
    print(f"mx_video_key call (with its output frame's creation) us_per_call={statistics.median(calls):.1f} rounds={' '.join(f'{x:.1f}' for x in calls)}", flush=True)
    for name, prm in (("inset 480x270", inset()), ("zoom 640x360 -> 1920x1080", video.PlaceParams(W, H, 0, 0, W, H, crop=(600, 300, 640, 360))),
                      ("1:1 whole frame", video.PlaceParams(W, H, 0, 0, W, H))):
        calls = [timed(lambda: video.place(long_ring[0], prm), 64) for _ in range(3)]
        print(f"mx_video_place {name} call (with its output frame's creation) us_per_call={statistics.median(calls):.1f} rounds={' '.join(f'{x:.1f}' for x in calls)}", flush=True)
    print(f"placer bytes written per canvas = {5 * W * H // 2} (Y, coverage, U, V): the kernel's own time is in the kernel trace (k_video_place)", flush=True)
    print("place_cost done")


if __name__ == "__main__":
    main()
