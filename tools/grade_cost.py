#!/usr/bin/env python
"""Cost of the colour corrector.

The pixel call first: mx_video_grade of one 1920 x 1080 frame, 64 back to back, for curve + matrix alone, for all three stages with the 33-lattice, and for all
three stages with the 17-lattice in BOTH gather forms -- the lattice read through the caches (MX_GRADE_GATHER=global) and the lattice staged in LDS (the default) --
in the same process, the cases alternating over three rounds.  Every call also creates its output frame (an allocation and a blank fill), the same for every case,
so the rows differ by their kernels; the row "no stage" (flags 0: the kernel copies) is the floor.  Beside them a device-to-device copy of the frame's 3.1 MB, 256
back to back.  The kernels' own times come from the kernel trace of the same run:
    rocprofv3 --kernel-trace --stats -d <dir> -o grade --output-format csv -- python tools/grade_cost.py
where k_video_grade<0, 0> is the path without a LUT, <1, 4> / <1, 5> the cached gather of the 17- / 33-lattice and <2, 4> the 17-lattice staged in LDS.

Then the graph: the 8-layer 1080p config-4 cascade (7 VideoMixers into the RGBA sink) with and without mx_graph_set_video_source_grade on layer 3 (1080p), whose
source is a ring of 72 distinct frames -- more than the source keeps graded (32), so with the grade set EVERY tick grades a frame it has not seen (a camera) -- and a
ring of two frames (graded twice, then reused).  The cases alternate on the one graph, three rounds each, median: wall time per tick, one-tick and 64-tick runs."""
import ctypes as C
import os
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import synth  # noqa: E402
import video_grade_model as gm  # noqa: E402
from benchlegs.common import VIDEO_SIZES, video_cascade  # noqa: E402
from mixlab_amd import video  # noqa: E402
from mixlab_amd.workspace import Workspace  # noqa: E402

W, H, BATCH, LAYER, RING = 1920, 1080, 256, 3, 72
FRAME_BYTES = W * H * 3 // 2
ALL = gm.CURVE | gm.CHROMA | gm.LUT


def prm(p):
    return video.GradeParams(p.flags, p.curve, p.m, p.off)


def pixel_calls():
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

    y, u, v = gm.noise_picture(W, H, 0)
    frame = video.DFrame(W, H).upload(y, u, v)
    p17, p33 = gm.shared_params(4, ALL, "smooth"), gm.shared_params(5, ALL, "smooth")
    l17, l33 = video.Lut(4, p17.nodes), video.Lut(5, p33.nodes)
    cases = {   # name -> (params, lattice, MX_GRADE_GATHER)
        "no_stage": (prm(p17.but(flags=0)), None, None),
        "curve_matrix": (prm(p17.but(flags=gm.CURVE | gm.CHROMA)), None, None),
        "all_lattice33_global": (prm(p33), l33, None),
        "all_lattice17_global": (prm(p17), l17, "global"),
        "all_lattice17_lds": (prm(p17), l17, "lds"),
    }
    res = {k: [] for k in cases}
    for _rnd in range(3):
        for name, (params, lut, gather) in cases.items():
            if gather is None:
                os.environ.pop("MX_GRADE_GATHER", None)
            else:
                os.environ["MX_GRADE_GATHER"] = gather
            res[name].append(timed(lambda: video.grade(frame, params, lut), 64))
    os.environ.pop("MX_GRADE_GATHER", None)
    floor = statistics.median(res["no_stage"])
    for name in cases:
        m = statistics.median(res[name])
        print(f"mx_video_grade call (with its output frame's creation) case={name} us_per_call={m:.1f} over_no_stage={m - floor:+.1f} "
              f"rounds={' '.join(f'{x:.1f}' for x in res[name])}", flush=True)
    print(f"corrector bytes moved per frame (no coverage plane) = {2 * FRAME_BYTES}: the kernels' own times are in the kernel trace (k_video_grade<gather, lattice_log2>)", flush=True)
    return p17, l17


def graph_cases(p17, l17):
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
    y, u, v = gm.noise_picture(W, H, 1)
    long_ring = [video.DFrame(W, H).upload(np.roll(y, 2 * j, axis=0), np.roll(u, j, axis=0), np.roll(v, j, axis=0)) for j in range(RING)]
    all17, cm = prm(p17), prm(p17.but(flags=gm.CURVE | gm.CHROMA))
    cases = {"none": (None, None, long_ring), "curve_matrix_every_tick": (cm, None, long_ring), "all17_every_tick": (all17, l17, long_ring),
             "all17_ring_of_2": (all17, l17, long_ring[:2])}
    tick = 0
    for ticks, reps in ((1, 128), (64, 4)):
        res = {k: [] for k in cases}
        for _rnd in range(3):
            for name, (params, lut, ring) in cases.items():
                video.graph_set_video_source_grade(g, srcs[LAYER], params, lut)
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
            print(f"graph grade={name} ticks_per_run={ticks} us_per_tick={m:.1f} over_none={m - base:+.1f} rounds={' '.join(f'{x:.1f}' for x in res[name])}", flush=True)
    g.close()


def main():
    p17, l17 = pixel_calls()
    graph_cases(p17, l17)
    print("grade_cost done")


if __name__ == "__main__":
    main()
