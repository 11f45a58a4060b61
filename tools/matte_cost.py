#!/usr/bin/env python
"""Cost of the matte refiner.

`--part pixel`: mx_video_matte of one 1920 x 1080 frame, 64 back to back per case, the cases alternating over three rounds -- no stage (the copy floor), MASK only
(a rectangle and a circle, on a frame with and without incoming coverage: the wipe), CLEAN + choke 2 + soften 2, and choke 6 + soften 6 -- and beside them, in the
same process and so in the same kernel trace, mx_video_key on the same picture and a device-to-device copy of a frame's 3.1 MB, 256 back to back.  Every pixel call
also creates its output frame (an allocation, a blank fill and an opaque fill), the same for every case, so the wall times differ by their kernels; the kernels' own
times come from the trace of the run:
    rocprofv3 --kernel-trace --stats -d <dir> -o matte --output-format csv -- python tools/matte_cost.py --part pixel
where k_video_matte_stream<CLEAN, MASK> is the streaming form (MASK 0 none, 1 rectangle, 2 circle) and k_video_matte_tile<HALO, MASK> the neighbourhood form
(HALO 4: choke 2 + soften 2; HALO 12: choke 6 + soften 6).  The copies of this part are the only __amd_rocclr_copyBuffer dispatches of its trace.

`--part graph`: the 8-layer 1080p config-4 cascade (7 VideoMixers into the RGBA sink) with layer 3 (1080p) plain, keyed, and keyed and matted (CLEAN + choke 1 +
soften 2), its source a ring of 72 distinct frames -- more than the source keeps (32), so EVERY tick transforms a frame it has not seen (a camera) -- and keyed and
matted over a ring of two (transformed twice, then reused).  The cases alternate on the one graph, three rounds each, median: wall time per tick, one-tick and
64-tick runs."""
import argparse
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
import video_matte_model as mm  # noqa: E402
from benchlegs.common import VIDEO_SIZES, video_cascade  # noqa: E402
from mixlab_amd import video  # noqa: E402
from mixlab_amd.workspace import Workspace  # noqa: E402

W, H, BATCH, LAYER, RING = 1920, 1080, 256, 3, 72
FRAME_BYTES = W * H * 3 // 2
KEY = km.DEFAULT_CHROMA
GRAPH_MATTE = mm.MatteP(clean=(24, 230), choke=1, soften=2)


def key_params():
    return video.KeyParams(KEY.mode, KEY.key_u, KEY.key_v, False, KEY.near_q4, KEY.far_q4, KEY.spill_far_q4, KEY.spill_strength)


def mp(p):
    return video.MatteParams(clean=p.clean, choke=p.choke, soften=p.soften, mask=p.mask, invert=bool(p.invert), feather_q4=p.feather, shape=p.shape)


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

    y, u, v, k = mm.keyed_picture(W, H)
    plain = video.DFrame(W, H).upload(y, u, v)
    cov = video.DFrame(W, H, fmt=video.PIXFMT_YUVA420P).upload(y, u, v)
    cov.upload_alpha(k)
    rect, iris = video.matte_wipe(video.WIPE_LEFT, 32768, 16 * 8, W, H), video.matte_wipe(video.WIPE_IRIS, 32768, 16 * 8, W, H)
    kprm = key_params()
    cases = {   # name -> (call, bytes the kernel moves)
        "key": (lambda: video.key(plain, kprm), 4 * W * H),
        "matte_no_stage": (lambda: video.matte(cov, mp(mm.MatteP())), 5 * W * H),
        "matte_mask_rect_no_coverage": (lambda: video.matte(plain, rect), 4 * W * H),
        "matte_mask_rect": (lambda: video.matte(cov, rect), 5 * W * H),
        "matte_mask_circle": (lambda: video.matte(cov, iris), 5 * W * H),
        "matte_clean_choke2_soften2": (lambda: video.matte(cov, mp(mm.MatteP(clean=(24, 230), choke=2, soften=2))), 5 * W * H),
        "matte_choke6_soften6": (lambda: video.matte(cov, mp(mm.MatteP(choke=6, soften=6))), 5 * W * H),
    }
    res = {name: [] for name in cases}
    for _rnd in range(3):
        for name, (fn, _b) in cases.items():
            res[name].append(timed(fn, 64))
    floor = statistics.median(res["matte_no_stage"])
    for name, (_fn, moved) in cases.items():
        m = statistics.median(res[name])
        print(f"pixel call (with its output frame's creation) case={name} us_per_call={m:.1f} over_matte_no_stage={m - floor:+.1f} kernel_bytes={moved} "
              f"rounds={' '.join(f'{x:.1f}' for x in res[name])}", flush=True)


def graph_cases():
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
    kprm, mprm = key_params(), mp(GRAPH_MATTE)
    cases = {"none": (None, None, long_ring), "keyed_every_tick": (kprm, None, long_ring), "keyed_matted_every_tick": (kprm, mprm, long_ring),
             "keyed_matted_ring_of_2": (kprm, mprm, long_ring[:2])}
    tick = 0
    for ticks, reps in ((1, 128), (64, 4)):
        res = {name: [] for name in cases}
        for _rnd in range(3):
            for name, (kp_, mp_, ring) in cases.items():
                video.graph_set_video_source_key(g, srcs[LAYER], kp_)
                video.graph_set_video_source_matte(g, srcs[LAYER], mp_)
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
            print(f"graph layer3={name} ticks_per_run={ticks} us_per_tick={m:.1f} over_none={m - base:+.1f} rounds={' '.join(f'{x:.1f}' for x in res[name])}", flush=True)
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("pixel", "graph", "all"), default="all")
    part = ap.parse_args().part
    if part in ("pixel", "all"):
        pixel_calls()
    if part in ("graph", "all"):
        graph_cases()
    print("matte_cost done")


if __name__ == "__main__":
    main()
