#!/usr/bin/env python
"""Cost of the multiviewer.

The graph: the 8-layer 1080p config-4 cascade (7 VideoMixers into the RGBA sink), every source a ring of two frames.  Four cases alternate on the one graph,
three rounds each, median -- a same-box A/B of the wall time per tick, one-tick runs and 64-tick runs:
  none      no setting
  4x4_hop1  a 1920 x 1080 canvas of sixteen 480 x 270 views, tally frame 4, keep-aspect: the eight sources, the cascade's program (a symbolic chain the tap
            materialises), and seven of the sources again; rendered on every tick (a 64-tick run renders ONE canvas, its last tick's: that is the specification)
  4x4_hop2  the same at hop 2
  2x2_hop1  four 960 x 540 views: the program and sources 0, 1, 6

Beside it, for the kernel trace: a device-to-device copy of a frame's 3.1 MB, the pixel-path call mx_video_multiview on sixteen 1080p frames (it also creates its
canvas), and the same sixteen-view picture by the means that existed before: sixteen mx_video_place calls alone -- a lower bound of that route, which would then need
a 15-step cascade to bring the sixteen canvases together.

Run it under `rocprofv3 --kernel-trace --stats -- python tools/multiview_cost.py` for the kernels' own times (k_video_multiview, k_video_place)."""
import ctypes as C
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import synth  # noqa: E402
from benchlegs.common import VIDEO_SIZES, video_cascade  # noqa: E402
from mixlab_amd import video  # noqa: E402
from mixlab_amd.workspace import Workspace  # noqa: E402

W, H, BATCH = 1920, 1080, 256
FRAME_BYTES = W * H * 3 // 2
RED, GREEN, GREY = (81, 90, 240), (145, 54, 34), (128, 128, 128)


def grid(n, hop, border=4):
    vw, vh = W // n, (H // n) & ~1
    views = [video.MultiviewView(vw * (i % n), vh * (i // n), vw, vh, border, (RED, GREEN, GREY)[min(i, 2)], 1) for i in range(n * n)]
    return video.MultiviewParams(W, H, views, bg=(16, 128, 128), hop=hop)


def main():
    ws = Workspace(44100, 60)
    srcs, _rgba = video_cascade(ws)
    prog = srcs[-1] + 7                        # the seven mixers follow the sources; the last is the program
    g = ws.build(max_ticks_per_run=64)
    keep = []
    for k, (s, (w, h)) in enumerate(zip(srcs, VIDEO_SIZES)):
        ring = [video.DFrame(w, h).upload(*synth.yuv_pattern(w, h, k, j, 0)) for j in range(2)]
        keep.append(ring)
        video.graph_set_video_source_ring(g, s, ring, dur=(1, 60), off=(0, 1))
    ports16 = [(s, 0) for s in srcs] + [(prog, 0)] + [(s, 0) for s in srcs[:7]]
    ports4 = [(prog, 0), (srcs[0], 0), (srcs[1], 0), (srcs[6], 0)]
    cases = {"none": None, "4x4_hop1": (ports16, grid(4, 1)), "4x4_hop2": (ports16, grid(4, 2)), "2x2_hop1": (ports4, grid(2, 1))}
    tick = 0
    for ticks, reps in ((1, 128), (64, 4)):
        res = {k: [] for k in cases}
        for _rnd in range(3):
            for name, setting in cases.items():
                if setting is None:
                    video.graph_set_multiview(g, [], None)
                else:
                    video.graph_set_multiview(g, *setting)
                for _ in range(2):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                t = time.perf_counter()
                for _ in range(reps):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                res[name].append((time.perf_counter() - t) * 1e6 / (reps * ticks))
                if setting is not None:
                    canvas, st = video.graph_multiview_output(g)
                    assert canvas is None or st.shown_mask == (1 << len(setting[0])) - 1, (name, st.shown_mask)   # (None: the last run recorded no tick)
        base = statistics.median(res["none"])
        for name in cases:
            m = statistics.median(res[name])
            print(f"graph multiview={name} ticks_per_run={ticks} us_per_tick={m:.1f} over_none={m - base:+.1f} rounds={' '.join(f'{x:.1f}' for x in res[name])}", flush=True)
    video.graph_set_multiview(g, [], None)
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
    frames = [keep[k % 6][0] for k in range(16)]                      # sixteen 1080p frames, six distinct
    for name, n in (("4x4", 4), ("2x2", 2)):
        prm = grid(n, 1)
        calls = [timed(lambda: video.multiview(frames[:n * n], prm), 64) for _ in range(3)]
        print(f"mx_video_multiview {name} of 1080p frames call (with its canvas' creation) us_per_call={statistics.median(calls):.1f} rounds={' '.join(f'{x:.1f}' for x in calls)}", flush=True)
    vw, vh = W // 4, H // 4

    def sixteen_places():
        for i in range(16):
            video.place(frames[i], video.PlaceParams(W, H, vw * (i % 4), vh * (i // 4), vw, vh))   # 4:1, 18 taps: the placer's LDS-tiled form

    calls = [timed(sixteen_places, 16) for _ in range(3)]
    print(f"16 x mx_video_place of 1080p frames into 480 x 270 insets (each with its canvas' creation; no compositing) us_per_16={statistics.median(calls):.1f} "
          f"rounds={' '.join(f'{x:.1f}' for x in calls)}", flush=True)
    print(f"multiview bytes written per canvas = {FRAME_BYTES} (Y, U, V); 16 placed canvases = {16 * 5 * W * H // 2}: the kernels' own times are in the kernel trace", flush=True)
    print("multiview_cost done")


if __name__ == "__main__":
    main()
