#!/usr/bin/env python
"""Cost of video scope taps.

Part 1, the graph: the 8-layer 1080p config-4 cascade (7 VideoMixers into the RGBA sink) with no tap and with one tap on the composite
(wave_cols 256, vectorscope on) at hop 1 and hop 2, one-tick runs and 64-tick runs.  The cases alternate on the one graph
(mx_graph_set_video_scopes between them), three rounds each, median: a same-box A/B of the wall time per run.

Part 2, the kernel: mx_video_scope alone, 256 calls back to back on one stream, on a blank, a uniform-noise and a smooth-gradient 1080p
frame, for hist only / + waveform / + vectorscope / everything; beside it a device-to-device copy of the same 3.1 MB x 256 (what a
read-once kernel reaches at this size) and the record's clearing fill alone.  Prints us per frame, the fraction of 8 TB/s the frame's
bytes reach, the ratio to the copy and blank / noise.

Run it under `rocprofv3 --kernel-trace --stats -- python tools/scope_cost.py --kernel-only` for the kernel's own time (k_video_scope)."""
import ctypes as C
import pathlib
import statistics
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "tests"))
import synth  # noqa: E402
from benchlegs.common import VIDEO_SIZES, video_cascade  # noqa: E402
from mixlab_amd import abi, video  # noqa: E402
from mixlab_amd.workspace import Workspace  # noqa: E402

W, H, BATCH = 1920, 1080, 256
FRAME_BYTES = W * H * 3 // 2


def graph_part():
    ws = Workspace(44100, 60)
    srcs, rgba = video_cascade(ws)
    composite = rgba - 1                       # the last VideoMixer
    g = ws.build(max_ticks_per_run=64)
    keep = []
    for k, (s, (w, h)) in enumerate(zip(srcs, VIDEO_SIZES)):
        ring = [video.DFrame(w, h).upload(*synth.yuv_pattern(w, h, k, j, 0)) for j in range(2)]
        keep.append(ring)
        video.graph_set_video_source_ring(g, s, ring, dur=(1, 60), off=(0, 1))
    cases = {"none": None, "hop1": 1, "hop2": 2}
    tick = 0
    for ticks, reps in ((1, 100), (64, 4)):
        res = {k: [] for k in cases}
        for _rnd in range(3):
            for name, hop in cases.items():
                g.set_video_scopes([(composite, 0)] if hop else [], wave_cols=256, vectorscope=True, hop=hop or 1)
                for _ in range(2):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                t = time.perf_counter()
                for _ in range(reps):
                    g.run_ticks(tick, ticks); tick += ticks
                g.sync()
                res[name].append((time.perf_counter() - t) * 1e6 / reps)
                if hop:
                    recs = g.read_video_scopes()
                    assert all(int(r[0]["hist"][0].sum()) == W * H for r in recs)
        for name in cases:
            m = statistics.median(res[name])
            print(f"graph taps={name} ticks={ticks} us_per_run={m:.1f} us_per_tick={m / ticks:.1f} rounds={' '.join(f'{v:.1f}' for v in res[name])}", flush=True)
    g.close()


def kernel_part():
    yy, xx = np.mgrid[0:H, 0:W]
    cy, cx = np.mgrid[0:H // 2, 0:W // 2]
    rng = np.random.default_rng(4)
    pics = {"blank": None,
            "noise": tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))),
            "gradient": (((xx * 160 // W + yy * 96 // H)).astype(np.uint8), (cx * 256 // (W // 2)).astype(np.uint8), (cy * 256 // (H // 2)).astype(np.uint8))}
    frames = {}
    for name, p in pics.items():
        f = video.DFrame(W, H)
        frames[name] = f.upload(*p) if p is not None else f
    scopes = {"hist": (0, False), "hist+wave": (256, False), "hist+vec": (0, True), "all": (256, True)}
    rec = video.DeviceBuffer(abi.video_scope_record_bytes(256, True))
    src, dst = video.DeviceBuffer(FRAME_BYTES), video.DeviceBuffer(FRAME_BYTES)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    hip.hipMemsetAsync.argtypes = [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p]
    hip.hipDeviceSynchronize.argtypes = []

    def timed(fn):
        for _ in range(8):
            fn()
        hip.hipDeviceSynchronize(); video.sync()
        t = time.perf_counter()
        for _ in range(BATCH):
            fn()
        hip.hipDeviceSynchronize(); video.sync()
        return (time.perf_counter() - t) * 1e6 / BATCH

    res = {}
    for _rnd in range(3):
        res.setdefault("copy", []).append(timed(lambda: hip.hipMemcpyAsync(dst.ptr, src.ptr, FRAME_BYTES, 3, None)))
        for sname, (cols, vec) in scopes.items():
            nb = abi.video_scope_record_bytes(cols, vec)
            res.setdefault(("fill", sname), []).append(timed(lambda: hip.hipMemsetAsync(rec.ptr, 0, nb, None)))
            par = abi.VideoScopeParams(cols, 1 if vec else 0, 1)
            for pname, f in frames.items():
                res.setdefault((pname, sname), []).append(timed(lambda: abi.lib.mx_video_scope(f._h, C.byref(par), rec.ptr, None)))
    copy = statistics.median(res["copy"])
    print(f"kernel copy_d2d bytes={FRAME_BYTES} us_per_frame={copy:.2f} frac_of_8TBs={FRAME_BYTES / (copy * 1e-6) / 8e12:.4f}", flush=True)
    for sname in scopes:
        fill = statistics.median(res[("fill", sname)])
        t = {p: statistics.median(res[(p, sname)]) for p in frames}
        for p in frames:
            print(f"kernel scope={sname} frame={p} us_per_frame={t[p]:.2f} frac_of_8TBs={FRAME_BYTES / (t[p] * 1e-6) / 8e12:.4f} "
                  f"ratio_to_copy={t[p] / copy:.2f} rounds={' '.join(f'{v:.2f}' for v in res[(p, sname)])}", flush=True)
        print(f"kernel scope={sname} fill_alone_us={fill:.2f} blank_over_noise={t['blank'] / t['noise']:.2f}", flush=True)
    got = abi.parse_video_scope_records(rec.download(), 256, True)[0]
    assert int(got["hist"][0].sum()) == W * H and int(got["vec"].sum()) == W * H // 4


if __name__ == "__main__":
    if "--kernel-only" not in sys.argv:
        graph_part()
    kernel_part()
    print("scope_cost done")
