"""The video scope record of include/mixlab_gpu.h (mx_graph_set_video_scopes) restated in numpy -- TEST INFRASTRUCTURE, written from the
header's text and independent of the kernel.  Planes are the VISIBLE samples: y (H, W), u and v (H >> 1, W >> 1), uint8."""
from __future__ import annotations

import numpy as np

WAVE_COLS = (0, 64, 128, 256)
PIXFMT_YUV420P, PIXFMT_YUVA420P = 0, 27


def record_bytes(wave_cols: int, vectorscope: bool) -> int:
    return 32 + 4 * (768 + 256 * wave_cols + (16384 if vectorscope else 0))


def counts(y, u, v, wave_cols: int, vectorscope: bool) -> dict:
    """hist [3, 256], wave [wave_cols, 256] or None, vec [128, 128] or None (uint32) of one counted frame"""
    y, u, v = (np.asarray(a, dtype=np.uint8) for a in (y, u, v))
    h, w = y.shape
    assert u.shape == v.shape == (h >> 1, w >> 1)
    hist = np.stack([np.bincount(a.ravel(), minlength=256) for a in (y, u, v)]).astype(np.uint32)
    wave = vec = None
    if wave_cols:
        bucket = (np.arange(w, dtype=np.int64) * wave_cols) // w            # floor(x * C / W), integer arithmetic
        wave = np.zeros((wave_cols, 256), np.uint32)
        np.add.at(wave, (np.broadcast_to(bucket, y.shape).ravel(), y.ravel()), 1)
    if vectorscope:
        vec = np.zeros((128, 128), np.uint32)
        np.add.at(vec, (v.ravel() >> 1, u.ravel() >> 1), 1)                  # vec[V >> 1][U >> 1]
    return {"hist": hist, "wave": wave, "vec": vec}


def record(frame, tick_in_run: int, wave_cols: int, vectorscope: bool) -> dict:
    """frame: None (the port held no frame), or (pixfmt, width, height, planes) with planes = (y, u, v) for yuv420p / yuva420p and
    anything else otherwise -> the record as mixlab_amd.abi.parse_video_scope_records presents it"""
    zero = {"hist": np.zeros((3, 256), np.uint32), "wave": np.zeros((wave_cols, 256), np.uint32) if wave_cols else None,
            "vec": np.zeros((128, 128), np.uint32) if vectorscope else None}
    r = {"present": 0, "counted": 0, "pixfmt": 0, "width": 0, "height": 0, "tick_in_run": tick_in_run, "reserved": (0, 0), **zero}
    if frame is None:
        return r
    pixfmt, w, h, planes = frame
    r.update(present=1, pixfmt=pixfmt, width=w, height=h)
    if pixfmt in (PIXFMT_YUV420P, PIXFMT_YUVA420P):
        r.update(counted=1, **counts(*planes, wave_cols, vectorscope))
    return r


def same(a: dict, b: dict) -> bool:
    for k in ("present", "counted", "pixfmt", "width", "height", "tick_in_run", "reserved"):
        if tuple(np.atleast_1d(a[k])) != tuple(np.atleast_1d(b[k])):
            return False
    for k in ("hist", "wave", "vec"):
        if (a[k] is None) != (b[k] is None) or (a[k] is not None and not np.array_equal(a[k], b[k])):
            return False
    return True


def first_difference(a: dict, b: dict) -> str:
    for k in ("present", "counted", "pixfmt", "width", "height", "tick_in_run", "reserved"):
        if tuple(np.atleast_1d(a[k])) != tuple(np.atleast_1d(b[k])):
            return f"{k}: {a[k]} != {b[k]}"
    for k in ("hist", "wave", "vec"):
        if (a[k] is None) != (b[k] is None):
            return f"{k}: present in one record only"
        if a[k] is not None and not np.array_equal(a[k], b[k]):
            i = tuple(int(x) for x in np.argwhere(a[k] != b[k])[0])
            return f"{k}{list(i)}: {a[k][i]} != {b[k][i]} ({int((a[k] != b[k]).sum())} counters differ)"
    return "equal"


# ---- test pictures with closed-form answers ----
def blank(w, h):
    return np.zeros((h, w), np.uint8), np.full((h >> 1, w >> 1), 0x80, np.uint8), np.full((h >> 1, w >> 1), 0x80, np.uint8)


def ramp(w, h):
    """a horizontal ramp: Y = floor(x * 256 / W), U = floor(x * 256 / pw), V = 255 - U"""
    y = np.broadcast_to(((np.arange(w) * 256) // w).astype(np.uint8), (h, w)).copy()
    pw = w >> 1
    u = np.broadcast_to(((np.arange(pw) * 256) // pw).astype(np.uint8), (h >> 1, pw)).copy()
    return y, u, (255 - u).astype(np.uint8)
