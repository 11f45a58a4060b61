"""numpy restatement of OutputDevice (reference src/module/output_device.rs) as MX_KIND_OUTPUT_DEVICE computes it: update (:152-169) and
run_tick (:174-246) with util::temporal_warning on the graph's sample clock.  Imports without a GPU.

`channels` stands for the open stream's config.channels (0: no stream, :95-150); left / right are None or a channel index."""
from __future__ import annotations

import numpy as np

NONE, RECENT, ACTIVE = 0, 1, 2   # mx_audio_out_tick.clip_status / lag_status (the encoding of mx_performance_info.lag)


def temporal_warning(now: int, last: int | None, rate: int) -> int:
    """util.rs temporal_warning on sample counts: Active below 100 ms, Recent below 5 s"""
    if last is None:
        return NONE
    d = now - last
    if d * 10 < rate:
        return ACTIVE
    if d < 5 * rate:
        return RECENT
    return NONE


class OutputDeviceModel:
    def __init__(self, rate: int, channels: int, left=None, right=None):
        self.rate = rate
        self.scratch = np.zeros(0, dtype=np.float32)   # scratch: Vec::new() (:75)
        self.channels = 0
        self.left = self.right = None
        self.last_clip = self.last_lag = None
        self.clip_status = self.lag_status = NONE       # indication.clip / lag: None (:65-70)
        self.lag_flag = False
        self.update(channels, left, right)              # creation = the adapter's first update from the empty state

    def update(self, channels: int, left=None, right=None):
        self.channels = channels
        if channels == 0:   # self.stream is None: nothing below runs (:152)
            return
        if self.left != left or self.right != right:   # STORED (filtered) against requested (:156)
            self.scratch[:] = 0.0
        self.left = left if left is not None and left < channels else None     # :163-164
        self.right = right if right is not None and right < channels else None  # :166-167

    def note_lag(self):
        self.lag_flag = True   # the cpal callback ran short (:126)

    def run_tick(self, t: int, stereo: np.ndarray):
        """one tick: (the floats pushed into the ring, (clip, clip_status, lag_status, changed, channels))"""
        stereo = np.asarray(stereo, dtype=np.float32)
        F = stereo.size // 2
        clip = False
        pushed = np.zeros(0, dtype=np.float32)
        C = self.channels
        if C:
            if self.scratch.size < F * C:   # resize, zero-filled (:184-186)
                self.scratch = np.concatenate([self.scratch, np.zeros(F * C - self.scratch.size, dtype=np.float32)])
            L, R = stereo[0::2], stereo[1::2]
            if self.left is not None:    # :189-197
                clip |= bool(np.any((L < -1.0) | (L > 1.0)))
                self.scratch[self.left:F * C:C] = L
            if self.right is not None:   # :199-208: right wins when left == right
                clip |= bool(np.any((R < -1.0) | (R > 1.0)))
                self.scratch[self.right:F * C:C] = R
            pushed = self.scratch[:F * C].copy()   # push_slice (:210)
        now = t
        if clip:
            self.last_clip = now          # :215-217
        if self.lag_flag:
            self.lag_flag = False         # swap(false) (:219-221)
            self.last_lag = now
        cs = temporal_warning(now, self.last_clip, self.rate)
        ls = temporal_warning(now, self.last_lag, self.rate)
        changed = cs != self.clip_status or ls != self.lag_status   # :225-244
        self.clip_status, self.lag_status = cs, ls
        return pushed, (int(clip), cs, ls, int(changed), C)

    def run(self, t0: int, spt: int, stereo_ticks):
        """consecutive ticks t0, t0 + spt, ...: (concatenated pushes, list of records)"""
        out, recs = [], []
        for k, x in enumerate(stereo_ticks):
            p, r = self.run_tick(t0 + k * spt, x)
            out.append(p)
            recs.append(r)
        return (np.concatenate(out) if out else np.zeros(0, np.float32)), recs
