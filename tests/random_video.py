"""Random video graphs: a scenario generator and the composed model of what the device must show -- TEST INFRASTRUCTURE, the picture half's counterpart of
tests/random_taps.py.  `scenario(seed)` draws a plain description (topology, frames, feeders, transforms, mixer parameters, scope taps, multiview, all per ABSOLUTE
tick, so it is the same however the ticks are grouped into runs); `groupings` cuts it into runs; `expect` composes the independent models per tick -- the oracle's
VideoMixer, the keyer's, placer's, scope's and multiviewer's numpy models, the oracle's scaler and RGBA conversion -- and returns what every run must leave behind.

The host logic here is written from the text of include/mixlab_gpu.h (the run_ticks video section, the mx_graph_set_video_source* comments, the scope and multiview
blocks), not from the engine.  `FAULTS` are the ways the engine could be wrong: each is a switch in this model, and tests/test_cpu_random_video.py proves that each
changes what is compared on named seeds.  Nothing here touches a device."""
from __future__ import annotations

import hashlib
import json
from fractions import Fraction

import numpy as np

import oracle_video as ov
import video_key_model as km
import video_multiview_model as mm
import video_place_model as pm
import video_scope_model as sm

SIZES = ((2, 2), (34, 18), (66, 38), (130, 74), (160, 90), (212, 120), (322, 182))
HOPS = (1, 2, 3, 7, 40)                    # 40 is longer than any run
MAX_RUN = 6
MATRIX = [3900, 150, 46, 4096, 60, 3980, 56, -2048, 20, 120, 3956, 0]   # the bench matrix (test_gpu_video_graph.MATRIX)
MONITOR_SIZES = ((80, 46), (48, 30), (100, 40))                          # none is a frame size: the Monitor's scaler always rescales
OFFSETS = ((0, 1), (1, 120), (-1, 120))
FEEDERS = ("ring", "repeat", "queue", "queue_over_ring", "shot")
TRANSFORMS = ("none", "key", "place", "key_place", "place_key", "band")
FAULTS = ("scope_c_per_run", "mv_uses_scope_counter", "set_does_not_reset_c", "mv_first_recorded_tick", "place_before_key", "stale_after_reset",
          "removed_transform_stays", "tap_sees_raw_source", "ab_ignore_update", "ring_restarts_per_run", "ring_beats_queue", "no_expiry", "mv_honours_coverage",
          "sink_shows_previous_tick")
PIXFMT_YUVA420P = 27


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the scenario: plain data
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def _pick(rng, seq):
    return seq[int(rng.integers(len(seq)))]


def _even(rng, lo, hi):
    """an even number in [lo, hi] (lo, hi even)"""
    return int(lo + 2 * rng.integers((hi - lo) // 2 + 1))


def _key_params(rng):
    """the model's defaults, perturbed"""
    if rng.random() < 0.7:
        near = int(rng.integers(0, 16 * 16))
        far = near + int(rng.integers(0, 48 * 16))
        spill = int(rng.integers(0, 256)) if rng.random() < 0.7 else 0
        return dict(mode=km.KEY_CHROMA, key_u=km.GREEN[0] + int(rng.integers(-3, 4)), key_v=km.GREEN[1] + int(rng.integers(-3, 4)), invert=int(rng.random() < 0.25),
                    near_q4=near, far_q4=far, spill_far_q4=far + int(rng.integers(0, 60 * 16)), spill_strength=spill)
    near = int(rng.integers(0, 120 * 16))
    return dict(mode=km.KEY_LUMA, key_u=0, key_v=0, invert=int(rng.random() < 0.25), near_q4=near, far_q4=near + int(rng.integers(0, 120 * 16)), spill_far_q4=0, spill_strength=0)


def _place_params(rng, min_w, min_h, whole):
    """a canvas of the list, a rectangle that may hang off it, a crop inside the source's smallest frame (whole: the whole-frame crop)"""
    cw, ch = _pick(rng, SIZES[1:])
    dw, dh = _even(rng, 12, cw + 20), _even(rng, 8, ch + 12)
    if rng.random() < 0.5:     # partly off the canvas
        dx, dy = _even(rng, -dw + 2, cw - 2), _even(rng, -dh + 2, ch - 2)
    else:
        dx, dy = _even(rng, 0, max(0, (cw - dw) & ~1)) if dw <= cw else -2, _even(rng, 0, max(0, (ch - dh) & ~1)) if dh <= ch else -2
    crop = (0, 0, 0, 0)
    if not whole and min_w >= 4 and min_h >= 4 and rng.random() < 0.6:
        w, h = _even(rng, 2, min_w), _even(rng, 2, min_h)
        crop = (_even(rng, 0, min_w - w), _even(rng, 0, min_h - h), w, h)
    return dict(canvas_w=cw, canvas_h=ch, dst_x=dx, dst_y=dy, dst_w=dw, dst_h=dh, crop_x=crop[0], crop_y=crop[1], crop_w=crop[2], crop_h=crop[3])


def _band_params(rng, w, h):
    fw, fh = _pick(rng, [s for s in SIZES[2:] if s != (w, h)])
    rows = _even(rng, 2, fh)
    return dict(in_w=w, in_full_h=h, src_row0=0, slice_rows=h, full_w=fw, full_h=fh, row0=_even(rng, 0, fh - rows), band_rows=rows)


def _multiview(rng, ports, n_views):
    cw, ch = _pick(rng, SIZES)
    if (cw, ch) == (2, 2):
        n_views = 1
    n = n_views
    cols = int(np.ceil(np.sqrt(n)))
    rows = (n + cols - 1) // cols
    vw, vh = (cw // cols) & ~1, (ch // rows) & ~1
    views = []
    for i in range(n):
        border = 2 if (rng.random() < 0.6 and vw >= 6 and vh >= 6) else 0
        w, h = (vw, vh) if rng.random() < 0.6 or vw < 12 or vh < 12 else (_even(rng, 2 * border + 2, vw), _even(rng, 2 * border + 2, vh))
        views.append(dict(x=vw * (i % cols), y=vh * (i // cols), w=w, h=h, border=border, colour=list(_pick(rng, (mm.RED, mm.GREEN, mm.WHITE))), fit=int(rng.integers(2))))
    return dict(ports=[list(_pick(rng, ports)) for _ in range(n)], canvas_w=cw, canvas_h=ch, views=views, bg=[int(x) for x in rng.integers(0, 256, 3)], hop=int(_pick(rng, HOPS)))


def _scopes(rng, ports):
    n = int(rng.integers(1, min(6, len(ports)) + 1))
    idx = rng.permutation(len(ports))[:n]
    return dict(ports=[list(ports[int(i)]) for i in idx], wave_cols=int(_pick(rng, (0, 64, 256))), vectorscope=int(rng.integers(2)), hop=int(_pick(rng, HOPS)))


def scenario(seed: int) -> dict:
    """The description of one random video graph and everything that happens to it, as plain data (ints, lists, dicts, None).  Node ids: the sources, then the
    mixers, then the RGBA sinks, then the Monitor.  `events[tick]` (tick relative to first_tick) is applied, in list order, at the run boundary before that tick;
    `mixer_updates[tick]` are VideoMixer parameter updates at the boundary before that tick, inside a run or not."""
    rng = np.random.default_rng(9000 + seed)
    rate = int(_pick(rng, (44100, 48000)))
    spt = rate // 60
    n_ticks = int(rng.integers(24, 37))
    first_tick = (2 ** 33 // spt) if seed % 4 == 3 else 0
    n_src, n_mix = int(rng.integers(2, 6)), int(rng.integers(1, 5))
    nv12_source = n_src - 1 if (n_src >= 3 and rng.random() < 0.5) else None          # feeds only taps
    # boundaries: the only ticks at which a setting changes.  b1, b1 + 1: a one-tick run with a re-set directly after it
    inner = sorted(int(x) for x in rng.permutation(np.arange(1, n_ticks - 1))[:int(rng.integers(4, 8))])
    b1 = int(rng.integers(1, n_ticks - 2))
    bounds = sorted(set([0, b1, b1 + 1] + inner))
    later = [b for b in bounds if b > 0]
    events = {b: [] for b in bounds}
    frames, sources = [], []

    def new_frame(w, h, fmt=0, alpha=False, kind="noise"):
        frames.append(dict(id=len(frames), w=w, h=h, fmt=fmt, alpha=bool(alpha), kind=kind))
        return len(frames) - 1

    def timing():
        return [int(rng.integers(1, 4)), 60], list(_pick(rng, OFFSETS))

    def frames_of(s):
        """the frames source s ever delivers"""
        ids = []
        for evs in events.values():
            for e in evs:
                if e.get("src") == s:
                    ids += [e["frame"]] if "frame" in e else list(e.get("frames", ())) + [q["frame"] for q in e.get("entries", ())]
        return [frames[i] for i in ids]

    for s in range(n_src):
        if s == nv12_source:
            w, h = _pick(rng, SIZES[1:4])
            f = new_frame(w, h, fmt=3, kind="fill")
            dur, off = timing()
            events[0].append(dict(op="repeat", src=s, frame=f, dur=dur, off=off))
            sources.append(dict(feeder="repeat", transform="none", nv12=True))
            continue
        # a third of the seeds pin a ring on the first source, another third a repeated frame on the second; the rest is drawn (rings and repeated frames twice as likely)
        feeder = FEEDERS[s] if (s < 2 and seed % 3 == s) else str(_pick(rng, FEEDERS + ("ring", "repeat")))
        transform = str(_pick(rng, TRANSFORMS + ("none",)))
        two_sizes = transform in ("place", "key_place", "place_key") and feeder in ("ring", "queue_over_ring") and rng.random() < 0.5
        size_a, size_b = _pick(rng, SIZES), _pick(rng, SIZES[1:4])
        if transform == "band":
            size_a = _pick(rng, SIZES[1:])

        def draw_frame():
            w, h = size_a if not two_sizes or rng.random() < 0.5 else size_b
            if transform == "none":
                fmt = int(_pick(rng, (0, 0, 0, 1, 2)))
                return new_frame(w, h, fmt, alpha=fmt == 0 and rng.random() < 0.4, kind="noise" if fmt == 0 else "fill")
            if transform == "band":
                return new_frame(w, h)
            return new_frame(w, h, 0, alpha=rng.random() < 0.4, kind="green" if "key" in transform else "noise")

        def ring():
            ids = [draw_frame() for _ in range(int(rng.integers(2, 6)))]
            if two_sizes:      # both sizes are there, next to each other
                frames[ids[0]].update(w=size_a[0], h=size_a[1]); frames[ids[1]].update(w=size_b[0], h=size_b[1])
            return ids

        if feeder in ("ring", "queue_over_ring"):
            dur, off = timing()
            events[0].append(dict(op="ring", src=s, frames=ring(), dur=dur, off=off))
            if feeder == "ring" and rng.random() < 0.3:
                dur, off = timing()
                events[_pick(rng, later)].append(dict(op="ring", src=s, frames=ring(), dur=dur, off=off))
            if feeder == "queue_over_ring":
                b = int(_pick(rng, later[:max(1, len(later) - 1)]))
                entries = []
                for k in range(b, min(n_ticks, b + int(rng.integers(4, 11)))):
                    if rng.random() < 0.6:
                        dur, off = timing()
                        entries.append(dict(tick=k, frame=draw_frame(), dur=dur, off=off))
                events[b].append(dict(op="queue", src=s, entries=entries))
        elif feeder == "repeat":
            dur, off = timing()
            events[0].append(dict(op="repeat", src=s, frame=draw_frame(), dur=dur, off=off))
            if rng.random() < 0.4:
                dur, off = timing()
                events[_pick(rng, later)].append(dict(op="repeat", src=s, frame=draw_frame(), dur=dur, off=off))
        elif feeder == "queue":
            entries = []
            for k in range(n_ticks):
                if rng.random() < 0.55:
                    dur, off = timing()
                    entries.append(dict(tick=k, frame=draw_frame(), dur=dur, off=off))
            events[0].append(dict(op="queue", src=s, entries=entries))
        else:
            for b in sorted(set([0] + [int(x) for x in rng.permutation(later)[:int(rng.integers(2, 6))]])):
                dur, off = timing()
                events[b].append(dict(op="shot", src=s, frame=draw_frame(), dur=dur, off=off))
        sources.append(dict(feeder=feeder, transform=transform, nv12=False, two_sizes=bool(two_sizes)))
        # the transform: set at tick 0, then set again with other parameters, removed, or put back at drawn boundaries
        min_w, min_h = min(f["w"] for f in frames_of(s)), min(f["h"] for f in frames_of(s))
        if transform == "none":
            continue
        if transform == "band":
            events[0].append(dict(op="band", src=s, params=_band_params(rng, *size_a)))
            on = True
            for b in sorted(int(x) for x in rng.permutation(later)[:int(rng.integers(0, 3))]):
                events[b].append(dict(op="band", src=s, params=_band_params(rng, *size_a) if (not on or rng.random() < 0.6) else None))
                on = events[b][-1]["params"] is not None
            continue
        steps = {"key": ["key"], "place": ["place"], "key_place": ["key", "place"], "place_key": ["place", "key"]}[transform]
        state = {}
        for op in steps:
            state[op] = _key_params(rng) if op == "key" else _place_params(rng, min_w, min_h, two_sizes)
            events[0].append(dict(op=op, src=s, params=state[op]))
        for b in sorted(int(x) for x in rng.permutation(later)[:int(rng.integers(1, 4))]):
            op = str(_pick(rng, steps))
            if state[op] is None or rng.random() < 0.65:
                state[op] = _key_params(rng) if op == "key" else _place_params(rng, min_w, min_h, two_sizes)
            else:
                state[op] = None
            events[b].append(dict(op=op, src=s, params=state[op]))
    # the re-set directly after the one-tick run: a transform with other parameters where there is one, else the scope taps (below)
    reset_src = next((s for s, d in enumerate(sources) if d["transform"] in ("key", "place", "key_place", "place_key")), None)
    if reset_src is not None:
        op = "key" if "key" in sources[reset_src]["transform"] else "place"
        mine = frames_of(reset_src)
        events[b1 + 1].append(dict(op=op, src=reset_src, params=_key_params(rng) if op == "key" else
                                   _place_params(rng, min(f["w"] for f in mine), min(f["h"] for f in mine), sources[reset_src].get("two_sizes", False))))
    # mixers: each input unconnected, or wired to a source port or to the program / A / B port of an earlier mixer
    wired_sources = [s for s in range(n_src) if s != nv12_source]
    mixers, mixer_updates = [], {}
    for k in range(n_mix):
        node = n_src + k
        outs = [(s, 0) for s in wired_sources] + [(n_src + j, p) for j in range(k) for p in (0, 0, 1, 2)]
        inputs = [None if rng.random() < 0.25 else list(_pick(rng, outs)) for _ in range(4)]
        if inputs[0] is None and inputs[1] is None:
            inputs[int(rng.integers(2))] = list(_pick(rng, outs))
        used = [i for i in range(4) if inputs[i] is not None]

        def params():
            sel = lambda: int(_pick(rng, used)) if rng.random() < 0.8 else int(rng.integers(-1, 4))
            return dict(a=sel(), b=sel(), fader=float(_pick(rng, (0.0, 1.0, 0.5, 0.25, 0.75, round(float(rng.random()), 3)))))
        mixers.append(dict(node=node, inputs=inputs, params=params()))
        for t in sorted(int(x) for x in rng.permutation(np.arange(1, n_ticks))[:int(rng.integers(0, 4))]):
            mixer_updates.setdefault(t, []).append(dict(node=node, params=params()))
    sinks = [dict(node=n_src + n_mix + i, mixer=int(rng.integers(n_mix)), matrix=bool(rng.integers(2))) for i in range(int(rng.integers(0, 3)))]
    monitor = None
    if rng.random() < 0.5:
        w, h = _pick(rng, MONITOR_SIZES)
        monitor = dict(node=n_src + n_mix + len(sinks), mixer=int(rng.integers(n_mix)), width=w, height=h)
    # taps: on any video output port
    ports = [(s, 0) for s in range(n_src)] + [(n_src + k, p) for k in range(n_mix) for p in range(3)]
    if nv12_source is not None:
        sc_ = _scopes(rng, ports)
        if [nv12_source, 0] not in sc_["ports"]:
            sc_["ports"][0] = [nv12_source, 0]
        events[0].append(dict(op="scopes", **sc_))
    elif rng.random() < 0.85:
        events[0 if rng.random() < 0.7 else later[0]].append(dict(op="scopes", **_scopes(rng, ports)))
    for b in sorted(int(x) for x in rng.permutation(later)[:int(rng.integers(0, 3))]):
        events[b].append(dict(op="scopes", **(_scopes(rng, ports) if rng.random() < 0.7 else dict(ports=[], wave_cols=0, vectorscope=0, hop=1))))
    if reset_src is None:
        events[b1 + 1].append(dict(op="scopes", **_scopes(rng, ports)))
    if rng.random() < 0.9 or nv12_source is not None:
        mv = _multiview(rng, ports, int(rng.integers(1, 7)))
        if nv12_source is not None:
            mv["ports"][-1] = [nv12_source, 0]
        events[0 if rng.random() < 0.7 else later[0]].append(dict(op="multiview", **mv))
    for b in sorted(int(x) for x in rng.permutation(later)[:int(rng.integers(0, 3))]):
        events[b].append(dict(op="multiview", **(_multiview(rng, ports, int(rng.integers(1, 7))) if rng.random() < 0.7 else dict(ports=[]))))
    return dict(seed=seed, rate=rate, spt=spt, first_tick=first_tick, n_ticks=n_ticks, n_sources=n_src, sources=sources, frames=frames, mixers=mixers,
                mixer_updates={int(k): v for k, v in sorted(mixer_updates.items())}, sinks=sinks, monitor=monitor,
                events={int(k): v for k, v in sorted(events.items())}, boundaries=bounds, one_tick_run=b1)


def digest(scenarios) -> str:
    """one number for what was drawn: the CPU and the GPU file pin it, so they draw the same things"""
    return hashlib.sha256(json.dumps([{k: v for k, v in sc.items() if not k.startswith("_")} for sc in scenarios], sort_keys=True).encode()).hexdigest()


def video_ports(sc):
    n = sc["n_sources"]
    return [(s, 0) for s in range(n)] + [(m["node"], p) for m in sc["mixers"] for p in range(3)]


def groupings(sc, kind: str):
    """[(first tick relative to first_tick, ticks)]: every setting boundary is a run boundary; between them "batched" cuts random runs of 1 .. 6 ticks, "single" runs
    every tick on its own"""
    rng = np.random.default_rng(7000 + sc["seed"])
    edges = list(sc["boundaries"]) + [sc["n_ticks"]]
    runs = []
    for lo, hi in zip(edges, edges[1:]):
        t = lo
        while t < hi:
            n = 1 if kind == "single" else int(min(rng.integers(1, MAX_RUN + 1), hi - t))
            runs.append((t, n)); t += n
    assert kind in ("single", "batched") and sum(n for _, n in runs) == sc["n_ticks"]
    return runs


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# pictures
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
class Pic:
    """A frame on a port: fmt (mx_pixfmt of the layout: 0 yuv420p, 1 yuv422p, 2 yuv444p, 3 nv12), size, the visible planes and the coverage plane or None"""

    def __init__(self, fmt, w, h, planes, a=None, uid=None, host=None):
        self.fmt, self.w, self.h, self.planes, self.a, self.uid, self._host, self._src = fmt, w, h, list(planes), a, uid, host, None

    @property
    def pixfmt(self):
        return PIXFMT_YUVA420P if (self.fmt == 0 and self.a is not None) else self.fmt

    def host(self):
        if self._host is None:
            hf = ov.HostFrame(self.w, self.h, self.fmt)
            for dst, src in zip(hf.visible(), self.planes):
                dst[:] = src
            if self.a is not None:
                hf.set_alpha(self.a)
            self._host = hf
        return self._host

    def src(self):
        """as the multiviewer's model meets it"""
        if self._src is None:
            self._src = mm.Src(self.w, self.h, *self.planes, self.a) if self.fmt == 0 else mm.Src(self.w, self.h, fmt="other")
        return self._src

    def same(self, o):
        return (o is not None and (self.fmt, self.w, self.h, self.a is None) == (o.fmt, o.w, o.h, o.a is None) and all(np.array_equal(x, y) for x, y in zip(self.planes, o.planes))
                and (self.a is None or np.array_equal(self.a, o.a)))


def source_frame(sc, fid) -> Pic:
    """the picture of frame `fid` of the scenario (made once)"""
    cache = sc.setdefault("_frames", {})
    if fid not in cache:
        f = sc["frames"][fid]
        w, h, fmt = f["w"], f["h"], f["fmt"]
        rng = np.random.default_rng([9000 + sc["seed"], fid])
        if f["kind"] == "green":
            planes = list(km.green_screen(w, h, seed=fid))
        elif f["kind"] == "fill":
            planes = [p.copy() for p in ov.HostFrame(w, h, fmt).fill(fid, seed=sc["seed"]).visible()]
        else:
            planes = [rng.integers(0, 256, size=(h, w)).astype(np.uint8), rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8), rng.integers(0, 256, size=(h // 2, w // 2)).astype(np.uint8)]
        a = None
        if f["alpha"]:
            a = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
            a[rng.random((h, w)) < 0.3] = 255
        cache[fid] = Pic(fmt, w, h, planes, a, uid=("f", fid))
    return cache[fid]


def _freeze(d):
    return None if d is None else tuple(sorted(d.items()))


def transformed(sc, pic: Pic, key, place, band, place_first=False) -> Pic:
    """what a SOURCE_VIDEO node delivers for `pic` under its settings: KEY, THEN PLACE, whichever call came first (place_first: the wrong order); a row band
    otherwise.  Made once per frame identity and setting."""
    if key is None and place is None and band is None:
        return pic
    cache = sc.setdefault("_transformed", {})
    uid = ("t", pic.uid, _freeze(key), _freeze(place), _freeze(band), place_first)
    if uid not in cache:
        if band is not None:
            full = ov.HostFrame(band["full_w"], band["full_h"])
            ov.dynamic_scale(pic.host(), full)
            r0, n = band["row0"], band["band_rows"]
            y, u, v = full.visible()
            out = Pic(0, band["full_w"], n, [y[r0:r0 + n].copy(), u[r0 >> 1:(r0 + n) >> 1].copy(), v[r0 >> 1:(r0 + n) >> 1].copy()], None, uid)
        else:
            y, u, v = pic.planes
            a = pic.a
            steps = [("key", key), ("place", place)]
            for op, par in (steps[::-1] if place_first else steps):
                if par is None:
                    continue
                if op == "key":
                    y, u, v, a = km.key_model(y, u, v, km.KeyP(**par), a)
                else:
                    y, u, v, a = pm.place_model(y, u, v, pm.PlaceP(**par), a)
            out = Pic(0, y.shape[1], y.shape[0], [y, u, v], a, uid)
        cache[uid] = out
    return cache[uid]


def _monitor_picture(sc, pic: Pic, w, h):
    cache = sc.setdefault("_monitor", {})
    k = (id(pic), w, h)
    if k not in cache:
        out = ov.HostFrame(w, h)
        ov.dynamic_scale(pic.host(), out)
        cache[k] = (pic, [p.copy() for p in out.visible()])      # the picture is kept: its id stays its own
    return cache[k][1]


def _scope_record(sc, pic, tick_in_run, wave_cols, vectorscope):
    if pic is None:
        return sm.record(None, tick_in_run, wave_cols, vectorscope)
    cache = sc.setdefault("_scoped", {})
    k = (id(pic), wave_cols, vectorscope)
    if k not in cache:
        cache[k] = (pic, sm.record((pic.pixfmt, pic.w, pic.h, pic.planes), 0, wave_cols, vectorscope))
    r = dict(cache[k][1])
    r["tick_in_run"] = tick_in_run
    return r


def mv_params(mv) -> mm.MvP:
    return mm.MvP(mv["canvas_w"], mv["canvas_h"], tuple(mm.View(v["x"], v["y"], v["w"], v["h"], v["border"], tuple(v["colour"]), v["fit"]) for v in mv["views"]), tuple(mv["bg"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# the composed model
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def expect(sc, grouping, fault=None):
    """What the device must show at the end of every run of `grouping` (groupings(sc, kind)): one dict per run --
         ports    {(node, port): Pic or None} of every video output port after the run's last tick
         sinks    {node: RGBA array or None}
         monitor  [(ts, None) or (ts, frame_ts, dur, [Y, U, V])] per tick of the run, exact Fractions (None: no Monitor)
         scopes   None (no taps set) or dict(wave_cols, vectorscope, records [recorded tick][tap])
         mv       None (no setting) or dict(status (recorded, tick_in_run, present_mask, shown_mask), canvas [Y, U, V] or None, params)
         info     what the coverage assertions of the CPU suite count
    `fault`: one of FAULTS switched into the model."""
    assert fault is None or fault in FAULTS
    n_src, rate, spt, tick0 = sc["n_sources"], sc["rate"], sc["spt"], sc["first_tick"]
    src = [dict(ring=[], pos=0, queue=[], frame=None, repeat=False, pending=False, dur=None, off=None, key=None, place=None, band=None, stale={}) for _ in range(n_src)]
    mixers = [dict(m, om=ov.OracleVideoMixer(None if m["params"]["a"] < 0 else m["params"]["a"], None if m["params"]["b"] < 0 else m["params"]["b"], m["params"]["fader"], rate),
                   now=dict(m["params"])) for m in sc["mixers"]]
    by_node = {m["node"]: m for m in mixers}
    scopes, scope_c, mv, mv_c = None, 0, None, 0
    mon_epoch = None
    out = []
    assert set(sc["events"]) <= {start for start, _ in grouping}, "every setting boundary is a run boundary"
    for start, n in grouping:
        for e in sc["events"].get(start, []):
            op = e["op"]
            if op in ("ring", "repeat", "shot", "queue", "key", "place", "band"):
                s = src[e["src"]]
            if op == "ring":                       # clears a set frame; the ring starts at its first frame
                s.update(ring=list(e["frames"]), pos=0, frame=None, repeat=False, pending=False, dur=tuple(e["dur"]), off=tuple(e["off"]))
            elif op in ("repeat", "shot"):
                s.update(frame=e["frame"], repeat=op == "repeat", pending=True, dur=tuple(e["dur"]), off=tuple(e["off"]))
            elif op == "queue":
                s["queue"] = s["queue"] + [(q["tick"], q["frame"], tuple(q["dur"]), tuple(q["off"])) for q in e["entries"]]
            elif op in ("key", "place", "band"):
                if e["params"] is None and fault == "removed_transform_stays":
                    continue
                if e["params"] is None or s[op] is None or fault != "stale_after_reset":
                    s["stale"] = {}                # the right model forgets here; the stale one only when the transform goes or comes
                s[op] = e["params"]
            elif op == "scopes":
                scopes = dict(e) if e["ports"] else None
                if fault != "set_does_not_reset_c":
                    scope_c = 0
            elif op == "multiview":
                mv = dict(e, params=mv_params(e)) if e["ports"] else None
                if fault != "set_does_not_reset_c":
                    mv_c = 0
        if fault == "scope_c_per_run":
            scope_c = 0
        if fault == "ring_restarts_per_run":
            for s in src:
                s["pos"] = 0
        records, mon_ticks, mv_recorded, sink_hist = [], [], [], []
        info = dict(scope_symbolic=0, scope_none=0, scope_nv12=0, mv_symbolic=0, mv_nv12=0, sink_size_change=0)
        ports = {}
        for k in range(n):
            rel = start + k
            tick = tick0 + rel
            for u in sc["mixer_updates"].get(rel, []):
                m = by_node[u["node"]]
                m["now"] = dict(u["params"])
                m["om"].update(None if u["params"]["a"] < 0 else u["params"]["a"], None if u["params"]["b"] < 0 else u["params"]["b"], u["params"]["fader"])
            ports, raw = {}, {}
            for i, s in enumerate(src):
                v = None
                s["queue"] = [q for q in s["queue"] if q[0] >= rel]               # entries of ticks that were never run
                if s["queue"] and not (fault == "ring_beats_queue" and s["ring"]):  # while any is queued they take the place of the set frame and the ring
                    if s["queue"][0][0] == rel:
                        _, f, dur, off = s["queue"].pop(0)
                        v = (f, dur, off)
                elif s["ring"]:
                    v = (s["ring"][s["pos"]], s["dur"], s["off"])
                    s["pos"] = (s["pos"] + 1) % len(s["ring"])
                elif s["frame"] is not None and (s["repeat"] or s["pending"]):
                    v = (s["frame"], s["dur"], s["off"])
                    s["pending"] = False
                raw[(i, 0)] = ports[(i, 0)] = None
                if v is not None:
                    pic = source_frame(sc, v[0])
                    raw[(i, 0)] = (pic, v[1], v[2])
                    if fault == "stale_after_reset" and (s["key"] or s["place"] or s["band"]):
                        if v[0] not in s["stale"]:
                            s["stale"][v[0]] = transformed(sc, pic, s["key"], s["place"], s["band"])
                        t = s["stale"][v[0]]
                    else:
                        t = transformed(sc, pic, s["key"], s["place"], s["band"], place_first=fault == "place_before_key")
                    ports[(i, 0)] = (t, v[1], v[2])
            for m in mixers:
                ins = []
                for ref in m["inputs"]:
                    v = None if ref is None else ports[tuple(ref)]
                    ins.append(v)
                forever = (10 ** 6, 1)
                res = m["om"].run_tick(tick * spt, [None if v is None else (v[0].host(), forever if fault == "no_expiry" else v[1], v[2]) for v in ins])
                node = m["node"]
                ports[(node, 0)] = None if res is None else (Pic(0, res.w, res.h, res.visible(), None, ("m", node, tick), host=res), (1, 60), (0, 1))
                sel = m["params"] if fault == "ab_ignore_update" else m["now"]
                for p, which in ((1, sel["a"]), (2, sel["b"])):
                    ports[(node, p)] = ins[which] if 0 <= which < 4 else None
            if sc["monitor"] is not None:
                mo = sc["monitor"]
                now = Fraction(tick * spt, rate)
                if mon_epoch is None:
                    mon_epoch = now
                v = ports[(mo["mixer"] + n_src, 0)]
                ts = now - mon_epoch
                mon_ticks.append((ts, None) if v is None else (ts, ts + Fraction(*v[2]), Fraction(*v[1]), _monitor_picture(sc, v[0], mo["width"], mo["height"])))
            sink_hist.append({s["node"]: ports[(s["mixer"] + n_src, 0)] for s in sc["sinks"]})
            if scopes is not None:
                if scope_c % scopes["hop"] == 0:
                    row = []
                    for node, port in scopes["ports"]:
                        v = ports[(node, port)]
                        if fault == "tap_sees_raw_source" and node < n_src:
                            v = raw[(node, 0)]
                        row.append(_scope_record(sc, None if v is None else v[0], k, scopes["wave_cols"], bool(scopes["vectorscope"])))
                        info["scope_none"] += v is None
                        info["scope_nv12"] += v is not None and v[0].fmt == 3
                        info["scope_symbolic"] += v is not None and node >= n_src and port == 0
                    records.append(row)
            if mv is not None:
                c = scope_c if (fault == "mv_uses_scope_counter" and scopes is not None) else mv_c
                if c % mv["hop"] == 0:
                    shown = []
                    for node, port in mv["ports"]:
                        v = ports[(node, port)]
                        if fault == "tap_sees_raw_source" and node < n_src:
                            v = raw[(node, 0)]
                        shown.append(None if v is None else v[0])
                    tapped = set() if scopes is None or scope_c % scopes["hop"] else {tuple(p) for p in scopes["ports"]}
                    mv_recorded.append((k, shown, tapped))
                mv_c += 1
            if scopes is not None:
                scope_c += 1
        sinks = {}
        for s in sc["sinks"]:
            hist = [h[s["node"]] for h in sink_hist]
            v = hist[-2] if (fault == "sink_shows_previous_tick" and n >= 2) else hist[-1]
            sinks[s["node"]] = None if v is None else ov.to_rgba(v[0].host(), MATRIX if s["matrix"] else None)
            info["sink_size_change"] += any(a is not None and b is not None and (a[0].w, a[0].h) != (b[0].w, b[0].h) for a, b in zip(hist, hist[1:]))
        mv_out = None
        if mv is not None:
            mv_out = dict(status=(0, 0, 0, 0), canvas=None, params=mv["params"], n_recorded=len(mv_recorded))
            if mv_recorded:
                k, shown, tapped = mv_recorded[0 if fault == "mv_first_recorded_tick" else -1]
                frames = [None if p is None else p.src() for p in shown]
                mv_out["status"] = (len(mv_recorded), k, sum(1 << i for i, p in enumerate(shown) if p is not None), mm.shown_mask(frames, mv["params"]))
                mv_out["canvas"] = mm.multiview_model(frames, mv["params"], bug="coverage_applied" if fault == "mv_honours_coverage" else None)
                info["mv_nv12"] = sum(p is not None and p.fmt == 3 for p in shown)
                mon_port = None if sc["monitor"] is None else (sc["monitor"]["mixer"] + n_src, 0)
                # a program no earlier consumer of the tick asked pixels of: no scope tap, no Monitor
                info["mv_symbolic"] = sum(p is not None and node >= n_src and port == 0 and (node, port) not in tapped and (node, port) != mon_port
                                          and bool(mv_out["status"][3] >> i & 1) for i, ((node, port), p) in enumerate(zip(mv["ports"], shown)))
        out.append(dict(start=start, n=n, ports={p: (None if v is None else v[0]) for p, v in ports.items()}, sinks=sinks,
                        monitor=mon_ticks if sc["monitor"] is not None else None,
                        scopes=None if scopes is None else dict(wave_cols=scopes["wave_cols"], vectorscope=bool(scopes["vectorscope"]), records=records),
                        mv=mv_out, info=info))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
# comparing two sets of expectations (the faults, the groupings)
# ---------------------------------------------------------------------------------------------------------------------------------------------------------------
def same_pic(a, b):
    return (a is None and b is None) or (a is not None and a.same(b))


def same_planes(a, b):
    return (a is None and b is None) or (a is not None and b is not None and len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)))


def same_monitor_tick(a, b):
    if len(a) != len(b) or a[0] != b[0]:
        return False
    return len(a) == 2 or (a[1:3] == b[1:3] and same_planes(a[3], b[3]))


def run_differences(a, b):
    """names of the compared items in which two expectations of the same run differ"""
    out = []
    out += [f"port {p}" for p in a["ports"] if not same_pic(a["ports"][p], b["ports"][p])]
    out += [f"sink {s}" for s in a["sinks"] if not same_planes(None if a["sinks"][s] is None else [a["sinks"][s]], None if b["sinks"][s] is None else [b["sinks"][s]])]
    if a["monitor"] is not None:
        out += [f"monitor tick {k}" for k, (x, y) in enumerate(zip(a["monitor"], b["monitor"])) if not same_monitor_tick(x, y)]
    if (a["scopes"] is None) != (b["scopes"] is None):
        out.append("scopes set")
    elif a["scopes"] is not None:
        ra, rb = a["scopes"]["records"], b["scopes"]["records"]
        if len(ra) != len(rb):
            out.append(f"scope records: {len(ra)} / {len(rb)} ticks")
        out += [f"scope record {i}.{j}" for i, (x, y) in enumerate(zip(ra, rb)) for j, (p, q) in enumerate(zip(x, y)) if not sm.same(p, q)]
    if (a["mv"] is None) != (b["mv"] is None):
        out.append("multiview set")
    elif a["mv"] is not None:
        if a["mv"]["status"] != b["mv"]["status"]:
            out.append("multiview status")
        if not same_planes(a["mv"]["canvas"], b["mv"]["canvas"]):
            out.append("multiview canvas")
    return out


def differences(a, b):
    """[(run index, item)] over two expectations under the same grouping"""
    assert [(r["start"], r["n"]) for r in a] == [(r["start"], r["n"]) for r in b]
    return [(i, d) for i, (x, y) in enumerate(zip(a, b)) for d in run_differences(x, y)]
