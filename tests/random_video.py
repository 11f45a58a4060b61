"""Random video graphs: a scenario generator and the composed model of what the device must show -- TEST INFRASTRUCTURE, the picture half's counterpart of
tests/random_taps.py.  `scenario(seed)` draws a plain description (topology, frames, feeders, transforms, mixer parameters, scope taps, multiview, all per ABSOLUTE
tick, so it is the same however the ticks are grouped into runs); `groupings` cuts it into runs; `expect` composes the independent models per tick -- the oracle's
VideoMixer, the colour corrector's, keyer's, matte refiner's, placer's, scope's and multiviewer's numpy models, the oracle's scaler and RGBA conversion -- and returns
what every run must leave behind.

Two families of scenarios.  `scenario(seed)` draws a source's transform from TRANSFORMS: none, key, place, key and place in either call order, or a row band.
`scenario(seed, chain=True)`, from an RNG base of its own, draws for every source that is neither NV12 nor banded a subset of STAGES -- grade, key, matte, place, or
none: the setters are called at tick 0 in a drawn permutation, at later boundaries a drawn stage is set again with other parameters (a matte now and then as a wipe
at a drawn position), removed or put back, and the re-set directly after the one-tick run falls on a stage that is not the last one on; a source with a grade or a
matte mixes yuv420p and yuva420p frames within its ring or queue, and its ring may alternate two sizes.  All parameters are plain data (a lattice is a seed of
video_grade_model.random_lattice or "smooth", a curve the arguments of gamma_curve), so the digest pins them.  The first family's draws do not depend on the second.

The host logic here is written from the text of include/mixlab_gpu.h (the run_ticks video section, the mx_graph_set_video_source* comments -- GRADE, THEN KEY, THEN
MATTE, THEN PLACE, whatever the call order -- the scope and multiview blocks), not from the engine.  `FAULTS` are the ways the engine could be wrong: each is a switch
in this model, and tests/test_cpu_random_video.py proves that each changes what is compared on named seeds.  `CHAIN_FAULTS` are those of the four-stage transform,
proved on the chain seeds by tests/test_cpu_random_video_chain.py together with the four older ones that meet the new ops (stale_after_reset, removed_transform_stays,
place_before_key, tap_sees_raw_source): matte_before_key (the matte refines the incoming coverage and the key then replaces it), grade_after_key (the key is decided
on the uncorrected colour), grade_drops_coverage (a graded yuva420p frame arrives without its coverage plane), matte_ignores_coverage (with no key set the matte
starts from opaque instead of the frame's own plane), old_lattice_after_reset (after a grade re-set that brings another LUT, the new curve and matrix run with the
old lattice).  Nothing here touches a device."""
from __future__ import annotations

import hashlib
import json
from fractions import Fraction

import numpy as np

import oracle_video as ov
import video_grade_model as gm
import video_key_model as km
import video_matte_model as mt
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
# the chain family (scenario(seed, chain=True)): the four stages of a source's transform in the order the header fixes, and the ways an engine could get THEM wrong
STAGES = ("grade", "key", "matte", "place")
CHAIN_FAULTS = ("matte_before_key", "grade_after_key", "grade_drops_coverage", "matte_ignores_coverage", "old_lattice_after_reset")
CHAIN_BASE = 19000                         # the chain family's RNG base (the first family's is 9000)
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


def _grade_params(rng):
    """plain data for mx_video_grade_params and its lattice: a non-empty flag set; the curve as gamma_curve's (gamma, black, white); the Q12 matrix and offsets inside
    the header's ranges (|m| <= 32767, |off| <= 255 * 4096), now and then AT them; the lattice as (k, a seed of random_lattice or "smooth")"""
    flags = int(rng.integers(1, 8))
    curve = [float(_pick(rng, (0.5, 0.8, 1.0, 1.25, 2.0))), int(rng.integers(0, 64)), int(rng.integers(160, 256))]
    m = [int(rng.integers(2000, 7001)), int(rng.integers(-2500, 2501)), int(rng.integers(-2500, 2501)), int(rng.integers(2000, 7001))]
    off = [int(rng.integers(-8 * 4096, 8 * 4096 + 1)), int(rng.integers(-8 * 4096, 8 * 4096 + 1))]
    if rng.random() < 0.15:
        m[int(rng.integers(4))] = int(_pick(rng, (-32767, 32767)))
    if rng.random() < 0.15:
        off[int(rng.integers(2))] = int(_pick(rng, (-255 * 4096, 255 * 4096)))
    k, lattice = 0, None
    if flags & gm.LUT:
        k = int(_pick(rng, (4, 5)))
        lattice = "smooth" if rng.random() < 0.4 else int(rng.integers(1, 1000))
    return dict(flags=flags, curve=curve, m=m, off=off, k=k, lattice=lattice)


def _matte_params(rng, w, h, wipe_ok):
    """plain data for mx_video_matte_params over a w x h frame: the stages drawn one by one (at least one on), the mask a rectangle or a circle in 1/16 pixel that may
    hang off the frame; where wipe_ok, now and then mx_video_matte_wipe's arguments instead: dict(wipe=[kind, pos, feather, w, h])"""
    if wipe_ok and rng.random() < 0.4:
        return dict(wipe=[int(rng.integers(4)), int(rng.integers(8192, 57345)), int(_pick(rng, (0, 24, 16 * 6 + 3))), w, h])
    on = [bool(rng.random() < 0.5) for _ in range(4)]
    if not any(on):
        on[int(rng.integers(4))] = True
    clean = None
    if on[0]:
        black = int(rng.integers(0, 129))
        clean = [black, black + int(rng.integers(0, 256 - black))]
    choke = int(_pick(rng, (-6, -3, -2, -1, 1, 2, 3, 6))) if on[1] else 0
    soften = int(_pick(rng, (1, 1, 2, 3, 6))) if on[2] else 0
    mask, shape, invert, feather = None, mt.RECT, 0, 0
    if on[3]:
        shape, invert = int(rng.integers(2)), int(rng.random() < 0.3)
        feather = int(_pick(rng, (0, 0, 9, 16 * 3 + 5, 16 * 8)))
        if shape == mt.RECT:
            x0, y0 = int(rng.integers(-4 * w, 12 * w + 1)), int(rng.integers(-4 * h, 12 * h + 1))
            mask = [x0, y0, x0 + int(rng.integers(0, 16 * w + 1)), y0 + int(rng.integers(0, 16 * h + 1))]
        else:
            mask = [int(rng.integers(-4 * w, 20 * w + 1)), int(rng.integers(-4 * h, 20 * h + 1)), int(rng.integers(0, 16 * max(w, h) + 1)), 0]
    return dict(clean=clean, choke=choke, soften=soften, mask=mask, shape=shape, invert=invert, feather=feather)


def _draw_stages(rng):
    """the transform of a chain source: None (a row band), or the stages that are set, in the chain's order -- () for none, else a non-empty subset of STAGES"""
    r = rng.random()
    if r < 0.1:
        return None
    if r < 0.2:
        return ()
    n = int(_pick(rng, (1, 1, 1, 2, 2, 2, 3, 3, 4, 4)))
    pick = sorted(int(i) for i in rng.permutation(4)[:n])
    return tuple(STAGES[i] for i in pick)


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


def scenario(seed: int, chain: bool = False) -> dict:
    """The description of one random video graph and everything that happens to it, as plain data (ints, lists, dicts, None).  Node ids: the sources, then the
    mixers, then the RGBA sinks, then the Monitor.  `events[tick]` (tick relative to first_tick) is applied, in list order, at the run boundary before that tick;
    `mixer_updates[tick]` are VideoMixer parameter updates at the boundary before that tick, inside a run or not.
    chain: the second family, with an RNG base of its own -- every source that is neither NV12 nor banded draws its transform as a subset of STAGES (ops "grade",
    "key", "matte", "place"; sources[s]["stages"] in the chain's order, ["order"] as the setters are called at tick 0), and a source with a grade or a matte mixes
    yuv420p and yuva420p frames.  What scenario(seed) draws does not depend on anything the chain family added."""
    rng = np.random.default_rng((CHAIN_BASE if chain else 9000) + seed)
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
        stages = ()
        if chain:
            stages = _draw_stages(rng)
            transform = "band" if stages is None else ("+".join(stages) or "none")
            stages = stages or ()
            two_sizes = bool(stages) and feeder in ("ring", "queue_over_ring") and rng.random() < 0.5
        else:
            transform = str(_pick(rng, TRANSFORMS + ("none",)))
            two_sizes = transform in ("place", "key_place", "place_key") and feeder in ("ring", "queue_over_ring") and rng.random() < 0.5
        mixed = "grade" in stages or "matte" in stages     # yuv420p and yuva420p frames within one ring or queue: the grade pool matches on the coverage plane
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
            if chain:
                return new_frame(w, h, 0, alpha=rng.random() < (0.5 if mixed else 0.4), kind="green" if "key" in stages else "noise")
            return new_frame(w, h, 0, alpha=rng.random() < 0.4, kind="green" if "key" in transform else "noise")

        def ring():
            ids = [draw_frame() for _ in range(int(rng.integers(2, 6)))]
            if two_sizes:      # both sizes are there, next to each other
                frames[ids[0]].update(w=size_a[0], h=size_a[1]); frames[ids[1]].update(w=size_b[0], h=size_b[1])
            if mixed:          # a frame with and a frame without coverage are there, next to each other
                frames[ids[0]].update(alpha=True); frames[ids[1]].update(alpha=False)
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
        if chain:
            sources[-1].update(stages=list(stages), order=[])
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
        if chain:
            # the setters at tick 0 in a drawn permutation of the chain's order; later a drawn stage is set again with other parameters, removed, or put back
            def draw(op, again):
                return (_grade_params(rng) if op == "grade" else _key_params(rng) if op == "key" else _matte_params(rng, size_a[0], size_a[1], again) if op == "matte"
                        else _place_params(rng, min_w, min_h, two_sizes))
            state = {op: draw(op, False) for op in stages}
            order = [stages[int(i)] for i in rng.permutation(len(stages))]
            sources[-1]["order"] = order
            for op in order:
                events[0].append(dict(op=op, src=s, params=state[op]))
            for b in sorted(int(x) for x in rng.permutation(later)[:int(rng.integers(1, 5))]):
                op = str(_pick(rng, stages))
                state[op] = draw(op, True) if (state[op] is None or rng.random() < 0.65) else None
                events[b].append(dict(op=op, src=s, params=state[op]))
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
    chain_srcs = [s for s, d in enumerate(sources) if d.get("stages")]
    reset_src = next((s for s, d in enumerate(sources) if d["transform"] in ("key", "place", "key_place", "place_key")), None)
    if chain:
        # on a stage that is NOT the last one active, where two or more are: a stale picture then comes out of a LATER stage's list
        reset_src = next((s for s in chain_srcs if len(sources[s]["stages"]) >= 2), chain_srcs[0] if chain_srcs else None)
    if chain and reset_src is not None:
        on = {}
        for b in sorted(events):
            if b <= b1 + 1:
                on.update({e["op"]: e["params"] is not None for e in events[b] if e.get("src") == reset_src and e["op"] in STAGES})
        on = [op for op in STAGES if on.get(op)]
        op = str(_pick(rng, on[:-1])) if len(on) >= 2 else (on[0] if on else str(_pick(rng, sources[reset_src]["stages"])))
        mine = frames_of(reset_src)
        big = max(mine, key=lambda f: f["w"])
        events[b1 + 1].append(dict(op=op, src=reset_src, params=_grade_params(rng) if op == "grade" else _key_params(rng) if op == "key" else
                                   _matte_params(rng, big["w"], big["h"], True) if op == "matte" else
                                   _place_params(rng, min(f["w"] for f in mine), min(f["h"] for f in mine), sources[reset_src]["two_sizes"])))
    elif reset_src is not None:
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

    def tapped(d):
        """chain family: the first tap (the last, where an NV12 source has the first) is on a chain source's port"""
        if chain and chain_srcs and not any(p[0] in chain_srcs for p in d["ports"]) and (nv12_source is None or len(d["ports"]) >= 2):
            d["ports"][-1 if nv12_source is not None else 0] = [chain_srcs[0], 0]
        return d
    if nv12_source is not None:
        sc_ = _scopes(rng, ports)
        if [nv12_source, 0] not in sc_["ports"]:
            sc_["ports"][0] = [nv12_source, 0]
        events[0].append(dict(op="scopes", **tapped(sc_)))
    elif rng.random() < 0.85:
        events[0 if rng.random() < 0.7 else later[0]].append(dict(op="scopes", **tapped(_scopes(rng, ports))))
    for b in sorted(int(x) for x in rng.permutation(later)[:int(rng.integers(0, 3))]):
        events[b].append(dict(op="scopes", **(_scopes(rng, ports) if rng.random() < 0.7 else dict(ports=[], wave_cols=0, vectorscope=0, hop=1))))
    if reset_src is None:
        events[b1 + 1].append(dict(op="scopes", **_scopes(rng, ports)))
    if rng.random() < 0.9 or nv12_source is not None:
        mv = _multiview(rng, ports, int(rng.integers(1, 7)))
        if nv12_source is not None:
            mv["ports"][-1] = [nv12_source, 0]
        if chain and chain_srcs and not any(p[0] in chain_srcs for p in mv["ports"]) and (nv12_source is None or len(mv["ports"]) >= 2):
            mv["ports"][0] = [chain_srcs[0], 0]
        events[0 if rng.random() < 0.7 else later[0]].append(dict(op="multiview", **mv))
    for b in sorted(int(x) for x in rng.permutation(later)[:int(rng.integers(0, 3))]):
        events[b].append(dict(op="multiview", **(_multiview(rng, ports, int(rng.integers(1, 7))) if rng.random() < 0.7 else dict(ports=[]))))
    sc = dict(seed=seed, rate=rate, spt=spt, first_tick=first_tick, n_ticks=n_ticks, n_sources=n_src, sources=sources, frames=frames, mixers=mixers,
              mixer_updates={int(k): v for k, v in sorted(mixer_updates.items())}, sinks=sinks, monitor=monitor,
              events={int(k): v for k, v in sorted(events.items())}, boundaries=bounds, one_tick_run=b1)
    if chain:
        sc["chain"] = True
    return sc


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
    if isinstance(d, dict):
        return tuple(sorted((k, _freeze(v)) for k, v in d.items()))
    return tuple(_freeze(v) for v in d) if isinstance(d, (list, tuple)) else d


_LATTICES = {}


def grade_p(par) -> gm.GradeP:
    """the model's parameters of a drawn grade setting"""
    nodes = None
    if par["flags"] & gm.LUT:
        at = (par["k"], par["lattice"])
        if at not in _LATTICES:
            _LATTICES[at] = gm.smooth_lattice(par["k"]) if par["lattice"] == "smooth" else gm.random_lattice(par["k"], par["lattice"])
        nodes = _LATTICES[at]
    return gm.GradeP(par["flags"], gm.gamma_curve(*par["curve"]), tuple(par["m"]), tuple(par["off"]), par["k"], nodes)


def matte_p(par) -> mt.MatteP:
    """the model's parameters of a drawn matte setting: the fields, or the model's own wipe() of the drawn position"""
    if "wipe" in par:
        return mt.wipe(*par["wipe"])
    return mt.MatteP(clean=None if par["clean"] is None else tuple(par["clean"]), choke=par["choke"], soften=par["soften"],
                     mask=None if par["mask"] is None else tuple(par["mask"]), shape=par["shape"], invert=par["invert"], feather=par["feather"])


def transformed(sc, pic: Pic, key, place, band, place_first=False, grade=None, matte=None, fault=None) -> Pic:
    """what a SOURCE_VIDEO node delivers for `pic` under its settings: GRADE, THEN KEY, THEN MATTE, THEN PLACE, each where it is set, whichever call came first -- the
    grade corrects the colour the key is decided on and passes a coverage plane through, the key multiplies its decision into the coverage the frame came with, the
    matte refines the coverage so far (the frame's own, or opaque, with no key), the placer resamples the refined plane with the picture; a row band otherwise.
    place_first and the CHAIN_FAULTS: the wrong orders and the lost planes.  Made once per frame identity and setting."""
    if key is None and place is None and band is None and grade is None and matte is None:
        return pic
    if place_first:
        fault = "place_before_key"
    cache = sc.setdefault("_transformed", {})
    uid = ("t", pic.uid, _freeze(key), _freeze(place), _freeze(band), fault) + ((_freeze(grade), _freeze(matte)) if (grade or matte) else ())
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
            order = {"place_before_key": ("grade", "place", "key", "matte"), "matte_before_key": ("grade", "matte", "key", "place"),
                     "grade_after_key": ("key", "grade", "matte", "place")}.get(fault, STAGES)
            pars = dict(grade=grade, key=key, matte=matte, place=place)
            for op in order:
                par = pars[op]
                if par is None:
                    continue
                if op == "grade":
                    y, u, v = gm.grade_model(y, u, v, grade_p(par))
                    if fault == "grade_drops_coverage":
                        a = None
                elif op == "key":     # matte_before_key: the key's decision replaces the plane the matte refined
                    y, u, v, a = km.key_model(y, u, v, km.KeyP(**par), None if (fault == "matte_before_key" and matte is not None) else a)
                elif op == "matte":
                    y, u, v, a = mt.matte_model(y, u, v, matte_p(par), a_in=None if (fault == "matte_ignores_coverage" and key is None) else a)
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
    assert fault is None or fault in FAULTS + CHAIN_FAULTS
    in_model = fault if fault in ("place_before_key", "matte_before_key", "grade_after_key", "grade_drops_coverage", "matte_ignores_coverage") else None
    n_src, rate, spt, tick0 = sc["n_sources"], sc["rate"], sc["spt"], sc["first_tick"]
    src = [dict(ring=[], pos=0, queue=[], frame=None, repeat=False, pending=False, dur=None, off=None, key=None, place=None, band=None, grade=None, matte=None, stale={}) for _ in range(n_src)]
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
            if op in ("ring", "repeat", "shot", "queue", "key", "place", "band", "grade", "matte"):
                s = src[e["src"]]
            if op == "ring":                       # clears a set frame; the ring starts at its first frame
                s.update(ring=list(e["frames"]), pos=0, frame=None, repeat=False, pending=False, dur=tuple(e["dur"]), off=tuple(e["off"]))
            elif op in ("repeat", "shot"):
                s.update(frame=e["frame"], repeat=op == "repeat", pending=True, dur=tuple(e["dur"]), off=tuple(e["off"]))
            elif op == "queue":
                s["queue"] = s["queue"] + [(q["tick"], q["frame"], tuple(q["dur"]), tuple(q["off"])) for q in e["entries"]]
            elif op in ("key", "place", "band", "grade", "matte"):
                if e["params"] is None and fault == "removed_transform_stays":
                    continue
                if e["params"] is None or s[op] is None or fault != "stale_after_reset":
                    s["stale"] = {}                # the right model forgets here; the stale one only when the transform goes or comes
                par = e["params"]
                if (op == "grade" and fault == "old_lattice_after_reset" and par is not None and par["flags"] & gm.LUT and s["grade"] is not None
                        and s["grade"]["flags"] & gm.LUT):
                    par = dict(par, k=s["grade"]["k"], lattice=s["grade"]["lattice"])    # the new curve and matrix, the lattice that was retained
                s[op] = par
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
        info = dict(scope_symbolic=0, scope_none=0, scope_nv12=0, mv_symbolic=0, mv_nv12=0, sink_size_change=0, subsets=set(), matte_no_key_on_coverage=0,
                    chain_into_program=0, scope_chain=0, mv_chain=0)
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
                    if fault == "stale_after_reset" and (s["key"] or s["place"] or s["band"] or s["grade"] or s["matte"]):
                        if v[0] not in s["stale"]:     # the whole chain's result under the setting the frame was first met with
                            s["stale"][v[0]] = transformed(sc, pic, s["key"], s["place"], s["band"], grade=s["grade"], matte=s["matte"])
                        t = s["stale"][v[0]]
                    else:
                        t = transformed(sc, pic, s["key"], s["place"], s["band"], grade=s["grade"], matte=s["matte"], fault=in_model)
                    ports[(i, 0)] = (t, v[1], v[2])
                    on = [op for op in STAGES if s[op] is not None]
                    if on:
                        info["subsets"].add("+".join(on))
                        info["matte_no_key_on_coverage"] += s["matte"] is not None and s["key"] is None and pic.a is not None
            for m in mixers:
                ins = []
                for ref in m["inputs"]:
                    v = None if ref is None else ports[tuple(ref)]
                    ins.append(v)
                forever = (10 ** 6, 1)
                res = m["om"].run_tick(tick * spt, [None if v is None else (v[0].host(), forever if fault == "no_expiry" else v[1], v[2]) for v in ins])
                node = m["node"]
                ports[(node, 0)] = None if res is None else (Pic(0, res.w, res.h, res.visible(), None, ("m", node, tick), host=res), (1, 60), (0, 1))
                info["chain_into_program"] += res is not None and any(ref is not None and ref[0] < n_src and v is not None and any(src[ref[0]][op] is not None for op in STAGES)
                                                                      for ref, v in zip(m["inputs"], ins))
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
                        info["scope_chain"] += v is not None and node < n_src and any(src[node][op] is not None for op in STAGES)
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
                        info["mv_chain"] += v is not None and node < n_src and any(src[node][op] is not None for op in STAGES)
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
                        raw={p: (None if v is None else v[0]) for p, v in raw.items()},
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
