"""Random taps of all seven audio tap sets for the full random graphs (tests/test_gpu_random_graphs.py run_full_graph), shared by the GPU
test and its CPU proof (tests/test_cpu_random_graphs.py): which ports each set taps, with which parameters, when each set is set again, and
what every set's records must be -- the set's numpy model (meter_model, spectrum_model, loudness_model, stereo_model, limiter_model,
tempo_model, tonality_model), one instance per set and tap, fed the ORACLE's samples of the tapped port.

Everything here is drawn from a random stream of its own (default_rng(8000 + seed)): the graph generator's stream and run_full_graph's
(7000 + seed) draw what they always drew.  Nothing here needs a GPU but `read`, which takes a built graph.

The rules the expected side follows are the header's (include/mixlab_gpu.h): meters keep the hold state of a tap that survives a
mx_graph_set_meters and start a new one from 0; every other set resets every tap and its emission counter c on every call; no set touches
another's state; a tap counts frames in its port's own rate domain; records come back in set order.  `fault` makes the expected side
wrong in exactly one of those ways (FAULTS): the CPU test shows that each of them changes the records the GPU test compares.
"""
from __future__ import annotations

import math

import numpy as np

import limiter_model
import loudness_model
import meter_model
import spectrum_model
import stereo_model
import tempo_model
import tonality_model
from mixlab_amd import abi

SETS = ("meters", "spectra", "loudness", "stereo", "limiters", "tempo", "tonality")
RESETTING = SETS[1:]                              # every call resets every tap (meters: survivors keep their hold)
EMITTING = ("stereo", "tempo", "tonality")        # a counter c per set: +1 per tick, c mod period == 0 emits
FAULTS = ("no_reset", "meters_reset", "reset_per_run", "c_per_run", "base_frames", "left_only", "sorted_order", "one_tick_late")
CAP = 4                                           # taps per set: the models' time, not the device's, is what this bounds
CAPS = {"loudness": 3}                            # (its model loops over every frame in Python; a dup-stored, a resampled and a mono port fit in 3)
MONO, STEREO = 1, 2
F32 = np.float32

# port classes of the coverage test (tests/test_cpu_random_graphs.py); the fill-up draw picks a class first, so the rare ones are tapped too
CLASS_OF = {abi.KIND_SOURCE_MONO: "source", abi.KIND_SOURCE_STEREO: "source", abi.KIND_OSCILLATOR: "oscillator", abi.KIND_FM_SINE: "oscillator",
            abi.KIND_EQ_THREE: "eq", abi.KIND_AMPLIFIER: "amplifier", abi.KIND_MIXER: "mixer", abi.KIND_FIR: "fir_resample",
            abi.KIND_RESAMPLE: "fir_resample", abi.KIND_TRIGGER: "control", abi.KIND_ENVELOPE: "control", abi.KIND_STEREO_PANNER: "panner",
            abi.KIND_STEREO_SPLITTER: "splitter"}


def predict_fusion(ws, order, n_inputs):
    """plan_fusion (mx_plan.cpp) restated: -> (ports the default build folds away, stereo ports it stores one float per frame).
    The GPU test asserts both against the built graph and tests/test_cpu_graph_plan.py against the compiler itself (mx_graph_debug_plan), so the
    CPU test, which builds no graph, draws the very same taps."""
    pos = {n: i for i, n in enumerate(order)}
    kind = lambda n: ws.nodes[n][0]
    in_src, cons = {}, {}
    for n in order:
        for k in range(n_inputs(*ws.nodes[n])):
            src = ws._conn.get((n, k))
            if src is not None and src[0] in pos and pos[src[0]] < pos[n]:   # (a back-edge reads Disconnected)
                in_src[(n, k)] = src
                cons.setdefault(src, []).append((n, k))

    def depends_on(start, target):
        stack, visited = [start], 0
        while stack:
            x = stack.pop()
            if x == target:
                return True
            visited += 1
            if visited > 256:
                return True
            stack += [in_src[(x, k)][0] for k in range(n_inputs(*ws.nodes[x])) if (x, k) in in_src]
        return False

    elided, dup, fuse_pan, fuse_amp, elided_nodes, fuse_trigger = set(), set(), {}, {}, set(), {}
    for e in order:
        c = cons.get((e, 0), [])
        if kind(e) != abi.KIND_EQ_THREE or len(c) != 2 or c[0][0] != c[1][0] or c[0][1] == c[1][1]:
            continue
        p = c[0][0]
        if kind(p) != abi.KIND_STEREO_PANNER or p in elided_nodes:
            continue
        fuse_pan[e] = p; elided.add((e, 0)); elided_nodes.add(p)
        pc = cons.get((p, 0), [])
        if len(pc) == 1 and kind(pc[0][0]) == abi.KIND_AMPLIFIER and pc[0][1] == 0:
            a = pc[0][0]
            ctl = in_src.get((a, 1))
            if ctl is None or not depends_on(ctl[0], e):
                fuse_amp[e] = a; elided.add((p, 0)); elided_nodes.add(a)
    for v in order:
        g = in_src.get((v, 0))
        if kind(v) == abi.KIND_ENVELOPE and g is not None and kind(g[0]) == abi.KIND_TRIGGER and len(cons.get((g[0], 0), [])) == 1:
            fuse_trigger[v] = g[0]; elided.add((g[0], 0))
    for e in order:
        if e not in fuse_pan:
            continue
        if e in fuse_amp:
            ctl = in_src.get((fuse_amp[e], 1))
            if ctl is not None and kind(ctl[0]) == abi.KIND_ENVELOPE and ctl[0] in fuse_trigger and len(cons.get((ctl[0], 0), [])) == 1:
                elided.add((ctl[0], 0))
        x = fuse_amp.get(e, fuse_pan[e])
        xc = cons.get((x, 0), [])
        if xc and all(kind(n) in (abi.KIND_MIXER, abi.KIND_OUTPUT_DEVICE) for n, _k in xc):
            dup.add((x, 0))
    return elided, dup


class RandomTaps:
    """`types[node][port]` MONO | STEREO, `frames[(node, port)]` the port's frames per tick, `rates[(node, port)]` its frames per second as the
    engine computes them, `common` the ports every build can read (taps go there only: a folded port cannot be tapped), `dup` the stereo
    ports the fused build stores one float per frame, `resampled` the ports behind a Resample."""

    def __init__(self, seed, ws, shape, types, frames, rates, common, dup, resampled, n_runs, tap_sets=SETS, fault=None, cap=CAP):
        assert fault is None or fault in FAULTS
        self.rng = np.random.default_rng(8000 + seed)
        self.ws, self.shape, self.types, self.frames, self.rates = ws, shape, types, frames, rates
        self.spt, self.sets, self.fault, self.cap = ws.spt, tuple(tap_sets), fault, cap
        self.dup, self.resampled = list(dup), list(resampled)
        self.also = []                              # further pools every set takes a port of (the deck sessions: the stereo source ports)
        self.cand = {name: [pt for pt in common if self.accepts(name, pt)] for name in self.sets}
        for name in self.sets:
            out = sorted({self.rates[pt] for pt in common if pt not in self.cand[name] and name != "stereo"})
            if out:
                print(f"random_taps: seed {seed}: {name} accepts no port at {out} Hz: ports of that rate left out")
        self.ports = {name: [] for name in self.sets}
        self.params = {name: None for name in self.sets}
        self.models = {name: {} for name in self.sets}
        self.c = {name: 0 for name in self.sets}
        self.n_runs_seen = 0
        self.last = {}                              # every port's previous tick (the one_tick_late fault reads it)
        self.tapped = {name: set() for name in self.sets}   # every port the set ever tapped
        self.orders = {name: [] for name in self.sets}      # every port list it was given
        self.one_tick_run = int(self.rng.integers(0, n_runs - 1))   # this run is one tick long, and it is not the last
        one_tick_run = self.one_tick_run
        # when each set is set again: runs of its own; one set at least directly after the one-tick run; sometimes [] and back
        self.plan = {}
        for i, name in enumerate(self.sets):
            runs = {r for r in range(1, n_runs) if self.rng.random() < 0.3}
            if not runs or (i + seed) % 2 == 0:
                runs.add(one_tick_run + 1)
            plan = {}
            for r in sorted(runs):
                if r in plan:
                    continue
                if self.rng.random() < 0.25 and r + 1 < n_runs:
                    plan[r], plan[r + 1] = "empty", "draw"
                else:
                    plan[r] = "draw"
            self.plan[name] = plan

    # ---- what a set accepts, and what it is given -----------------------------------------------------------------------------------
    def accepts(self, name, pt):
        if name == "stereo":
            return self.types[pt[0]][pt[1]] == STEREO
        if name == "loudness":                      # a rate above twice the shelf frequency
            try:
                loudness_model.tables(self.rates[pt], self.frames[pt])
                return True
            except abi.MxError:
                return False
        return True

    def draw_params(self, name):
        rng = self.rng
        pick = lambda xs: xs[int(rng.integers(0, len(xs)))]
        if name == "spectra":
            n_fft = pick((256, 512))
            sr = float(self.shape.sample_rate)
            return {"n_fft": n_fft, "edges": abi.log_band_edges(n_fft, int(rng.integers(4, 9)), sr / 64.0, 0.45 * sr, sr)}
        if name == "loudness":
            return {"momentary_ticks": int(rng.integers(1, 7)), "short_ticks": int(rng.integers(1, 7))}
        if name == "stereo":
            return {"window_ticks": int(rng.integers(1, 7)), "grid": pick((0, 64, 128)), "zoom_log2": int(rng.integers(0, 3)), "hop": int(rng.integers(1, 5))}
        if name == "limiters":
            return {"ceiling": float(F32(rng.uniform(0.25, 1.0))), "lookahead": pick((0, 1, 7, 64, 512))}
        if name == "tempo":
            W = pick((64, 128))
            return {"hop_frames": pick((64, 128)), "window_hops": W, "max_lag": int(rng.integers(16, W + 1)), "emit_ticks": int(rng.integers(1, 5))}
        if name == "tonality":                      # f_lo_mhz follows the ports (fit_tonality)
            return {"decim": pick((4, 8)), "hop_frames": pick((128, 256)), "octaves": int(rng.integers(2, 4)), "f_lo_mhz": 0, "emit_ticks": int(rng.integers(1, 5))}
        return {}                                   # meters: one MeterParams per tap

    def fit_tonality(self, par, ports):
        """f_lo_mhz from the rates of `ports`: the lowest bin must be short enough at the highest rate (N_0 <= 2048) and the top bin below
        0.45 fs_d at the lowest.  Where no f_lo serves both ends, the ports of the lowest rates are left out.  -> the ports kept"""
        D, O = par["decim"], par["octaves"]
        span = 2.0 ** ((12 * O - 1) / 12.0 + 1.0 / 24.0)
        ports = list(ports)
        while ports:
            lo = 17.0 * max(self.rates[pt] for pt in ports) / D / 2048.0 * 1.02
            hi = 0.45 * min(self.rates[pt] for pt in ports) / D / span * 0.98
            if lo <= hi:
                par["f_lo_mhz"] = max(1, int(math.ceil(1000.0 * lo * min(hi / lo, float(self.rng.uniform(1.0, 3.0))))))
                for pt in ports:                    # the library's own word on it
                    abi.tonality_tables(self.rates[pt], D, par["hop_frames"], O, par["f_lo_mhz"])
                return ports
            worst = min(self.rates[pt] for pt in ports)
            print(f"random_taps: tonality D {D} O {O}: no f_lo serves {worst} Hz beside {max(self.rates[pt] for pt in ports)} Hz: ports of that rate left out")
            ports = [pt for pt in ports if self.rates[pt] != worst]
        return ports

    def tonality_fits(self, par, ports):
        try:
            for pt in ports:
                abi.tonality_tables(self.rates[pt], par["decim"], par["hop_frames"], par["octaves"], par["f_lo_mhz"])
            return True
        except abi.MxError:
            return False

    def port_class(self, pt):
        kind, params = self.ws.nodes[pt[0]]
        if kind == abi.KIND_MIXER and not params:
            return "empty_mixer"                    # its outputs are silence nobody mixed
        if kind == abi.KIND_OSCILLATOR and pt[1] == 1:
            return "stereo_twin"
        return CLASS_OF[kind]

    def draw_ports(self, name, old=()):
        """a list in shuffled order: a dup-stored port, a port whose tick is not spt frames, a port behind a Resample, a mono and a stereo port
        wherever the set accepts one, about half of `old`, and others up to the cap, drawn class by class"""
        rng, cand = self.rng, self.cand[name]
        ok = set(cand)
        keep = [pt for pt in old if pt in ok and rng.random() < 0.5]
        chosen = []

        def need(pool):
            pool = [pt for pt in pool if pt in ok]
            if not pool or any(pt in chosen for pt in pool):
                return
            kept = [pt for pt in keep if pt in pool]
            chosen.append(kept[0] if kept else pool[int(rng.integers(0, len(pool)))])

        need(self.dup)
        need([pt for pt in self.resampled if self.frames[pt] != self.spt])
        need(self.resampled)
        need([pt for pt in cand if self.types[pt[0]][pt[1]] == MONO])
        need([pt for pt in cand if self.types[pt[0]][pt[1]] == STEREO])
        for pool in self.also:
            need(pool)
        cap =min(self.cap, CAPS.get(name, self.cap))
        for pt in keep:
            if len(chosen) < cap and pt not in chosen:
                chosen.append(pt)
        while len(chosen) < min(cap, len(cand)):
            classes = {}
            for pt in cand:
                if pt not in chosen:
                    classes.setdefault(self.port_class(pt), []).append(pt)
            names = sorted(classes)
            pool = classes[names[int(rng.integers(0, len(names)))]]
            chosen.append(pool[int(rng.integers(0, len(pool)))])
        return [chosen[int(i)] for i in rng.permutation(len(chosen))]

    # ---- setting --------------------------------------------------------------------------------------------------------------------
    def channels(self, pt):
        ty = self.types[pt[0]][pt[1]]
        return MONO if self.fault == "left_only" else ty

    def model_frames(self, pt):
        return self.spt if self.fault == "base_frames" else self.frames[pt]

    def new_model(self, name, pt, par):
        ch = self.channels(pt)
        if name == "meters":
            return meter_model.MeterModel(ch, par[pt].hold_ticks, par[pt].release)
        if name == "spectra":
            return spectrum_model.SpectrumModel(ch, par["n_fft"], par["edges"])
        if name == "loudness":
            return loudness_model.LoudnessModel(ch, self.rates[pt], self.model_frames(pt), par["momentary_ticks"], par["short_ticks"])
        if name == "stereo":
            return stereo_model.StereoModel(par["window_ticks"], par["grid"], par["zoom_log2"], par["hop"])
        if name == "limiters":
            return limiter_model.LimiterModel(par["ceiling"], par["lookahead"], ch)
        if name == "tempo":
            return tempo_model.TempoModel(par["hop_frames"], par["window_hops"], par["max_lag"], par["emit_ticks"], ch)
        return tonality_model.TonalityModel(self.rates[pt], par["decim"], par["hop_frames"], par["octaves"], par["f_lo_mhz"], par["emit_ticks"], ch)

    def set(self, name, graphs, empty=False):
        """draws the set's next port list (and sometimes new parameters), sets it on every graph and brings the models where the header says
        they then are"""
        rng, old, old_par = self.rng, self.ports[name], self.params[name]
        ports = [] if empty else self.draw_ports(name, old)
        par, same_par = old_par, old_par is not None
        if name == "meters":
            par = dict(old_par or {})
            for pt in ports:
                if pt not in old:                   # a surviving tap keeps its parameters too
                    par[pt] = abi.MeterParams(int(rng.integers(0, 9)), float(rng.uniform(0.5, 1.0)))
        elif not empty and (old_par is None or rng.random() < 0.5):
            par, same_par = self.draw_params(name), False
        if name == "tonality" and ports and not (same_par and self.tonality_fits(par, ports)):
            par, same_par = dict(par), False
            ports = self.fit_tonality(par, ports)
        if name == "meters":
            keep = old if self.fault != "meters_reset" else []
        else:                                       # no_reset: a tap that was there runs on (its parameters the same: a model cannot change them)
            keep = old if self.fault == "no_reset" and same_par else []
            if not keep:
                self.c[name] = 0
        self.models[name] = {pt: (self.models[name][pt] if pt in keep and pt in self.models[name] else self.new_model(name, pt, par)) for pt in ports}
        self.ports[name], self.params[name] = ports, par
        self.tapped[name] |= set(ports)
        self.orders[name].append(list(ports))
        for g in graphs:
            if name == "meters":
                g.set_meters(ports, [par[pt] for pt in ports])
            elif name == "spectra":
                g.set_spectra(ports, par["n_fft"], par["edges"])
            else:
                getattr(g, {"loudness": "set_loudness", "stereo": "set_stereo", "limiters": "set_limiters", "tempo": "set_tempo",
                            "tonality": "set_tonality"}[name])(ports, **par)

    def before_run(self, run, graphs):
        """run 0: every set is set; later runs: the sets whose plan names the run are set again, each on its own"""
        graphs = list(graphs)
        for name in self.sets:
            what = "draw" if run == 0 else self.plan[name].get(run)
            if what:
                self.set(name, graphs, empty=what == "empty")

    # ---- the expected side ----------------------------------------------------------------------------------------------------------
    def samples(self, pt, outs):
        """the run's samples of `pt` as the tap takes them: outs[k][pt] tick after tick (a fault: not quite)"""
        ty = self.types[pt[0]][pt[1]]
        ticks = [o[pt] for o in outs]
        if self.fault == "one_tick_late":
            ticks = [self.last.get(pt, np.zeros(self.frames[pt] * ty, F32))] + ticks[:-1]
        if self.fault == "base_frames" and self.frames[pt] != self.spt:
            short = []
            for x in ticks:
                y = np.zeros(self.spt * ty, F32)
                n = min(y.size, x.size)
                y[:n] = x[:n]
                short.append(y)
            ticks = short
        x = np.concatenate(ticks).astype(F32, copy=False)
        if self.fault == "left_only" and ty == STEREO:
            x = np.ascontiguousarray(x.reshape(-1, 2)[:, 0])
        return x

    def expect_run(self, L, outs):
        """outs[k][(node, port)]: the oracle's output of every port in tick k of the run.  -> {set: records}, records as `read` returns them:
        "ports" the set order, "ticks" [tick][tap] (or None), "emitted" [(tick in run, [payload per tap])] (or None), "limited" one array per tap"""
        want = {}
        for name in self.sets:
            ports = self.ports[name]
            rec = {"ports": list(ports), "ticks": None, "emitted": None, "limited": None, "i16": None}
            want[name] = rec
            if self.fault == "reset_per_run":
                self.models[name] = {pt: self.new_model(name, pt, self.params[name]) for pt in ports}
                self.c[name] = 0
            if not ports:
                continue
            models = [self.models[name][pt] for pt in ports]
            c0 = 0 if self.fault == "c_per_run" else self.c[name]
            xs = []
            for pt in ports:
                x = self.samples(pt, outs)
                if name == "stereo" and self.fault == "left_only":
                    x = np.repeat(x, 2)             # L = R = the left channel
                xs.append(x)
            if name in EMITTING:
                for m in models:
                    m.c = c0
            if name == "meters":
                rec["ticks"] = np.stack([m.run(x, L) for m, x in zip(models, xs)], axis=1)
            elif name == "spectra":
                rec["ticks"] = np.stack([m.run(x, L) for m, x in zip(models, xs)], axis=1)
            elif name == "loudness":                # (one walk for the taps that share a tick length: the model's time is its loop over frames)
                rec["ticks"] = np.stack(loudness_model.run_many(models, xs, L), axis=1)
            elif name == "stereo":
                res = [m.run(x, L) for m, x in zip(models, xs)]
                rec["ticks"] = np.stack([r[0] for r in res], axis=1)
                if self.params[name]["grid"]:
                    rec["emitted"] = rows([[(e["tick_in_run"], e) for e in r[1]] for r in res])
            elif name == "limiters":
                # (what the copy is compared with where a test asks whether the limiter did anything: the input delayed by the lookahead)
                rec["delayed"] = [np.concatenate([m.hist, x.reshape(-1, m.C)])[m.D:m.D + x.size // m.C].reshape(-1) for m, x in zip(models, xs)]
                res = [m.run(x, L) for m, x in zip(models, xs)]
                rec["ticks"] = np.stack([r[1] for r in res], axis=1)
                rec["limited"] = [r[0] for r in res]
                tap = self.n_runs_seen % len(ports)
                rec["i16"] = (tap, limiter_model.to_i16(rec["limited"][tap]))
            else:
                res = [m.run(x, L) for m, x in zip(models, xs)]
                rec["emitted"] = rows([[(int.from_bytes(b[:4], "little"), b[4:]) for b in r] for r in res])
            self.c[name] = c0 + L
            if self.fault == "sorted_order":        # the records in sorted port order
                perm = sorted(range(len(ports)), key=lambda i: ports[i])
                if rec["ticks"] is not None:
                    rec["ticks"] = rec["ticks"][:, perm]
                if rec["emitted"] is not None:
                    rec["emitted"] = [(t, [row[i] for i in perm]) for t, row in rec["emitted"]]
                if rec["limited"] is not None:
                    rec["limited"] = [rec["limited"][i] for i in perm]
                    rec["i16"] = (rec["i16"][0], limiter_model.to_i16(rec["limited"][rec["i16"][0]]))
        self.last = outs[-1]
        self.n_runs_seen += 1
        return want

    # ---- the device side ------------------------------------------------------------------------------------------------------------
    def read(self, g, n_ticks, want):
        """the last run's (n_ticks ticks) records of every set of graph `g`, in the shape of expect_run's"""
        got = {}
        for name in self.sets:
            ports = self.ports[name]
            rec = {"ports": list(ports), "ticks": None, "emitted": None, "limited": None, "i16": None}
            got[name] = rec
            if not ports:
                continue
            if name == "meters":
                rec["ticks"] = g.read_meters(0, n_ticks)
            elif name == "spectra":
                rec["ticks"] = g.read_spectra(0, n_ticks)
            elif name == "loudness":
                rec["ticks"] = g.read_loudness(0, n_ticks)
            elif name == "stereo":
                rec["ticks"] = g.read_stereo(0, n_ticks)
                if self.params[name]["grid"]:
                    rec["emitted"] = [(row[0]["tick_in_run"], row) for row in g.read_goniometers()]
            elif name == "limiters":
                rec["ticks"] = g.read_limiters(0, n_ticks)
                rec["limited"] = [g.read_limited(i, 0, n_ticks) for i in range(len(ports))]
                tap = want[name]["i16"][0]
                rec["i16"] = (tap, g.read_limited(tap, 0, n_ticks, i16=True))
            else:
                read = g.read_tempo if name == "tempo" else g.read_tonality
                emitted = read()
                assert all(r["tick_in_run"] == row[0]["tick_in_run"] for row in emitted for r in row)
                rec["emitted"] = [(row[0]["tick_in_run"], [r["raw"][4:] for r in row]) for row in emitted]
        return got


def rows(per_tap):
    """[tap][emission] (tick, payload) -> [emission] (tick, [payload per tap]); every tap of a set emits at the same ticks"""
    assert all([t for t, _p in r] == [t for t, _p in per_tap[0]] for r in per_tap)
    return [(per_tap[0][e][0], [r[e][1] for r in per_tap]) for e in range(len(per_tap[0]))]


def join(pieces):
    """[(first tick of the piece in the run, {set: records})] of one run read in several submissions -> {set: records} of the run"""
    out = {}
    for name in pieces[0][1]:
        recs = [(k0, p[name]) for k0, p in pieces]
        first = recs[0][1]
        rec = {"ports": first["ports"], "ticks": None, "emitted": None, "limited": None, "i16": None}
        if first["ticks"] is not None:
            rec["ticks"] = np.concatenate([r["ticks"] for _k0, r in recs], axis=0)
        if first["emitted"] is not None:
            rec["emitted"] = [(k0 + t, row) for k0, r in recs for t, row in r["emitted"]]
        if first["limited"] is not None:
            rec["limited"] = [np.concatenate([r["limited"][i] for _k0, r in recs]) for i in range(len(first["limited"]))]
            rec["i16"] = (first["i16"][0], np.concatenate([r["i16"][1] for _k0, r in recs]))
        out[name] = rec
    return out


def difference(name, got, want):
    """None where the records of set `name` equal `want` by the set's own comparison (its model module's), else a line on the first difference"""
    if got["ports"] != want["ports"]:
        return f"ports {got['ports']} != {want['ports']}"
    ports = want["ports"]
    for key in ("ticks", "emitted", "limited"):
        if (got[key] is None) != (want[key] is None):
            return f"{key}: one side has none"
    a, b = got["ticks"], want["ticks"]
    if a is not None:
        if a.shape != b.shape:
            return f"records shaped {a.shape}, want {b.shape}"
        for i, pt in enumerate(ports):
            u, v = np.ascontiguousarray(a[:, i]), np.ascontiguousarray(b[:, i])
            if name == "meters":
                ok = bool(meter_model.records_equal(u, v).all())
            elif name == "spectra":
                ok = bool(spectrum_model.records_equal(u, v).all())
            elif name == "loudness":
                ok = loudness_model.records_equal(u, v)
            elif name == "stereo":
                ok = stereo_model.records_equal(u, v)
            else:
                ok = limiter_model.records_equal(u, v)
            if not ok:
                k = next((k for k in range(len(u)) if u[k:k + 1].tobytes() != v[k:k + 1].tobytes()), 0)
                return f"tap {i} {pt} tick {k}: got {u[k]}, want {v[k]}"
    a, b = got["emitted"], want["emitted"]
    if a is not None:
        if [t for t, _r in a] != [t for t, _r in b]:
            return f"emissions at ticks {[t for t, _r in a]}, want {[t for t, _r in b]}"
        for (t, ra), (_t, rb) in zip(a, b):
            if len(ra) != len(rb):
                return f"emission at tick {t}: {len(ra)} records, want {len(rb)}"
            for i, pt in enumerate(ports):
                if name == "stereo":
                    ok = stereo_model.gonio_equal(dict(ra[i], tick_in_run=0), dict(rb[i], tick_in_run=0))
                else:
                    ok = bytes(ra[i]) == bytes(rb[i])
                if not ok:
                    return f"tap {i} {pt}: the record emitted at tick {t} differs"
    if got["limited"] is not None:
        for i, pt in enumerate(ports):
            u, v = got["limited"][i], want["limited"][i]
            if u.size != v.size or not np.array_equal(u.view(np.uint32), v.view(np.uint32)):
                return f"tap {i} {pt}: the limited copy differs"
        (ta, ia), (tb, ib) = got["i16"], want["i16"]
        if ta != tb or not np.array_equal(ia, ib):
            return f"tap {tb}: the limited copy's i16 form differs"
    return None
