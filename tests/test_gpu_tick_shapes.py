"""GPU parity at every tick shape of tests/tick_shapes.py: sample rates and tick rates other than 44 100 / 48 000 Hz at 60 ticks/s.

The exact EqThree path picks its chunk unit, warm-up and kernel form from the tick length; every group here asserts the form
mx_graph_debug_eq_launch reports against the table, so a shape that stops reaching its branch fails instead of passing on
another path.  Bars as everywhere in the suite: bit-exact against the oracle for the exact order (and the oracle's contract mode
for MX_FLAG_FP_CONTRACT), <= 1 ULP with the scan tests' rarity bound for MX_FLAG_EQ_FAST.

Every graph runs three submissions that carry state: a long one (the planner speculates where the shape allows), one tick
(no speculation), and a long one again.
"""
import ctypes as C
import math

import numpy as np
import pytest

import ingest_model as im
import oracle
import oracle_video as ov
import synth
from mixlab_amd import abi, video
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import assert_bit_exact, assert_ulp, config1, strips
from test_gpu_ingest import AbiMedia, FrameBook
from test_gpu_random_graphs import MONO, STEREO, port_types, random_graph
from test_gpu_video_graph import FADERS, MATRIX, cascade, upload
from test_ingest_oracle import play_media
from tick_shapes import FAR_EPOCHS, INVALID, SHAPE_STRIPS, SHAPES, by_id, far_first_tick

pytestmark = pytest.mark.gpu

SHAPE_PARAMS = [pytest.param(s, id=s.id) for s in SHAPES]


def submissions(shape):
    return [shape.long_ticks, 1, shape.long_ticks]


def gate_open(tick, k, period):
    return ((tick + k) // period) % 2 == 1


def schedule_gates(g, trigs, t0, n, period):
    """Every gate for tick t0, and its toggles inside [t0, t0 + n) through mx_graph_schedule_params_batch."""
    keep, events = [], []
    for k, tr in enumerate(trigs):
        g.update_params(tr, abi.TriggerParams(1 if gate_open(t0, k, period) else 0))
        for c in range(1, n):
            if gate_open(t0 + c, k, period) != gate_open(t0 + c - 1, k, period):
                p = abi.TriggerParams(1 if gate_open(t0 + c, k, period) else 0)
                keep.append(p)
                events.append(abi.ParamEvent(tr, c, C.cast(C.pointer(p), C.c_void_p), C.sizeof(p)))
    if events:
        g.schedule_params_batch((abi.ParamEvent * len(events))(*events))


def lfo_strips(n_strips, sr, tps):
    """config-2 strips whose Amplifier is modulated by an LFO's buffer instead of an Envelope: the control-tile form."""
    ws = Workspace(sr, tps)
    gains = synth.uniform(13, 3 * n_strips, -24.0, 6.0)
    mix = ws.mixer([(-1.5 * (k % 5), 0.25 + 0.05 * k, k % 3 == 0) for k in range(n_strips)])
    srcs, amps = [], []
    for k in range(n_strips):
        lfo = ws.oscillator(0.75 + 1.25 * k, abi.WAVE_TRIANGLE)
        src = ws.source_mono()
        eq = ws.eq_three(float(gains[3 * k]), float(gains[3 * k + 1]), float(gains[3 * k + 2]))
        pan = ws.stereo_panner()
        amp = ws.amplifier(0.9, 0.6)
        ws.connect(src, 0, eq, 0); ws.connect(eq, 0, pan, 0); ws.connect(eq, 0, pan, 1)
        ws.connect(pan, 0, amp, 0); ws.connect(lfo, 0, amp, 1); ws.connect(amp, 0, mix, k)
        srcs.append(src); amps.append(amp)
    return ws, mix, srcs, [], amps


def make_graph(shape, lfo=False):
    if lfo:
        return lfo_strips(SHAPE_STRIPS, shape.sample_rate, shape.ticks_per_second)
    ws, mix, srcs, trigs = strips(SHAPE_STRIPS, shape.sample_rate, shape.ticks_per_second)
    return ws, mix, srcs, trigs, mixer_inputs(ws, mix)


def mixer_inputs(ws, mix):
    """the nodes feeding the Mixer's channels, in channel order (each strip's Amplifier), looked up in the workspace's connections"""
    by_port = {dp: s for (s, _sp, d, dp) in ws.edges if d == mix}
    amps = [by_port[k] for k in range(len(by_port))]
    assert all(ws.nodes[a][0] == abi.KIND_AMPLIFIER for a in amps)
    return amps


_oracle_cache = {}


def oracle_outputs(shape, lfo, contract):
    """Per submission: (master, cue, [Amplifier output of every strip]) of the oracle ticked one tick at a time (cached: the forced
    variants change only the device's path, never what it must produce)."""
    key = (shape.id, lfo, contract)
    if key in _oracle_cache:
        return _oracle_cache[key]
    ws, mix, srcs, trigs, amps = make_graph(shape, lfo)
    spt, period = shape.spt, max(1, shape.long_ticks // 4)
    noise = [synth.noise(700 + k, sum(submissions(shape)) * spt) for k in range(SHAPE_STRIPS)]
    og = oracle.OracleGraph(ws)
    res, tick = [], 0
    with oracle.fp_contract(contract):
        for n in submissions(shape):
            m, c, a = [], [], [[] for _ in amps]
            for _ in range(n):
                for k, tr in enumerate(trigs):
                    og.update_params(tr, abi.TriggerParams(1 if gate_open(tick, k, period) else 0))
                for k, s in enumerate(srcs):
                    og.set_source(s, noise[k][tick * spt:(tick + 1) * spt])
                og.run_tick(tick)
                m.append(og.output(mix, 0)); c.append(og.output(mix, 1))
                for j, amp in enumerate(amps):
                    a[j].append(og.output(amp, 0))
                tick += 1
            res.append((np.concatenate(m), np.concatenate(c), [np.concatenate(x) for x in a]))
    _oracle_cache[key] = (noise, res)
    return noise, res


def run_strips(shape, flags=0, lfo=False):
    """The config-2 strips through the device at `shape`, every submission bit for bit against the oracle.
    -> ([debug_eq_launch after each submission], eq_repair_stats)"""
    contract = bool(flags & abi.FLAG_FP_CONTRACT)
    noise, want = oracle_outputs(shape, lfo, contract)
    ws, mix, srcs, trigs, amps = make_graph(shape, lfo)
    spt, period = shape.spt, max(1, shape.long_ticks // 4)
    g = ws.build(max_ticks_per_run=shape.long_ticks, flags=flags)
    launches, t0 = [], 0
    for i, n in enumerate(submissions(shape)):
        schedule_gates(g, trigs, t0, n, period)
        for k, s in enumerate(srcs):
            g.write_source(s, noise[k][t0 * spt:(t0 + n) * spt], n)
        g.run_ticks(t0, n)
        launches.append(g.debug_eq_launch())
        w_m, w_c, w_a = want[i]
        what = f"{shape.id} submission {i} ({n} ticks from {t0}, {launches[-1]})"
        for j, amp in enumerate(amps):
            assert_bit_exact(g.read_output(amp, 0, n, True), w_a[j], f"{what}: strip {j} Amplifier")
        assert_bit_exact(g.read_output(mix, 0, n, True), w_m, f"{what}: master")
        assert_bit_exact(g.read_output(mix, 1, n, True), w_c, f"{what}: cue")
        t0 += n
    return launches, g.eq_repair_stats()


def assert_forms(shape, launches, long_form, short_form=None):
    forms = [x["form"] for x in launches]
    want = [long_form, short_form or shape.short, long_form]
    assert forms == want, f"{shape.id}: EqThree launch forms {launches}, table says {want}"


# ------------------------------------------------------------------------------------------------
# 1. the config-2 strip, fused, default flags and the contracted order
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("contract", [False, True], ids=["exact", "contract"])
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_config2_fused_strips_bit_exact(shape, contract):
    launches, stats = run_strips(shape, abi.FLAG_FP_CONTRACT if contract else 0)
    assert_forms(shape, launches, shape.fused)
    print(f"{shape.id} {'contract' if contract else 'exact'}: {launches[0]} {stats}")
    if shape.fused != "sequential":
        assert launches[0]["n_chunks"] >= 2 and launches[0]["chunk"] > 0
        assert stats["chunks_run"] > 0
        # the warm-up is long enough that speculation pays: few boundaries need the repair pass (a warm-up that ignores a negative pole's
        # slow forgetting -- 128 samples at 6 kHz -- had nearly every chunk repaired)
        assert stats["chunks_repaired"] <= stats["chunks_run"] // 8, stats


# ------------------------------------------------------------------------------------------------
# 2. MX_FLAG_NO_FUSE: the standalone Envelope, the scheduled Trigger, the Amplifier with a buffer control
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("segments", ["auto", "4"])
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_config2_unfused_strips_bit_exact(shape, segments, monkeypatch):
    if segments != "auto":
        assert shape.long_ticks * shape.spt >= 2 * 1024        # segments are at least 1 Ki samples: every long submission has some
        monkeypatch.setenv("MX_ENV_SEGMENTS", segments)
    launches, _ = run_strips(shape, abi.FLAG_NO_FUSE)
    assert_forms(shape, launches, shape.unfused, "sequential" if shape.short == "sequential" else shape.unfused)   # (44k1_1: one tick is a long stream)


# ------------------------------------------------------------------------------------------------
# 3. forced kernel variants: they change the path, never a bit
# ------------------------------------------------------------------------------------------------
VARIANTS = {
    "sb16": {"MX_EQ_SPEC_SB": "16"},
    "sb32": {"MX_EQ_SPEC_SB": "32"},
    "sb321": {"MX_EQ_SPEC_SB": "321"},
    "direct": {"MX_EQ_SPEC_DIRECT": "1"},
    "chunks": {"MX_EQ_SPEC_CHUNKS": "3"},         # (44k1_1: 3 chunks are 3 whole ticks -- 2 leave the last one ragged)
    "warm16": {"MX_EQ_SPEC_WARM": "16"},
    "repair_test3": {"MX_EQ_REPAIR_TEST": "3"},
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_forced_eq_variants_change_no_bit(shape, variant, monkeypatch):
    for k, v in VARIANTS[variant].items():
        monkeypatch.setenv(k, "2" if (variant, shape.id) == ("chunks", "44k1_1") else v)
    launches, stats = run_strips(shape)
    print(f"{shape.id} {variant}: {launches[0]} {stats}")
    long = launches[0]
    frames = shape.long_ticks * shape.spt
    if variant.startswith("sb") and long["form"] == "tiled":
        assert long["super_block"] == int(variant[2:]), long
    if variant == "direct":
        assert long["form"] == ("sequential" if shape.fused == "sequential" else "direct"), long
    if variant == "chunks" and long["form"] != "sequential":
        assert long["n_chunks"] in (2, 3) and long["n_chunks"] * long["chunk"] > frames, f"last chunk not ragged: {long}"
    if variant == "warm16" and long["form"] != "sequential":
        assert stats["chunks_repaired"] > 0, stats      # a 16-sample warm-up proves (almost) no boundary: the repair pass does the work
    if variant in ("sb16", "sb32", "sb321", "repair_test3"):
        assert_forms(shape, launches, shape.fused)


@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_amplifier_modulated_by_a_buffer_takes_the_control_tile(shape):
    launches, stats = run_strips(shape, lfo=True)
    print(f"{shape.id} control tile: {launches[0]} {stats}")
    long_form = "sequential" if shape.unfused == "sequential" else "control_tile"
    short = "sequential" if shape.short == "sequential" else None
    assert [x["form"] for x in launches][0::2] == [long_form, long_form], launches
    if short:
        assert launches[1]["form"] == short, launches


# ------------------------------------------------------------------------------------------------
# 4. oscillators (every waveform), FmSine, and config 1 with its Plotter
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hours", [0, 5, *FAR_EPOCHS], ids=["tick0", "5h", *FAR_EPOCHS])
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_oscillators_and_fm_sine_bit_exact(shape, hours):
    sr, tps, spt = shape.sample_rate, shape.ticks_per_second, shape.spt
    T = min(shape.long_ticks, max(1, 8192 // spt))
    ws = Workspace(sr, tps)
    oscs = [ws.oscillator(f, w) for w in (abi.WAVE_SAW, abi.WAVE_TRIANGLE, abi.WAVE_ON, abi.WAVE_OFF, abi.WAVE_SINE, abi.WAVE_SQUARE)
            for f in (97.0, 1234.5)]
    fms = []
    for k in range(3):
        lfo = ws.oscillator(0.5 + 2 * k, abi.WAVE_TRIANGLE)
        fm = ws.fm_sine(110.0 * (k + 1), 150.0 * (k + 1) + 40.0)
        ws.connect(lfo, 0, fm, 0)
        fms.append(fm)
    g = ws.build(max_ticks_per_run=T)
    og = oracle.OracleGraph(ws)
    # (an epoch of tick_shapes.FAR_EPOCHS: the three runs end below 2^31 samples / the first holds sample 2^32 / they start at 2^40)
    tick = far_first_tick(hours, spt, T if hours == "across_2p32" else 2 * T + 1) if isinstance(hours, str) else hours * 3600 * tps
    for n in (T, 1, T):
        g.run_ticks(tick, n)
        got_o = [g.read_output(o, 0, n, False) for o in oscs]
        got_s = [g.read_output(o, 1, n, True) for o in oscs]
        got_f = [g.read_output(f, 0, n, True) for f in fms]
        for kk in range(n):
            og.run_tick(tick + kk)
            for j, o in enumerate(oscs):
                want = og.output(o, 0)
                assert_bit_exact(got_o[j][kk * spt:(kk + 1) * spt], want, f"{shape.id} oscillator {j} tick {tick + kk}")
                assert_bit_exact(got_s[j][kk * 2 * spt:(kk + 1) * 2 * spt], og.output(o, 1), f"{shape.id} oscillator {j} stereo tick {tick + kk}")
            for j, f in enumerate(fms):
                assert_bit_exact(got_f[j][kk * 2 * spt:(kk + 1) * 2 * spt], og.output(f, 0), f"{shape.id} FmSine {j} tick {tick + kk}")
        tick += n


@pytest.mark.parametrize("batch", [1, 12])
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_config1_plotter_fires_every_sixth_call(shape, batch):
    ws, oscs, mix, plot = config1(shape.sample_rate, shape.ticks_per_second)
    spt, n_ticks = shape.spt, 36
    og = oracle.OracleGraph(ws)
    g = ws.build(max_ticks_per_run=batch)
    n_fired = 0
    for t0 in range(0, n_ticks, batch):
        g.run_ticks(t0, batch)
        got_m = g.read_output(mix, 0, batch, True)
        got_c = g.read_output(mix, 1, batch, True)
        for k in range(batch):
            og.run_tick(t0 + k)
            sl = slice(k * 2 * spt, (k + 1) * 2 * spt)
            assert_bit_exact(got_m[sl], og.output(mix, 0), f"{shape.id} master tick {t0 + k}")
            assert_bit_exact(got_c[sl], og.output(mix, 1), f"{shape.id} cue tick {t0 + k}")
            want_p, got_p = og.plotter(plot), g.read_plotter(plot, k)
            assert (want_p is None) == (got_p is None)
            if want_p is not None:
                n_fired += 1
                assert (t0 + k + 1) % 6 == 0 and got_p[0].size == spt and got_p[1].size == spt
                assert_bit_exact(got_p[0], want_p[0], "Plotter left"); assert_bit_exact(got_p[1], want_p[1], "Plotter right")
    assert n_fired == n_ticks // 6


# ------------------------------------------------------------------------------------------------
# 5. the fast scan (MX_FLAG_EQ_FAST) with the time split: spans several times the pre-pass window
# ------------------------------------------------------------------------------------------------
FAST_FRAMES = 3 * 4 * 16384     # per long submission: 4 spans of >= 3 x the longest window (16 Ki samples: 192 kHz, 6 kHz)


def fast_graph(shape, n_inst):
    ws = Workspace(shape.sample_rate, shape.ticks_per_second)
    gains = synth.uniform(82, 3 * n_inst, -24.0, 6.0)
    srcs, eqs = [], []
    for k in range(n_inst):
        s = ws.source_mono(); e = ws.eq_three(*[float(v) for v in gains[3 * k:3 * k + 3]])
        ws.connect(s, 0, e, 0); srcs.append(s); eqs.append(e)
    return ws, srcs, eqs, [tuple(float(v) for v in gains[3 * k:3 * k + 3]) for k in range(n_inst)]


BURST_BEFORE_BOUNDARY = 4000   # samples: beyond a 2 048-sample window, inside the 9 088 samples the 6 kHz high band needs to forget


@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_fast_scan_time_split_within_one_ulp_and_window_equals_full_prepass(shape, monkeypatch):
    n_inst, spt = 2, shape.spt
    T = -(-FAST_FRAMES // spt)
    subs = [T, 1, T]
    frames = T * spt
    never_forgets = abs(1.0 - 2.0 * math.sin(math.pi * 2700.0 / shape.sample_rate)) >= 1.0   # the high pole (5.4 kHz: -1)
    # MX_EQ_SPLIT=4: spans of whole 1 Ki samples where a pre-pass window applies, whole 8 Ki-sample segments for the full pre-pass
    seg = 8192 if never_forgets else 1024
    span = -(-(-(-frames // 4)) // seg) * seg
    ws, srcs, eqs, gains = fast_graph(shape, n_inst)
    noise = [synth.noise(800 + k, sum(subs) * spt) for k in range(n_inst)]
    noise[1] = noise[1].copy(); noise[1][10000:10050] *= np.float32(1e30); noise[1][10050:30000] *= np.float32(1e-30)
    # a burst that a pre-pass window shorter than the forgetting length leaves out of the first span's end state
    b = span - BURST_BEFORE_BOUNDARY
    noise[0] = noise[0].copy(); noise[0][b:b + 50] *= np.float32(1e30)
    monkeypatch.setenv("MX_EQ_SPLIT", "4")
    outs = []
    for full in ("1", "0"):
        monkeypatch.setenv("MX_EQ_FULL_PREPASS", full)
        g = ws.build(max_ticks_per_run=T, flags=abi.FLAG_EQ_FAST)
        res, t0 = [], 0
        for n in subs:
            for k, s in enumerate(srcs):
                g.write_source(s, noise[k][t0 * spt:(t0 + n) * spt], n)
            g.run_ticks(t0, n)
            launch = g.debug_eq_launch()
            assert launch["form"] == "scan"
            if n == T and full == "0":   # the split and the window were used: the burst sits that far before a span boundary
                assert launch["n_chunks"] == -(-frames // span) >= 2 and launch["chunk"] == span, launch
                if never_forgets:
                    assert launch["warm"] == span, launch          # the full pre-pass
                else:
                    assert launch["warm"] < span, launch
                    if shape.id == "6k":
                        assert launch["warm"] > BURST_BEFORE_BOUNDARY, launch   # the window covers the burst
            res.append([g.read_output(e, 0, n, False) for e in eqs])
            t0 += n
        outs.append(res)
    diffs, total = 0, 0
    for k in range(n_inst):
        st = oracle.eq_three_new(shape.sample_rate)
        t0 = 0
        for i, n in enumerate(subs):
            want = oracle.eq_three_run(st, gains[k], noise[k][t0 * spt:(t0 + n) * spt])
            diffs += assert_ulp(outs[1][i][k], want, 1, f"{shape.id} fast scan inst {k} submission {i}")
            total += want.size
            t0 += n
    assert diffs <= max(2, total // 20000), f"{diffs} of {total} samples differ by 1 ULP"
    full = np.concatenate([np.concatenate(r) for r in outs[0]])
    win = np.concatenate([np.concatenate(r) for r in outs[1]])
    bad = np.flatnonzero(full.view(np.uint32) != win.view(np.uint32))
    assert bad.size == 0, f"{shape.id}: windowed pre-pass differs from the full pre-pass on {bad.size} samples, first at {bad[:5]}"


# ------------------------------------------------------------------------------------------------
# 6. random graphs (tests/test_gpu_random_graphs.py's generator)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [3, 17, 40])
@pytest.mark.parametrize("shape", SHAPE_PARAMS)
def test_random_graphs_match_the_oracle(shape, seed):
    ws, sources = random_graph(seed, shape.sample_rate, shape.ticks_per_second)
    spt, T = shape.spt, min(shape.long_ticks, 16)
    og = oracle.OracleGraph(ws)
    order = og.run_order()
    graphs = {"fused": ws.build(max_ticks_per_run=T), "unfused": ws.build(max_ticks_per_run=T, flags=abi.FLAG_NO_FUSE)}
    subs = [T, 1, T]
    data = {n: synth.noise(4100 + 31 * seed + n, sum(subs) * spt * (1 if ty == MONO else 2)) for (n, ty) in sources}
    types = port_types(ws)
    t0 = 0
    for n_t in subs:
        want = {}
        for t in range(t0, t0 + n_t):
            for (n, ty) in sources:
                w = spt * (1 if ty == MONO else 2)
                og.set_source(n, data[n][t * w:(t + 1) * w])
            og.run_tick(t)
            for n in order:
                for p in range(len(types[n])):
                    want.setdefault((n, p), []).append(og.output(n, p))
        for name, g in graphs.items():
            for (n, ty) in sources:
                w = spt * (1 if ty == MONO else 2)
                g.write_source(n, data[n][t0 * w:(t0 + n_t) * w], n_t)
            g.run_ticks(t0, n_t)
            for n in order:
                for p, ty in enumerate(types[n]):
                    try:
                        got = g.read_output(n, p, n_t, ty == STEREO)
                    except abi.MxError as e:
                        assert name != "unfused" and "MX_FLAG_NO_FUSE" in str(e)
                        continue
                    assert_bit_exact(got, np.concatenate(want[(n, p)]), f"{shape.id} seed {seed} {name} ticks {t0}+{n_t}: node {n} port {p}")
        t0 += n_t


# ------------------------------------------------------------------------------------------------
# 7. FIR and resampler where spt * up / down is whole: 441 * 160 / 147 = 480
# ------------------------------------------------------------------------------------------------
def test_fir_and_resampler_at_441_sample_ticks():
    from test_gpu_fir_resample import polyphase_table, reverb_taps
    shape = by_id("44k1_100")
    spt, n_ch, out_spt = shape.spt, 3, 480
    ws = Workspace(shape.sample_rate, shape.ticks_per_second)
    srcs, outs = [], []
    for k in range(n_ch):
        s = ws.source_stereo(); f = ws.fir(reverb_taps(96, seed=40 + k)); r = ws.resample(160, 147, polyphase_table())
        ws.connect(s, 0, f, 0); ws.connect(f, 0, r, 0)
        srcs.append(s); outs.append((f, r))
    g = ws.build(max_ticks_per_run=8)
    og = oracle.OracleGraph(ws)
    subs = [8, 1, 8]
    noise = [synth.noise(90 + k, 2 * spt * sum(subs)) for k in range(n_ch)]
    t0 = 0
    for n in subs:
        for k, s in enumerate(srcs):
            g.write_source(s, noise[k][t0 * 2 * spt:(t0 + n) * 2 * spt], n)
        g.run_ticks(t0, n)
        got = [(g.read_output(f, 0, n, True), g.read_output(r, 0, n, True, rate=(160, 147))) for f, r in outs]
        assert got[0][1].size == n * 2 * out_spt
        for kk in range(n):
            for k, s in enumerate(srcs):
                og.set_source(s, noise[k][(t0 + kk) * 2 * spt:(t0 + kk + 1) * 2 * spt])
            og.run_tick(t0 + kk)
            for k, (f, r) in enumerate(outs):
                assert_bit_exact(got[k][0][kk * 2 * spt:(kk + 1) * 2 * spt], og.output(f, 0), f"FIR {k} tick {t0 + kk}")
                assert_bit_exact(got[k][1][kk * 2 * out_spt:(kk + 1) * 2 * out_spt], og.output(r, 0), f"resampler {k} tick {t0 + kk}")
        t0 += n
    # 441 * 147 / 160 is not whole: refused at build
    ws2 = Workspace(shape.sample_rate, shape.ticks_per_second)
    s = ws2.source_stereo(); r = ws2.resample(147, 160, polyphase_table(147, 160))
    ws2.connect(s, 0, r, 0)
    with pytest.raises(abi.MxError) as e:
        ws2.build()
    assert e.value.code == abi.MX_ERR_INVALID


# ------------------------------------------------------------------------------------------------
# 8. shapes whose tick is not whole samples are refused, not run
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr,tps", INVALID)
def test_invalid_tick_shapes_are_refused(sr, tps):
    ws = Workspace(sr, tps)
    ws.oscillator(440.0, abi.WAVE_SAW)
    with pytest.raises(abi.MxError) as e:
        ws.build()
    assert e.value.code == abi.MX_ERR_INVALID


# ------------------------------------------------------------------------------------------------
# 9. video and ingest at other tick rates: frame expiry, output durations and pacing use 1 / ticks_per_second as an exact rational
# ------------------------------------------------------------------------------------------------
VIDEO_RATES = [pytest.param(48000, 50, id="48k_50"), pytest.param(44100, 30, id="44k1_30")]


@pytest.mark.parametrize("sr,tps", VIDEO_RATES)
def test_video_mixer_cascade_with_frame_durations_ending_between_ticks(sr, tps):
    """Three layers through two cross-fades.  Each layer's frames last 7/100 s, 1/45 s or 3/40 s: at 50 ticks/s 3.5, 1.1 and 3.75 ticks,
    at 30 ticks/s 2.1, 0.67 and 2.25 -- a stored frame expires between ticks, on the tick whose start is at or past its end
    (video_mixer.rs).  The cross-fades hand their output on with a duration of one tick.  Every tick bit for bit against the oracle."""
    spt = sr // tps
    sizes = [(320, 180), (160, 120), (212, 120)]
    durs = [(7, 100), (1, 45), (3, 40)]
    ws, srcs, mixers, rgba = cascade(sizes, MATRIX, sr, tps)
    g = ws.build()
    oms = [ov.OracleVideoMixer(a=0, b=1, fader=FADERS[k], sample_rate=sr) for k in range(len(sizes) - 1)]
    plan = {0: {0: ((320, 180), 1), 1: ((160, 120), 2), 2: ((212, 120), 3)}, 2: {1: ((100, 180), 4)}, 3: {0: ((320, 180), 5), 2: ((212, 120), 6)},
            5: {1: ((160, 120), 7)}, 8: {2: ((300, 100), 8)}}
    keep, n_present = [], 0
    for tick in range(11):
        new = {}
        for k, (size, seed) in plan.get(tick, {}).items():
            hf = ov.HostFrame(*size).fill(k, seed=seed)
            d = upload(hf); keep.append(d)
            video.graph_set_video_source(g, srcs[k], d, dur=durs[k], off=(0, 1), repeat=False)
            new[k] = hf
        g.run_ticks(tick, 1)
        prev = (new[0], durs[0], (0, 1)) if 0 in new else None
        for k in range(len(sizes) - 1):
            b = (new[k + 1], durs[k + 1], (0, 1)) if (k + 1) in new else None
            out = oms[k].run_tick(tick * spt, [prev, b, None, None])
            prev = (out, (1, tps), (0, 1)) if out is not None else None
        want = prev[0] if prev else None
        got = video.graph_rgba_output(g, rgba)
        if want is None:
            assert got is None or got.size == 0, f"tick {tick}: the device shows a picture the oracle does not"
            continue
        n_present += 1
        assert np.array_equal(got, ov.to_rgba(want, MATRIX)), f"{tps} ticks/s, tick {tick}: RGBA differs"
        prog = video.graph_video_output(g, mixers[-1], 0)
        for p, (a, b) in enumerate(zip(prog.download(), want.visible())):
            assert np.array_equal(a, b), f"{tps} ticks/s, tick {tick} plane {p}"
    assert 3 <= n_present <= 10     # pictures come and go: at least one tick where every stored frame has expired


@pytest.mark.parametrize("seed", range(6))
def test_media_source_pacing_at_50_ticks_per_second(seed):
    """MediaSource pacing (presentation times against the tick clock, in 1/50 s ticks of 960 samples) against OMediaSource."""
    sr, tps = 48000, 50
    acts = im.media_scenario(seed, sr=sr)
    got = play_media(AbiMedia(FrameBook(), sr, tps), acts, sr, sr // tps)
    want = play_media(oracle.OMediaSource(sr, tps), acts, sr, sr // tps)
    assert got == want
    assert sum(x is not None for x in want) > 20
