"""The device against the independent numpy model of the reference's audio modules (tests/audio_model.py), directly: no oracle in between.

Every comparison is bit for bit over the cases of tests/audio_cases.py (a NaN of the model accepts any NaN: the reference does not specify an
arithmetic NaN's payload and sign; +-0 is distinguished).  tests/test_cpu_audio_model.py shows that each of audio_model.MIS_MODELS changes a
bit of one of these cases, so a kernel that shared one of those misreadings with the oracle fails here.

  * the module path (abi.Module.run_tick): every single-module case at both rates, Envelope and EqThree state carried across calls, the
    cooperative Mixer also with the streaming kernel forced;
  * the graph path (Workspace.build): the Envelope, Amplifier, Oscillator, FmSine and one-tick Mixer cases, in one multi-tick submission and
    in one-tick submissions;
  * the config-2 strips on the graph path under default flags (the fused strip kernel with the inline Envelope and Amplifier),
    FLAG_NO_FUSE (every intermediate port compared) and FLAG_EQ_EXACT, in submissions of 1 and 4 ticks, at both rates, from tick 0 and
    across sample time 2^32.

The model's runs are computed once per process (audio_cases.model) and shared.  The contracted order and FLAG_EQ_FAST are specified as
"<= 1 ULP of the exact order" and stay pinned where they are.
"""
import numpy as np
import pytest

import audio_cases as ac
import audio_model as am
from audio_cases import assert_same_bits
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

WAVE = {name: k for k, name in enumerate(am.WAVES)}
assert (abi.WAVE_ON, abi.WAVE_OFF, abi.WAVE_SINE, abi.WAVE_SQUARE, abi.WAVE_TRIANGLE, abi.WAVE_SAW) == tuple(WAVE[w] for w in am.WAVES)
F32 = np.float32
SUBMISSIONS = ["whole", "ticked"]          # one multi-tick submission / one-tick submissions


def by_id(cases):
    return pytest.mark.parametrize("case", cases, ids=[c.id for c in cases])


def line(kind, a):
    return (kind if a is not None else abi.MX_DISCONNECTED, a)


def mixer_params(channels):
    return [abi.MixerChannelParams(g, f, 1 if c else 0) for g, f, c in channels]


# ------------------------------------------------------------------------------------------------
# the module path
# ------------------------------------------------------------------------------------------------
@by_id(ac.ENVELOPE)
def test_module_envelope_equals_the_model(case):
    m = abi.Module(abi.KIND_ENVELOPE, abi.EnvelopeParams(*case.params), sample_rate=case.sr)
    got, o = np.empty(case.gate.size, F32), 0
    for n in case.calls:                                            # the state is carried from call to call
        m.run_tick(case.t0 + o, [(abi.MX_MONO, case.gate[o:o + n])], [(abi.MX_MONO, got[o:o + n])]); o += n
    assert_same_bits(got, ac.model("envelope", case), f"Envelope {case.id}")


# every case under the default kernel choice; the case that takes the cooperative kernel also with the streaming kernel forced (the switch of
# test_gpu_audio_parity.test_mixer_bit_exact)
MIXER_RUNS = [pytest.param(c, "512", id=c.id) for c in ac.MIXER] + [pytest.param(c, "0", id=c.id + "-streaming-forced") for c in ac.MIXER if c.coop]
assert len(MIXER_RUNS) > len(ac.MIXER)


@pytest.mark.parametrize("case,coop_blocks", MIXER_RUNS)
def test_module_mixer_equals_the_model(case, coop_blocks, monkeypatch):
    monkeypatch.setenv("MX_MIXER_COOP_BLOCKS", coop_blocks)
    want_m, want_c = ac.model("mixer", case)
    m = abi.Module(abi.KIND_MIXER, mixer_params(case.channels))
    got_m, got_c = np.empty(case.length, F32), np.empty(case.length, F32)
    m.run_tick(0, [line(abi.MX_STEREO, a) for a in case.inputs], [(abi.MX_STEREO, got_m), (abi.MX_STEREO, got_c)])
    assert_same_bits(got_m, want_m, f"Mixer {case.id} master")
    assert_same_bits(got_c, want_c, f"Mixer {case.id} cue")


@by_id(ac.AMPLIFIER)
def test_module_amplifier_equals_the_model(case):
    m = abi.Module(abi.KIND_AMPLIFIER, abi.AmplifierParams(case.amplitude, case.depth), sample_rate=case.sr)
    got = np.empty_like(case.x)
    m.run_tick(0, [(abi.MX_STEREO, case.x), line(abi.MX_MONO, case.ctl)], [(abi.MX_STEREO, got)])
    assert_same_bits(got, ac.model("amplifier", case), f"Amplifier {case.id}")


@by_id(ac.OSCILLATOR)
def test_module_oscillator_equals_the_model(case):
    want = ac.model("oscillator", case)
    m = abi.Module(abi.KIND_OSCILLATOR, abi.OscillatorParams(case.freq, WAVE[case.wave], 0), sample_rate=case.sr)
    mono, stereo = np.empty(case.spt, F32), np.empty(2 * case.spt, F32)
    m.run_tick(case.first_tick * case.spt, [], [(abi.MX_MONO, mono), (abi.MX_STEREO, stereo)])
    assert_same_bits(mono, want, f"Oscillator {case.id}")
    assert_same_bits(stereo, np.repeat(want, 2), f"Oscillator {case.id} stereo")


@by_id(ac.FM_SINE)
def test_module_fm_sine_equals_the_model(case):
    m = abi.Module(abi.KIND_FM_SINE, abi.FmSineParams(case.freq_lo, case.freq_hi), sample_rate=case.sr)
    got = np.empty(2 * case.spt, F32)
    m.run_tick(case.first_tick * case.spt, [line(abi.MX_MONO, case.x)], [(abi.MX_STEREO, got)])
    assert_same_bits(got, ac.model("fm_sine", case), f"FmSine {case.id}")


_EQ = {}


def eq_model(sr, spt, gains):
    if (sr, gains) not in _EQ:
        _EQ[sr, gains] = ac.model_eq_three(sr, spt, gains)
    return _EQ[sr, gains]


@pytest.mark.parametrize("flags", [0, abi.FLAG_EQ_EXACT], ids=["default", "eq-exact"])
@pytest.mark.parametrize("rate", ac.RATES, ids=["44k1", "48k"])
@pytest.mark.parametrize("gains", ac.EQ_GAINS)
def test_module_eq_three_equals_the_model(gains, rate, flags):
    sr, spt = rate
    x = ac.eq_input(spt)
    m = abi.Module(abi.KIND_EQ_THREE, abi.EqThreeParams(*gains), sample_rate=sr, flags=flags)
    got = np.empty_like(x)
    for k in range(ac.EQ_TICKS):                                    # the state is carried from tick to tick
        m.run_tick(k * spt, [(abi.MX_MONO, x[k * spt:(k + 1) * spt])], [(abi.MX_MONO, got[k * spt:(k + 1) * spt])])
    assert_same_bits(got, eq_model(sr, spt, gains), f"EqThree {gains}")


@pytest.mark.parametrize("rate", ac.RATES, ids=["44k1", "48k"])
def test_module_trigger_panner_splitter_equal_the_model(rate):
    sr, spt = rate
    for gate_open in (True, False):
        got = np.empty(spt, F32)
        abi.Module(abi.KIND_TRIGGER, abi.TriggerParams(int(gate_open)), sample_rate=sr).run_tick(0, [], [(abi.MX_MONO, got)])
        assert_same_bits(got, am.trigger(gate_open, spt), f"Trigger {gate_open}")
    xl, xr, xs = ac.synth.noise(41, spt).copy(), ac.synth.noise(42, spt), ac.synth.noise(43, 2 * spt)
    xl[3] = -0.0; xl[4] = F32(1e-42)                                # a shuffle keeps every bit
    for left, right in ((xl, xr), (None, xr), (xl, None)):
        got = np.empty(2 * spt, F32)
        abi.Module(abi.KIND_STEREO_PANNER, sample_rate=sr).run_tick(0, [line(abi.MX_MONO, left), line(abi.MX_MONO, right)], [(abi.MX_STEREO, got)])
        assert_same_bits(got, am.stereo_panner(left, right, spt), f"StereoPanner L {left is not None} R {right is not None}")
    for x in (xs, None):
        l, r = np.empty(spt, F32), np.empty(spt, F32)
        abi.Module(abi.KIND_STEREO_SPLITTER, sample_rate=sr).run_tick(0, [line(abi.MX_STEREO, x)], [(abi.MX_MONO, l), (abi.MX_MONO, r)])
        want = am.stereo_splitter(x, spt)
        assert_same_bits(l, want[0], "StereoSplitter left"); assert_same_bits(r, want[1], "StereoSplitter right")


# ------------------------------------------------------------------------------------------------
# the graph path
# ------------------------------------------------------------------------------------------------
def run_graph(ws, submission, first_tick, n_ticks, sources, reads):
    """sources: {node: (samples of the whole stretch, floats per tick)}; reads: [(node, port, stereo)] -> [samples of the whole stretch]"""
    batch = n_ticks if submission == "whole" else 1
    g = ws.build(max_ticks_per_run=batch)
    out = [[] for _ in reads]
    for t0 in range(0, n_ticks, batch):
        for node, (x, per_tick) in sources.items():
            g.write_source(node, x[t0 * per_tick:(t0 + batch) * per_tick], batch)
        g.run_ticks(first_tick + t0, batch)
        for o, (node, port, stereo) in zip(out, reads):
            o.append(g.read_output(node, port, batch, stereo))
    g.close()
    return [np.concatenate(o) for o in out]


@pytest.mark.parametrize("submission", SUBMISSIONS)
@by_id([c for c in ac.ENVELOPE if c.whole_ticks])
def test_graph_envelope_equals_the_model(case, submission):
    ws = Workspace(case.sr, 60)
    src, env = ws.source_mono(), ws.envelope(*case.params)
    ws.connect(src, 0, env, 0)
    got, = run_graph(ws, submission, case.first_tick, len(case.calls), {src: (case.gate, case.spt)}, [(env, 0, False)])
    assert_same_bits(got, ac.model("envelope", case), f"Envelope {case.id}, {submission}")


@pytest.mark.parametrize("submission", SUBMISSIONS)
@by_id(ac.AMPLIFIER)
def test_graph_amplifier_equals_the_model(case, submission):
    ws = Workspace(case.sr, 60)
    src, amp = ws.source_stereo(), ws.amplifier(case.amplitude, case.depth)
    ws.connect(src, 0, amp, 0)
    sources = {src: (case.x, 2 * case.spt)}
    if case.ctl is not None:
        ctl = ws.source_mono()
        ws.connect(ctl, 0, amp, 1)
        sources[ctl] = (case.ctl, case.spt)
    got, = run_graph(ws, submission, 0, case.n_ticks, sources, [(amp, 0, True)])
    assert_same_bits(got, ac.model("amplifier", case), f"Amplifier {case.id}, {submission}")


def run_one_tick_of(ws, submission, first_tick, spt, sources, reads):
    """The case is ONE tick.  ticked: that tick alone.  whole: a two-tick submission that holds it (the tick before it, or after tick 0, beside it, its
    sources silent), of which the case's tick is compared: the tick's offset inside a run then counts."""
    if submission == "ticked":
        return run_graph(ws, submission, first_tick, 1, sources, reads)
    at = 1 if first_tick > 0 else 0
    padded = {}
    for node, (x, per_tick) in sources.items():
        buf = np.zeros(2 * per_tick, F32); buf[at * per_tick:(at + 1) * per_tick] = x
        padded[node] = (buf, per_tick)
    got = run_graph(ws, "whole", first_tick - at, 2, padded, reads)
    return [v[at * (v.size // 2):(at + 1) * (v.size // 2)] for v in got]


@pytest.mark.parametrize("submission", SUBMISSIONS)
@by_id(ac.OSCILLATOR)
def test_graph_oscillator_equals_the_model(case, submission):
    want = ac.model("oscillator", case)
    ws = Workspace(case.sr, 60)
    osc = ws.oscillator(case.freq, WAVE[case.wave])
    mono, stereo = run_one_tick_of(ws, submission, case.first_tick, case.spt, {}, [(osc, 0, False), (osc, 1, True)])
    assert_same_bits(mono, want, f"Oscillator {case.id}, {submission}")
    assert_same_bits(stereo, np.repeat(want, 2), f"Oscillator {case.id} stereo, {submission}")


@pytest.mark.parametrize("submission", SUBMISSIONS)
@by_id(ac.FM_SINE)
def test_graph_fm_sine_equals_the_model(case, submission):
    ws = Workspace(case.sr, 60)
    fm = ws.fm_sine(case.freq_lo, case.freq_hi)
    sources = {}
    if case.x is not None:
        src = ws.source_mono()
        ws.connect(src, 0, fm, 0)
        sources[src] = (case.x, case.spt)
    got, = run_one_tick_of(ws, submission, case.first_tick, case.spt, sources, [(fm, 0, True)])
    assert_same_bits(got, ac.model("fm_sine", case), f"FmSine {case.id}, {submission}")


@by_id([c for c in ac.MIXER if c.graph])
def test_graph_mixer_equals_the_model(case):
    sr, spt = case.graph
    assert case.length == 2 * spt
    ws = Workspace(sr, 60)
    mix = ws.mixer(case.channels)
    sources = {}
    for k, x in enumerate(case.inputs):
        if x is not None:                                            # a Disconnected input: no edge
            src = ws.source_stereo()
            ws.connect(src, 0, mix, k)
            sources[src] = (x, 2 * spt)
    want_m, want_c = ac.model("mixer", case)
    got_m, got_c = run_graph(ws, "whole", 0, 1, sources, [(mix, 0, True), (mix, 1, True)])
    assert_same_bits(got_m, want_m, f"Mixer {case.id} master")
    assert_same_bits(got_c, want_c, f"Mixer {case.id} cue")


# ------------------------------------------------------------------------------------------------
# the config-2 strips: fused (the default), unfused, FLAG_EQ_EXACT
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [1, ac.STRIP_TICKS], ids=["1-tick", "4-ticks"])
@pytest.mark.parametrize("flags", [0, abi.FLAG_NO_FUSE, abi.FLAG_EQ_EXACT], ids=["default", "no-fuse", "eq-exact"])
@by_id(ac.STRIPS)
def test_graph_strips_equal_the_model(case, flags, batch):
    want = ac.model("strip", case)
    spt = case.spt
    ws, mix, nodes = ac.strip_workspace(case)
    g = ws.build(max_ticks_per_run=batch, flags=flags)
    # fused, a strip keeps its Amplifier's port alone (the others are folded into the strip kernel and not readable); unfused, every port
    ports = ("trigger", "envelope", "eq", "panner", "amplifier") if flags & abi.FLAG_NO_FUSE else ("amplifier",)
    if not flags & abi.FLAG_NO_FUSE:
        with pytest.raises(abi.MxError):                             # the strip kernel is what runs: the EqThree's own port does not exist
            g.read_output(nodes[0]["eq"], 0, 1, False)
    for t0 in range(0, ac.STRIP_TICKS, batch):
        for s, nd in enumerate(nodes):
            g.update_params(nd["trigger"], abi.TriggerParams(int(case.gates[t0][s])))
            for k in range(t0 + 1, t0 + batch):                      # the Trigger's parameter of every later tick of the run, changed or not
                g.schedule_params(nd["trigger"], k - t0, abi.TriggerParams(int(case.gates[k][s])))
            g.write_source(nd["source"], case.sources[s][t0 * spt:(t0 + batch) * spt], batch)
        g.run_ticks(case.first_tick + t0, batch)
        what = f"{case.id} ticks {t0}..{t0 + batch - 1}"
        assert_same_bits(g.read_output(mix, 0, batch, True), want["master"][2 * t0 * spt:2 * (t0 + batch) * spt], f"{what}: Master")
        assert_same_bits(g.read_output(mix, 1, batch, True), want["cue"][2 * t0 * spt:2 * (t0 + batch) * spt], f"{what}: Cue")
        for s, nd in enumerate(nodes):
            for name in ports:
                stereo = name in ac.STEREO_PORTS
                w = 2 if stereo else 1
                assert_same_bits(g.read_output(nd[name], 0, batch, stereo), want[name][s][w * t0 * spt:w * (t0 + batch) * spt], f"{what} strip {s}: {name}")
    g.close()
