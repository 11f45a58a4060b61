"""GPU parity: hand-written HIP kernels (through the C ABI) vs the CPU oracle on the same seeded inputs.

Bars: bit-exact for every module whose arithmetic order is preserved (Mixer, EqThree exact mode,
Envelope, Amplifier, shuffles, every oscillator waveform, FmSine -- the f32 of a sine is made independent of whose libm computed
the f64 sine: mixlab_amd/csrc/mx_sin_f32.hpp); <= 1 ULP only for the opt-in modes that change the order of operations.

Everything except EqThree is unpinned by reference tests: the oracle restates the
reference source and these tests are only as good as that restatement.
"""
import pathlib

import numpy as np
import pytest

import oracle
import synth
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
SR = 44100
SPT = 735
# The reference is compile-time 44 100 Hz (src/engine.rs:53); BASELINE configs[1] is quoted at 48 000 Hz.  Everything whose
# arithmetic depends on SAMPLE_RATE -- 2 sin(pi fc / SR) (eq_three.rs:113-115), ms = dt / SR * 1000 (envelope.rs:16-18),
# t / SR (oscillator.rs:77, fm_sine.rs:47) -- is checked against the oracle at BOTH rates.
RATES = [pytest.param((44100, 735), id="44k1"), pytest.param((48000, 800), id="48k")]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def assert_bit_exact(got, want, what=""):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size}/{got.size} samples differ, first at {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"


def assert_ulp(got, want, max_ulp, what=""):
    d = synth.ulp_diff(got, want)
    assert d.max() <= max_ulp, f"{what}: max {d.max()} ULP (> {max_ulp}); {np.count_nonzero(d)} / {d.size} samples differ"
    return int(np.count_nonzero(d))


# ------------------------------------------------------------------------------------------------
# the reference's own golden vectors (src/module/eq_three.rs:150-167), through the device
# ------------------------------------------------------------------------------------------------
def _golden():
    x = np.fromfile(GOLDEN / "eq_three_chronos_prefix131072.f32.raw", dtype="<f4")
    y = np.fromfile(GOLDEN / "eq_three_chronos-eq_prefix131072.f32.raw", dtype="<f4")
    return x, y


def test_eq_three_reference_golden_one_call_exact_mode():
    x, y = _golden()
    m = abi.Module(abi.KIND_EQ_THREE, abi.EqThreeParams(4.0, 0.0, 4.0), flags=abi.FLAG_EQ_EXACT)
    out = np.zeros_like(x)
    m.run_tick(0, [(abi.MX_MONO, x)], [(abi.MX_MONO, out)])
    assert_bit_exact(out, y, "EqThree golden, one call")


def test_eq_three_reference_golden_ticked_state_carry_exact_mode():
    x, y = _golden()
    n_ticks = 64
    m = abi.Module(abi.KIND_EQ_THREE, abi.EqThreeParams(4.0, 0.0, 4.0), flags=abi.FLAG_EQ_EXACT)
    out = np.zeros(n_ticks * SPT, dtype=np.float32)
    for k in range(n_ticks):
        m.run_tick(k * SPT, [(abi.MX_MONO, x[k * SPT:(k + 1) * SPT])], [(abi.MX_MONO, out[k * SPT:(k + 1) * SPT])])
    assert_bit_exact(out, y[: n_ticks * SPT], "EqThree golden, 735-sample ticks")


def test_eq_three_reference_golden_default_flags_bit_exact():
    # the reference's own test (eq_three.rs:150-167: `assert!(output == expected_output)`) through the drop-in's defaults
    x, y = _golden()
    m = abi.Module(abi.KIND_EQ_THREE, abi.EqThreeParams(4.0, 0.0, 4.0))
    out = np.zeros_like(x)
    m.run_tick(0, [(abi.MX_MONO, x)], [(abi.MX_MONO, out)])
    assert_bit_exact(out, y, "EqThree golden, default flags")


def test_eq_three_reference_golden_fast_mode_within_one_ulp():
    x, y = _golden()
    m = abi.Module(abi.KIND_EQ_THREE, abi.EqThreeParams(4.0, 0.0, 4.0), flags=abi.FLAG_EQ_FAST)
    out = np.zeros_like(x)
    m.run_tick(0, [(abi.MX_MONO, x)], [(abi.MX_MONO, out)])
    assert_ulp(out, y, 1, "EqThree golden, opt-in time-parallel mode")


# ------------------------------------------------------------------------------------------------
# per-module parity through mx_module_run_tick (the ModuleT::run_tick surface)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_ch,length", [(1, 2 * SPT), (4, 2 * SPT), (37, 2 * SPT), (256, 2 * 800), (3, 2 * 733),
                                         (200, 2 * SPT), (129, 2 * 733), (1031, 2 * 70)])   # >= 128 channels on short streams: k_mixer_coop, ragged batches
@pytest.mark.parametrize("coop_blocks", ["512", "0"])   # default kernel choice / streaming kernel forced
def test_mixer_bit_exact(n_ch, length, coop_blocks, monkeypatch):
    monkeypatch.setenv("MX_MIXER_COOP_BLOCKS", coop_blocks)
    gains = synth.uniform(1, n_ch, -24.0, 6.0)
    faders = synth.uniform(2, n_ch, 0.0, 1.0)
    chans = [(float(gains[i]), float(faders[i]), i % 3 == 1) for i in range(n_ch)]
    ins = [synth.noise(100 + i, length) for i in range(n_ch)]
    if n_ch > 2:
        ins[2] = None  # Disconnected input reads the zero buffer (src/engine/io.rs:45-52)
    want_m, want_c = oracle.mixer_run(chans, ins, length)
    m = abi.Module(abi.KIND_MIXER, [abi.MixerChannelParams(g, f, 1 if c else 0) for g, f, c in chans])
    got_m = np.empty(length, np.float32)
    got_c = np.empty(length, np.float32)
    m.run_tick(0, [(abi.MX_STEREO if a is not None else abi.MX_DISCONNECTED, a) for a in ins],
               [(abi.MX_STEREO, got_m), (abi.MX_STEREO, got_c)])
    assert_bit_exact(got_m, want_m, "Mixer master")
    assert_bit_exact(got_c, want_c, "Mixer cue")


def test_mixer_default_channels_are_silent():
    # MixerChannelParams::default has fader 0.0 (protocol/src/lib.rs:342-347)
    ins = [synth.noise(7, 2 * SPT), synth.noise(8, 2 * SPT)]
    m = abi.Module(abi.KIND_MIXER, [abi.MixerChannelParams(0.0, 0.0, 0)] * 2)
    got_m = np.ones(2 * SPT, np.float32)
    got_c = np.ones(2 * SPT, np.float32)
    m.run_tick(0, [(abi.MX_STEREO, a) for a in ins], [(abi.MX_STEREO, got_m), (abi.MX_STEREO, got_c)])
    assert not got_m.any() and not got_c.any()


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("gains", [(4.0, 0.0, 4.0), (-24.0, 6.0, -3.5), (0.0, 0.0, 0.0)])
def test_eq_three_exact_vs_oracle_with_state(gains, rate):
    SR, SPT = rate
    x = synth.noise(11, 40 * SPT)
    st = oracle.eq_three_new(SR)
    want = oracle.eq_three_run(st, gains, x)
    m = abi.Module(abi.KIND_EQ_THREE, abi.EqThreeParams(*gains), sample_rate=SR, flags=abi.FLAG_EQ_EXACT)
    got = np.empty_like(x)
    for k in range(40):
        m.run_tick(k * SPT, [(abi.MX_MONO, x[k * SPT:(k + 1) * SPT])], [(abi.MX_MONO, got[k * SPT:(k + 1) * SPT])])
    assert_bit_exact(got, want, "EqThree exact")


def test_eq_three_disconnected_input():
    st = oracle.eq_three_new(SR)
    want = oracle.eq_three_run(st, (3.0, -2.0, 1.0), np.zeros(SPT, np.float32))
    m = abi.Module(abi.KIND_EQ_THREE, abi.EqThreeParams(3.0, -2.0, 1.0), flags=abi.FLAG_EQ_EXACT)
    got = np.empty(SPT, np.float32)
    m.run_tick(0, [(abi.MX_DISCONNECTED, None)], [(abi.MX_MONO, got)])
    assert_bit_exact(got, want, "EqThree disconnected")


def _gate_patterns():
    n = 12 * SPT
    pats = {}
    g = np.zeros(n, np.float32); g[100:3000] = 1.0; g[5000:5010] = 1.0; g[7000:] = 1.0
    pats["blocks"] = g
    g = synth.noise(5, n).copy(); g[::97] = 1.0; g[50::131] = 0.0            # markers sprinkled in noise
    pats["sprinkled"] = g
    g = np.full(n, 0.5, np.float32); g[63] = 1.0; g[64] = 0.0; g[127] = 1.0; g[128] = 1.0; g[191] = 0.0  # wave-boundary edges
    pats["boundaries"] = g
    pats["always_on"] = np.ones(n, np.float32)
    pats["never"] = np.full(n, 0.25, np.float32)
    g = np.zeros(n, np.float32); g[1::2] = 1.0
    pats["alternating"] = g
    return pats


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("name", list(_gate_patterns().keys()))
@pytest.mark.parametrize("params", [(25.0, 500.0, 0.8, 200.0), (1.0, 10.0, 0.3, 5.0)])
def test_envelope_bit_exact(name, params, rate):
    SR, SPT = rate
    gate = _gate_patterns()[name]
    n_ticks = gate.size // SPT
    st = oracle.EnvState()
    want = np.concatenate([oracle.envelope_run(st, params, SR, k * SPT, gate[k * SPT:(k + 1) * SPT], SPT) for k in range(n_ticks)])
    m = abi.Module(abi.KIND_ENVELOPE, abi.EnvelopeParams(*params), sample_rate=SR)
    got = np.empty_like(want)
    for k in range(n_ticks):
        m.run_tick(k * SPT, [(abi.MX_MONO, gate[k * SPT:(k + 1) * SPT])], [(abi.MX_MONO, got[k * SPT:(k + 1) * SPT])])
    assert_bit_exact(got, want, f"Envelope {name}")


@pytest.mark.parametrize("ctl_connected", [True, False])
@pytest.mark.parametrize("amp,depth", [(1.0, 0.5), (0.7, 0.1), (2.0, 1.0), (1.0, 0.0)])
def test_amplifier_bit_exact(ctl_connected, amp, depth):
    x = synth.noise(21, 2 * SPT)
    ctl = synth.noise(22, SPT) if ctl_connected else None
    want = oracle.amplifier_run(amp, depth, x, ctl)
    m = abi.Module(abi.KIND_AMPLIFIER, abi.AmplifierParams(amp, depth))
    got = np.empty_like(x)
    m.run_tick(0, [(abi.MX_STEREO, x), (abi.MX_MONO if ctl_connected else abi.MX_DISCONNECTED, ctl)], [(abi.MX_STEREO, got)])
    assert_bit_exact(got, want, "Amplifier")


@pytest.mark.parametrize("wave,exact", [(abi.WAVE_SAW, True), (abi.WAVE_TRIANGLE, True), (abi.WAVE_ON, True), (abi.WAVE_OFF, True),
                                        (abi.WAVE_SINE, True), (abi.WAVE_SQUARE, True)])   # Sine: Ziv's strategy (mx_sin_f32.hpp); Square: exact sign of sin on the device
@pytest.mark.parametrize("freq,tick", [(100.0, 0), (440.0, 1000), (880.5, 216000)])
@pytest.mark.parametrize("rate", RATES)
def test_oscillator(wave, exact, freq, tick, rate):
    SR, SPT = rate
    t = tick * SPT
    want_m, want_s = oracle.oscillator_run(freq, wave, SR, t, SPT)
    m = abi.Module(abi.KIND_OSCILLATOR, abi.OscillatorParams(freq, wave, 0), sample_rate=SR)
    got_m = np.empty(SPT, np.float32)
    got_s = np.empty(2 * SPT, np.float32)
    m.run_tick(t, [], [(abi.MX_MONO, got_m), (abi.MX_STEREO, got_s)])
    assert_bit_exact(got_s[0::2], got_m, "stereo L == mono")
    assert_bit_exact(got_s[1::2], got_m, "stereo R == mono")
    if exact:
        assert_bit_exact(got_m, want_m, "Oscillator")
    else:
        assert_ulp(got_m, want_m, 1, "Oscillator sine (device sin vs host libm)")


@pytest.mark.parametrize("tick", [0, 5000])
@pytest.mark.parametrize("rate", RATES)
def test_fm_sine(tick, rate):
    SR, SPT = rate
    t = tick * SPT
    x = synth.noise(31, SPT)
    want = oracle.fm_sine_run(220.0, 880.0, SR, t, x, SPT)
    m = abi.Module(abi.KIND_FM_SINE, abi.FmSineParams(220.0, 880.0), sample_rate=SR)
    got = np.empty(2 * SPT, np.float32)
    m.run_tick(t, [(abi.MX_MONO, x)], [(abi.MX_STEREO, got)])
    assert_bit_exact(got, want, "FmSine")


@pytest.mark.parametrize("mode", ["0", "2"], ids=["ziv", "double-double-everywhere"])
def test_sine_and_fm_sine_over_a_long_stretch_are_the_oracles_bits(mode, monkeypatch):
    """1.5 M sines per module kind: 16 Sine oscillators (27.5 Hz .. 19 kHz) and 16 FmSines over 60 ticks starting five hours into the clock (arguments up to 2e9 rad) in
    one batched graph, bit for bit against the oracle's (float)glibc_sin.  MX_SIN_MODE=2 runs the double-double path on EVERY sample: the rare path of the default
    is then the one under test.  (The residual the design admits -- the real sine within glibc's own error of a rounding boundary -- is ~2 in 10^9.)"""
    monkeypatch.setenv("MX_SIN_MODE", mode)
    n_ticks, tick0 = 60, 5 * 3600 * 60
    ws = Workspace(SR, 60)
    freqs = [27.5 * (19000.0 / 27.5) ** (k / 15.0) for k in range(16)]
    oscs = [ws.oscillator(f, abi.WAVE_SINE) for f in freqs]
    fms = []
    for k in range(16):
        lfo = ws.oscillator(0.5 + k, abi.WAVE_TRIANGLE)
        fm = ws.fm_sine(110.0 * (k + 1), 110.0 * (k + 1) + 80.0 * k)      # (freq_lo, freq_hi): mid + amp * in, fm_sine.rs:41-45
        ws.connect(lfo, 0, fm, 0)
        fms.append(fm)
    g = ws.build(max_ticks_per_run=n_ticks)
    og = oracle.OracleGraph(ws)
    g.run_ticks(tick0, n_ticks)
    got_o = [g.read_output(o, 0, n_ticks, False) for o in oscs]
    got_f = [g.read_output(f, 0, n_ticks, True) for f in fms]
    for k in range(n_ticks):
        og.run_tick(tick0 + k)
        for j, o in enumerate(oscs):
            assert_bit_exact(got_o[j][k * SPT:(k + 1) * SPT], og.output(o, 0), f"Sine {freqs[j]:.1f} Hz tick {k}")
        for j, f in enumerate(fms):
            assert_bit_exact(got_f[j][k * 2 * SPT:(k + 1) * 2 * SPT], og.output(f, 0), f"FmSine {j} tick {k}")


def test_trigger_panner_splitter_exact():
    for gate_open in (True, False):
        m = abi.Module(abi.KIND_TRIGGER, abi.TriggerParams(1 if gate_open else 0))
        got = np.empty(SPT, np.float32)
        m.run_tick(0, [], [(abi.MX_MONO, got)])
        assert (got == (1.0 if gate_open else 0.0)).all()
    l, r = synth.noise(41, SPT), synth.noise(42, SPT)
    m = abi.Module(abi.KIND_STEREO_PANNER)
    st = np.empty(2 * SPT, np.float32)
    m.run_tick(0, [(abi.MX_MONO, l), (abi.MX_MONO, r)], [(abi.MX_STEREO, st)])
    assert_bit_exact(st[0::2], l); assert_bit_exact(st[1::2], r)
    m = abi.Module(abi.KIND_STEREO_SPLITTER)
    l2, r2 = np.empty(SPT, np.float32), np.empty(SPT, np.float32)
    m.run_tick(0, [(abi.MX_STEREO, st)], [(abi.MX_MONO, l2), (abi.MX_MONO, r2)])
    assert_bit_exact(l2, l); assert_bit_exact(r2, r)
    # panner with R disconnected
    m = abi.Module(abi.KIND_STEREO_PANNER)
    m.run_tick(0, [(abi.MX_MONO, l), (abi.MX_DISCONNECTED, None)], [(abi.MX_STEREO, st)])
    assert_bit_exact(st[0::2], l); assert not st[1::2].any()


def test_plotter_fires_every_sixth_call():
    m = abi.Module(abi.KIND_PLOTTER)
    x = synth.noise(51, 2 * SPT)
    ind = np.empty(2 * SPT, np.float32)
    fired = []
    for k in range(13):
        n = m.run_tick(k * SPT, [(abi.MX_STEREO, x)], [], ind)
        fired.append(n > 0)
        if n:
            assert n == 2 * SPT * 4
            assert_bit_exact(ind[:SPT], x[0::2]); assert_bit_exact(ind[SPT:], x[1::2])
    assert fired == [(k + 1) % 6 == 0 for k in range(13)]   # first fires on the 6th call (plotter.rs:38-40)


def test_type_mismatch_is_reported_not_crashed():
    m = abi.Module(abi.KIND_EQ_THREE, abi.EqThreeParams(0, 0, 0))
    with pytest.raises(abi.MxError) as e:
        m.run_tick(0, [(abi.MX_STEREO, np.zeros(2 * SPT, np.float32))], [(abi.MX_MONO, np.zeros(SPT, np.float32))])
    assert e.value.code == abi.MX_ERR_TYPE   # the reference panics here (src/engine/io.rs:40-41)


# ------------------------------------------------------------------------------------------------
# graphs (Engine::run_tick): SURVEY.md section 8d configs 1 and 2
# ------------------------------------------------------------------------------------------------
def config1(sr=SR, tps=60):
    ws = Workspace(sr, tps)
    oscs = [ws.oscillator(100.0, abi.WAVE_SINE), ws.oscillator(220.0, abi.WAVE_SAW),
            ws.oscillator(440.0, abi.WAVE_SQUARE), ws.oscillator(880.0, abi.WAVE_TRIANGLE)]
    mix = ws.mixer([(0.0, 1.0, False), (-6.0, 0.8, True), (3.0, 0.5, False), (-12.0, 0.25, True)])
    plot = ws.plotter()
    for i, o in enumerate(oscs):
        ws.connect(o, 1, mix, i)
    ws.connect(mix, 0, plot, 0)
    return ws, oscs, mix, plot


@pytest.mark.parametrize("batch", [1, 12])
def test_config1_four_osc_mixer_plotter(batch):
    """SURVEY 8d config 1 (BASELINE.json configs[0]), all 600 ticks, BIT-EXACT: Saw, Triangle, Square (exact sign of sin) and -- since round 6 -- Sine (Ziv's
    strategy, mx_sin_f32.hpp) are the oracle's bits, so both buses and the Plotter indication are."""
    ws, oscs, mix, plot = config1()
    n_ticks = 600
    og = oracle.OracleGraph(ws)
    g = ws.build(max_ticks_per_run=batch)
    assert g.run_order() == og.run_order()
    n_fired = 0
    for t0 in range(0, n_ticks, batch):
        g.run_ticks(t0, batch)
        got_m = g.read_output(mix, 0, batch, True)
        got_c = g.read_output(mix, 1, batch, True)
        for k in range(batch):
            og.run_tick(t0 + k)
            sl = slice(k * 2 * SPT, (k + 1) * 2 * SPT)
            wm, wc = og.output(mix, 0), og.output(mix, 1)
            assert_bit_exact(got_c[sl], wc, f"Cue tick {t0 + k}")
            assert_bit_exact(got_m[sl], wm, f"Master tick {t0 + k}")
            want_p = og.plotter(plot)
            got_p = g.read_plotter(plot, k)
            assert (want_p is None) == (got_p is None)
            if want_p is not None:
                n_fired += 1
                assert (t0 + k + 1) % 6 == 0
                assert_bit_exact(got_p[0], want_p[0], "Plotter left vs oracle"); assert_bit_exact(got_p[1], want_p[1], "Plotter right vs oracle")
                assert_bit_exact(got_p[0], got_m[sl][0::2]); assert_bit_exact(got_p[1], got_m[sl][1::2])
    assert n_fired == n_ticks // 6


def strips(n_strips, sr=SR, tps=60):
    """per strip Trigger->Envelope ; Source->EqThree->Panner(L=R)->Amplifier(ctl=Envelope) -> Mixer."""
    ws = Workspace(sr, tps)
    gains = synth.uniform(10, 3 * n_strips, -24.0, 6.0)
    mg = synth.uniform(11, n_strips, -24.0, 6.0)
    mf = synth.uniform(12, n_strips, 0.0, 1.0)
    mix = ws.mixer([(float(mg[k]), float(mf[k]), k % 8 == 0) for k in range(n_strips)])
    srcs, trigs = [], []
    for k in range(n_strips):
        trig = ws.trigger(False)
        env = ws.envelope()
        src = ws.source_mono()
        eq = ws.eq_three(float(gains[3 * k]), float(gains[3 * k + 1]), float(gains[3 * k + 2]))
        pan = ws.stereo_panner()
        amp = ws.amplifier(1.0, 0.5)
        ws.connect(trig, 0, env, 0)
        ws.connect(src, 0, eq, 0)
        ws.connect(eq, 0, pan, 0); ws.connect(eq, 0, pan, 1)
        ws.connect(pan, 0, amp, 0); ws.connect(env, 0, amp, 1)
        ws.connect(amp, 0, mix, k)
        srcs.append(src); trigs.append(trig)
    return ws, mix, srcs, trigs


@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("batch", [1, 6])
def test_config2_strips_exact_mode_bit_exact(batch, rate):
    SR, SPT = rate
    n_strips, n_ticks = 48, 60
    ws, mix, srcs, trigs = strips(n_strips, SR)
    og = oracle.OracleGraph(ws)
    g = ws.build(max_ticks_per_run=batch, flags=abi.FLAG_EQ_EXACT)
    assert g.run_order() == og.run_order()
    noise = [synth.noise(k, n_ticks * SPT) for k in range(n_strips)]
    for t0 in range(0, n_ticks, batch):
        # gate toggles every 30 ticks with per-strip phase k mod 60; params only change between runs,
        # so batches are aligned to toggle points by construction (30 % batch == 0)
        for k, tr in enumerate(trigs):
            open_ = ((t0 + k) // 30) % 2 == 1
            g.update_params(tr, abi.TriggerParams(1 if open_ else 0))
            og.update_params(tr, abi.TriggerParams(1 if open_ else 0))
        for k, s in enumerate(srcs):
            g.write_source(s, noise[k][t0 * SPT:(t0 + batch) * SPT], batch)
        g.run_ticks(t0, batch)
        got_m = g.read_output(mix, 0, batch, True)
        got_c = g.read_output(mix, 1, batch, True)
        for kk in range(batch):
            tick = t0 + kk
            for k, s in enumerate(srcs):
                og.set_source(s, noise[k][tick * SPT:(tick + 1) * SPT])
            sl = slice(kk * 2 * SPT, (kk + 1) * 2 * SPT)
            og.run_tick(tick)
            assert_bit_exact(got_m[sl], og.output(mix, 0), f"master tick {tick}")
            assert_bit_exact(got_c[sl], og.output(mix, 1), f"cue tick {tick}")


# ------------------------------------------------------------------------------------------------
# EqThree default mode: time-parallel chunked scan, <= 1 ULP (north_star: "within 1 ULP for f32 audio")
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("n_calls,frames", [(1, 131072), (40, SPT), (7, 800), (3, 12345), (5, 1), (4, 5), (2, 1024), (2, 1025), (1, 8192 * 3 + 17)])
def test_eq_three_scan_vs_oracle_within_one_ulp(n_calls, frames, rate):
    SR, _ = rate
    gains = (4.0, -7.5, 2.25)
    x = synth.noise(61, n_calls * frames)
    st = oracle.eq_three_new(SR)
    want = oracle.eq_three_run(st, gains, x)
    m = abi.Module(abi.KIND_EQ_THREE, abi.EqThreeParams(*gains), sample_rate=SR, flags=abi.FLAG_EQ_FAST)
    got = np.empty_like(x)
    for k in range(n_calls):
        m.run_tick(k * frames, [(abi.MX_MONO, x[k * frames:(k + 1) * frames])], [(abi.MX_MONO, got[k * frames:(k + 1) * frames])])
    n_diff = assert_ulp(got, want, 1, f"EqThree scan {n_calls}x{frames}")
    # the f32 cast absorbs almost every f64 last-bit difference: mismatches must be rare
    assert n_diff <= max(2, got.size // 20000), f"{n_diff} of {got.size} samples differ by 1 ULP"


def test_eq_three_scan_many_instances_batched_ticks():
    n_inst, T = 96, 16
    ws = Workspace(SR, 60)
    gains = synth.uniform(70, 3 * n_inst, -24.0, 6.0)
    srcs, eqs = [], []
    for k in range(n_inst):
        s = ws.source_mono(); e = ws.eq_three(*[float(v) for v in gains[3 * k:3 * k + 3]])
        ws.connect(s, 0, e, 0); srcs.append(s); eqs.append(e)
    g = ws.build(max_ticks_per_run=T, flags=abi.FLAG_EQ_FAST)
    noise = [synth.noise(200 + k, 2 * T * SPT) for k in range(n_inst)]
    states = [oracle.eq_three_new(SR) for _ in range(n_inst)]
    total_diff = 0
    for run in range(2):   # state carried across runs
        for k, s in enumerate(srcs):
            g.write_source(s, noise[k][run * T * SPT:(run + 1) * T * SPT], T)
        g.run_ticks(run * T, T)
        for k, e in enumerate(eqs):
            got = g.read_output(e, 0, T, False)
            want = oracle.eq_three_run(states[k], tuple(float(v) for v in gains[3 * k:3 * k + 3]), noise[k][run * T * SPT:(run + 1) * T * SPT])
            total_diff += assert_ulp(got, want, 1, f"EqThree scan inst {k} run {run}")
    assert total_diff <= 200


def test_config2_strips_default_mode_within_tolerance():
    """Whole config-2 graph with the time-parallel EQ: each strip is within 1 ULP of the oracle, so the
    1024-way mix (an f32 sum of those strips) is compared against the oracle mix with a bound of
    n_strips ULPs of the largest partial sum -- and, more sharply, the mixer itself is bit-exact
    given the device's own strip outputs (checked by feeding them to the oracle mixer)."""
    n_strips, T = 32, 8
    ws, mix, srcs, trigs = strips(n_strips)
    g = ws.build(max_ticks_per_run=T, flags=abi.FLAG_EQ_FAST)
    og = oracle.OracleGraph(ws)
    noise = [synth.noise(k, T * SPT) for k in range(n_strips)]
    for k, s in enumerate(srcs):
        g.write_source(s, noise[k], T)
    g.run_ticks(0, T)
    got_m = g.read_output(mix, 0, T, True)
    # mixer inputs = amplifier outputs: node ids are mix+6k+6 by construction of strips()
    chans = [(float(synth.uniform(11, n_strips, -24.0, 6.0)[k]), float(synth.uniform(12, n_strips, 0.0, 1.0)[k]), k % 8 == 0) for k in range(n_strips)]
    amp_ids = [mix + 6 * k + 6 for k in range(n_strips)]
    dev_amp = [g.read_output(a, 0, T, True) for a in amp_ids]
    want_m, _ = oracle.mixer_run(chans, dev_amp, 2 * T * SPT)
    assert_bit_exact(got_m, want_m, "mixer over device strip outputs")
    for t in range(T):
        for k, s in enumerate(srcs):
            og.set_source(s, noise[k][t * SPT:(t + 1) * SPT])
        og.run_tick(t)
        for k, a in enumerate(amp_ids):
            assert_ulp(dev_amp[k][t * 2 * SPT:(t + 1) * 2 * SPT], og.output(a, 0), 1, f"strip {k} tick {t}")


# ------------------------------------------------------------------------------------------------
# EqThree time-split across workgroups (few instances, long streams): pre-pass + boundaries + main
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", RATES)
@pytest.mark.parametrize("n_inst,T,force", [(3, 64, 4), (20, 48, 0), (2, 100, 16), (1, 23, 2)])
def test_eq_three_time_split_within_one_ulp_and_state_carries(n_inst, T, force, rate, monkeypatch):
    SR, SPT = rate
    if force:
        monkeypatch.setenv("MX_EQ_SPLIT", str(force))
    ws = Workspace(SR, 60)
    gains = synth.uniform(80, 3 * n_inst, -24.0, 6.0)
    srcs, eqs = [], []
    for k in range(n_inst):
        s = ws.source_mono(); e = ws.eq_three(*[float(v) for v in gains[3 * k:3 * k + 3]])
        ws.connect(s, 0, e, 0); srcs.append(s); eqs.append(e)
    g = ws.build(max_ticks_per_run=T, flags=abi.FLAG_EQ_FAST)
    noise = [synth.noise(300 + k, 3 * T * SPT) for k in range(n_inst)]
    states = [oracle.eq_three_new(SR) for _ in range(n_inst)]
    diffs = 0
    for run in range(3):
        for k, s in enumerate(srcs):
            g.write_source(s, noise[k][run * T * SPT:(run + 1) * T * SPT], T)
        g.run_ticks(run * T, T)
        for k, e in enumerate(eqs):
            want = oracle.eq_three_run(states[k], tuple(float(v) for v in gains[3 * k:3 * k + 3]), noise[k][run * T * SPT:(run + 1) * T * SPT])
            diffs += assert_ulp(g.read_output(e, 0, T, False), want, 1, f"split EQ inst {k} run {run}")
    assert diffs <= max(3, 3 * n_inst * T * SPT // 20000)


def test_eq_three_prepass_window_equals_full_prepass(monkeypatch):
    # the pre-pass reads only the tail of each span (what the poles have not forgotten, < 2^-280 left out):
    # the result must be the very bits the full-span pre-pass gives, bursts of 1e30 followed by 1e-30 included
    n_inst, T = 4, 80
    ws = Workspace(SR, 60)
    gains = synth.uniform(81, 3 * n_inst, -24.0, 6.0)
    srcs, eqs = [], []
    for k in range(n_inst):
        s = ws.source_mono(); e = ws.eq_three(*[float(v) for v in gains[3 * k:3 * k + 3]])
        ws.connect(s, 0, e, 0); srcs.append(s); eqs.append(e)
    noise = [synth.noise(500 + k, 2 * T * SPT) for k in range(n_inst)]
    noise[1] = noise[1].copy(); noise[1][10000:10050] *= np.float32(1e30); noise[1][10050:30000] *= np.float32(1e-30)
    noise[2] = (noise[2] * np.float32(1e-20)).astype(np.float32)
    monkeypatch.setenv("MX_EQ_SPLIT", "4")
    outs = []
    for full in ("1", "0"):
        monkeypatch.setenv("MX_EQ_FULL_PREPASS", full)
        g = ws.build(max_ticks_per_run=T, flags=abi.FLAG_EQ_FAST)
        res = []
        for run in range(2):
            for k, s in enumerate(srcs):
                g.write_source(s, noise[k][run * T * SPT:(run + 1) * T * SPT], T)
            g.run_ticks(run * T, T)
            res.append(np.concatenate([g.read_output(e, 0, T, False) for e in eqs]))
        outs.append(np.concatenate(res))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))


def test_fused_strips_with_time_split_equal_unsplit(monkeypatch):
    # the whole fused strip (inline Envelope, Amplifier, mono-stored result) through the split path
    ws, mix, srcs, trigs = strips(6)
    T = 60
    noise = [synth.noise(k, 2 * T * SPT) for k in range(6)]
    outs = []
    for force in ("1", "5"):
        monkeypatch.setenv("MX_EQ_SPLIT", force)
        g = ws.build(max_ticks_per_run=T, flags=abi.FLAG_EQ_FAST)
        res = []
        for run in range(2):
            for k, tr in enumerate(trigs):
                g.update_params(tr, abi.TriggerParams((run + k) % 2))
            for k, s in enumerate(srcs):
                g.write_source(s, noise[k][run * T * SPT:(run + 1) * T * SPT], T)
            g.run_ticks(run * T, T)
            res.append(g.read_output(mix, 0, T, True))
        outs.append(np.concatenate(res))
    # span-initial states differ by ~1e-16 relative, so strips may differ by 1 ULP on rare samples; the mix of 6 strips
    # is compared with a few-ULP bound
    assert np.max(np.abs(outs[0] - outs[1])) <= 8 * np.spacing(np.float32(4.0))
    assert np.count_nonzero(outs[0] != outs[1]) <= outs[0].size // 2000


def test_mixer_and_amplifier_keep_f32_subnormals_nan_and_infinity_like_the_cpu():
    # Rust's f32 arithmetic is IEEE with subnormals; the kernels must not flush them (and NaN / infinity must travel)
    n_ch, length = 6, 2 * SPT
    base = synth.noise(900, length)
    ins = [(base * np.float32(s)).astype(np.float32) for s in (1e-40, 3e-39, 1e-38, 1.0, 1e-44, 1e-41)]
    ins[3] = ins[3].copy(); ins[3][5] = np.float32("nan"); ins[3][9] = np.float32("inf"); ins[3][11] = np.float32("-inf"); ins[3][13] = np.float32(-0.0)
    chans = [(0.0, 1.0, True), (-6.0, 0.5, False), (3.0, 1.0, True), (0.0, 1e-3, False), (6.0, 1.0, True), (0.0, 1.0, False)]
    want_m, want_c = oracle.mixer_run(chans, ins, length)
    m = abi.Module(abi.KIND_MIXER, [abi.MixerChannelParams(g, f, 1 if c else 0) for g, f, c in chans])
    got_m = np.empty(length, np.float32); got_c = np.empty(length, np.float32)
    m.run_tick(0, [(abi.MX_STEREO, a) for a in ins], [(abi.MX_STEREO, got_m), (abi.MX_STEREO, got_c)])
    assert_bit_exact(got_m, want_m, "Mixer master with subnormals / NaN / inf")
    assert_bit_exact(got_c, want_c, "Mixer cue with subnormals / NaN / inf")
    x = ins[0]
    want = oracle.amplifier_run(0.5, 0.25, x, None)
    a = abi.Module(abi.KIND_AMPLIFIER, abi.AmplifierParams(0.5, 0.25))
    got = np.empty_like(x)
    a.run_tick(0, [(abi.MX_STEREO, x), (abi.MX_DISCONNECTED, None)], [(abi.MX_STEREO, got)])
    assert_bit_exact(got, want, "Amplifier on subnormal input")


def test_cooperative_mixer_special_values_bit_exact():
    # >= 128 channels on a short stream takes k_mixer_coop, whose cue bus adds +0.0 for non-cue channels: must stay exact for
    # -0.0 (every cue channel -0.0 at one frame), NaN, infinities and subnormals
    n_ch, length = 131, 2 * 70
    ins = [synth.noise(1000 + i, length).copy() for i in range(n_ch)]
    for i in range(n_ch):
        ins[i][8:10] = np.float32(-0.0)                     # all channels -0.0 on frame 4: master and cue end at +0.0 like the CPU
    ins[7][20] = np.float32("nan"); ins[40][30] = np.float32("inf"); ins[41][30] = np.float32("-inf"); ins[90][40:44] = np.float32(1e-42)
    ins[129] = (ins[129] * np.float32(1e-40)).astype(np.float32)
    gains = synth.uniform(3, n_ch, -24.0, 6.0); faders = synth.uniform(4, n_ch, 0.0, 1.0)
    chans = [(float(gains[i]), float(faders[i]), i % 5 == 2) for i in range(n_ch)]
    want_m, want_c = oracle.mixer_run(chans, ins, length)
    m = abi.Module(abi.KIND_MIXER, [abi.MixerChannelParams(g, f, 1 if c else 0) for g, f, c in chans])
    got_m = np.empty(length, np.float32); got_c = np.empty(length, np.float32)
    m.run_tick(0, [(abi.MX_STEREO, a) for a in ins], [(abi.MX_STEREO, got_m), (abi.MX_STEREO, got_c)])
    assert_bit_exact(got_m, want_m, "coop Mixer master, special values")
    assert_bit_exact(got_c, want_c, "coop Mixer cue, special values")


def test_empty_cases_zero_ticks_zero_channels_empty_graph():
    # a Mixer with no channels still zeroes its buses (mixer.rs:54-55); zero ticks is a no-op; an empty graph builds and runs
    ws = Workspace(SR, 60)
    mix = ws.mixer([])
    osc = ws.oscillator(440.0, abi.WAVE_SAW)
    g = ws.build(max_ticks_per_run=2)
    g.run_ticks(0, 0)
    g.run_ticks(0, 2)
    assert not g.read_output(mix, 0, 2, True).any() and not g.read_output(mix, 1, 2, True).any()
    assert g.read_output(osc, 0, 2, False).any()
    g.run_ticks(2, 0)
    assert g.read_output(mix, 0, 0, True).size == 0
    empty = Workspace(SR, 60).build()
    empty.run_ticks(0, 1)
    with pytest.raises(abi.MxError):
        g.run_ticks(0, 3)           # more ticks than max_ticks_per_run
    with pytest.raises(abi.MxError):
        g.read_output(mix, 2, 1, True)   # no such port


def test_zero_channel_mixer_sharing_a_launch_with_a_cooperative_mixer():
    # a Mixer with no channels (params_len 0) in the same (level, kind) group as a >= 128-channel Mixer on a short stream:
    # the group takes k_mixer_coop, whose producers must not fetch a descriptor for the empty one
    n_ch = 130
    ws = Workspace(SR, 60)
    empty = ws.mixer([])
    srcs = [ws.source_stereo() for _ in range(n_ch)]
    chans = [(-3.0, 0.5, k % 2 == 0) for k in range(n_ch)]
    big = ws.mixer(chans)
    for k, s in enumerate(srcs):
        ws.connect(s, 0, big, k)
    g = ws.build()
    ins = [synth.noise(1200 + k, 2 * SPT) for k in range(n_ch)]
    for k, s in enumerate(srcs):
        g.write_source(s, ins[k], 1)
    g.run_ticks(0, 1)
    want_m, want_c = oracle.mixer_run(chans, ins, 2 * SPT)
    assert_bit_exact(g.read_output(big, 0, 1, True), want_m, "coop Mixer next to an empty Mixer: master")
    assert_bit_exact(g.read_output(big, 1, 1, True), want_c, "coop Mixer next to an empty Mixer: cue")
    assert not g.read_output(empty, 0, 1, True).any() and not g.read_output(empty, 1, 1, True).any()
