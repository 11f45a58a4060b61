"""The audio path's checker is checked: oracle/mixlab_oracle.c against an independent numpy model of the reference's audio modules
(tests/audio_model.py, written from the Rust text), that model against exact values within derived bounds, and the shared cases
(tests/audio_cases.py) against deliberate mis-models.  No GPU.

(a) the oracle's Mixer, Envelope, Amplifier, Oscillator, FmSine, EqThree, Trigger, StereoPanner, StereoSplitter and its graph runner on the
    config-2 strip equal the model on every bit (a NaN of the model accepts any NaN: the reference does not specify an arithmetic NaN's
    payload and sign), over the cases of tests/audio_cases.py; the EqThree model itself is first pinned
    to the reference's golden pair;
(b) the model's f64 Envelope amplitude stays within audio_model.envelope_bound of the same expression in exact rationals, and the Mixer's
    master within audio_model.mixer_bound of the exactly rounded sum (the largest fractions seen are recorded in DESIGN.md section 3);
(c) every entry of audio_model.MIS_MODELS changes at least one bit of f32 output of at least one case -- so a kernel and an oracle that
    shared that misreading would fail the bit comparisons."""
import math
import pathlib
from fractions import Fraction

import numpy as np
import pytest

import audio_cases as ac
import audio_model as am
import oracle
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace

GOLDEN = pathlib.Path(__file__).resolve().parent / "golden"
WAVE = {name: k for k, name in enumerate(am.WAVES)}
assert (abi.WAVE_ON, abi.WAVE_OFF, abi.WAVE_SINE, abi.WAVE_SQUARE, abi.WAVE_TRIANGLE, abi.WAVE_SAW) == tuple(WAVE[w] for w in am.WAVES)


from audio_cases import (STEREO_PORTS, assert_same_bits, bits, model_envelope, model_fm, model_oscillator, model_strip,  # noqa: E402
                         same_bits, strip_workspace)


def by_id(cases):
    return pytest.mark.parametrize("case", cases, ids=[c.id for c in cases])


# ------------------------------------------------------------------------------------------------
# (a) the oracle equals the model
# ------------------------------------------------------------------------------------------------
def test_decibel_to_linear_is_within_one_ulp_of_the_real_power_and_equals_the_oracles():
    import mpmath
    mpmath.mp.dps = 60
    assert am.decibel_to_linear(0.0) == 1.0 and am.decibel_to_linear(20.0) == 10.0 and am.decibel_to_linear(-0.0) == 1.0
    gains = [float(g) for g in np.concatenate([np.linspace(-96.0, 24.0, 241), ac.synth.uniform(90, 400, -96.0, 24.0)])]
    for db in gains:
        got = float(am.decibel_to_linear(db))
        exact = mpmath.power(10, mpmath.mpf(db / 20.0))             # pow's own error: of the f64 quotient the reference hands it
        assert abs(mpmath.mpf(got) - exact) <= math.ulp(got), db
        assert got == oracle.lib.orc_decibel_to_linear(db), db


def test_the_eq_three_coefficients_are_the_correctly_rounded_sines():
    import mpmath
    mpmath.mp.dps = 60
    for sr in (44100, 48000):
        st = am.EqThreeState(sr)
        for f, freq in ((st.f_lo, 420.0), (st.f_hi, 2700.0)):
            arg = float(am.PI * am.F64(freq) / am.F64(sr))
            exact = 2 * mpmath.sin(mpmath.mpf(arg))
            assert abs(mpmath.mpf(float(f)) - exact) <= mpmath.mpf(math.ulp(float(f))) / 2, (sr, freq)      # 2 sin(x): the doubling is exact
            assert float(f) == oracle.lib.orc_lowpass_coeff(freq, float(sr))


def test_the_eq_three_model_reproduces_the_references_golden_prefix():
    x = np.fromfile(GOLDEN / "eq_three_chronos_prefix131072.f32.raw", dtype="<f4")[:8192]
    y = np.fromfile(GOLDEN / "eq_three_chronos-eq_prefix131072.f32.raw", dtype="<f4")[:8192]
    out = am.eq_three(am.EqThreeState(44100), (4.0, 0.0, 4.0), x)          # Decibel(4.0), Decibel(0.0), Decibel(4.0): eq_three.rs:154-158
    assert np.array_equal(bits(out), bits(y))
    ticked_state = am.EqThreeState(44100)
    ticked = np.concatenate([am.eq_three(ticked_state, (4.0, 0.0, 4.0), x[o:o + 735]) for o in range(0, 8192, 735)])
    assert np.array_equal(bits(ticked), bits(y))


@pytest.mark.parametrize("rate", ac.RATES, ids=["44k1", "48k"])
@pytest.mark.parametrize("gains", ac.EQ_GAINS)
def test_oracle_eq_three_equals_the_model(gains, rate):
    sr, spt = rate
    x = ac.eq_input(spt)
    st, ms = oracle.eq_three_new(float(sr)), am.EqThreeState(sr)
    for k in range(4):
        assert_same_bits(oracle.eq_three_run(st, gains, x[k * spt:(k + 1) * spt]), am.eq_three(ms, gains, x[k * spt:(k + 1) * spt]), f"EqThree tick {k}")


@by_id(ac.ENVELOPE)
def test_oracle_envelope_equals_the_model(case):
    want, _ = model_envelope(case)
    st, got, o = oracle.EnvState(), [], 0
    for n in case.calls:
        got.append(oracle.envelope_run(st, case.params, float(case.sr), case.t0 + o, case.gate[o:o + n], n)); o += n
    assert_same_bits(np.concatenate(got), want, f"Envelope {case.id}")


def test_the_envelope_cases_reach_what_they_are_listed_for():
    by = {c.id: c for c in ac.ENVELOPE}
    for name in ("release_0", "all_0"):
        assert np.isnan(model_envelope(by[f"edges-{name}-44k1-0"])[0]).any(), f"{name}: no NaN reached"
    # decay = 0: 1.0 / 0.0 * x is NaN only where ms equals the attack time exactly, +inf (clamped to 1) after it
    assert any(np.isnan(model_envelope(by[f"edges-decay_0-{r}-0"])[0]).any() for r in ("44k1", "48k")), "decay_0: no NaN reached at either rate"
    # attack = 0 alone never divides: ms < 0.0 is false from the on edge on, the decay branch runs with ms - 0.0 (envelope.rs:40-48)
    assert np.isfinite(model_envelope(by["edges-attack_0-44k1-0"])[0]).all()
    out, out64 = model_envelope(by["decay_completes-default-48k-0"])
    assert out[5 + 1200 + 24000] == np.float32(0.8) and out[33 * 800 + 6] == np.float32(0.8) and 0 < out[33 * 800 + 7 + 100] < 0.8     # the sustain, then the release
    trace = []
    model_envelope(by["edges-default-44k1-0"], trace=trace)
    assert {k[0] for k in trace} == {am.INITIAL, am.TRIGGER_ON, am.TRIGGER_OFF}
    assert by["edges-default-48k-far"].t0 < 1 << 32 < by["edges-default-48k-far"].t0 + 4 * 800
    assert any(not c.whole_ticks and 1 in c.calls for c in ac.ENVELOPE)


@by_id(ac.MIXER)
def test_oracle_mixer_equals_the_model(case):
    want_m, want_c = am.mixer(case.channels, case.inputs, case.length)
    got_m, got_c = oracle.mixer_run(case.channels, case.inputs, case.length)
    assert_same_bits(got_m, want_m, f"Mixer {case.id} master")
    assert_same_bits(got_c, want_c, f"Mixer {case.id} cue")


@by_id(ac.AMPLIFIER)
def test_oracle_amplifier_equals_the_model(case):
    assert_same_bits(oracle.amplifier_run(case.amplitude, case.depth, case.x, case.ctl), am.amplifier(case.amplitude, case.depth, case.x, case.ctl), f"Amplifier {case.id}")


@by_id(ac.OSCILLATOR)
def test_oracle_oscillator_equals_the_model(case):
    want = model_oscillator(case)
    mono, stereo = oracle.oscillator_run(case.freq, WAVE[case.wave], float(case.sr), case.first_tick * case.spt, case.spt)
    assert_same_bits(mono, want, f"Oscillator {case.id}")
    assert_same_bits(stereo, np.repeat(want, 2), f"Oscillator {case.id} stereo")


@by_id(ac.FM_SINE)
def test_oracle_fm_sine_equals_the_model(case):
    got = oracle.fm_sine_run(case.freq_lo, case.freq_hi, float(case.sr), case.first_tick * case.spt, case.x, case.spt)
    assert_same_bits(got, model_fm(case), f"FmSine {case.id}")


def test_every_sine_argument_is_clear_of_an_f32_rounding_boundary():
    """A condition on the inputs, not a tolerance: no listed argument may fail it (replace the case's frequency or start time if one does)."""
    args = ac.sine_arguments()
    assert 4500 <= len({abs(a) for _cid, a in args}) <= 6000      # the budget: Square repeats Sine's arguments and the sine is odd, so about 5 400 decimal sines
    worst = min((ac.sine_margin(a), cid, a) for cid, a in args)
    assert worst[0] > Fraction(1, 1 << 52), f"{worst[1]}: sin({worst[2]!r}) is within {float(worst[0]):.3g} (relative) of an f32 rounding boundary"


@pytest.mark.parametrize("rate", ac.RATES, ids=["44k1", "48k"])
def test_oracle_trigger_panner_splitter_equal_the_model(rate):
    sr, spt = rate
    ws = Workspace(sr, 60)
    t_on, t_off = ws.trigger(True), ws.trigger(False)
    l, r, st = ws.source_mono(), ws.source_mono(), ws.source_stereo()
    pan, half, split, split_open = ws.stereo_panner(), ws.stereo_panner(), ws.stereo_splitter(), ws.stereo_splitter()
    ws.connect(l, 0, pan, 0); ws.connect(r, 0, pan, 1); ws.connect(r, 0, half, 1); ws.connect(st, 0, split, 0)
    sinks = ws.mixer([(0.0, 1.0, False)] * 2)              # (the runner evaluates what a terminal reaches: give every node a reader)
    og = oracle.OracleGraph(ws)
    xl, xr, xs = ac.synth.noise(41, spt), ac.synth.noise(42, spt), ac.synth.noise(43, 2 * spt)
    xl = xl.copy(); xl[3] = -0.0; xl[4] = np.float32(1e-42)                     # a shuffle keeps every bit
    og.set_source(l, xl); og.set_source(r, xr); og.set_source(st, xs)
    og.run_tick(7)
    assert_same_bits(og.output(t_on, 0), am.trigger(True, spt), "Trigger open")
    assert_same_bits(og.output(t_off, 0), am.trigger(False, spt), "Trigger closed")
    assert_same_bits(og.output(pan, 0), am.stereo_panner(xl, xr, spt), "StereoPanner")
    assert_same_bits(og.output(half, 0), am.stereo_panner(None, xr, spt), "StereoPanner, L Disconnected")
    for port in (0, 1):
        assert_same_bits(og.output(split, port), am.stereo_splitter(xs, spt)[port], f"StereoSplitter port {port}")
        assert_same_bits(og.output(split_open, port), am.stereo_splitter(None, spt)[port], f"StereoSplitter Disconnected port {port}")
    del sinks


@by_id(ac.STRIPS)
def test_oracle_graph_on_the_strips_equals_the_model(case):
    want = model_strip(case)
    ws, mix, nodes = strip_workspace(case)
    og = oracle.OracleGraph(ws)
    spt = case.spt
    for k in range(ac.STRIP_TICKS):
        for s, nd in enumerate(nodes):
            og.update_params(nd["trigger"], abi.TriggerParams(int(case.gates[k][s])))
            og.set_source(nd["source"], case.sources[s][k * spt:(k + 1) * spt])
        og.run_tick(case.first_tick + k)
        assert_same_bits(og.output(mix, 0), want["master"][2 * k * spt:2 * (k + 1) * spt], f"{case.id} tick {k}: Master")
        assert_same_bits(og.output(mix, 1), want["cue"][2 * k * spt:2 * (k + 1) * spt], f"{case.id} tick {k}: Cue")
        for s, nd in enumerate(nodes):
            for name in ("trigger", "envelope", "eq", "panner", "amplifier"):
                w = 2 if name in STEREO_PORTS else 1
                assert_same_bits(og.output(nd[name], 0), want[name][s][w * k * spt:w * (k + 1) * spt], f"{case.id} tick {k} strip {s}: {name}")


def test_the_strip_gates_toggle_inside_the_stretch():
    for case in ac.STRIPS:
        for s in range(ac.N_STRIPS):
            col = [case.gates[k][s] for k in range(ac.STRIP_TICKS)]
            assert True in col and False in col, (case.id, s, col)
        assert model_strip(case)["cue"].any() and model_strip(case)["master"].any()


# ------------------------------------------------------------------------------------------------
# (b) the model against exact values
# ------------------------------------------------------------------------------------------------
# branch -> the largest |model - exact| / bound seen.  DESIGN.md section 3 records these fractions; to regenerate them run
#   pytest tests/test_cpu_audio_model.py -s -k "derived_bound"
# and read the last "largest fraction of the bound so far" and "largest so far" lines.  (The bounds are what is asserted; the fractions are a record.)
OBSERVED = {}


@by_id([c for c in ac.ENVELOPE if c.finite and c.gate.size <= 4 * c.spt] + [c for c in ac.ENVELOPE if c.id.startswith("decay_completes")])
def test_the_envelope_model_is_within_the_derived_bound_of_exact_arithmetic(case):
    trace = []
    _out, out64 = model_envelope(case, trace=trace)
    step = 1 if case.gate.size <= 4 * case.spt else 37          # (the 36-tick case: every 37th sample, 715 of them)
    for i in range(0, out64.size, step):
        exact, branch, figures, same_side = am.envelope_exact(case.params, trace[i], case.t0 + i, case.sr)
        assert same_side, f"{case.id} sample {i}: the f64 ms and the exact ms fall on different sides of the attack time, farther apart than the rounding of ms"
        bound = am.envelope_bound(branch, figures)
        err = abs(Fraction(float(out64[i])) - exact)
        assert err <= bound, f"{case.id} sample {i} ({branch}): |model - exact| = {float(err):.3e} > {float(bound):.3e}"
        if bound:
            OBSERVED[branch] = max(OBSERVED.get(branch, 0.0), float(err / bound))
    print(f"\n{case.id}: largest fraction of the bound so far {OBSERVED}")


@by_id(ac.MIXER)
def test_the_mixer_model_is_within_the_derived_bound_of_the_exact_sum(case):
    master, _cue = am.mixer(case.channels, case.inputs, case.length)
    exact, magnitude = am.mixer_exact_master(case.channels, case.inputs, case.length)
    bound = am.mixer_bound(len(case.channels), magnitude)
    err = np.abs(master.astype(np.float64) - exact)
    assert (err <= bound).all(), f"{case.id}: sample {int(np.argmax(err - bound))}: {err.max():.3e}"
    frac = float(np.max(err[bound > 0] / bound[bound > 0])) if (bound > 0).any() else 0.0
    OBSERVED["mixer"] = max(OBSERVED.get("mixer", 0.0), frac)
    print(f"\n{case.id}: {frac:.3f} of the bound; largest so far {OBSERVED['mixer']:.3f}")


# ------------------------------------------------------------------------------------------------
# (c) every mis-model changes at least one bit of at least one case
# ------------------------------------------------------------------------------------------------
def differs(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return bool(np.any((bits(a) != bits(b)) & ~(np.isnan(a) & np.isnan(b))))


_REF = {}


def ref(kind, case, run):
    key = (kind, case.id)
    if key not in _REF:
        _REF[key] = run(case)
    return _REF[key]


def caught_by(kind, mis):
    """-> the id of the first case of `kind` on which the mis-model's f32 output differs from the model's"""
    if kind == "envelope":
        order = sorted(ac.ENVELOPE, key=lambda c: c.gate.size)      # the short cases first: most misreadings show on `edges`
        for c in order:
            if differs(model_envelope(c, mis)[0], ref(kind, c, lambda c: model_envelope(c)[0])):
                return c.id
    elif kind == "mixer":
        for c in ac.MIXER:
            want = ref(kind, c, lambda c: np.concatenate(am.mixer(c.channels, c.inputs, c.length)))
            if differs(np.concatenate(am.mixer(c.channels, c.inputs, c.length, mis=mis)), want):
                return c.id
    elif kind == "amplifier":
        for c in ac.AMPLIFIER:
            if differs(am.amplifier(c.amplitude, c.depth, c.x, c.ctl, mis=mis), ref(kind, c, lambda c: am.amplifier(c.amplitude, c.depth, c.x, c.ctl))):
                return c.id
    elif kind == "oscillator":
        for c in ac.OSCILLATOR:
            if mis in ("saw_half_even",) and c.wave not in ("saw", "triangle"):
                continue
            if mis.startswith("sign_") and c.wave != "square":
                continue
            if mis == "argument_regrouped" and c.wave not in ("sine", "square"):
                continue
            if differs(model_oscillator(c, mis), ref(kind, c, model_oscillator)):
                return c.id
    elif kind == "fm_sine":
        for c in ac.FM_SINE:
            if differs(model_fm(c, mis), ref(kind, c, model_fm)):
                return c.id
    return None


@pytest.mark.parametrize("kind,mis", [(k, m) for k, ms in am.MIS_MODELS.items() for m in ms])
def test_every_mis_model_is_caught_by_a_named_case(kind, mis):
    cid = caught_by(kind, mis)
    assert cid is not None, f"{kind}: the misreading `{mis}` changes no bit of any shared case: the cases are too weak, add one"
    print(f"\n{kind} mis-model {mis}: caught by case {cid}")


def test_the_tie_cases_catch_the_f64_spellings_at_both_rates():
    """ms / attack and d * 1000 / sr differ from the reference's spelling below the f32 rounding except at engineered ties: each rate has its own"""
    by = {c.id: c for c in ac.ENVELOPE}
    for rate in ("44k1", "48k"):
        for mis, name in (("ms_div_attack", "tie_div"), ("ms_times_1000_first", "tie_mul")):
            c = by[f"edges-{name}_{rate}-{rate}-0"]
            assert differs(model_envelope(c, mis)[0], model_envelope(c)[0]), (mis, c.id)
