"""The cases of tests/test_cpu_audio_model.py (oracle == model, model vs exact values, every mis-model caught) and of
tests/test_gpu_audio_model.py (device == model), with the model's own runs of them and the bit comparison both files use.  Importable without a GPU.  Every case is the smallest shape at which its path can go
wrong, not the workload: one to four ticks, a handful of channels.

Two rates unless said otherwise: (44 100, 735) and (48 000, 800).  The far start is tick_shapes.far_first_tick("across_2p32", ...): sample time 2^32
falls inside the stretch.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np

import audio_model as am
import synth
from tick_shapes import far_first_tick

RATES = [(44100, 735), (48000, 800)]
RATE_ID = {44100: "44k1", 48000: "48k"}
F32 = np.float32


def far(spt, n_ticks):
    return far_first_tick("across_2p32", spt, max(2, n_ticks))


# ------------------------------------------------------------------------------------------------
# Envelope
# ------------------------------------------------------------------------------------------------
# Attack times at which two f64 spellings of the attack ramp round to DIFFERENT f32: attack = ms(d0) / q0 with q0 an f32 tie (25 significant bits), so
# that d0 samples after the on edge `ms / attack` is the tie itself (to even) while `1.0 / attack * ms` is one f64 ULP off it; likewise for
# `d * 1000 / sr` against `d / sr * 1000`.  Without them the two spellings differ only below the f32 rounding, and a shared misreading could not show.
# (d0 of each: 3, 3, 5 and 23 samples after an on edge.)  None is a whole number of samples.
TIE_ATTACKS = {
    "tie_div_44k1": float.fromhex("0x1.16a393cf40872p-3"),
    "tie_mul_44k1": float.fromhex("0x1.16a3b24924935p-3"),
    "tie_div_48k": float.fromhex("0x1.aaaa8e5557370p-3"),
    "tie_mul_48k": float.fromhex("0x1.eaaa996aab45ep-1"),
}
ENV_PARAMS = {
    "default": (25.0, 500.0, 0.8, 200.0),
    "short": (1.0, 10.0, 0.3, 5.0),
    "sustain_above_1": (2.0, 20.0, 1.5, 8.0),
    "sustain_0": (2.0, 20.0, 0.0, 8.0),
    "attack_30p87_samples": (0.7, 10.0, 0.3, 5.0),
    "release_below_a_sample": (1.0, 10.0, 0.3, 0.01),
    "attack_0": (0.0, 10.0, 0.3, 5.0),                 # ms < 0.0 is never true: the decay branch from the on edge on, 1.0 / 0.0 is never formed, finite
    "decay_0": (1.0, 0.0, 0.3, 5.0),                   # 1.0 / 0.0 * 0.0 = NaN where ms = attack exactly; clamp passes it
    "release_0": (1.0, 10.0, 0.3, 0.0),                # NaN at the off edge, +inf clamped to 1 after it
    "all_0": (0.0, 0.0, 0.5, 0.0),
    **{k: (v, 10.0, 0.3, 5.0) for k, v in TIE_ATTACKS.items()},
}
FINITE_ENV_PARAMS = [k for k, p in ENV_PARAMS.items() if p[1] and p[3] and (p[0] or k == "attack_0")]     # every 1.0 / x that is formed is finite


def _edges(spt):
    """4 ticks.  0.5 (neither on nor off, envelope.rs:102,107) wherever nothing is written."""
    g = np.full(4 * spt, 0.5, F32)
    g[10] = 1.0; g[40] = 0.0                                     # an off during the attack
    g[63] = 1.0; g[64] = 0.0                                     # an on edge and an off edge in consecutive samples, across a wave boundary
    g[127] = 1.0; g[128] = 1.0                                   # an on edge at the end of a wave, a second 1.0 that changes nothing
    g[400] = 0.0                                                 # off (default: in the attack; short: on the sustain)
    g[450] = 1.0                                                 # a re-trigger during the release: the ramp starts again from 0
    g[500] = np.nan                                              # while on: nothing
    g[520] = 1.5                                                 # while on: nothing
    g[560] = -0.0                                                # -0.0 == 0.0: an off
    g[600] = 1.5                                                 # while off: not == 1.0, nothing
    g[650] = np.nan                                              # while off: nothing
    g[spt - 1] = 1.0; g[spt] = 0.0                               # on at the last sample of a tick, off at the first of the next
    g[spt + 50] = 1.0                                            # held over the whole of tick 1 and into tick 2
    g[2 * spt + 300] = 0.0
    g[3 * spt - 1] = 1.0; g[3 * spt] = 1.0; g[3 * spt + 1] = 0.0; g[3 * spt + 2] = 1.0
    g[4 * spt - 1] = 0.0
    return g


def _blocks12(spt):
    n = 12 * spt
    g = np.zeros(n, F32); g[100:3000] = 1.0; g[5000:5010] = 1.0; g[7000:] = 1.0       # test_gpu_audio_parity._gate_patterns()["blocks"]
    return g


def _alternating(spt):
    g = np.zeros(4 * spt, F32); g[1::2] = 1.0
    return g


def _sprinkled(spt):
    g = synth.noise(5, 4 * spt).copy(); g[::97] = 1.0; g[50::131] = 0.0
    return g


def _decay_completes(spt):
    """36 ticks = 600 ms: the 25 ms attack and the 500 ms decay of the default parameters complete (12 ticks are 200 ms), then an off on the sustain"""
    g = np.full(36 * spt, 0.5, F32); g[5] = 1.0; g[33 * spt + 7] = 0.0
    return g


@dataclass
class EnvCase:
    id: str
    sr: int
    spt: int
    params: tuple
    first_tick: int
    gate: np.ndarray
    calls: list                      # lengths of the successive run_tick calls (all spt: the case also runs on the graph path)
    finite: bool

    @property
    def whole_ticks(self):
        return all(c == self.spt for c in self.calls)

    @property
    def t0(self):
        return self.first_tick * self.spt


def _env_cases():
    out = []

    def add(name, pname, sr, spt, gate, start="0", calls=None):
        n_ticks = gate.size // spt
        first = {"0": 0, "tick1000": 1000, "far": far(spt, n_ticks)}[start]
        out.append(EnvCase(f"{name}-{pname}-{RATE_ID[sr]}-{start}", sr, spt, ENV_PARAMS[pname], first, gate, calls or [spt] * n_ticks, pname in FINITE_ENV_PARAMS))

    for sr, spt in RATES:
        for pname in ENV_PARAMS:
            add("edges", pname, sr, spt, _edges(spt))
        for pname in ("default", "short"):
            add("alternating", pname, sr, spt, _alternating(spt))
            add("sprinkled", pname, sr, spt, _sprinkled(spt))
            add("blocks12", pname, sr, spt, _blocks12(spt))
        add("decay_completes", "default", sr, spt, _decay_completes(spt))
        # single-sample calls, then ragged ones (the module path takes any length)
        add("ragged_calls", "short", sr, spt, _edges(spt)[:2 * spt], calls=[1, 1, 61, 1, 64, spt - 128, 7, spt - 7])
        for start in ("tick1000", "far"):
            for pname in ("default", "short", "all_0"):
                add("edges", pname, sr, spt, _edges(spt), start)
    return out


ENVELOPE = _env_cases()


# ------------------------------------------------------------------------------------------------
# Mixer
# ------------------------------------------------------------------------------------------------
@dataclass
class MixCase:
    id: str
    channels: list                   # (gain_db, fader, cue)
    inputs: list                     # f32 arrays, None = Disconnected
    length: int                      # floats (interleaved stereo)
    graph: tuple | None = None       # (sr, spt): also run on the graph path, one tick (length == 2 * spt)
    coop: bool = False               # takes the cooperative kernel by default: also run with the streaming kernel forced


def _mix_channels(n, seed):
    gains = synth.uniform(seed, n, -96.0, 24.0)
    faders = synth.uniform(seed + 1, n, 0.0, 1.0)
    ch = [(float(gains[i]), float(faders[i]), i % 3 == 1) for i in range(n)]
    if n >= 4:
        ch[3] = (0.0, 0.0, True)                                  # MixerChannelParams::default: fader 0.0 (protocol/src/lib.rs:342-347), on the cue bus all the same
    return ch


def _mix_inputs(n, length, seed):
    ins = [synth.noise(seed + i, length) for i in range(n)]
    if n > 2:
        ins[2] = None                                             # Disconnected
    if n > 16:
        ins[16] = None
    return ins


def _mixer_cases():
    out = []
    for n, length in ((1, 2), (3, 126), (4, 514), (5, 126), (16, 514), (17, 126), (4, 2), (17, 2), (5, 514)):
        out.append(MixCase(f"n{n}-len{length}", _mix_channels(n, 20 + n), _mix_inputs(n, length, 300 + 10 * n), length))
    out.append(MixCase("n129-len126-coop", _mix_channels(129, 60), _mix_inputs(129, 126, 2000), 126, coop=True))
    # order made visible: ((0 + 1e8) - 1e8) + 1 = 1 but ((0 + 1) - 1e8) + 1e8 = 0 in f32; all on the cue bus, unity gain
    a, b, c = np.array([1e8, 1.0], F32), np.array([-1e8, 1.0], F32), np.array([1.0, -3.0], F32)
    out.append(MixCase("order-1e8", [(0.0, 1.0, True)] * 3, [a, b, c], 2))
    # +20 dB is 10.0 exactly from pow, 10.000000000000002 from exp(db ln10 / 20); x = m 2^-24 with m = 4 (mod 8) and 5 m >= 2^26 makes x * 10 an f32 tie
    m = (0xD00004 + 8 * np.arange(63)).astype(np.float64) * 2.0 ** -24
    tie = np.repeat(m.astype(F32), 2)
    out.append(MixCase("tie-20dB", [(20.0, 1.0, False), (-20.0, 1.0, True)], [tie, synth.noise(77, 126)], 126))
    for sr, spt in RATES:
        for n in (4, 17):
            out.append(MixCase(f"n{n}-tick-{RATE_ID[sr]}", _mix_channels(n, 40 + n), _mix_inputs(n, 2 * spt, 700 + 10 * n), 2 * spt, graph=(sr, spt)))
    return out


MIXER = _mixer_cases()


# ------------------------------------------------------------------------------------------------
# Amplifier
# ------------------------------------------------------------------------------------------------
# (x * D) * A against x * (D * A) differ in the last f64 bit only; with depth 1 the factor D is the control value itself, and this amplitude puts
# x * v * A one f64 ULP from an f32 tie for the pair (x, v) below, so the two groupings round to different f32.
AMP_TIE = dict(x=float.fromhex("0x1.5109700000000p-1"), v=float.fromhex("0x1.ee3f060000000p-1"), amplitude=float.fromhex("0x1.66665458fc285p-1"))
AMP_PARAMS = [(1.0, 0.5), (0.7, 0.1), (2.0, 1.0), (1.0, 0.0), (AMP_TIE["amplitude"], 1.0)]


@dataclass
class AmpCase:
    id: str
    sr: int
    spt: int
    amplitude: float
    depth: float
    x: np.ndarray                    # 2 * n_ticks * spt
    ctl: np.ndarray | None           # n_ticks * spt, None = Disconnected
    n_ticks: int = 2


def _amp_cases():
    out = []
    for sr, spt in RATES:
        for k, (a, d) in enumerate(AMP_PARAMS):
            for connected in (True, False):
                x = synth.noise(21 + k, 4 * spt).copy()
                ctl = synth.noise(22 + k, 2 * spt).copy()         # noise: the two frames of neighbouring stereo pairs see different values, [i] and [i / 2] differ
                x[10] = x[11] = AMP_TIE["x"]; ctl[5] = AMP_TIE["v"]
                out.append(AmpCase(f"a{a:.3g}-d{d:g}-{'ctl' if connected else 'open'}-{RATE_ID[sr]}", sr, spt, a, d, x, ctl if connected else None))
    return out


AMPLIFIER = _amp_cases()


# ------------------------------------------------------------------------------------------------
# Oscillator, FmSine
# ------------------------------------------------------------------------------------------------
@dataclass
class OscCase:
    id: str
    sr: int
    spt: int
    freq: float
    wave: str
    first_tick: int


@dataclass
class FmCase:
    id: str
    sr: int
    spt: int
    freq_lo: float
    freq_hi: float
    first_tick: int
    x: np.ndarray | None


def _osc_cases():
    out = []
    for sr, spt in RATES:
        starts = {"0": 0, "tick1000": 1000, "far": far(spt, 1) + 1}      # (the far tick is the one that holds sample time 2^32)
        freqs = {"100": 100.0, "440": 440.0, "880p5": 880.5, "nyquist": sr / 2, "quarter": sr / 4, "minus440": -440.0}
        for sname, first in starts.items():
            for fname, f in freqs.items():
                for wave in ("saw", "triangle"):                  # sr / 2 and sr / 4 sit on n = k + 0.5 and k + 0.25: floor(0.5 + n) at its ties
                    out.append(OscCase(f"{wave}-{fname}-{RATE_ID[sr]}-{sname}", sr, spt, f, wave, first))
            for wave in ("on", "off"):
                out.append(OscCase(f"{wave}-{RATE_ID[sr]}-{sname}", sr, spt, 440.0, wave, first))
    # Sine and Square: one tick each, about 3 100 decimal sines (Square repeats Sine's arguments; the sine is odd: -440 Hz costs nothing beside 440 Hz)
    f48 = far(800, 1) + 1
    for wave in ("sine", "square"):
        out += [OscCase(f"{wave}-440-44k1-0", 44100, 735, 440.0, wave, 0), OscCase(f"{wave}-440-48k-0", 48000, 800, 440.0, wave, 0),
                OscCase(f"{wave}-minus440-44k1-0", 44100, 735, -440.0, wave, 0),          # sample 0 is sin(-0.0) = -0.0: Square gives -1
                OscCase(f"{wave}-880p5-48k-far", 48000, 800, 880.5, wave, f48),
                OscCase(f"{wave}-100-44k1-tick1000", 44100, 735, 100.0, wave, 1000)]
    return out


def _fm_cases():
    """about 2 300 decimal sines: with the Oscillator's, about 5 400 in all"""
    return [FmCase("220-880-noise-44k1-tick5000", 44100, 735, 220.0, 880.0, 5000, synth.noise(31, 735)),
            FmCase("880-220-noise-48k-0", 48000, 800, 880.0, 220.0, 0, synth.noise(33, 800)),                  # freq_lo > freq_hi: a negative freq_amp
            FmCase("220-880-open-48k-far", 48000, 800, 220.0, 880.0, far(800, 1) + 1, None)]


OSCILLATOR = _osc_cases()
FM_SINE = _fm_cases()


def sine_arguments():
    """-> [(case id, f64 argument)] of every sine the Oscillator and FmSine cases take"""
    out = []
    for c in OSCILLATOR:
        if c.wave in ("sine", "square"):
            out += [(c.id, float(a)) for a in am.oscillator_argument(c.freq, c.sr, c.first_tick * c.spt, c.spt)]
    for c in FM_SINE:
        out += [(c.id, float(a)) for a in am.fm_sine_argument(c.freq_lo, c.freq_hi, c.sr, c.first_tick * c.spt, c.x, c.spt)]
    return out


def sine_margin(arg: float) -> Fraction:
    """The distance of the real sine of `arg` from the nearest f32 rounding boundary, relative to the sine.  Above 2^-52 the f32 of ANY f64 within one
    f64 ULP of the real sine is the correctly rounded f32: libm's double rounding cannot be the cause of a difference.  (+-0: no rounding at all.)"""
    if arg == 0.0:
        return Fraction(1)
    s = Fraction(am.sin_decimal_cached(arg))
    f = np.float32(float(s))
    lo, hi = np.nextafter(f, F32(-np.inf)), np.nextafter(f, F32(np.inf))
    cands = sorted(Fraction(float(v)) for v in (np.nextafter(lo, F32(-np.inf)), lo, f, hi, np.nextafter(hi, F32(np.inf))))
    mids = [(a + b) / 2 for a, b in zip(cands[:-1], cands[1:])]
    return min(abs(s - m) for m in mids) / abs(s)


# ------------------------------------------------------------------------------------------------
# the config-2 strips (test_gpu_audio_parity.strips)
# ------------------------------------------------------------------------------------------------
N_STRIPS, STRIP_TICKS = 3, 4
STRIP_ENV = ENV_PARAMS["default"]                               # Workspace.envelope() defaults = EnvelopeParams::default
STRIP_AMP = (1.0, 0.5)


@dataclass
class StripCase:
    id: str
    sr: int
    spt: int
    first_tick: int
    gates: list = field(default_factory=list)                   # [tick][strip] bool: the Trigger's parameter during that tick
    sources: list = field(default_factory=list)

    @property
    def eq_gains(self):
        g = synth.uniform(10, 3 * N_STRIPS, -24.0, 6.0)
        return [tuple(float(v) for v in g[3 * k:3 * k + 3]) for k in range(N_STRIPS)]

    @property
    def mixer_channels(self):
        mg, mf = synth.uniform(11, N_STRIPS, -24.0, 6.0), synth.uniform(12, N_STRIPS, 0.0, 1.0)
        return [(float(mg[k]), float(mf[k]), k % 8 == 0) for k in range(N_STRIPS)]


def _strip_cases():
    out = []
    for sr, spt in RATES:
        for sname, first in (("0", 0), ("far", far(spt, STRIP_TICKS))):
            gates = [[(k + s) % 3 != 0 if s < 2 else k == 1 for s in range(N_STRIPS)] for k in range(STRIP_TICKS)]   # every strip toggles inside the stretch
            out.append(StripCase(f"{RATE_ID[sr]}-{sname}", sr, spt, first, gates, [synth.noise(k, STRIP_TICKS * spt) for k in range(N_STRIPS)]))
    return out


STRIPS = _strip_cases()


# ------------------------------------------------------------------------------------------------
# EqThree: (lo, mid, hi) dB over 4 ticks of noise, state carried (the first is the golden pair's)
# ------------------------------------------------------------------------------------------------
EQ_GAINS = [(4.0, 0.0, 4.0), (-24.0, 6.0, -3.5), (-96.0, 24.0, 0.0)]
EQ_TICKS = 4


def eq_input(spt):
    return synth.noise(11, EQ_TICKS * spt)


# ------------------------------------------------------------------------------------------------
# the comparison: bit for bit, a NaN of the model accepting any NaN
# ------------------------------------------------------------------------------------------------
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want):
    """want: the model.  Its NaNs accept any NaN; everything else bit for bit, +-0 distinguished."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan])


def assert_same_bits(got, want, what):
    if not same_bits(got, want):
        got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
        assert got.shape == want.shape, f"{what}: {got.shape} against the model's {want.shape}"
        bad = np.flatnonzero((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError(f"{what}: {bad.size}/{got.size} samples differ from the model, first at {bad[:5]}: got {got[bad[:5]]} model {want[bad[:5]]}")


# ------------------------------------------------------------------------------------------------
# the model's own runs of the cases
# ------------------------------------------------------------------------------------------------
def model_envelope(case, mis=None, trace=None):
    st, out, out64, o = am.EnvelopeState(), [], [], 0
    for n in case.calls:
        a, b = am.envelope(st, case.params, case.sr, case.t0 + o, case.gate[o:o + n], mis=mis, trace=trace)
        out.append(a); out64.append(b); o += n
    return np.concatenate(out), np.concatenate(out64)


def model_oscillator(case, mis=None):
    return am.oscillator(case.freq, case.wave, case.sr, case.first_tick * case.spt, case.spt, spt=case.spt, mis=mis)[0]


def model_fm(case, mis=None):
    return am.fm_sine(case.freq_lo, case.freq_hi, case.sr, case.first_tick * case.spt, case.x, case.spt, mis=mis)


def model_strip(case):
    states = [am.StripState(case.sr) for _ in range(N_STRIPS)]
    return am.strip(states, case.sr, case.spt, case.first_tick, case.gates, case.sources, case.eq_gains, STRIP_ENV, STRIP_AMP, case.mixer_channels)


def model_eq_three(sr, spt, gains):
    st, x = am.EqThreeState(sr), eq_input(spt)
    return np.concatenate([am.eq_three(st, gains, x[k * spt:(k + 1) * spt]) for k in range(EQ_TICKS)])


_MODEL = {}


def model(kind, case):
    """The reference run of `case` by the model, computed once per process and shared: callers must leave it unchanged.
    envelope -> f32 output; mixer -> (master, cue); amplifier, oscillator (mono), fm_sine -> f32 output; strip -> am.strip's dict"""
    key = (kind, case.id)
    if key not in _MODEL:
        _MODEL[key] = {"envelope": lambda c: model_envelope(c)[0], "mixer": lambda c: am.mixer(c.channels, c.inputs, c.length),
                       "amplifier": lambda c: am.amplifier(c.amplitude, c.depth, c.x, c.ctl), "oscillator": model_oscillator,
                       "fm_sine": model_fm, "strip": model_strip}[kind](case)
    return _MODEL[key]


STEREO_PORTS = ("panner", "amplifier")


def strip_workspace(case):
    """test_gpu_audio_parity.strips(): per strip Trigger -> Envelope ; Source -> EqThree -> Panner(L = R) -> Amplifier(ctl = Envelope) -> Mixer"""
    from mixlab_amd.workspace import Workspace
    ws = Workspace(case.sr, 60)
    mix = ws.mixer(case.mixer_channels)
    nodes = []
    for k in range(N_STRIPS):
        trig, env, src = ws.trigger(False), ws.envelope(), ws.source_mono()
        eq, pan, amp = ws.eq_three(*case.eq_gains[k]), ws.stereo_panner(), ws.amplifier(*STRIP_AMP)
        ws.connect(trig, 0, env, 0); ws.connect(src, 0, eq, 0)
        ws.connect(eq, 0, pan, 0); ws.connect(eq, 0, pan, 1)
        ws.connect(pan, 0, amp, 0); ws.connect(env, 0, amp, 1); ws.connect(amp, 0, mix, k)
        nodes.append(dict(trigger=trig, envelope=env, source=src, eq=eq, panner=pan, amplifier=amp))
    return ws, mix, nodes
