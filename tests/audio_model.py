"""An independent numpy model of the reference's audio modules -- TEST INFRASTRUCTURE, the checker of the checker.

Written from the Rust text alone (src/module/*.rs, protocol/src/lib.rs; file:line cited at every step), not from oracle/mixlab_oracle.c and
not from the kernels: tests/test_cpu_audio_model.py holds the oracle to it bit for bit (and the parity tests hold the device to the oracle).

Rules that make it exact and independent of any C compiler:
  * every f64 step is one numpy float64 operation, in the reference's written order and association (numpy's scalar and element-wise
    float64 operations are individually rounded IEEE operations: no contraction, no excess precision);
  * every `as f32` / `as Sample` is np.float32(...) (round to nearest even, overflow to infinity, as Rust's cast);
  * u64 sample times are Python ints, converted to f64 once, where the Rust converts (`as f64`);
  * a sine is the correctly rounded f32 of the REAL sine (tests/sin_reference.py, no libm).  The reference stores (f32) of libm's f64 sine;
    the two are equal wherever the real sine is farther than libm's error from an f32 rounding boundary, which audio_cases.sine_margin
    asserts for every argument the cases use;
  * Decibel::to_linear is math.pow, as the reference calls libm's pow (protocol/src/lib.rs:469-471).

Every function takes `mis`: None is the reference; a name from MIS_MODELS is the model with that ONE deliberate misreading.  The shared cases
(tests/audio_cases.py) must tell every one of them from the reference in at least one bit of f32 output.

Bounds of the model against exact arithmetic (asserted by tests/test_cpu_audio_model.py part (b), u = 2^-53, one rounding = a relative
error of at most u):

  Envelope, one step from the carried state, finite parameters (exact value: the same expression in fractions.Fraction over the f64
  parameters and the f64 off_amplitude of the state):
    ms = d / sr * 1000                         2 roundings:          |ms~ - ms| <= 2u ms (1 + u)                      =: e_ms
    attack   1/a * ms                          +2 roundings:         <= (4u + 7u^2) ms / a                            ENV_BOUND attack
    decay    x = ms - a is one rounding of a difference of an inexact ms: |x~ - x| <= e_ms + u |x~|   (the cancellation: e_ms is
             relative to ms, not to x); r = 1/dcy * x: <= (e_x / dcy)(1 + 2u) + 2u |r| (1 + u) =: e_r; clamp does not grow an error
             (1-Lipschitz); 1 - c: + u; (1 - s): u relative, the product and the sum one rounding each:
             <= (e_r + u) |1 - s| (1 + 3u) + 3u |1 - s| + u (|s| + |1 - s|)(1 + 3u)                                   ENV_BOUND decay
    release  r = 1/rel * ms: e_r = (4u + 7u^2) ms / rel; 1 - c: + u; times off_amplitude: + u
             <= |off| ((e_r + u)(1 + u) + u (1 + u))                                                                   ENV_BOUND release
  Mixer, master over n channels: each addend p_k = f32(x_k * g_k) carries u32 = 2^-24 relative to the exact x_k * g_k (the f64 product's
  own u is absorbed: (1 + u)(1 + u32) - 1 <= 1.0000001 u32) and g_k = fader * 10^(db/20) carries 2u (pow within 1 ULP, one product);
  n sequential f32 additions starting from +0.0 (the first is exact) carry (n - 1) u32 relative to sum |p_k| to first order:
    |master - sum x_k g_k| <= ((n - 1) u32 (1 + u32)^(n - 1) (1 + 2 u32) + 1.0000002 u32 + 14u) * sum |x_k g_k|     mixer_bound
  (the factor 1 + 2 u32 turns sum |p_k| into sum |x_k g_k|; of the 14u, 2u is the rounding of the f64 yardstick itself (math.fsum of products
  rounded once) and 12u the f64 quotient db / 20 in the exponent: |db| <= 96, so |db / 20| ln 10 <= 11.06 and 10^(x (1 + u)) is within 12u of 10^x).
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

import sin_reference

F64 = np.float64
F32 = np.float32
ONE, ZERO, TWO = F64(1.0), F64(0.0), F64(2.0)
PI = F64(math.pi)                                   # f64::consts::PI: the f64 nearest pi, and so is math.pi (0x400921FB54442D18)
assert PI.view(np.uint64) == 0x400921FB54442D18

WAVES = ("on", "off", "sine", "square", "triangle", "saw")      # the order of mixlab_amd.abi.WAVE_*

MIS_MODELS = {
    "envelope": ["gate_on_ge", "gate_off_ne", "off_amplitude_after_change", "off_amplitude_one_late", "retrigger_resumes", "ms_div_attack",
                 "ms_times_1000_first", "duration_f32", "clamp_nan_to_zero"],
    "mixer": ["accumulate_f64", "gain_f32", "cue_scaled", "reverse_order", "to_linear_exp"],
    "amplifier": ["control_at_i", "disconnected_control_zero", "depth_times_amplitude_first"],
    "oscillator": ["saw_half_even", "sign_zero_is_zero", "sign_negative_zero_is_plus", "argument_regrouped", "time_is_tick_index"],
    "fm_sine": ["fm_argument_regrouped", "fm_disconnected_one"],
}


def _u64_as_f64(n: int) -> np.float64:
    """`n as f64` of a u64: round to nearest even, which is what Python's int -> float conversion does"""
    assert 0 <= n < 1 << 64
    return F64(float(n))


# ---- Decibel::to_linear (protocol/src/lib.rs:469-471) ----
def decibel_to_linear(db, mis=None) -> np.float64:
    if mis == "to_linear_exp":
        return F64(math.exp(float(db) * math.log(10.0) / 20.0))
    return F64(math.pow(10.0, float(F64(db) / F64(20.0))))


# ---- Mixer (mixer.rs:46-71) ----
def mixer(channels, inputs, length, mis=None):
    """channels: [(gain_db, fader, cue)]; inputs: [f32 array | None (Disconnected: the zero buffer, engine/io.rs:47)] -> (master, cue)"""
    master = np.zeros(length, F32)                                  # util::zero, mixer.rs:54-55
    cue = np.zeros(length, F32)
    acc64 = np.zeros(length, F64)
    order = list(zip(channels, inputs))
    if mis == "reverse_order":
        order.reverse()
    with np.errstate(over="ignore", invalid="ignore"):
        for (db, fader, cue_on), x in order:                        # mixer.rs:57: in parameter order
            x = np.zeros(length, F32) if x is None else np.ascontiguousarray(x, F32)
            gain = F64(fader) * decibel_to_linear(db, mis)          # mixer.rs:59
            if mis == "gain_f32":
                gain = F64(F32(gain))
            prod = x.astype(F64) * gain                             # mixer.rs:62: input[i] as f64 * channel_gain
            if mis == "accumulate_f64":
                acc64 = acc64 + prod
            else:
                master = master + prod.astype(F32)                  # ... as Sample, then the f32 +=
            if cue_on:
                cue = cue + (prod.astype(F32) if mis == "cue_scaled" else x)    # mixer.rs:64-66: the raw input
        if mis == "accumulate_f64":
            master = acc64.astype(F32)
    return master, cue


def mixer_exact_master(channels, inputs, length):
    """-> (sum_k x_k * fader_k * 10^(db_k / 20), sum_k |...|) per sample in f64: math.fsum (exactly rounded) of the per-channel products, each formed
    with a 60-digit 10^(db/20) and rounded once, i.e. within u of exact"""
    import mpmath
    mpmath.mp.dps = 60
    gains = [mpmath.mpf(float(f)) * mpmath.power(10, mpmath.mpf(float(db)) / 20) for (db, f, _c) in channels]
    total, mag = np.empty(length, F64), np.empty(length, F64)
    for i in range(length):
        terms = [float(g * float(x[i])) for g, x in zip(gains, inputs) if x is not None]
        total[i], mag[i] = math.fsum(terms), math.fsum(abs(t) for t in terms)
    return total, mag


def mixer_bound(n_channels, magnitude):
    u32, u = 2.0 ** -24, 2.0 ** -53
    return ((n_channels - 1) * u32 * (1 + u32) ** max(0, n_channels - 1) * (1 + 2 * u32) + 1.0000002 * u32 + 14 * u) * magnitude


# ---- Envelope (envelope.rs:16-58, 91-120) ----
INITIAL, TRIGGER_ON, TRIGGER_OFF = 0, 1, 2


class EnvelopeState:
    """envelope.rs:9-13"""

    def __init__(self):
        self.tag, self.seq, self.off_amplitude = INITIAL, 0, ZERO
        self.stale_off_amplitude = ZERO           # only the mis-model off_amplitude_after_change reads it
        self.previous_on = 0                      # only the mis-model retrigger_resumes reads it

    def key(self):
        return (self.tag, self.seq, self.off_amplitude)


def _duration_ms(first: int, last: int, sr, mis) -> np.float64:
    """envelope.rs:16-18: (last - first) as f64 / SAMPLE_RATE as f64 * 1000.0"""
    d = _u64_as_f64(last - first)
    if mis == "ms_times_1000_first":
        return d * F64(1000.0) / F64(sr)
    if mis == "duration_f32":
        return F64(F32(d) / F32(sr) * F32(1000.0))
    return d / F64(sr) * F64(1000.0)


def _clamp(x, mis):
    """envelope.rs:20-28: a NaN is neither > 1.0 nor < 0.0 and passes"""
    if mis == "clamp_nan_to_zero" and np.isnan(x):
        return ZERO
    if x > ONE:
        return ONE
    if x < ZERO:
        return ZERO
    return x


def _amplitude(params, tag, seq, off_amplitude, t: int, sr, mis) -> np.float64:
    """envelope.rs:34-58"""
    attack, decay, sustain, release = params                                   # f64 each (envelope() converts once)
    if tag == INITIAL:
        return ZERO
    if tag == TRIGGER_ON:
        ms = _duration_ms(seq, t, sr, mis)
        if ms < attack:                                                        # :40
            return ms / attack if mis == "ms_div_attack" else ONE / attack * ms    # :42
        since_decay = ms - attack                                              # :45
        decay_amplitude = ONE - _clamp(ONE / decay * since_decay, mis)         # :46
        return sustain + ((ONE - sustain) * decay_amplitude)                   # :48
    ms = _duration_ms(seq, t, sr, mis)                                         # :52
    release_amplitude = ONE - _clamp(ONE / release * ms, mis)                  # :53
    return off_amplitude * release_amplitude                                   # :55


def envelope(state: EnvelopeState, params, sr, t: int, gate, n=None, mis=None, trace=None):
    """One run_tick (envelope.rs:91-120) from sample time t.  gate: f32 array, or None (Disconnected: zeros, engine/io.rs:38) with n samples.
    -> (f32 output, f64 amplitude); `state` is advanced; trace, a list, receives the (tag, seq, off_amplitude) each sample was evaluated in."""
    gate = np.zeros(n, F32) if gate is None else np.ascontiguousarray(gate, F32)
    params = tuple(F64(p) for p in params)
    out32, out64 = np.empty(gate.size, F32), np.empty(gate.size, F64)
    f1, f0 = F32(1.0), F32(0.0)
    with np.errstate(all="ignore"):
        for i in range(gate.size):
            seq = t + i                                                        # :97
            g = gate[i]
            if state.tag != TRIGGER_ON:                                        # :101-105
                if (g >= f1) if mis == "gate_on_ge" else (g == f1):
                    seq_on = state.previous_on if mis == "retrigger_resumes" and state.tag == TRIGGER_OFF else seq    # (the misreading: the ramp goes on from the previous on edge)
                    state.tag, state.seq, state.previous_on = TRIGGER_ON, seq_on, seq_on
            else:                                                              # :106-113
                if (g != f1) if mis == "gate_off_ne" else (g == f0):
                    if mis == "off_amplitude_after_change":
                        off = _amplitude(params, TRIGGER_OFF, seq, state.stale_off_amplitude, seq, sr, mis)
                    elif mis == "off_amplitude_one_late":
                        off = _amplitude(params, TRIGGER_ON, state.seq, ZERO, seq + 1, sr, mis)
                    else:
                        off = _amplitude(params, TRIGGER_ON, state.seq, ZERO, seq, sr, mis)     # :110: in the TriggerOn state, before the change
                    state.tag, state.seq, state.off_amplitude = TRIGGER_OFF, seq, off
                    state.stale_off_amplitude = off
            if trace is not None:
                trace.append(state.key())
            a = _amplitude(params, state.tag, state.seq, state.off_amplitude, seq, sr, mis)
            out64[i] = a
            out32[i] = F32(a)                                                  # :116
    return out32, out64


def envelope_exact(params, key, t: int, sr):
    """-> (the expression of envelope.rs:34-58 in exact rational arithmetic over the f64 parameters and the f64 off_amplitude of `key`, the branch,
    the figures envelope_bound needs, whether the exact ms picks the same side of envelope.rs:40 as the model's f64 ms).  The attack / decay branch is
    the one the MODEL's f64 `ms < attack` took, so that the bound speaks of one expression's roundings; where the exact ms falls on the other side it
    has to be within the rounding of ms of the attack time, which the test asserts."""
    tag, seq, off = key
    a, dcy, s, rel = (Fraction(float(p)) for p in params)
    if tag == INITIAL:
        return Fraction(0), "initial", (), True
    ms = Fraction(t - seq) * 1000 / sr
    clamp = lambda x: min(Fraction(1), max(Fraction(0), x))
    if tag == TRIGGER_ON:
        in_attack = bool(_duration_ms(seq, t, sr, None) < F64(float(a)))
        same_side = in_attack == (ms < a) or abs(ms - a) <= 2 * Fraction(1, 1 << 53) * ms * (1 + Fraction(1, 1 << 53))
        if in_attack:
            return ms / a, "attack", (ms, a), same_side
        return s + (1 - s) * (1 - clamp((ms - a) / dcy)), "decay", (ms, a, dcy, s), same_side
    return Fraction(float(off)) * (1 - clamp(ms / rel)), "release", (ms, rel, Fraction(float(off))), True


def envelope_bound(branch, figures) -> Fraction:
    """the derived one-step bound of the module docstring, in exact rationals (so the assertion itself rounds nothing)"""
    u = Fraction(1, 1 << 53)
    if branch == "initial":
        return Fraction(0)
    if branch == "attack":
        ms, a = figures
        return (4 * u + 7 * u * u) * ms / a
    if branch == "decay":
        ms, a, dcy, s = figures
        e_ms = 2 * u * ms * (1 + u)
        x = abs(ms - a)
        e_x = e_ms + u * (x + e_ms)
        r = x / dcy
        e_r = e_x / dcy * (1 + 2 * u) + 2 * u * (r + e_x / dcy) * (1 + u)
        return (e_r + u) * abs(1 - s) * (1 + 3 * u) + 3 * u * abs(1 - s) + u * (abs(s) + abs(1 - s)) * (1 + 3 * u)
    ms, rel, off = figures
    e_r = (4 * u + 7 * u * u) * ms / rel
    return abs(off) * ((e_r + u) * (1 + u) + u * (1 + u))


# ---- Amplifier (amplifier.rs:38-73) ----
def amplifier(amplitude, mod_depth, x, ctl, mis=None):
    """x: interleaved stereo; ctl: mono of half the length, or None (Disconnected: 1.0, amplifier.rs:54)"""
    x = np.ascontiguousarray(x, F32)
    amp, dep = F64(amplitude), F64(mod_depth)
    if ctl is None:
        value = np.full(x.size, 0.0 if mis == "disconnected_control_zero" else 1.0, F64)
    else:
        ctl = np.ascontiguousarray(ctl, F32)
        idx = np.arange(x.size) % ctl.size if mis == "control_at_i" else np.arange(x.size) // 2     # :54: buff[i / 2]
        value = ctl[idx].astype(F64)
    with np.errstate(all="ignore"):
        depth = ONE - dep + dep * value                                        # :71-73: (1.0 - depth) + (depth * value)
        if mis == "depth_times_amplitude_first":
            return (x.astype(F64) * (depth * amp)).astype(F32)
        return (x.astype(F64) * depth * amp).astype(F32)                       # :56: left to right


# ---- the sine: correctly rounded f32 of the real sine, and its sign ----
_SIN_CACHE: dict = {}


def _sin32_and_sign(arg: float):
    """-> (f32 of the real sine of the f64 `arg`, is the sine's sign bit set).  The sine is odd, exactly: keyed by |arg|.  Of a finite non-zero f64 the real
    sine is never zero and its f64 rounding keeps the sign; sin(+-0) = +-0."""
    arg = float(arg)
    if arg == 0.0:
        return F32(arg), math.copysign(1.0, arg) < 0
    a = abs(arg)
    if a not in _SIN_CACHE:
        d = sin_reference.sin_decimal(a)
        _SIN_CACHE[a] = (sin_reference.round_to_f32(d), d, d < 0)
    s32, _d, neg = _SIN_CACHE[a]
    return (s32, neg) if arg > 0 else (F32(-s32), not neg)


def sin_decimal_cached(arg: float):
    """the 130-digit sine of |arg| that _sin32_and_sign used (audio_cases.sine_margin reads it)"""
    _sin32_and_sign(arg)
    return _SIN_CACHE[abs(float(arg))][1]


# ---- Oscillator (oscillator.rs:15-37, 65-92) ----
def _times(t: int, n: int) -> np.ndarray:
    """(t + i as u64) as f64"""
    return np.array([float(_u64_as_f64(t + i)) for i in range(n)], F64)


def oscillator_argument(freq, sr, t: int, n: int, mis=None) -> np.ndarray:
    """-> the f64 handed to sin, per sample: t0 = (t + i) as f64 / SAMPLE_RATE as f64 (:74); n = t0 * freq (:75); n * 2.0 * PI (:26)"""
    if mis == "argument_regrouped":
        return _times(t, n) * (F64(freq) * TWO * PI / F64(sr))
    return (_times(t, n) / F64(sr)) * F64(freq) * TWO * PI


def oscillator(freq, wave: str, sr, t: int, n: int, spt=None, mis=None):
    """-> (mono, stereo): the sample on both channels (oscillator.rs:86-88).  t is the SAMPLE time of the tick's first sample (engine.rs:490)."""
    if mis == "time_is_tick_index":
        t = t // spt
    if wave in ("sine", "square"):
        arg = oscillator_argument(freq, sr, t, n, mis)
        if wave == "sine":
            mono = np.array([_sin32_and_sign(a)[0] for a in arg], F32)
        else:                                                                   # :15-23: is_sign_positive / is_sign_negative, -0.0 is negative
            def sign(a):
                _s, neg = _sin32_and_sign(a)
                if a == 0.0 and mis == "sign_zero_is_zero":
                    return 0.0
                if a == 0.0 and neg and mis == "sign_negative_zero_is_plus":
                    return 1.0
                return -1.0 if neg else 1.0
            mono = np.array([sign(a) for a in arg], F32)
    elif wave in ("saw", "triangle"):
        nn = (_times(t, n) / F64(sr)) * F64(freq)                              # :74-75
        whole = np.rint(nn) if mis == "saw_half_even" else np.floor(F64(0.5) + nn)
        saw = TWO * (nn - whole)                                               # :30-32
        mono = (saw if wave == "saw" else TWO * np.abs(saw) - ONE).astype(F32)  # :35-37
    else:
        mono = np.full(n, 1.0 if wave == "on" else 0.0, F32)                   # :82-83
    return mono, np.repeat(mono, 2)


# ---- FmSine (fm_sine.rs:37-56) ----
def fm_sine_argument(freq_lo, freq_hi, sr, t: int, x, n: int, mis=None) -> np.ndarray:
    if x is None:
        x = np.full(n, 1.0 if mis == "fm_disconnected_one" else 0.0, F32)      # Disconnected: zeros (engine/io.rs:38)
    x = np.ascontiguousarray(x, F32)
    amp = (F64(freq_hi) - F64(freq_lo)) / TWO                                  # :42
    mid = F64(freq_lo) + amp                                                   # :43
    tt = _times(t, n) / F64(sr)                                                # :46
    if mis == "fm_argument_regrouped":
        return TWO * PI * ((mid + amp * x.astype(F64)) * tt)
    co = (mid + amp * x.astype(F64)) * TWO * PI                                # :47
    return co * tt                                                             # :48


def fm_sine(freq_lo, freq_hi, sr, t: int, x, n: int, mis=None) -> np.ndarray:
    """-> interleaved stereo"""
    arg = fm_sine_argument(freq_lo, freq_hi, sr, t, x, n, mis)
    return np.repeat(np.array([_sin32_and_sign(a)[0] for a in arg], F32), 2)


# ---- Trigger, StereoPanner, StereoSplitter (trigger.rs:35-48, stereo_panner.rs:30-41, stereo_splitter.rs:33-47) ----
def trigger(gate_open: bool, n: int) -> np.ndarray:
    return np.full(n, 1.0 if gate_open else 0.0, F32)


def stereo_panner(left, right, n: int) -> np.ndarray:
    out = np.zeros(2 * n, F32)
    out[0::2] = 0.0 if left is None else left
    out[1::2] = 0.0 if right is None else right
    return out


def stereo_splitter(x, n: int):
    x = np.zeros(2 * n, F32) if x is None else np.ascontiguousarray(x, F32)
    return x[0::2].copy(), x[1::2].copy()


# ---- EqThree (eq_three.rs) ----
FREQ_LO, FREQ_HI = F64(420.0), F64(2700.0)                                    # :8-9
VSA = ONE / F64(4294967295.0)                                                  # :11


class EqThreeState:
    def __init__(self, sr):
        # :113-115: 2.0 * sin(PI * freq / SAMPLE_RATE); the arguments are small and the test file holds math.sin to mpmath's correctly rounded value there
        self.f_lo = TWO * F64(math.sin(float(PI * FREQ_LO / F64(sr))))
        self.f_hi = TWO * F64(math.sin(float(PI * FREQ_HI / F64(sr))))
        self.lo = [ZERO] * 4
        self.hi = [ZERO] * 4
        self.history = [ZERO] * 3


def _pump(poles, f, sample):
    """eq_three.rs:117-124"""
    poles[0] = poles[0] + (f * (sample - poles[0]) + VSA)
    poles[1] = poles[1] + f * (poles[0] - poles[1])
    poles[2] = poles[2] + f * (poles[1] - poles[2])
    poles[3] = poles[3] + f * (poles[2] - poles[3])
    return poles[3]


def eq_three(state: EqThreeState, gains_db, x) -> np.ndarray:
    """eq_three.rs:58-89; x None: Disconnected is not modelled here (callers pass zeros)"""
    x = np.ascontiguousarray(x, F32)
    g_lo, g_mid, g_hi = (decibel_to_linear(g) for g in gains_db)               # :62-64
    out = np.empty(x.size, F32)
    h = state.history
    with np.errstate(all="ignore"):
        for i in range(x.size):
            sample = F64(x[i])                                                 # :67
            lo = _pump(state.lo, state.f_lo, sample)                           # :69
            hi = h[0] - _pump(state.hi, state.f_hi, sample)                    # :70
            mid = h[0] - (hi + lo)                                             # :72
            h[0], h[1], h[2] = h[1], h[2], sample                              # :75-77
            out[i] = F32(lo * g_lo + mid * g_mid + hi * g_hi)                  # :81-85: (lo + mid) + hi
    return out


# ---- the config-2 strip: Trigger -> Envelope ; Source -> EqThree -> Panner(L = R) -> Amplifier(ctl = Envelope) -> Mixer ----
class StripState:
    def __init__(self, sr):
        self.env, self.eq = EnvelopeState(), EqThreeState(sr)


def strip(states, sr, spt, first_tick: int, gates, sources, eq_gains, env_params, amp_params, mixer_channels):
    """Run the strip graph tick by tick.  states: [StripState] carried by the caller; gates: [n_ticks][n_strips] bool (the Trigger's parameter
    during that tick); sources: [n_strips] f32 arrays of n_ticks * spt samples.
    -> {"trigger" | "envelope" | "eq" | "panner" | "amplifier": [per strip, whole stretch], "master", "cue"}"""
    n_ticks, n_strips = len(gates), len(states)
    per = {k: [[] for _ in range(n_strips)] for k in ("trigger", "envelope", "eq", "panner", "amplifier")}
    master, cue = [], []
    for k in range(n_ticks):
        t = (first_tick + k) * spt                                             # engine.rs:490
        amp_out = []
        for s in range(n_strips):
            trig = trigger(gates[k][s], spt)
            env, _ = envelope(states[s].env, env_params, sr, t, trig)
            eq = eq_three(states[s].eq, eq_gains[s], sources[s][k * spt:(k + 1) * spt])
            pan = stereo_panner(eq, eq, spt)
            amp = amplifier(amp_params[0], amp_params[1], pan, env)
            for name, v in (("trigger", trig), ("envelope", env), ("eq", eq), ("panner", pan), ("amplifier", amp)):
                per[name][s].append(v)
            amp_out.append(amp)
        m, c = mixer(mixer_channels, amp_out, 2 * spt)
        master.append(m); cue.append(c)
    out = {name: [np.concatenate(v) for v in lists] for name, lists in per.items()}
    out["master"], out["cue"] = np.concatenate(master), np.concatenate(cue)
    return out
