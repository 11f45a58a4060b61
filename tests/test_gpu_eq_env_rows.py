"""The ROW FORM of the inline Envelope in the tiled speculative EqThree kernel (mx_k_eq_exact.hip: eq_env_rows): where at most two
waves share a SIMD the wave keeps a control tile, fills every row with its constant at the tick's start and evaluates only the rows
that ramp, row by row, in passes that know their phase.  It changes who evaluates the closed form and for which rows, never a
rounding: every case is compared bit for bit with oracle.OracleGraph, and asserts through mx_graph_debug_eq_env_rows that the row
form really ran (or, where the case says so, that it did not).

Strips are source -> EqThree -> StereoPanner -> Amplifier with Trigger -> Envelope on the control, 48 kHz, 800 samples per tick.
A wave is 64 chunks of ONE strip, so with one-tick chunks lane j of wave w is tick 64 w + j: the gate schedule decides which Envelope
phases sit side by side in a wave.  `phases()` below is a numpy model of the schedule (the class of every tick at its first and last
sample) that the cases check BEFORE the GPU run, so that a schedule that stops producing its classes fails instead of passing on
less."""
import numpy as np
import pytest

import oracle
import synth
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import assert_bit_exact

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def one_tile(request, monkeypatch):
    """The launcher takes the row form where the one-tile form is its choice anyway: more than one wave per SIMD, or MX_EQ_SPEC_SB=321.  These
    graphs are a wave or two, which on their own would get two tiles and the lockstep form -- test_the_launchers_own_choice
    runs without the override."""
    if not request.node.name.startswith("test_the_launchers_own_choice"):
        monkeypatch.setenv("MX_EQ_SPEC_SB", "321")

SR, SPT = 48000, 800
DEFAULT_ENV = (25.0, 500.0, 0.8, 200.0)


def phases(toggles, T, env_p=DEFAULT_ENV, first_tick=0, gate0=0):
    """-> the class of every tick of a run: 'never' | 'attack' | 'crossing' (attack -> decay inside the tick, not on a super-block
    boundary) | 'decay' | 'sustain' | 'release' | 'released'.  `toggles`: {tick in run: gate}; ms as envelope.rs:16-18 computes it."""
    attack, decay, _, release = env_p
    tag, seq, gate, out = 0, 0, gate0, []
    for t in range(T):
        gate = toggles.get(t, gate)
        now = (first_tick + t) * SPT
        if tag != 1 and gate == 1: tag, seq = 1, now
        elif tag == 1 and gate == 0: tag, seq = 2, now
        ms = (np.arange(now, now + SPT, dtype=np.float64) - seq) / SR * 1000.0
        if tag == 0: out.append("never")
        elif tag == 1:
            if ms[-1] < attack: out.append("attack")
            elif ms[0] < attack:
                k = int(np.argmax(ms >= attack))          # first sample at or beyond attack_ms
                out.append("crossing" if k % 32 else "attack")
            else: out.append("sustain" if (ms[0] - attack) / decay >= 1.0 else "decay")
        else: out.append("released" if ms[0] / release >= 1.0 else "release")
    return out


RAMPING = ("attack", "crossing", "decay", "release")


def build_strips(n, env_p=DEFAULT_ENV, T=64, flags=0, mono_dup=False, kinds=None):
    """`kinds`: strip j gets the parameters of strip j % kinds (many strips of a few kinds)"""
    ws = Workspace(SR, 60)
    strips = []
    for j in range(n):
        k = j % kinds if kinds else j
        src = ws.source_mono(); eq = ws.eq_three(2.0 - k, -1.0 + 0.5 * k, 3.0 - 0.25 * k); pan = ws.stereo_panner()
        trig = ws.trigger(False); env = ws.envelope(*env_p); amp = ws.amplifier(0.9 + 0.05 * k, 0.8 - 0.1 * k)
        ws.connect(src, 0, eq, 0); ws.connect(eq, 0, pan, 0); ws.connect(eq, 0, pan, 1); ws.connect(pan, 0, amp, 0)
        ws.connect(trig, 0, env, 0); ws.connect(env, 0, amp, 1)
        strips.append((src, trig, amp))
    if mono_dup:   # read by a Mixer only: the fused result is stored as one float per frame (L == R)
        mix = ws.mixer([(0.0, 1.0, False)] * n)
        for k, (_, _, amp) in enumerate(strips):
            ws.connect(amp, 0, mix, k)
    return ws, strips, ws.build(max_ticks_per_run=T, flags=flags)


def run_and_compare(ws, strips, g, toggles, T, runs=((0, None),), seed=4100, what=""):
    """`toggles`: per strip {tick in run: gate}, applied in every run; runs: (first_tick, rows expected after it or None).  Every
    Amplifier output of every run against the oracle graph, bit for bit.  -> the outputs, for A/B comparisons."""
    og = oracle.OracleGraph(ws)
    outs = []
    for r, (t0, want_rows) in enumerate(runs):
        x = [synth.noise(seed + 16 * r + k, T * SPT) for k in range(len(strips))]
        for k, (src, trig, _) in enumerate(strips):
            g.write_source(src, x[k], T)
            for t, v in toggles[k].items():
                g.schedule_params(trig, t, abi.TriggerParams(v))
        g.run_ticks(t0, T)
        got = [g.read_output(amp, 0, T, True) for (_, _, amp) in strips]
        rows = g.debug_eq_env_rows()
        print(f"{what} run {r} from tick {t0}: {g.debug_eq_launch()} rows {rows} {g.eq_repair_stats()}")
        for t in range(T):
            for k, (src, trig, _) in enumerate(strips):
                if t in toggles[k]: og.update_params(trig, abi.TriggerParams(toggles[k][t]))
                og.set_source(src, x[k][t * SPT:(t + 1) * SPT])
            og.run_tick(t0 + t)
            for k, (_, _, amp) in enumerate(strips):
                gv, w = got[k][t * 2 * SPT:(t + 1) * 2 * SPT], og.output(amp, 0)
                msg = f"{what} run {r} strip {k} tick {t} ({phases(toggles[k], T)[t] if t0 == 0 and r == 0 else ''})"
                # (infinite slopes make NaNs; their sign and payload are the ISA's business, as in test_gpu_eq_exact_spec.py: same samples, every other sample bit for bit)
                ok = ~np.isnan(w)
                assert np.array_equal(np.isnan(gv), ~ok), f"{msg}: NaNs at different samples"
                assert_bit_exact(gv[ok], w[ok], msg)
        if want_rows is not None:
            assert rows == want_rows, f"{what} run {r}: the row form {'did not run' if want_rows else 'ran'}"
        outs.append(got)
    return outs


# 1 ------------------------------------------------------------------------------------------------
def test_every_phase_side_by_side_in_one_wave(monkeypatch):
    """One strip, 96 one-tick chunks: wave 0 is ticks 0 .. 63, wave 1 ticks 64 .. 95 with 32 idle lanes.  Gate on at tick 2 and held
    for 36 ticks (attack 1.5 ticks -- the default 25 ms is sample 400 of the second tick, the middle of super-block 12 -- decay to tick
    33.5, then sustain), off at 38 (release 12 ticks, then released); again on at 70, off at 80 in mid-decay."""
    T, toggles = 96, {2: 1, 38: 0, 70: 1, 80: 0}
    ph = phases(toggles, T)
    for w in (ph[:64],):
        assert set(w) == {"never", "attack", "crossing", "decay", "sustain", "release", "released"}, sorted(set(w))
    assert {"attack", "crossing", "decay", "release", "released"} <= set(ph[64:]), sorted(set(ph[64:]))
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", "96")
    ws, strips, g = build_strips(1, T=T)
    run_and_compare(ws, strips, g, [toggles], T, runs=((0, True),), what="every phase")
    launch = g.debug_eq_launch()
    assert launch["form"] == "tiled" and launch["chunk"] == SPT and launch["n_chunks"] == 96, launch


# 2 ------------------------------------------------------------------------------------------------
SHORT_ENV = (2.5, 6.0, 0.6, 8.0)    # attack + decay and the release end inside one tick: a toggle makes exactly one tick ramp
LONG_ENV = (25.0, 4000.0, 0.5, 4000.0)   # four seconds of decay: every tick of a 64-tick run ramps


@pytest.mark.parametrize("name,env_p,toggles,n_ramping,kinds,rows", [
    ("one_row", SHORT_ENV, {10: 1}, 1, {"crossing"}, True),                       # the half pass
    ("two_rows_two_phases", SHORT_ENV, {10: 1, 20: 0}, 2, {"crossing", "release"}, True),
    ("all_64_rows", LONG_ENV, {0: 1}, 64, {"attack", "crossing", "decay"}, True),
    ("no_row", DEFAULT_ENV, {}, 0, set(), False),                                 # every lane flat: the constant-depth form, not rows
])
def test_row_count_edges(name, env_p, toggles, n_ramping, kinds, rows, monkeypatch):
    T = 64
    ph = phases(toggles, T, env_p)
    ramping = [p for p in ph if p in RAMPING]
    assert len(ramping) == n_ramping and set(ramping) == kinds, ph
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", "64")     # one wave of one-tick chunks
    ws, strips, g = build_strips(1, env_p, T)
    run_and_compare(ws, strips, g, [toggles], T, runs=((0, rows),), what=name)
    assert g.debug_eq_launch()["form"] == "tiled"


# 3 ------------------------------------------------------------------------------------------------
def test_multi_tick_chunks_change_tick_inside_a_chunk(monkeypatch):
    """Eight chunks of eight ticks: eight active lanes, and every lane's tick -- its table entry, its constant, its class -- changes
    seven times inside its chunk."""
    T = 64
    toggles = [{3: 1, 21: 0, 30: 1, 52: 0}, {0: 1, 9: 0, 17: 1, 18: 0, 40: 1}]
    for tg in toggles:
        assert {"attack", "crossing", "decay", "release"} <= set(phases(tg, T))
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", "8")
    ws, strips, g = build_strips(2, T=T)
    run_and_compare(ws, strips, g, toggles, T, runs=((0, True), (T, True)), what="8-tick chunks")
    launch = g.debug_eq_launch()
    assert launch["chunk"] == 8 * SPT and launch["n_chunks"] == 8, launch


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mono_dup", [False, True], ids=["interleaved", "mono_dup"])
@pytest.mark.parametrize("flags", [0, abi.FLAG_FP_CONTRACT], ids=["exact", "contracted"])
def test_store_forms_and_orders(flags, mono_dup, monkeypatch):
    T = 64
    toggles = [{2: 1, 38: 0}, {0: 1, 5: 0, 30: 1}]
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", "64")
    ws, strips, g = build_strips(2, T=T, flags=flags, mono_dup=mono_dup)
    # the premise: read by a Mixer only, the Amplifier's port is stored as one float per frame and has no stereo buffer to hand out
    if mono_dup:
        with pytest.raises(abi.MxError):
            g.output_device_ptr(strips[0][2], 0)
    else:
        assert g.output_device_ptr(strips[0][2], 0)[0]
    with oracle.fp_contract(bool(flags & abi.FLAG_FP_CONTRACT)):
        run_and_compare(ws, strips, g, toggles, T, runs=((0, True),), what=f"flags {flags} mono_dup {mono_dup}")


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_p,rows", [((5.0, 0.0, 0.7, 0.0), False),      # zero decay / release times: infinite slopes, every tick in the general form
                                        ((10.0, 40.0, 1.5, 30.0), True)])   # sustain above 1: finite, non-negative slopes and a positive off_amplitude -- the row form, no silent fallback
def test_unusual_parameters_fall_back_to_the_general_form(env_p, rows, monkeypatch):
    T = 64
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", "64")
    ws, strips, g = build_strips(1, env_p, T)
    run_and_compare(ws, strips, g, [{4: 1, 30: 0, 31: 1, 50: 0}], T, runs=((0, rows),), what=f"envelope {env_p}")


def test_distances_past_2_to_the_32_take_the_general_form(monkeypatch):
    """The gate opens in a first submission at tick 0; the second begins 2^32 samples later: its On lanes are more than 32 bits from their
    trigger (the general form, 64-bit distances), the lanes behind the gate's closing in that run are a release a few ticks old.  One wave
    of one-tick chunks is one wave-tick: a general lane in it sends the whole wave to the general form."""
    T = 64
    far = (1 << 32) // SPT + 1
    assert far * SPT > (1 << 32)
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", "64")
    ws, strips, g = build_strips(1, T=T)
    og = oracle.OracleGraph(ws)
    src, trig, amp = strips[0]
    for r, (t0, toggles, want_rows) in enumerate([(0, {0: 1}, True), (far, {20: 0}, False)]):
        x = synth.noise(4300 + r, T * SPT)
        g.write_source(src, x, T)
        for t, v in toggles.items():
            g.schedule_params(trig, t, abi.TriggerParams(v))
        g.run_ticks(t0, T)
        got = g.read_output(amp, 0, T, True)
        rows = g.debug_eq_env_rows()
        print(f"far clock run {r}: {g.debug_eq_launch()} rows {rows}")
        for t in range(T):
            if t in toggles: og.update_params(trig, abi.TriggerParams(toggles[t]))
            og.set_source(src, x[t * SPT:(t + 1) * SPT])
            og.run_tick(t0 + t)
            assert_bit_exact(got[t * 2 * SPT:(t + 1) * 2 * SPT], og.output(amp, 0), f"run {r} tick {t0 + t}")
        assert rows == want_rows, f"run {r}: rows {rows}"


# 6 ------------------------------------------------------------------------------------------------
def test_repair_over_the_row_form(monkeypatch):
    """A warm-up of 64 samples proves no boundary: the repair pass re-derives every chunk through its own emitters, over outputs the row
    form wrote first."""
    T = 48
    monkeypatch.setenv("MX_EQ_SPEC_WARM", "64")
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", "24")
    toggles = [{2: 1, 20: 0, 33: 1}, {0: 1, 40: 0}]
    ws, strips, g = build_strips(2, T=T)
    run_and_compare(ws, strips, g, toggles, T, runs=((0, True), (T, True)), what="repair")
    st = g.eq_repair_stats()
    assert st["chunks_repaired"] >= st["chunks_run"] // 2, st


# 7 ------------------------------------------------------------------------------------------------
def test_rows_switch_changes_no_byte(monkeypatch):
    """MX_EQ_ENV_ROWS=0 (read when the graph is built) keeps the lockstep form: the same job gives the same bytes, in the first submission
    and in a second one that starts from the state the first carried (EqThree poles, Envelope states)."""
    T = 64
    toggles = [{2: 1, 38: 0}, {0: 1, 9: 0, 17: 1, 18: 0, 40: 1}, {}]
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", "64")
    outs = {}
    for sw in ("0", None):
        if sw is None: monkeypatch.delenv("MX_EQ_ENV_ROWS", raising=False)
        else: monkeypatch.setenv("MX_EQ_ENV_ROWS", sw)
        ws, strips, g = build_strips(3, T=T)
        outs[sw] = run_and_compare(ws, strips, g, toggles, T, runs=((0, sw is None), (T, sw is None)), what=f"MX_EQ_ENV_ROWS={sw}")
        g.close()
    for r in range(2):
        for k in range(3):
            assert outs["0"][r][k].tobytes() == outs[None][r][k].tobytes(), f"run {r} strip {k}"


# 8 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,T,chunks,waves,rows", [(2, 64, "64", 2, False),          # a wave alone on its SIMD: two tiles, lockstep (the parent's launch)
                                                   (513, 128, "128", 1026, True),    # more than one wave per SIMD, at most two: one tile, rows
                                                   (513, 128, "128", 1026, False)],  # ... and MX_EQ_ENV_ROWS=0 keeps the lockstep form there
                         ids=["one_wave_per_simd", "two_waves_per_simd", "two_waves_per_simd_rows_off"])
def test_the_launchers_own_choice(n, T, chunks, waves, rows, monkeypatch):
    """No MX_EQ_SPEC_SB: launch_eq_three_spec's own rule.  1 024 SIMDs: 513 strips in two waves each are 1 026 waves.  The strips are of four kinds
    (parameters, input, gate schedule by j % 4): the first four are compared with the oracle graph of a four-strip workspace, every other one byte
    for byte with its twin among them."""
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", chunks)
    if waves > 1024 and not rows:
        monkeypatch.setenv("MX_EQ_ENV_ROWS", "0")
    toggles = [{2: 1, 38: 0, 70: 1, 80: 0}, {0: 1, 9: 0, 17: 1, 18: 0, 40: 1}, {}, {5: 1}]
    ws, strips, g = build_strips(n, T=T, kinds=4)
    x = [synth.noise(4400 + k, T * SPT) for k in range(4)]
    for j, (src, trig, _) in enumerate(strips):
        g.write_source(src, x[j % 4], T)
        for t, v in toggles[j % 4].items():
            if t < T: g.schedule_params(trig, t, abi.TriggerParams(v))
    g.run_ticks(0, T)
    launch = g.debug_eq_launch()
    print(launch, g.debug_eq_env_rows())
    assert launch["form"] == "tiled" and launch["n_chunks"] == int(chunks) and n * ((launch["n_chunks"] + 63) // 64) == waves, launch
    assert launch["super_block"] == (321 if waves > 1024 else 32), launch
    assert g.debug_eq_env_rows() == rows
    got = [g.read_output(amp, 0, T, True) for (_, _, amp) in strips]
    ws4, strips4, _ = build_strips(min(n, 4), T=T, kinds=4)
    og = oracle.OracleGraph(ws4)
    for t in range(T):
        for k, (src, trig, _) in enumerate(strips4):
            if t in toggles[k]: og.update_params(trig, abi.TriggerParams(toggles[k][t]))
            og.set_source(src, x[k][t * SPT:(t + 1) * SPT])
        og.run_tick(t)
        for k, (_, _, amp) in enumerate(strips4):
            assert_bit_exact(got[k][t * 2 * SPT:(t + 1) * 2 * SPT], og.output(amp, 0), f"strip {k} tick {t}")
    for j in range(4, n):
        assert got[j].tobytes() == got[j % 4].tobytes(), f"strip {j} differs from its twin {j % 4}"
