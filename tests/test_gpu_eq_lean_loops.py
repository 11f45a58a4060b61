"""The LEAN forms of the tiled speculative EqThree kernel's whole-tick loops (mx_k_eq_exact.hip: eq_tile_compute TRACK / UNITY): the
input tracker is dropped for the ticks at whose start every lane of the wave has already seen two different input patterns, and the
multiply by an Amplifier amplitude of exactly 1.0 is dropped.  Both are exact no-ops for the result: every output here is compared
bit for bit with oracle.OracleGraph and byte for byte with MX_EQ_LEAN=0, the chunk records' min / max are checked against numpy's
answer to "was this chunk's input constant", and mx_graph_debug_eq_lean says whether the lean loops really ran.

Strips are those of test_gpu_eq_env_rows.py (source -> EqThree -> StereoPanner -> Amplifier, Trigger -> Envelope on the control, 48 kHz),
with chunks of THREE ticks: the decision is taken per tick and changes inside a chunk.  A wave is 64 chunks of one strip; lane j of
wave w walks ticks 3 (64 w + j) .. + 2, and the wave's k-th tick is flat (the constant-depth loop) when no lane's tick 3 j + k ramps."""
import ctypes as C

import numpy as np
import pytest

import oracle
import synth
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import assert_bit_exact
from test_gpu_eq_env_rows import LONG_ENV, RAMPING, SHORT_ENV, phases

pytestmark = pytest.mark.gpu

SR, SPT = 48000, 800
CT = 3                      # ticks per chunk
REC_BYTES = 144             # EqChunkRec: start[8], end[8], xmin, xmax, pad[2]


@pytest.fixture(autouse=True)
def one_tile_three_tick_chunks(monkeypatch):
    """One whole-line tile (the row form's and the headline's shape) for graphs of a few waves, as in test_gpu_eq_env_rows.py."""
    monkeypatch.setenv("MX_EQ_SPEC_SB", "321")
    monkeypatch.delenv("MX_EQ_LEAN", raising=False)


def build(amplitudes, T, env_p=SHORT_ENV, flags=0, mono_dup=True):
    ws = Workspace(SR, 60)
    strips = []
    for k, a in enumerate(amplitudes):
        src = ws.source_mono(); eq = ws.eq_three(2.0 - k, -1.0 + 0.5 * k, 3.0 - 0.25 * k); pan = ws.stereo_panner()
        trig = ws.trigger(False); env = ws.envelope(*env_p); amp = ws.amplifier(a, 0.8 - 0.1 * k)
        ws.connect(src, 0, eq, 0); ws.connect(eq, 0, pan, 0); ws.connect(eq, 0, pan, 1); ws.connect(pan, 0, amp, 0)
        ws.connect(trig, 0, env, 0); ws.connect(env, 0, amp, 1)
        strips.append((src, trig, amp))
    if mono_dup:   # read by a Mixer only: one float per frame, the headline's instantiation
        mix = ws.mixer([(0.0, 1.0, False)] * len(amplitudes))
        for k, (_, _, amp) in enumerate(strips):
            ws.connect(amp, 0, mix, k)
    return ws, strips, ws.build(max_ticks_per_run=T, flags=flags)


def run_device(g, strips, x, toggles, T):
    for k, (src, trig, _) in enumerate(strips):
        g.write_source(src, x[k], T)
        for t, v in toggles[k].items():
            g.schedule_params(trig, t, abi.TriggerParams(v))
    g.run_ticks(0, T)
    return [g.read_output(amp, 0, T, True) for (_, _, amp) in strips]


def run_oracle(ws, strips, x, toggles, T):
    og = oracle.OracleGraph(ws)
    out = [np.empty(T * 2 * SPT, np.float32) for _ in strips]
    for t in range(T):
        for k, (src, trig, _) in enumerate(strips):
            if t in toggles[k]: og.update_params(trig, abi.TriggerParams(toggles[k][t]))
            og.set_source(src, x[k][t * SPT:(t + 1) * SPT])
        og.run_tick(t)
        for k, (_, _, amp) in enumerate(strips):
            out[k][t * 2 * SPT:(t + 1) * 2 * SPT] = og.output(amp, 0)
    return out


def compare(got, want, what):
    """the rule of test_gpu_eq_env_rows.py: NaNs at the same samples (their sign and payload are the ISA's business), every other sample bit for bit"""
    for k, (gv, w) in enumerate(zip(got, want)):
        ok = ~np.isnan(w)
        assert np.array_equal(np.isnan(gv), ~ok), f"{what} strip {k}: NaNs at different samples"
        assert_bit_exact(gv[ok], w[ok], f"{what} strip {k}")


def lean_and_plain(amplitudes, T, x, toggles, monkeypatch, n_chunks, **kw):
    """the same job with the lean loops and with MX_EQ_LEAN=0 -> {switch: (outputs, debug_eq_lean, debug_eq_env_rows, repair stats, chunk records)}; the oracle's outputs"""
    monkeypatch.setenv("MX_EQ_SPEC_CHUNKS", str(n_chunks))
    res, ws = {}, None
    for sw in (None, "0"):
        if sw is None: monkeypatch.delenv("MX_EQ_LEAN", raising=False)
        else: monkeypatch.setenv("MX_EQ_LEAN", sw)
        ws, strips, g = build(amplitudes, T, **kw)
        got = run_device(g, strips, x, toggles, T)
        launch = g.debug_eq_launch()
        assert launch["form"] == "tiled" and launch["super_block"] == 321 and launch["chunk"] == CT * SPT and launch["n_chunks"] == n_chunks, launch
        p, nbytes = g.debug_eq_records()
        rec = np.empty(len(amplitudes) * n_chunks * REC_BYTES, np.uint8)
        assert nbytes >= rec.size
        abi.check(abi.lib.mx_device_download(rec.ctypes.data_as(C.c_void_p), C.c_void_p(p), C.c_size_t(rec.size), None))
        mm = rec.reshape(-1, REC_BYTES)[:, 128:136].copy().view(np.uint32).reshape(len(amplitudes), n_chunks, 2)
        res[sw] = (got, g.debug_eq_lean(), g.debug_eq_env_rows(), g.eq_repair_stats(), mm)
        print(f"MX_EQ_LEAN={sw}: {launch} lean {res[sw][1]} rows {res[sw][2]} {res[sw][3]}")
        g.close()
    assert res["0"][1] == {"untracked": False, "unity": False}, "MX_EQ_LEAN=0 ran a lean loop"
    for k in range(len(amplitudes)):
        assert res[None][0][k].tobytes() == res["0"][0][k].tobytes(), f"strip {k}: MX_EQ_LEAN=0 gives other bytes"
    assert res[None][3] == res["0"][3], "the repair pass did something else"
    return res, run_oracle(ws, strips, x, toggles, T)


def wave_tick_is_flat(toggles, T, env_p, n_chunks):
    """-> [wave][k]: no lane of the wave ramps in the k-th tick of its chunk (numpy model of the schedule, test_gpu_eq_env_rows.phases)"""
    ph = phases(toggles, T, env_p)
    out = []
    for w0 in range(0, n_chunks, 64):
        out.append([all(ph[CT * j + k] not in RAMPING for j in range(w0, min(w0 + 64, n_chunks)) if CT * j + k < T) for k in range(CT)])
    return out


# 1 ------------------------------------------------------------------------------------------------
def test_amplitudes_and_both_loops(monkeypatch):
    """Four strips of one launch with amplitudes 1.0 / 0.9 / 2.0 / -1.0 on noise, one wave each (64 chunks of three ticks).  With SHORT_ENV a toggle
    makes exactly one tick ramp: strip 0 toggles in ticks = 1 (mod 3), so its wave's tick 0 is flat and tracked, tick 1 takes the row loop
    untracked and tick 2 the flat loop untracked; strip 1 ramps in tick 2, strip 2 in tick 0 (the row loop tracked), strip 3 in all three."""
    T, n_chunks = 192, 64
    toggles = [{10: 1, 40: 0, 100: 1, 160: 0}, {11: 1, 41: 0, 101: 1, 161: 0}, {9: 1, 39: 0, 99: 1, 159: 0}, {9: 1, 40: 0, 101: 1, 159: 0}]
    flat = [wave_tick_is_flat(tg, T, SHORT_ENV, n_chunks)[0] for tg in toggles]
    assert flat == [[True, False, True], [True, True, False], [False, True, True], [False, False, False]], flat
    x = [synth.noise(5100 + k, T * SPT) for k in range(4)]
    res, want = lean_and_plain([1.0, 0.9, 2.0, -1.0], T, x, toggles, monkeypatch, n_chunks)
    compare(res[None][0], want, "amplitudes")
    assert res[None][1] == {"untracked": True, "unity": True}, res[None][1]
    assert res[None][2], "no wave took the row form"
    assert np.all(res[None][4][:, :, 0] < res[None][4][:, :, 1]), "a chunk of noise recorded as constant"


# 2 ------------------------------------------------------------------------------------------------
def constancy_inputs(T, n_chunks):
    """Three strips of noise with designed chunks.  -> inputs, {class: [(strip, chunk)]}"""
    L = CT * SPT
    x = [synth.noise(5200 + k, T * SPT).copy() for k in range(3)]
    cls = {"a_zeros": [(0, 66)], "a_dc": [(0, 68)], "a_negzero": [(0, 70)],    # strip 0, wave 1 (16 chunks, 48 idle lanes): constant chunks keep the wave tracking
           "c": [(0, 5), (0, 40), (1, 71)],                                     # strip 0, wave 0: proven after the first tick, untracked from the second
           "b": [(1, 9), (1, 73)], "d": [(1, 30), (1, 75)]}                     # strip 1: unproven until the last tick / the last sample
    def chunk(s, j): return x[s][j * L:(j + 1) * L]
    chunk(0, 66)[:] = 0.0
    chunk(0, 68)[:] = 0.25
    chunk(0, 70)[:] = -0.0
    for s, j in cls["c"]: chunk(s, j)[SPT:] = chunk(s, j)[SPT - 1]
    for s, j in cls["b"]: chunk(s, j)[:2 * SPT] = np.float32(-0.375)
    for s, j in cls["d"]:
        chunk(s, j)[:] = np.float32(0.5)
        chunk(s, j)[-1] = np.float32(0.5000001)
    return x, cls


def test_input_constancy_per_chunk(monkeypatch):
    """T = 240 ticks in 80 chunks of three: wave 0 of a strip has 64 live lanes, wave 1 has 16 and 48 idle ones (e).  Strip 2 is plain noise: its wave 0
    is a wave with every lane live."""
    T, n_chunks, L = 240, 80, CT * SPT
    x, cls = constancy_inputs(T, n_chunks)
    bits = [v.view(np.uint32).reshape(n_chunks, L) for v in x]
    konst = np.array([[np.all(b[j] == b[j][0]) for j in range(n_chunks)] for b in bits])
    # the premises, before the GPU run
    for name, where in cls.items():
        for s, j in where:
            assert konst[s, j] == name.startswith("a_"), (name, s, j)
            w0 = j // 64 * 64
            assert not konst[s, w0:min(w0 + 64, n_chunks)].all(), f"{name}: no live lane beside chunk {j} of strip {s}"
    for s, j in cls["b"]: assert np.all(bits[s][j][:2 * SPT] == bits[s][j][0]) and len(set(bits[s][j][2 * SPT:])) > 2
    for s, j in cls["c"]: assert len(set(bits[s][j][:SPT])) > 2 and np.all(bits[s][j][SPT:] == bits[s][j][SPT])
    for s, j in cls["d"]: assert np.all(bits[s][j][:-1] == bits[s][j][0]) and bits[s][j][-1] != bits[s][j][0]
    assert n_chunks % 64 != 0 and not konst[2, :64].any() and not konst[0, :64].any()
    assert int(np.float32(-0.0).view(np.uint32)) == 0x80000000 == int(bits[0][70][0])
    toggles = [{4: 1, 100: 0}, {7: 1, 50: 0, 120: 1}, {}]
    res, want = lean_and_plain([1.0, 0.7, 1.0], T, x, toggles, monkeypatch, n_chunks)
    compare(res[None][0], want, "constancy")
    assert res[None][1]["untracked"], "no wave dropped its tracker"
    for sw in (None, "0"):
        mm = res[sw][4]
        for s in range(3):
            for j in range(n_chunks):
                assert (mm[s, j, 0] == mm[s, j, 1]) == konst[s, j], f"MX_EQ_LEAN={sw} strip {s} chunk {j}: min {mm[s, j, 0]:#x} max {mm[s, j, 1]:#x}, constant {konst[s, j]}"
                if konst[s, j]: assert mm[s, j, 0] == bits[s][j][0], f"MX_EQ_LEAN={sw} strip {s} chunk {j}: recorded {mm[s, j, 0]:#x}, input {bits[s][j][0]:#x}"


# 3 ------------------------------------------------------------------------------------------------
def test_specials_at_unity_amplitude(monkeypatch):
    """amplitude 1.0 on both strips.  Strip 0: subnormals and signed zeros, then +inf, -inf and a NaN (from the first infinity on the poles are NaN: the
    rest of the stream is).  Strip 1 stays finite: runs of subnormals and of -0.0 / +0.0, so that subnormal and zero products reach the dropped multiply."""
    T, n_chunks = 192, 64
    x = [synth.noise(5300 + k, T * SPT).copy() for k in range(2)]
    sub = np.array([1, 0x7fffff, 0x80000001, 0x807fffff], np.uint32).view(np.float32)
    x[0][1000:1004] = sub; x[0][5000] = 0.0; x[0][5001] = -0.0
    x[0][150 * SPT + 17] = np.inf; x[0][160 * SPT + 3] = -np.inf; x[0][170 * SPT + 801] = np.nan
    x[1][20 * SPT:23 * SPT] = np.tile(sub, 3 * SPT // 4)
    x[1][60 * SPT:62 * SPT] = -0.0; x[1][62 * SPT:64 * SPT] = 0.0
    x[1][100 * SPT:101 * SPT] *= np.float32(2.0 ** -120)
    toggles = [{10: 1, 40: 0, 100: 1, 160: 0}, {11: 1, 41: 0, 101: 1, 161: 0}]
    res, want = lean_and_plain([1.0, 1.0], T, x, toggles, monkeypatch, n_chunks)
    assert np.isnan(want[0]).any() and not np.isnan(want[0][:150 * 2 * SPT]).any() and not np.isnan(want[1]).any()
    compare(res[None][0], want, "specials")
    assert res[None][1]["unity"], res[None][1]


# 4 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,flags,mono_dup,toggles,rows", [
    ("contracted", abi.FLAG_FP_CONTRACT, True, [{10: 1, 40: 0, 100: 1, 160: 0}, {9: 1, 41: 0}], True),
    ("interleaved", 0, False, [{10: 1, 40: 0, 100: 1, 160: 0}, {9: 1, 41: 0}], True),
    ("gates_held", 0, True, [{}, {}], False),                                  # every tick flat: only the constant-depth loop
    ("lockstep", 0, True, [{0: 1}, {0: 1}], False),   # MX_EQ_ENV_ROWS=0 and a four-second decay: EVERY tick ramps, so the untracked ticks are the lockstep kernel's ENVK == 2 loop
])
def test_other_instantiations(name, flags, mono_dup, toggles, rows, monkeypatch):
    T, n_chunks = 192, 64
    kw = {}
    if name == "lockstep":
        monkeypatch.setenv("MX_EQ_ENV_ROWS", "0")
        kw["env_p"] = LONG_ENV
        assert all(ph in RAMPING for tg in toggles for ph in phases(tg, T, LONG_ENV)), "a flat tick: untracked could come from the flat loop"

    x = [synth.noise(5400 + k, T * SPT) for k in range(2)]
    with oracle.fp_contract(bool(flags & abi.FLAG_FP_CONTRACT)):
        res, want = lean_and_plain([1.0, 1.25], T, x, toggles, monkeypatch, n_chunks, flags=flags, mono_dup=mono_dup, **kw)
    compare(res[None][0], want, name)
    assert res[None][1] == {"untracked": True, "unity": True}, res[None][1]
    assert res[None][2] == rows
