"""The far clock on the CPU: (1) every case of tests/far_clock_cases.py -- the very inputs tests/test_gpu_far_clock.py runs -- is able to fail;
(2) mx_sin_f32.hpp's host build at module-shaped arguments of the far epochs, against the 130-digit reference.

(1) is a condition, not a measurement.  The kernels' fast paths keep the distance since the Envelope's last edge in 32 bits; a guard that lets a
distance of 2^32 or more through makes them see the distance modulo 2^32, which is what the oracle computes when the carried `seq` is moved
forward by 2^32 (by the multiple of 2^32 below the distance, for the far places).  Over the span the GPU test compares, the oracle's expected
output must differ from that in at least one sample, and a live Envelope must take at least two f32 values, so a constant would not pass.
One combination cannot meet it and is asserted to be exactly that: at `last_below` every distance is below 2^32 and `seq + 2^32` lies in the
future, where u64 subtraction wraps to a distance of about 2^64 -- the value of an Envelope at rest, which a resting Envelope has anyway.  That
case discriminates through its two live Envelopes.
"""
import pathlib
import subprocess

import numpy as np
import pytest

import far_clock_cases as fc
import oracle
import synth
from sin_reference import sin_f32
from tick_shapes import by_id

ROOT = pathlib.Path(__file__).resolve().parent.parent


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_discriminates(case, mode, pset, want, wrapped, what, ulp=0):
    """ulp: the tolerance of the GPU comparison this protects (0: bit equality; 1: the scan) -- the wrapped output must lie outside it"""
    if case.place == "last_below" and pset == "resting":
        assert np.array_equal(bits(want), bits(wrapped)), f"{what}: expected to be out of reach (module docstring), but the outputs differ"
        return
    assert synth.ulp_diff(want, wrapped).max() > ulp, f"{what}: the oracle's output is within {ulp} ULP of what a 32-bit distance gives -- the case cannot fail"
    if pset == "live":
        assert np.unique(bits(want)).size >= 2, f"{what}: a live Envelope's expected output is one constant"


def test_the_case_table_covers_every_place():
    """each form reaches what its gate allows: one sample per tick (8k_8000) and the free forms reach every place; k_envelope's steps are places
    of the forms that run k_envelope, counted from the start of each launch"""
    edges = {"last_below", "last_at", "first_at", "tick_boundary", "far_2p33", "far_2p40"}
    steps = {"step_first", "step_inside", "step_last"}
    for name, cs in fc.ALL.items():
        assert all(c.n_ticks * c.spt == c.n and 0 <= c.i0 <= c.n for c in cs)
        every = edges | (steps if name.startswith(("unfused", "module")) else set())
        by_shape = {}
        for c in cs:
            by_shape.setdefault(c.shape_id, set()).add(c.place)
        for sid, got in by_shape.items():
            if sid == "8k_8000":
                assert every <= got, (name, sid, every - got)
            elif cs[0].gate in ("buffer", "module") and not name.endswith("segmented"):
                assert every | {"mid_tick"} <= got, (name, sid, (every | {"mid_tick"}) - got)
            else:
                assert {"mid_tick", "far_2p33", "far_2p40"} <= got, (name, sid, got)
        if name.startswith("fused"):
            assert not steps & {c.place for c in cs}
    assert {"segment_first", "segment_last", "segment_inside"} <= {c.place for c in fc.UNFUSED_SEGMENTED}
    assert {"chunk_first", "chunk_last", "chunk_inside"} <= {c.place for c in fc.FUSED_SPEC}
    # the step a place names is the one k_envelope takes: 512 samples from the launch's first sample -- the submission's, or each tick's on the per-module path
    for c in fc.UNFUSED_BUFFER + fc.UNFUSED_TRIGGER + fc.UNFUSED_SCHEDULED + fc.UNFUSED_SEGMENTED + fc.MODULE:
        in_launch = c.i0 % c.spt if c.gate == "module" else c.i0
        assert (c.spt if c.gate == "module" else c.n) > 256
        if c.place == "step_first":
            assert in_launch % fc.STEP == 0 and in_launch > 0
        if c.place == "step_last":
            assert in_launch % fc.STEP == fc.STEP - 1
        if c.place == "step_inside":
            assert 0 < in_launch % fc.STEP < fc.STEP - 1 and in_launch > fc.STEP
    for c in fc.UNFUSED_BUFFER + fc.MODULE:                       # live: decay and release of at least 2 D / sr s
        p = fc.env_params("live", c.shape.sample_rate, c.X)
        assert min(p[1], p[3]) >= 2.0 * fc.D / c.shape.sample_rate * 1000.0


UNFUSED = [(n, c) for n in ("unfused_buffer", "unfused_trigger", "unfused_scheduled", "unfused_segmented", "module") for c in fc.ALL[n]]


@pytest.mark.parametrize("name,case", UNFUSED, ids=[f"{n}-{i}" for n in ("unfused_buffer", "unfused_trigger", "unfused_scheduled", "unfused_segmented", "module")
                                                    for i in fc.ids(fc.ALL[n])])
def test_unfused_and_module_cases_can_fail(name, case):
    alone = {}
    for mode, pset in fc.ENVS:
        want, wrapped = fc.envelope_alone(case, mode, pset, False), fc.envelope_alone(case, mode, pset, True)
        assert_discriminates(case, mode, pset, want, wrapped, f"{name} {case.id} {mode} {pset}")
        alone[(mode, pset)] = want
    if case.gate == "module":
        return
    # the graph the GPU test compares against gives those very samples
    ws, gates, envs = fc.unfused_graph(case)
    og = oracle.OracleGraph(ws)
    fc.oracle_graph_run(case, og, ("unfused", gates, envs), fc.A_TICK - 1, 2, 0, envs)
    got = fc.oracle_graph_run(case, og, ("unfused", gates, envs), case.first_tick, case.n_ticks, 1, envs)
    for k, e in enumerate(envs):
        assert np.array_equal(bits(got[e]), bits(alone[fc.ENVS[k]])), f"{name} {case.id}: the oracle graph and Envelope::run_tick alone disagree"


FUSED = [(n, c) for n in ("fused_spec", "fused_short", "fused_scan") for c in fc.ALL[n]]


@pytest.mark.parametrize("name,case", FUSED, ids=[f"{n}-{i}" for n in ("fused_spec", "fused_short", "fused_scan") for i in fc.ids(fc.ALL[n])])
def test_fused_cases_can_fail(name, case):
    """The fused strip is compared at the Amplifier's output: the oracle's Panner output through Amplifier::run_tick with the wrapped Envelope as
    the control must differ from the oracle's Amplifier output (and give it back, bit for bit, with the true Envelope)."""
    ws, srcs, trigs, pans, amps = fc.fused_graph(case)
    og = oracle.OracleGraph(ws)
    fc.oracle_graph_run(case, og, ("fused", srcs, trigs), fc.A_TICK - 1, 2, 0, [])
    out = fc.oracle_graph_run(case, og, ("fused", srcs, trigs), case.first_tick, case.n_ticks, 1, pans + amps)
    for k in range(fc.FUSED_STRIPS):
        mode, pset = fc.ENVS[k % 4]
        want = out[amps[k]]
        again = oracle.amplifier_run(*fc.AMP, out[pans[k]], fc.envelope_alone(case, mode, pset, False))
        assert np.array_equal(bits(again), bits(want)), f"{name} {case.id} strip {k}: Amplifier over the lone Envelope is not the graph's"
        wrapped = oracle.amplifier_run(*fc.AMP, out[pans[k]], fc.envelope_alone(case, mode, pset, True))
        assert_discriminates(case, mode, pset, want, wrapped, f"{name} {case.id} strip {k} {mode} {pset}", ulp=1 if name == "fused_scan" else 0)


# ------------------------------------------------------------------------------------------------
# (2) the sine at the far epochs
# ------------------------------------------------------------------------------------------------
EPOCHS = {"below_2p31": (1 << 31) - 4096, "across_2p32": (1 << 32) - 400, "at_2p40": 1 << 40}     # the run's first sample time (tests/test_gpu_far_clock.py part B)


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sin_far") / "sin_f32_check"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-o", str(exe), str(ROOT / "tests" / "helpers" / "sin_f32_check.cpp")], check=True)

    def run(xs):
        xs = np.ascontiguousarray(xs, dtype="<f8")
        out = subprocess.run([str(exe)], input=xs.tobytes(), capture_output=True, check=True).stdout
        return np.frombuffer(out, dtype="<f4").reshape(-1, 3)
    return run


@pytest.mark.parametrize("epoch", list(EPOCHS))
def test_sine_at_module_shaped_arguments_of_the_far_epochs(checker, epoch):
    """Oscillator: n 2.0 pi with n = (t / SR) freq (oscillator.rs:69-70,77); FmSine: co (t / SR), co = (lo + (hi - lo) x) 2 pi for an f32 x
    (fm_sine.rs:44-52) -- operation for operation, as tests/test_cpu_sin_f32.py forms them.  The slow path and the Ziv form over the host libm
    must both be the correctly rounded f32 of the real sine; where they are, a device / oracle disagreement at such a time is not the header's."""
    rng = np.random.default_rng(0xFA2C10C + len(epoch))
    t0, xs = EPOCHS[epoch], []
    freqs = [27.5, 55.0, 97.0, 110.0, 440.0, 1000.0, 1234.5, 4186.0, 12000.0, 19000.0]
    for sr in (44100.0, 48000.0, 8000.0):
        for f in freqs + [float(v) for v in rng.uniform(27.5, 19000.0, 6)]:
            for t in [t0, t0 + 1, t0 + 399, t0 + 400, t0 + 401] + [int(t0 + v) for v in rng.integers(0, 8192, 3)]:
                xs.append((float(t) / sr) * f * 2.0 * np.pi)
                co = (f + float(rng.uniform(0.0, 500.0)) * float(np.float32(rng.uniform(-1.0, 1.0)))) * 2.0 * np.pi
                xs.append(co * (float(t) / sr))
    xs = np.array(xs)
    got = checker(xs)
    n_cast = 0
    for i, x in enumerate(xs):
        want = sin_f32(float(x))
        assert got[i, 0].view(np.uint32) == want.view(np.uint32), ("slow path", epoch, float(x).hex(), float(got[i, 0]), float(want))
        assert got[i, 1].view(np.uint32) == want.view(np.uint32), ("ziv", epoch, float(x).hex(), float(got[i, 1]), float(want))
        n_cast += int(got[i, 2].view(np.uint32) != want.view(np.uint32))
    # (float)libm_sin -- what the oracle stores -- is the real sine's f32 as well, unless the real sine lies within libm's error of a rounding boundary
    assert n_cast == 0, f"{epoch}: the host libm's sine rounds to another f32 than the real sine at {n_cast} of {xs.size} arguments"
