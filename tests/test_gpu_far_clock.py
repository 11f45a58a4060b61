"""The clock past 2^32 samples, part A: Envelope sample distances of 2^32 and more (24.8 h at 48 kHz) on every path that evaluates one.

Distances below 2^32 take the Markstein quotient ms_of_u32 (tests/test_fastdiv.py proves it for all of them); from 2^32 on seq_ms divides
truly, k_envelope leaves its fast step, env_lane_coeffs marks the lane `general`, and k_env_ticks' `flat` / env_saturated go through seq_ms.
Each guard decides per sample, step, tick or chunk, so every case of tests/far_clock_cases.py puts the sample at distance exactly 2^32 at a
chosen place of a submission: last sample (and one past it), first sample, mid-tick, a tick boundary, first / inside / last sample of a
k_envelope step, of an Envelope segment and of a speculative EqThree chunk -- and far beyond (2^33 + 12345, 2^40).  Two submissions, nothing
run in between: the clock may be started anywhere and jumped between runs.  Bit for bit against the oracle graph (contract mode for
MX_FLAG_FP_CONTRACT); the scan (MX_FLAG_EQ_FAST) within 1 ULP as everywhere.  tests/test_cpu_far_clock.py proves that each case differs from
what a distance kept in 32 bits would give.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import far_clock_cases as fc
import oracle
from mixlab_amd import abi
from test_gpu_audio_parity import assert_bit_exact, assert_ulp

pytestmark = pytest.mark.gpu


def param(cs):
    return pytest.mark.parametrize("case", cs, ids=fc.ids(cs))


def sub_runs(case, which, n, modes):
    """[(first tick, end tick)] of one submission: whole, except for the constant-Trigger form, which is cut wherever a Trigger changes (its
    Triggers are then set between runs, never scheduled inside one)"""
    if case.gate != "trigger":
        return [(0, n)]
    spt = case.spt
    bits = [[int((case.gate1(m) if which == 0 else case.gate2(m))[t * spt]) for m in modes] for t in range(n)]
    cuts = [0] + [t for t in range(1, n) if bits[t] != bits[t - 1]] + [n]
    return list(zip(cuts[:-1], cuts[1:]))


def device_submission(g, case, kind, a, b, which, t0, n, read, stereo):
    """The device's side of fc.oracle_graph_run: -> {node: samples of the whole submission}"""
    spt = case.spt
    modes = [fc.ENVS[k % 4][0] for k in range(len(a))]
    out = {r: [] for r in read}
    for (c0, c1) in sub_runs(case, which, n, modes):
        for k, mode in enumerate(modes):
            gate = (case.gate1(mode) if which == 0 else case.gate2(mode))
            if kind == "unfused" and case.gate == "buffer":
                g.write_source(a[k], gate[c0 * spt:c1 * spt], c1 - c0)
            else:
                trig = (a if kind == "unfused" else b)[k]
                g.update_params(trig, abi.TriggerParams(int(gate[c0 * spt])))
                for t in range(c0 + 1, c1):
                    v, before = int(gate[t * spt]), int(gate[(t - 1) * spt])
                    # scheduled form: every change, and one update that changes nothing (the per-tick gate bits are used either way)
                    if v != before or (case.gate == "scheduled" and t == c0 + 1):
                        g.schedule_params(trig, t - c0, abi.TriggerParams(v))
            if kind == "fused":
                g.write_source(a[k], fc.fused_noise(case, k, which)[c0 * spt:c1 * spt], c1 - c0)
        g.run_ticks(t0 + c0, c1 - c0)
        for r in read:
            out[r].append(g.read_output(r, 0, c1 - c0, stereo))
    return {r: np.concatenate(v) for r, v in out.items()}


def run_unfused(case, flags=0):
    ws, gates, envs = fc.unfused_graph(case)
    g = ws.build(max_ticks_per_run=max(2, case.n_ticks), flags=flags | abi.FLAG_NO_FUSE)
    with oracle.fp_contract(bool(flags & abi.FLAG_FP_CONTRACT)):
        og = oracle.OracleGraph(ws)
        for which, (t0, n) in enumerate([(fc.A_TICK - 1, 2), (case.first_tick, case.n_ticks)]):
            got = device_submission(g, case, "unfused", gates, None, which, t0, n, envs, False)
            want = fc.oracle_graph_run(case, og, ("unfused", gates, envs), t0, n, which, envs)
            for k, e in enumerate(envs):
                assert_bit_exact(got[e], want[e], f"{case.id} submission {which} from tick {t0}: Envelope {fc.ENVS[k]}")
    g.close()


def run_fused(case, flags, check_launch, ulp=0):
    ws, srcs, trigs, pans, amps = fc.fused_graph(case)
    g = ws.build(max_ticks_per_run=max(2, case.n_ticks), flags=flags)
    n_diff = n_all = 0
    with oracle.fp_contract(bool(flags & abi.FLAG_FP_CONTRACT)):
        og = oracle.OracleGraph(ws)
        for which, (t0, n) in enumerate([(fc.A_TICK - 1, 2), (case.first_tick, case.n_ticks)]):
            got = device_submission(g, case, "fused", srcs, trigs, which, t0, n, amps, True)
            if which == 1:
                check_launch(g.debug_eq_launch())
            want = fc.oracle_graph_run(case, og, ("fused", srcs, trigs), t0, n, which, amps)
            for k, a in enumerate(amps):
                what = f"{case.id} submission {which} from tick {t0}: strip {k} {fc.ENVS[k % 4]} Amplifier"
                if ulp:
                    n_diff += assert_ulp(got[a], want[a], ulp, what); n_all += want[a].size
                else:
                    assert_bit_exact(got[a], want[a], what)
    g.close()
    return n_diff, n_all


# ------------------------------------------------------------------------------------------------
# k_envelope (MX_FLAG_NO_FUSE): gate buffer, constant Trigger, Trigger updates scheduled inside the run, segments
# ------------------------------------------------------------------------------------------------
@param(fc.UNFUSED_BUFFER)
def test_envelope_gated_by_a_buffer(case):
    run_unfused(case)


@param(fc.UNFUSED_TRIGGER)
def test_envelope_gated_by_a_constant_trigger(case):
    run_unfused(case)


@param(fc.UNFUSED_SCHEDULED)
def test_envelope_with_trigger_updates_scheduled_inside_the_run(case):
    run_unfused(case)


@param(fc.UNFUSED_SEGMENTED)
def test_envelope_in_segments(case, monkeypatch):
    """MX_ENV_SEGMENTS as tests/test_gpu_envelope_segments.py forces it: k_env_resolve leaves the carried state at every segment's start, one wave per segment"""
    monkeypatch.setenv("MX_ENV_SEGMENTS", str(fc.SEGMENTS_FORCED))
    assert fc.segment_len(case.n, fc.SEGMENTS_FORCED) < case.n
    run_unfused(case)


CONTRACT_UNFUSED = [c for c in fc.UNFUSED_BUFFER + fc.UNFUSED_SCHEDULED if c.shape_id in ("8k_8000", "44k1")]


@param(CONTRACT_UNFUSED)
def test_envelope_contracted_order(case):
    run_unfused(case, abi.FLAG_FP_CONTRACT)


# ------------------------------------------------------------------------------------------------
# the per-module path: mx_module_run_tick takes any sample time
# ------------------------------------------------------------------------------------------------
@param(fc.MODULE)
def test_envelope_module_at_any_sample_time(case):
    spt, sr = case.spt, case.shape.sample_rate
    for mode, pset in fc.ENVS:
        p = fc.env_params(pset, sr, case.X)
        m = abi.Module(abi.KIND_ENVELOPE, abi.EnvelopeParams(*p), sample_rate=sr, ticks_per_second=case.shape.ticks_per_second)
        st = oracle.EnvState()
        for t0, gate in (((fc.A_TICK - 1) * spt, case.gate1(mode)), (case.start, case.gate2(mode))):
            for k in range(gate.size // spt):
                got = np.empty(spt, np.float32)
                m.run_tick(t0 + k * spt, [(abi.MX_MONO, gate[k * spt:(k + 1) * spt])], [(abi.MX_MONO, got)])
                want = oracle.envelope_run(st, p, float(sr), t0 + k * spt, gate[k * spt:(k + 1) * spt], spt)
                assert_bit_exact(got, want, f"{case.id} {mode} {pset}: module call at sample time {t0 + k * spt}")
        m.close()


# ------------------------------------------------------------------------------------------------
# the fused strip (Trigger -> Envelope inline in the EqThree epilogue), exact order: speculative forms, split cascade, one lane
# ------------------------------------------------------------------------------------------------
def expect_spec(case):
    form, chunk = fc.SPEC_LAUNCH[case.shape_id]

    def check(launch):
        assert launch["form"] == form and launch["chunk"] == chunk and launch["n_chunks"] >= 2, f"{case.id}: {launch}, the case table says {form}, chunk {chunk}"
    return check


def expect_sequential(case):
    def check(launch):   # (a sequential launch reports its lanes per instance as `super_block`: 2 = the split cascade, 1 = one lane)
        assert launch["form"] == "sequential" and launch["super_block"] == (1 if ONE_LANE else 2), f"{case.id}: {launch}, MX_EQ_POLES_BELOW=0 {ONE_LANE}"
    return check


@param(fc.FUSED_SPEC)
def test_fused_strip_speculative_forms(case):
    run_fused(case, abi.FLAG_EQ_EXACT, expect_spec(case))


@param([c for c in fc.FUSED_SPEC if c.shape_id in ("48k", "8k_8000")])      # the tiled form, and the shape whose Trigger reaches every place (direct form)
def test_fused_strip_speculative_forms_contracted_order(case):
    run_fused(case, abi.FLAG_EQ_EXACT | abi.FLAG_FP_CONTRACT, expect_spec(case))


ONE_LANE = os.environ.get("MX_EQ_POLES_BELOW") == "0"    # read once per process by the library, too


@param(fc.FUSED_SHORT)
def test_fused_strip_short_stream(case):
    """Fewer samples than two warm-ups: no speculation.  With the default switch 8 strips take the split-cascade form (k_eq_three_poles +
    k_eq_three_emit); under MX_EQ_POLES_BELOW=0 -- the child process below -- the one-lane form (k_eq_three_exact).  Both report `sequential`,
    with 2 resp. 1 lanes per instance."""
    run_fused(case, abi.FLAG_EQ_EXACT, expect_sequential(case))
    run_fused(case, abi.FLAG_EQ_EXACT | abi.FLAG_FP_CONTRACT, expect_sequential(case))


def test_fused_strip_one_lane_form_in_a_child_process():
    """The switch between the split-cascade and the one-lane form is read once per process (tests/test_gpu_eq_exact_spec.py does the same)."""
    assert not ONE_LANE, "this process was started with MX_EQ_POLES_BELOW=0: the split-cascade cases did not run"
    here = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", os.path.join(here, "test_gpu_far_clock.py"),
                        "-k", "test_fused_strip_short_stream"], env=dict(os.environ, MX_EQ_POLES_BELOW="0"), capture_output=True, text=True, cwd=os.path.dirname(here), timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert f"{len(fc.FUSED_SHORT)} passed" in r.stdout, r.stdout[-500:]


# ------------------------------------------------------------------------------------------------
# the default time-parallel scan (MX_FLAG_EQ_FAST): its own arithmetic for the filter, <= 1 ULP; the Envelope in its epilogue is the same closed form
# ------------------------------------------------------------------------------------------------
@param(fc.FUSED_SCAN)
def test_fused_strip_scan_within_one_ulp(case):
    def check(launch):
        assert launch["form"] == "scan", launch
    run_fused(case, abi.FLAG_EQ_FAST, check, ulp=1)    # the bar of test_config2_strips_default_mode_within_tolerance: every strip within 1 ULP
