"""The graph compiler's fusion (EqThree -> StereoPanner(L=R) [-> Amplifier]; Trigger -> Envelope) must be
invisible: every port that still exists carries bit-identical samples with and without it."""
import numpy as np
import pytest

import oracle
import synth
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import SPT, assert_bit_exact, strips

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("eq_flag", [abi.FLAG_EQ_FAST, 0])
def test_fused_equals_unfused_on_every_surviving_port(eq_flag):
    n_strips, T = 24, 5
    ws, mix, srcs, trigs = strips(n_strips)
    gf = ws.build(max_ticks_per_run=T, flags=eq_flag)
    gu = ws.build(max_ticks_per_run=T, flags=eq_flag | abi.FLAG_NO_FUSE)
    noise = [synth.noise(k, 3 * T * SPT) for k in range(n_strips)]
    for run in range(3):
        for g in (gf, gu):
            for k, tr in enumerate(trigs):
                g.update_params(tr, abi.TriggerParams(1 if (run + k) % 2 else 0))      # folded Trigger: update must reach the Envelope
            if run == 2:
                g.update_params(mix + 6, abi.AmplifierParams(0.7, 0.25))               # folded Amplifier of strip 0
            for k, s in enumerate(srcs):
                g.write_source(s, noise[k][run * T * SPT:(run + 1) * T * SPT], T)
            g.run_ticks(run * T, T)
        for port in (0, 1):
            assert_bit_exact(gf.read_output(mix, port, T, True), gu.read_output(mix, port, T, True), f"mixer port {port} run {run}")
        for k in (0, 7, n_strips - 1):
            amp = mix + 6 * k + 6
            # the strip's stereo result is stored as one float per frame in the fused graph (L == R): read_output expands it
            assert_bit_exact(gf.read_output(amp, 0, T, True), gu.read_output(amp, 0, T, True), f"amp out strip {k}")


def test_folded_ports_are_not_readable_and_say_why():
    ws, mix, srcs, trigs = strips(2)
    g = ws.build()
    eq, pan, trig, env = mix + 4, mix + 5, mix + 1, mix + 2
    for node in (eq, pan, trig, env):
        with pytest.raises(abi.MxError) as e:
            g.read_output(node, 0, 1, node == pan)
        assert e.value.code == abi.MX_ERR_INVALID and "MX_FLAG_NO_FUSE" in str(e.value)
    g2 = ws.build(flags=abi.FLAG_NO_FUSE)
    g2.run_ticks(0, 1)
    assert g2.read_output(eq, 0, 1, False).shape == (SPT,)


def test_fusion_is_not_applied_when_a_port_has_another_consumer():
    # the EQ output also feeds a second mixer through its own panner input: it must stay materialised
    ws = Workspace(44100, 60)
    s = ws.source_mono(); e = ws.eq_three(3.0, 0.0, -3.0); p = ws.stereo_panner(); a = ws.amplifier(1.0, 0.0)
    e2 = ws.eq_three(0.0, 0.0, 0.0)
    ws.connect(s, 0, e, 0); ws.connect(e, 0, p, 0); ws.connect(e, 0, p, 1); ws.connect(p, 0, a, 0); ws.connect(e, 0, e2, 0)
    g = ws.build(flags=abi.FLAG_EQ_EXACT)
    x = synth.noise(5, SPT)
    g.write_source(s, x, 1); g.run_ticks(0, 1)
    st = oracle.eq_three_new(44100.0)
    want = oracle.eq_three_run(st, (3.0, 0.0, -3.0), x)
    assert_bit_exact(g.read_output(e, 0, 1, False), want, "EQ port with two consumers")
    assert_bit_exact(g.read_output(a, 0, 1, True)[0::2], want, "through panner + unity amplifier")


def test_eq_panner_only_fusion():
    ws = Workspace(44100, 60)
    s = ws.source_mono(); e = ws.eq_three(-6.0, 2.0, 1.0); p = ws.stereo_panner(); m = ws.mixer([(0.0, 1.0, True)])
    ws.connect(s, 0, e, 0); ws.connect(e, 0, p, 0); ws.connect(e, 0, p, 1); ws.connect(p, 0, m, 0)
    x = synth.noise(6, 4 * SPT)
    outs = []
    for flags in (abi.FLAG_EQ_EXACT, abi.FLAG_EQ_EXACT | abi.FLAG_NO_FUSE):
        g = ws.build(max_ticks_per_run=4, flags=flags)
        g.write_source(s, x, 4); g.run_ticks(0, 4)
        outs.append((g.read_output(p, 0, 4, True), g.read_output(m, 1, 4, True)))
    assert_bit_exact(outs[0][0], outs[1][0], "panner out"); assert_bit_exact(outs[0][1], outs[1][1], "cue")
    st = oracle.eq_three_new(44100.0)
    want = oracle.eq_three_run(st, (-6.0, 2.0, 1.0), x)
    assert_bit_exact(outs[0][0][0::2], want); assert_bit_exact(outs[0][0][1::2], want)


def test_inline_envelope_state_carries_across_runs_and_gate_flips():
    """F3: the Envelope folded into the EQ epilogue must keep its state machine exact across runs:
    attack -> decay -> sustain while the Trigger is open, release after it closes, re-trigger."""
    ws, mix, srcs, trigs = strips(3)
    T = 7
    gf = ws.build(max_ticks_per_run=T)
    gu = ws.build(max_ticks_per_run=T, flags=abi.FLAG_NO_FUSE)
    pattern = [1, 1, 1, 0, 0, 1, 0, 0, 0, 1]   # gate per run
    noise = [synth.noise(40 + k, len(pattern) * T * SPT) for k in range(3)]
    for run, gate in enumerate(pattern):
        for g in (gf, gu):
            for k, tr in enumerate(trigs):
                g.update_params(tr, abi.TriggerParams(gate if k != 1 else 1 - gate))
            for k, s in enumerate(srcs):
                g.write_source(s, noise[k][run * T * SPT:(run + 1) * T * SPT], T)
            g.run_ticks(run * T, T)
        assert_bit_exact(gf.read_output(mix, 0, T, True), gu.read_output(mix, 0, T, True), f"master run {run}")
        for k in range(3):
            assert_bit_exact(gf.read_output(mix + 6 * k + 6, 0, T, True), gu.read_output(mix + 6 * k + 6, 0, T, True), f"strip {k} run {run}")


def plan_graphs():
    """64-frame ticks.  Two strips into a Mixer, the second strip's Amplifier controlled by a Trigger -> Envelope; a Resample 3 / 2 with a Fir behind it"""
    ws = Workspace(64 * 60, 60)
    amps = []
    for i in range(2):
        s = ws.source_mono(); e = ws.eq_three(3.0, -6.0, 1.5); p = ws.stereo_panner(); a = ws.amplifier(1.0, 0.5)
        ws.connect(s, 0, e, 0); ws.connect(e, 0, p, 0); ws.connect(e, 0, p, 1); ws.connect(p, 0, a, 0)
        amps.append(a)
    t = ws.trigger(True); v = ws.envelope(); ws.connect(t, 0, v, 0); ws.connect(v, 0, amps[1], 1)
    m = ws.mixer([(0.0, 1.0, False)] * 2); ws.connect(amps[0], 0, m, 0); ws.connect(amps[1], 0, m, 1)
    rs = Workspace(64 * 60, 60)
    s = rs.source_stereo(); r = rs.resample(3, 2, np.full((3, 4), 0.25)); f = rs.fir([0.5, 0.25, 0.25]); rs.connect(s, 0, r, 0); rs.connect(r, 0, f, 0)
    return {"fused": (ws, 0), "unfused": (ws, abi.FLAG_NO_FUSE), "resampled": (rs, 0)}


@pytest.mark.parametrize("name", ["fused", "unfused", "resampled"])
def test_the_built_graph_is_the_one_the_host_only_plan_describes(name):
    ws, flags = plan_graphs()[name]
    recs, info = abi.debug_plan(ws.nodes, ws.edges, ws.sample_rate, ws.ticks_per_second, 2, flags)
    g = ws.build(max_ticks_per_run=2, flags=flags)
    order = [n for _pos, n in sorted((r.pos, n) for n, r in enumerate(recs) if r.pos >= 0)]
    assert g.run_order() == order and info.n_order == len(order)
    g.run_ticks(0, 2)
    elided, dup, not_there, one_float = set(), set(), set(), set()
    for n, r in enumerate(recs):
        for p in range(r.n_out):
            if r.out_elided[p]:
                elided.add((n, p))
            if r.out_dup[p]:
                dup.add((n, p))
            try:
                g.read_output(n, p, 1, True, rate=(r.dom_num, r.dom_den))   # (room for a stereo port; a mono one fills half)
            except abi.MxError as e:
                assert "not materialised" in str(e)
                not_there.add((n, p))
            try:
                g.output_device_ptr(n, p)
            except abi.MxError as e:
                assert (n, p) in not_there or "one float per frame" in str(e)
                if (n, p) not in not_there:
                    one_float.add((n, p))
    assert not_there == elided and one_float == dup
    assert (name == "fused") == bool(elided) and (name == "fused") == bool(dup)
    g.close()
