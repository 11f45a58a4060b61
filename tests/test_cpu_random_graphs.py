"""The full random-graph generator (tests/test_gpu_random_graphs.py, random_graph(full=True)) and the oracle's graph runner without a GPU:
what the generator draws, that every graph it draws builds and runs in the oracle, and the oracle's sample-rate domain pass, which
follows Graph::Graph (mx_engine.cpp): back-edges carry no domain, and a module whose inputs live in two domains is refused."""
import hashlib

import numpy as np
import pytest

import oracle
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from test_gpu_random_graphs import FULL_SEEDS, engine_domains, port_types, random_graph
from tick_shapes import by_id

AUDIO_KINDS = {abi.KIND_AMPLIFIER, abi.KIND_ENVELOPE, abi.KIND_EQ_THREE, abi.KIND_FM_SINE, abi.KIND_MIXER, abi.KIND_OSCILLATOR, abi.KIND_PLOTTER,
               abi.KIND_STEREO_PANNER, abi.KIND_STEREO_SPLITTER, abi.KIND_TRIGGER, abi.KIND_SOURCE_MONO, abi.KIND_SOURCE_STEREO, abi.KIND_FIR,
               abi.KIND_RESAMPLE, abi.KIND_OUTPUT_DEVICE}


def test_full_graphs_draw_every_kind_waveform_and_resampled_domains():
    kinds, waves, fed, cross, inside = set(), set(), 0, 0, 0
    for seed in range(64):
        ws, _sources = random_graph(seed, full=True)
        og = oracle.OracleGraph(ws)
        order = og.run_order()
        types = port_types(ws)
        kinds |= {ws.nodes[n][0] for n in order}
        waves |= {ws.nodes[n][1].waveform for n in order if ws.nodes[n][0] == abi.KIND_OSCILLATOR}
        # a resampled domain (read from the oracle's port lengths) that feeds a module other than a Resample
        resampled = {n for n in order for p, ty in enumerate(types[n]) if og.output(n, p).size != ty * ws.spt}
        pos = {n: i for i, n in enumerate(order)}
        edges = [(s, d) for (s, _sp, d, _dp) in ws.edges if s in pos and d in pos]
        fed += any(s in resampled and pos[s] < pos[d] and ws.nodes[d][0] != abi.KIND_RESAMPLE for (s, d) in edges)
        # back-edges out of a resampled port: into the same domain, and into a base-domain module
        _order, dom, _bad = engine_domains(ws)
        cross += any(s in resampled and pos[s] >= pos[d] and dom[d] == 1 for (s, d) in edges)
        inside += any(s in resampled and pos[s] >= pos[d] and dom[d] == dom[s] for (s, d) in edges)
    assert kinds == AUDIO_KINDS
    assert waves == {abi.WAVE_ON, abi.WAVE_OFF, abi.WAVE_SINE, abi.WAVE_SQUARE, abi.WAVE_TRIANGLE, abi.WAVE_SAW}
    assert fed >= 16
    assert cross >= 1 and inside >= 1


def test_round_one_graphs_are_unchanged():
    """full=False draws what it always drew: the 64 seeds of the first GPU test and the tick-shape tests keep their graphs (the digest
    of every node's kind and params, every edge and the source list, as the generator drew them before full=True existed)"""
    h = hashlib.sha256()
    for seed in range(64):
        ws, sources = random_graph(seed)
        for kind, params in ws.nodes:
            h.update(bytes([kind])); h.update(abi.params_bytes(params))
        h.update(repr(sorted(ws.edges)).encode()); h.update(repr(sources).encode())
    assert h.hexdigest() == "ed5c93852e1f4dc787cc8146f87fa7782a35c035bb30c35216b1df6f80c8d33b"


@pytest.mark.parametrize("shape_id,seed", [("44k1", s) for s in range(64)] + FULL_SEEDS)
def test_every_full_graph_builds_and_runs_in_the_oracle(shape_id, seed):
    shape = by_id(shape_id)
    ws, sources = random_graph(seed, shape.sample_rate, shape.ticks_per_second, full=True)
    order, dom, refusal = engine_domains(ws)
    assert refusal is None
    og = oracle.OracleGraph(ws)
    assert og.run_order() == order
    assert any(ws.nodes[n][0] == abi.KIND_MIXER for n in order)
    types = port_types(ws)
    for t in range(3):
        for (n, ty) in sources:
            og.set_source(n, np.full(ws.spt * ty, 0.25 * (t + 1), np.float32))
        og.run_tick(t)
        for n in order:
            for p, ty in enumerate(types[n]):
                assert og.output(n, p).size == ty * ws.spt * dom[n]


def back_edge_graph(splitter_reads_mixer):
    """source -> Resample(160 / 147) -> Mixer input 0; Amplifier -> Mixer input 1; Mixer -> Amplifier; a Splitter reads the Amplifier
    (the Mixer runs first, the Amplifier's edge into it is the back-edge) or the Mixer (the Amplifier runs first: its input is the back-edge)"""
    ws = Workspace(44100, 60)
    s = ws.source_stereo()
    r = ws.resample(160, 147, np.full((160, 4), 0.25))
    y = ws.mixer([(0.0, 1.0, False), (-6.0, 0.5, True)])
    m = ws.amplifier(0.5, 0.0)
    sp = ws.stereo_splitter()
    ws.connect(s, 0, r, 0); ws.connect(r, 0, y, 0); ws.connect(m, 0, y, 1); ws.connect(y, 0, m, 0)
    ws.connect(y if splitter_reads_mixer else m, 0, sp, 0)
    return ws, s, r, y, m, sp


def test_oracle_domain_pass_ignores_back_edges():
    ws, s, r, y, m, sp = back_edge_graph(False)
    og = oracle.OracleGraph(ws)
    assert og.run_order() == [s, r, y, m, sp]
    x = np.linspace(-1, 1, 2 * 735).astype(np.float32)
    og.set_source(s, x)
    og.run_tick(0)
    rs = og.output(r, 0)
    assert rs.size == 2 * 800
    for port in (og.output(y, 0), og.output(y, 1), og.output(m, 0)):
        assert port.size == 2 * 800   # the Mixer and the Amplifier live in the Resample's domain: the back-edge gave them none
    assert og.output(sp, 0).size == 800
    # the Mixer's input 1 reads Disconnected: its outputs are input 0's alone
    master, cue = oracle.mixer_run([(0.0, 1.0, False), (-6.0, 0.5, True)], [rs, None], rs.size)
    assert np.array_equal(og.output(y, 0).view(np.uint32), master.view(np.uint32))
    assert np.array_equal(og.output(y, 1).view(np.uint32), cue.view(np.uint32))
    order, dom, refusal = engine_domains(ws)
    assert refusal is None and dom[y] == dom[m] == dom[r] != 1


def test_oracle_refuses_a_module_whose_inputs_live_in_two_domains():
    ws, s, r, y, m, sp = back_edge_graph(True)
    with pytest.raises(RuntimeError):
        oracle.OracleGraph(ws)   # the Amplifier runs first in the base domain; the Mixer mixes it with the Resample's output
    order, dom, refusal = engine_domains(ws)
    assert order == [s, r, m, y, sp] and refusal == (y, "mixed")


def test_oracle_runs_an_output_device_as_a_sink_in_the_engine_run_order():
    ws = Workspace(48000, 60)
    src = ws.source_stereo()
    od_a = ws.output_device(2, 0, 1)
    amp = ws.amplifier(1.5, 0.0)
    od_b = ws.output_device(6, 9, None)
    ws.connect(src, 0, amp, 0); ws.connect(amp, 0, od_b, 0)
    og = oracle.OracleGraph(ws)
    assert og.run_order() == engine_domains(ws)[0] == [od_a, src, amp, od_b]
    og.set_source(src, np.ones(1600, np.float32))
    og.run_tick(0)
    og.update_params(od_a, abi.OutputDeviceParams(8, 7, 7, 0))
    og.run_tick(1)
    assert np.all(og.output(amp, 0) == np.float32(1.5))
