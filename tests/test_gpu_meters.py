"""Level meters on the device against tests/meter_model.py, bit for bit (sum_sq: any NaN equals any NaN).  The model is fed what the graph
itself wrote on each tapped port (read back with read_output), so what is tested here is the meter; the ports have their own parity tests."""
import numpy as np
import pytest

import synth
from meter_model import MeterModel, records_equal
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import strips
from tick_shapes import SHAPES, by_id

pytestmark = pytest.mark.gpu

MP = abi.MeterParams


def spicy(seed, n, scale=1.5):
    """noise that crosses +-1, with the special values every meter field must get right"""
    x = (synth.noise(seed, n) * np.float32(scale)).astype(np.float32)
    sp = np.array([np.nan, np.inf, -np.inf, 1.0, -1.0, np.nextafter(np.float32(1), np.float32(2)), -0.0,
                   np.array([1], np.uint32).view(np.float32)[0], -np.array([0x007FFFFF], np.uint32).view(np.float32)[0]], np.float32)
    rng = np.random.default_rng(seed)
    if n >= 64:
        at = rng.choice(n, size=min(n // 8, 3 * sp.size), replace=False)
        x[at] = np.resize(sp, at.size)
    x[rng.choice(n, size=max(1, n // 50), replace=False)] *= np.float32(1e-41)   # subnormal products through the f64 squares
    return x


class Tap:
    """one tap and its model; `rate` is the port's (up, down) domain, channels what read_output returns per frame"""

    def __init__(self, node, port, channels, hold_ticks=2, release=0.75, rate=(1, 1)):
        self.node, self.port, self.channels, self.rate = node, port, channels, rate
        self.params = MP(hold_ticks, release)
        self.model = MeterModel(channels, hold_ticks, release)

    def port_data(self, g, n_ticks):
        return g.read_output(self.node, self.port, n_ticks, self.channels == 2, rate=self.rate)


def set_taps(g, taps):
    g.set_meters([(t.node, t.port) for t in taps], [t.params for t in taps])


def check_run(g, taps, n_ticks, what, port_source=None):
    """the last run's records of every tap against its model fed the port's samples (read from `port_source`, default g)"""
    got = g.read_meters(0, n_ticks)
    assert got.shape == (n_ticks, len(taps))
    for i, t in enumerate(taps):
        want = t.model.run(t.port_data(port_source or g, n_ticks), n_ticks)
        ok = records_equal(got[:, i], want)
        if not ok.all():
            k = int(np.flatnonzero(~ok)[0])
            raise AssertionError(f"{what}: tap {i} ({t.node}, {t.port}) tick {k}: got {got[k, i]}, want {want[k]}")
    return got


def io_graph(sr, tps, max_ticks, flags=0):
    ws = Workspace(sr, tps)
    ss, sm = ws.source_stereo(), ws.source_mono()
    amp = ws.amplifier(1.5, 0.0)
    ws.connect(ss, 0, amp, 0)
    return ws, ss, sm, amp, ws.build(max_ticks_per_run=max_ticks, flags=flags)


@pytest.mark.parametrize("shape", SHAPES, ids=[s.id for s in SHAPES])
@pytest.mark.parametrize("n_ticks", [1, 7])
def test_every_tick_shape_mono_and_stereo(shape, n_ticks):
    spt = shape.spt
    ws, ss, sm, amp, g = io_graph(shape.sample_rate, shape.ticks_per_second, n_ticks)
    taps = [Tap(amp, 0, 2), Tap(sm, 0, 1, hold_ticks=0, release=0.5), Tap(ss, 0, 2, hold_ticks=5, release=1.0)]
    set_taps(g, taps)
    for r in range(3):   # the hold carries across runs
        g.write_source(ss, spicy(10 * r + 1, n_ticks * 2 * spt), n_ticks)
        g.write_source(sm, spicy(10 * r + 2, n_ticks * spt) * np.float32(0.5 + r), n_ticks)
        g.run_ticks(r * n_ticks, n_ticks)
        got = check_run(g, taps, n_ticks, f"{shape.id} run {r}")
        assert all(int(v) == spt for v in got["frames"].ravel())
        assert list(got["channels"][0]) == [2, 1, 2]
    # a window of the last run is the matching slice
    assert g.read_meters(n_ticks - 1, 1).tobytes() == got[n_ticks - 1:].tobytes()


def test_dup_stored_strip_ports_equal_the_unfused_graph():
    sr, n = 48000, 6
    ws, mix, srcs, trigs = strips(8, sr)
    amps = [mix + 6 * (k + 1) for k in range(8)]
    assert all(ws.nodes[a][0] == abi.KIND_AMPLIFIER for a in amps)
    fused, plain = ws.build(max_ticks_per_run=n), ws.build(max_ticks_per_run=n, flags=abi.FLAG_NO_FUSE)
    with pytest.raises(abi.MxError):
        fused.output_device_ptr(amps[0], 0)   # stored one float per frame
    tf = [Tap(a, 0, 2, 1, 0.9) for a in amps] + [Tap(mix, 0, 2), Tap(mix, 1, 2)]
    tp = [Tap(a, 0, 2, 1, 0.9) for a in amps] + [Tap(mix, 0, 2), Tap(mix, 1, 2)]
    set_taps(fused, tf); set_taps(plain, tp)
    for r in range(3):
        for g in (fused, plain):
            for k, tr in enumerate(trigs):
                g.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                g.write_source(s, synth.noise(k + 10 * r, n * 800) * np.float32(6.0), n)
            g.run_ticks(r * n, n)
        a = check_run(fused, tf, n, f"fused run {r}")
        b = check_run(plain, tp, n, f"unfused run {r}")
        assert records_equal(a, b).all(), "a dup-stored port meters as the unfused graph's stereo port"


def test_resample_output_and_bound_source():
    sr, n = 44100, 5
    ws = Workspace(sr, 60)
    src = ws.source_stereo()
    rs = ws.resample(160, 147, np.full((160, 4), 0.4))
    ws.connect(src, 0, rs, 0)
    g = ws.build(max_ticks_per_run=n)
    taps = [Tap(rs, 0, 2, rate=(160, 147)), Tap(src, 0, 2)]
    set_taps(g, taps)
    for r in range(2):
        g.write_source(src, spicy(r, n * 2 * 735), n)
        g.run_ticks(r * n, n)
        got = check_run(g, taps, n, f"resampled run {r}")
        assert set(got["frames"][:, 0].tolist()) == {800} and set(got["frames"][:, 1].tolist()) == {735}
    # a source bound to a device buffer (here another graph's port)
    feed_ws = Workspace(sr, 60); feed = feed_ws.source_stereo(); fg = feed_ws.build(max_ticks_per_run=n)
    ws2 = Workspace(sr, 60); bsrc = ws2.source_stereo(); amp = ws2.amplifier(0.5, 0.0); ws2.connect(bsrc, 0, amp, 0)
    g2 = ws2.build(max_ticks_per_run=n)
    taps2 = [Tap(bsrc, 0, 2), Tap(amp, 0, 2)]
    set_taps(g2, taps2)   # before the bind: the descriptors follow it
    g2.bind_source_device(bsrc, fg.output_device_ptr(feed, 0)[0])
    for r in range(2):
        fg.write_source(feed, spicy(20 + r, n * 2 * 735), n)
        g2.run_ticks(r * n, n)
        check_run(g2, taps2, n, f"bound run {r}")


@pytest.mark.parametrize("n_taps,shape_id,n", [pytest.param(k, "48k", 3, id=str(k)) for k in (1, 7, 1024, 1031)]
                         # beyond 16 384 (tap, tick) pairs: k_meter_reduce's grid (4096 blocks of 4 waves) strides over the rest
                         + [pytest.param(9, "8k_8000", 5000, id="9-8k_8000-5000"), pytest.param(1031, "48k", 20, id="1031-48k-20")])
def test_many_taps(n_taps, shape_id, n):
    shape = by_id(shape_id)
    spt = shape.spt
    ws, mix, strip_srcs, trigs = strips(2, shape.sample_rate, shape.ticks_per_second)
    n_dup = 2 if n_taps >= 3 else 0   # the strips' Amplifiers, read by the Mixer alone: stored one float per frame
    nodes = [ws.source_mono() if k % 3 else ws.source_stereo() for k in range(n_taps - n_dup)]
    g = ws.build(max_ticks_per_run=n)
    taps = [Tap(s, 0, 1 if k % 3 else 2, hold_ticks=k % 4, release=0.5 + (k % 5) / 10) for k, s in enumerate(nodes)]
    taps += [Tap(mix + 6 * (k + 1), 0, 2, hold_ticks=k, release=0.9) for k in range(n_dup)]
    set_taps(g, taps)
    for r in range(2):
        for k, s in enumerate(nodes):
            g.write_source(s, synth.noise(k + 7 * r, n * spt * taps[k].channels) * np.float32(1 + k % 3), n)
        for k, s in enumerate(strip_srcs):
            g.write_source(s, synth.noise(5000 + k + 7 * r, n * spt) * np.float32(3.0), n)
        g.run_ticks(r * n, n)
        check_run(g, taps, n, f"{n_taps} taps run {r}")


@pytest.mark.parametrize("shape_id,n", [("48k", 2048), ("8k_8000", 5000)])   # 5000 ticks: more than two of k_meter_hold's 2048-tick chunks
def test_long_runs_and_one_tick_runs(shape_id, n):
    shape = by_id(shape_id)
    spt = shape.spt
    ws, ss, sm, amp, g = io_graph(shape.sample_rate, shape.ticks_per_second, n)
    taps = [Tap(amp, 0, 2, hold_ticks=30, release=0.9), Tap(sm, 0, 1, hold_ticks=3, release=0.99),
            Tap(ss, 0, 2, hold_ticks=1500, release=0.999)]   # holds that span the chunk boundaries
    set_taps(g, taps)
    g.write_source(ss, spicy(1, n * 2 * spt), n); g.write_source(sm, spicy(2, n * spt, 0.8), n)
    g.run_ticks(0, n)
    got = check_run(g, taps, n, f"{n} ticks")
    if n > 2048:   # a hold taken before a chunk boundary is still held after it
        h = got["hold"][:, 2, 0].view(np.uint32)
        assert any(h[b - 1] == h[b] and got["peak"][b, 2, 0] < got["hold"][b, 2, 0] for b in (2048, 4096))
    for r in range(4):   # one-tick runs on the same graph, the hold carried on
        g.write_source(ss, spicy(30 + r, 2 * spt), 1); g.write_source(sm, spicy(40 + r, spt), 1)
        g.run_ticks(n + r, 1)
        check_run(g, taps, 1, f"one tick {r}")


def test_runs_cut_by_scheduled_updates():
    sr, n, spt = 48000, 16, 800
    ws, ss, sm, amp, g = io_graph(sr, 60, n)
    taps = [Tap(amp, 0, 2, 1, 0.8), Tap(sm, 0, 1)]
    set_taps(g, taps)
    for r in range(2):
        g.write_source(ss, spicy(50 + r, n * 2 * spt), n); g.write_source(sm, spicy(60 + r, n * spt), n)
        g.schedule_params(amp, 3, abi.AmplifierParams(0.25, 0.0))
        g.schedule_params(amp, 9 + r, abi.AmplifierParams(2.0, 0.0))
        g.run_ticks(r * n, n)
        check_run(g, taps, n, f"cut run {r}")


def test_hold_kept_for_surviving_taps_and_reset_for_new_ones():
    sr, n = 48000, 4
    ws, ss, sm, amp, g = io_graph(sr, 60, n)
    a, s = Tap(amp, 0, 2, 100, 0.5), Tap(ss, 0, 2, 100, 0.5)
    set_taps(g, [a, s])
    g.write_source(ss, synth.noise(1, n * 1600) * np.float32(4.0), n); g.write_source(sm, synth.noise(2, n * 800) * np.float32(4.0), n)
    g.run_ticks(0, n)
    first = check_run(g, [a, s], n, "first set")
    with pytest.raises(abi.MxError):
        g.set_meters([(amp, 0), (sm, 0)], MP(0, 0.0))   # refused: the set stays as it was
    assert g.read_meters(0, n).tobytes() == first.tobytes()
    # the amplifier's tap survives (its hold of the loud run stays), the mono source's is new (from 0), the stereo source's goes
    m2 = Tap(sm, 0, 1, 100, 0.5)
    set_taps(g, [m2, a])
    with pytest.raises(abi.MxError):
        g.read_meters(0, 1)   # no run since the taps were set
    g.write_source(ss, synth.noise(3, n * 1600) * np.float32(0.01), n); g.write_source(sm, synth.noise(4, n * 800) * np.float32(0.01), n)
    g.run_ticks(n, n)
    got = check_run(g, [m2, a], n, "second set")
    assert float(got["hold"][0, 1][0]) > 0.5 and float(got["hold"][0, 0][0]) < 0.5
    g.set_meters([])
    g.run_ticks(2 * n, n)
    with pytest.raises(abi.MxError):
        g.read_meters(0, 1)   # no taps


@pytest.mark.parametrize("mode", ["flag", "auto", "auto-off"])
def test_strips_and_master_in_every_tail_mode(mode, monkeypatch):
    """Runs go out in pairs: a tap on the Master goes behind the held-back Mixer bank; taps on strips read that run's buffer parity"""
    sr, spt, n, n_runs, n_strips = 48000, 800, 16, 8, 64
    if mode == "auto-off":
        monkeypatch.setenv("MX_OVERLAP_AUTO", "0")
    flags = abi.FLAG_OVERLAP_TAIL if mode == "flag" else 0
    ws, mix, srcs, trigs = strips(n_strips, sr)
    plain = ws.build(max_ticks_per_run=n, flags=flags)   # the same desk without meters
    g = ws.build(max_ticks_per_run=n, flags=flags)
    amps = [mix + 6 * (k + 1) for k in (0, 1, 17, 63)]
    taps = [Tap(mix, 0, 2, 3, 0.7), Tap(amps[0], 0, 2), Tap(mix, 1, 2), Tap(srcs[5], 0, 1)] + [Tap(a, 0, 2, 1, 0.9) for a in amps[1:]]
    set_taps(g, taps)
    mono = {abi.KIND_SOURCE_MONO, abi.KIND_TRIGGER, abi.KIND_ENVELOPE, abi.KIND_EQ_THREE}
    ports = []   # every materialised audio port: (node, port, stereo)
    for node in range(len(ws.nodes)):
        for port in range(2 if node == mix else 1):
            try:
                plain.read_output(node, port, 1, ws.nodes[node][0] not in mono)
                ports.append((node, port, ws.nodes[node][0] not in mono))
            except abi.MxError:
                pass
    assert len(ports) == 2 + 2 * n_strips   # Master, Cue; per strip the source and the Amplifier (the rest is fused)
    noise = [synth.noise(k, n_runs * n * spt) * np.float32(8.0) for k in range(n_strips)]
    for r in range(n_runs):
        for gr in (plain, g):
            for k, tr in enumerate(trigs):
                gr.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                gr.write_source(s, noise[k][r * n * spt:(r + 1) * n * spt], n)
        plain.run_ticks(r * n, n)
        g.run_ticks(r * n, n)
        if r % 2 == 0:   # not read: the next run is queued behind it first; the models take the desk's ports from the plain graph
            for t in taps:
                t.model.run(t.port_data(plain, n), n)
            continue
        for node, port, st in ports:
            want = plain.read_output(node, port, n, st).view(np.uint32)
            assert np.array_equal(g.read_output(node, port, n, st).view(np.uint32), want), f"meters changed port ({node}, {port})"
        check_run(g, taps, n, f"{mode} run {r}", port_source=plain)
    assert (g.tail_stream() is not None) == (mode != "auto-off")   # the meters do not end the automatic mode
    if mode != "auto-off":
        gated, at_once = g.debug_tail_releases()
        assert gated > 0


def test_refusals():
    ws = Workspace(48000, 60)
    ss = ws.source_stereo()
    vm = ws.video_mixer(a=None, b=None, fader=1.0)
    ws2, mix, srcs, trigs = strips(2, 48000)
    eq = mix + 4
    assert ws2.nodes[eq][0] == abi.KIND_EQ_THREE
    g = ws.build(max_ticks_per_run=4)
    g2 = ws2.build(max_ticks_per_run=4)

    def code(gr, ports, params=MP(0, 1.0)):
        try:
            gr.set_meters(ports, params)
        except abi.MxError as e:
            return e.code, str(e)
        return 0, ""

    assert code(g, [(vm, 0)])[0] == abi.MX_ERR_TYPE
    assert code(g, [(len(ws.nodes), 0)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 1)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 0), (ss, 0)])[0] == abi.MX_ERR_INVALID
    for rel in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        assert code(g, [(ss, 0)], MP(0, rel))[0] == abi.MX_ERR_INVALID, rel
    c, msg = code(g2, [(eq, 0)])
    with pytest.raises(abi.MxError) as e:
        g2.read_output(eq, 0, 1, True)
    assert c == abi.MX_ERR_INVALID and msg == str(e.value)
    with pytest.raises(abi.MxError):
        g.read_meters(0, 1)   # no meters
    g.set_meters([(ss, 0)])
    g.write_source(ss, spicy(1, 4 * 1600), 4)
    g.run_ticks(0, 3)
    g.read_meters(0, 3)
    for first, cnt in ((0, 4), (3, 1), (2, 2)):
        with pytest.raises(abi.MxError):
            g.read_meters(first, cnt)   # beyond the last run
    out = np.zeros(2, abi.METER_TICK_DTYPE)
    assert abi.lib.mx_graph_read_meters(g._h, 0, 3, out.ctypes.data, 2) == abi.MX_ERR_INVALID   # cap too small
    assert abi.lib.mx_graph_read_meters(g._h, 0, 2, out.ctypes.data, 2) == abi.MX_OK


def test_profile_run_keeps_18_kinds_and_counts_meters_in_the_total():
    ws, ss, sm, amp, g = io_graph(48000, 60, 8)
    set_taps(g, [Tap(amp, 0, 2), Tap(sm, 0, 1)])
    g.write_source(ss, spicy(1, 8 * 1600), 8); g.write_source(sm, spicy(2, 8 * 800), 8)
    for r in range(2):
        by_kind, total = g.profile_run(8 * r, 8)
        assert total > 0 and set(by_kind) <= set(abi.KIND_NAMES[:abi.PROFILE_KINDS])
        info, us = g.performance_info(len(ws.nodes))
        tick_us = total * 1000.0 / 8
        assert abs(sum(us) + info.engine_us - tick_us) <= len(ws.nodes) + 2
    assert g.read_meters(0, 8).shape == (8, 2)
