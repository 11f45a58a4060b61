"""Spectrum taps on the device against tests/spectrum_model.py, bit for bit (any NaN equals any NaN).  The model is fed what the graph itself
wrote on each tapped port (read back with read_output), so what is tested here is the analyser; the ports have their own parity tests."""
import numpy as np
import pytest

import synth
import spectrum_model as sm
from meter_model import MeterModel
from meter_model import records_equal as meter_records_equal
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import strips
from tick_shapes import SHAPES, by_id

pytestmark = pytest.mark.gpu


def edges_for(n_fft, b):
    """B = 1: everything; 31: log bands (one-bin bands at the bottom, > 64 bins at the top of the larger sizes); 128: narrow bands and a wide last one"""
    top = n_fft // 2 + 1
    if b == 1:
        return np.array([0, top], np.uint16)
    if b == 31:
        return abi.log_band_edges(n_fft, 31, 20.0, 20000.0, 48000.0)
    e = np.arange(129, dtype=np.uint16)   # 127 bands of one bin ...
    e[128] = top                          # ... and one of the rest
    return e


class Tap:
    """one tap and its model; `rate` is the port's (up, down) domain, channels what read_output returns per frame"""

    def __init__(self, node, port, channels, n_fft, edges, rate=(1, 1)):
        self.node, self.port, self.channels, self.rate = node, port, channels, rate
        self.model = sm.SpectrumModel(channels, n_fft, edges)

    def port_data(self, g, n_ticks):
        return g.read_output(self.node, self.port, n_ticks, self.channels == 2, rate=self.rate)


def set_taps(g, taps, n_fft, edges):
    g.set_spectra([(t.node, t.port) for t in taps], n_fft, edges)


def check_run(g, taps, n_ticks, what, port_source=None):
    """the last run's records of every tap against its model fed the port's samples (read from `port_source`, default g)"""
    got = g.read_spectra(0, n_ticks)
    assert got.shape[:3] == (n_ticks, len(taps), 2)
    for i, t in enumerate(taps):
        want = t.model.run(t.port_data(port_source or g, n_ticks), n_ticks)
        ok = sm.records_equal(got[:, i], want)
        if not ok.all():
            k, c, j = (int(v[0]) for v in np.nonzero(~ok))
            raise AssertionError(f"{what}: tap {i} ({t.node}, {t.port}) tick {k} channel {c} band {j}: got {got[k, i, c, j]!r}, want {want[k, c, j]!r} "
                                 f"({int((~ok).sum())} of {ok.size} differ)")
    return got


def io_graph(sr, tps, max_ticks, flags=0):
    ws = Workspace(sr, tps)
    ss, sm_ = ws.source_stereo(), ws.source_mono()
    amp = ws.amplifier(1.5, 0.0)
    ws.connect(ss, 0, amp, 0)
    return ws, ss, sm_, amp, ws.build(max_ticks_per_run=max_ticks, flags=flags)


def wide(seed, n):
    """noise over a wide dynamic range, so that the order of every addition shows in the last bits"""
    rng = np.random.default_rng(seed)
    return (synth.noise(seed, n) * np.exp2(rng.integers(-12, 3, n))).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=[s.id for s in SHAPES])
@pytest.mark.parametrize("n_fft", sm.SIZES)
def test_every_size_and_tick_shape_mono_and_stereo(shape, n_fft):
    spt, n_ticks = shape.spt, 5
    ws, ss, smn, amp, g = io_graph(shape.sample_rate, shape.ticks_per_second, n_ticks)
    for b in (31, 1, 128):
        edges = edges_for(n_fft, b)
        taps = [Tap(amp, 0, 2, n_fft, edges), Tap(smn, 0, 1, n_fft, edges), Tap(ss, 0, 2, n_fft, edges)]
        set_taps(g, taps, n_fft, edges)   # every set starts from silence again
        for r in range(2 if b == 31 else 1):   # the history carries across runs
            g.write_source(ss, wide(10 * r + 1, n_ticks * 2 * spt), n_ticks)
            g.write_source(smn, wide(10 * r + 2, n_ticks * spt), n_ticks)
            g.run_ticks(r * n_ticks, n_ticks)
            got = check_run(g, taps, n_ticks, f"{shape.id} N {n_fft} B {b} run {r}")
            assert got.shape == (n_ticks, 3, 2, b) and not got[:, 1, 1].any()   # a mono port's [1] is 0
        assert g.read_spectra(n_ticks - 1, 1).tobytes() == got[n_ticks - 1:].tobytes()   # a window of the last run is the matching slice


@pytest.mark.parametrize("n_fft", [512, 2048, 4096])
def test_history_one_run_one_tick_runs_and_uneven_runs_agree(n_fft):
    sr, spt, n = 44100, 735, 64
    edges = edges_for(n_fft, 31)
    xs, xm = wide(1, n * 2 * spt), wide(2, n * spt)
    records = []
    for cuts in ([n], [1] * n, [3, 1, 17, 2, 40, 1]):
        assert sum(cuts) == n
        ws, ss, smn, amp, g = io_graph(sr, 60, max(cuts))
        taps = [Tap(amp, 0, 2, n_fft, edges), Tap(smn, 0, 1, n_fft, edges)]
        set_taps(g, taps, n_fft, edges)
        out, at = [], 0
        for c in cuts:
            g.write_source(ss, xs[at * 2 * spt:(at + c) * 2 * spt], c); g.write_source(smn, xm[at * spt:(at + c) * spt], c)
            g.run_ticks(at, c)
            out.append(check_run(g, taps, c, f"N {n_fft} runs {cuts[:3]}.. at {at}"))
            at += c
        records.append(np.concatenate(out))
    assert records[0].tobytes() == records[1].tobytes() == records[2].tobytes()
    # the first tick saw zeros before the set point: its frame is n_fft - 735 zeros and the tick (n_fft = 512 < 735 needs no history)
    ws, ss, smn, amp, g = io_graph(sr, 60, 1)
    t = Tap(smn, 0, 1, n_fft, edges)
    set_taps(g, [t], n_fft, edges)
    for r in range(3):
        g.write_source(smn, xm[r * spt:(r + 1) * spt], 1); g.run_ticks(r, 1)
    set_taps(g, [t], n_fft, edges)   # a second set starts from zeros again: the model starts anew too
    t.model = sm.SpectrumModel(1, n_fft, edges)
    g.write_source(smn, xm[:spt], 1); g.run_ticks(3, 1)
    got = check_run(g, [t], 1, "after a second set")
    assert got[0, 0].tobytes() == records[0][0, 1].tobytes()


def test_dup_stored_strip_ports_equal_the_unfused_graph():
    sr, n, n_fft = 48000, 6, 1024
    edges = edges_for(n_fft, 31)
    ws, mix, srcs, trigs = strips(8, sr)
    amps = [mix + 6 * (k + 1) for k in range(8)]
    fused, plain = ws.build(max_ticks_per_run=n), ws.build(max_ticks_per_run=n, flags=abi.FLAG_NO_FUSE)
    with pytest.raises(abi.MxError):
        fused.output_device_ptr(amps[0], 0)   # stored one float per frame
    mk = lambda: [Tap(a, 0, 2, n_fft, edges) for a in amps] + [Tap(mix, 0, 2, n_fft, edges), Tap(mix, 1, 2, n_fft, edges)]
    tf, tp = mk(), mk()
    set_taps(fused, tf, n_fft, edges); set_taps(plain, tp, n_fft, edges)
    for r in range(3):
        for g in (fused, plain):
            for k, tr in enumerate(trigs):
                g.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                g.write_source(s, synth.noise(k + 10 * r, n * 800) * np.float32(6.0), n)
            g.run_ticks(r * n, n)
        a = check_run(fused, tf, n, f"fused run {r}")
        b = check_run(plain, tp, n, f"unfused run {r}")
        assert sm.records_equal(a, b).all(), "a dup-stored port reads as the unfused graph's stereo port"
        assert np.array_equal(a[:, 0, 0].view(np.uint32), a[:, 0, 1].view(np.uint32)) or np.isnan(a[:, 0]).any()


def test_resample_output_and_bound_source():
    sr, n, n_fft = 44100, 5, 2048
    edges = edges_for(n_fft, 31)
    ws = Workspace(sr, 60)
    src = ws.source_stereo()
    rs = ws.resample(160, 147, np.full((160, 4), 0.4))
    ws.connect(src, 0, rs, 0)
    g = ws.build(max_ticks_per_run=n)
    taps = [Tap(rs, 0, 2, n_fft, edges, rate=(160, 147)), Tap(src, 0, 2, n_fft, edges)]   # 800 and 735 frames per tick
    set_taps(g, taps, n_fft, edges)
    for r in range(2):
        g.write_source(src, wide(r, n * 2 * 735), n)
        g.run_ticks(r * n, n)
        check_run(g, taps, n, f"resampled run {r}")
    # a source bound to a device buffer (here another graph's port)
    feed_ws = Workspace(sr, 60); feed = feed_ws.source_stereo(); fg = feed_ws.build(max_ticks_per_run=n)
    ws2 = Workspace(sr, 60); bsrc = ws2.source_stereo(); amp = ws2.amplifier(0.5, 0.0); ws2.connect(bsrc, 0, amp, 0)
    g2 = ws2.build(max_ticks_per_run=n)
    taps2 = [Tap(bsrc, 0, 2, n_fft, edges), Tap(amp, 0, 2, n_fft, edges)]
    set_taps(g2, taps2, n_fft, edges)   # before the bind: the descriptors follow it
    g2.bind_source_device(bsrc, fg.output_device_ptr(feed, 0)[0])
    for r in range(2):
        fg.write_source(feed, wide(20 + r, n * 2 * 735), n)
        g2.run_ticks(r * n, n)
        check_run(g2, taps2, n, f"bound run {r}")


def test_a_thousand_taps():
    shape = by_id("48k")
    spt, n, n_taps, n_fft = shape.spt, 3, 1031, 1024
    edges = edges_for(n_fft, 31)
    ws, mix, strip_srcs, trigs = strips(2, shape.sample_rate, shape.ticks_per_second)
    nodes = [ws.source_mono() if k % 3 else ws.source_stereo() for k in range(n_taps - 2)]
    g = ws.build(max_ticks_per_run=n)
    taps = [Tap(s, 0, 1 if k % 3 else 2, n_fft, edges) for k, s in enumerate(nodes)]
    taps += [Tap(mix + 6 * (k + 1), 0, 2, n_fft, edges) for k in range(2)]   # the strips' Amplifiers: stored one float per frame
    set_taps(g, taps, n_fft, edges)
    for r in range(2):   # 3 093 (tap, tick) pairs: below the grid's cap; test_long_run strides beyond it
        for k, s in enumerate(nodes):
            g.write_source(s, synth.noise(k + 7 * r, n * spt * taps[k].channels) * np.float32(1 + k % 3), n)
        for k, s in enumerate(strip_srcs):
            g.write_source(s, synth.noise(5000 + k + 7 * r, n * spt) * np.float32(3.0), n)
        g.run_ticks(r * n, n)
        check_run(g, taps, n, f"{n_taps} taps run {r}")


def test_long_run_strides_the_grid():
    shape = by_id("8k_8000")   # one frame per tick at 8 kHz / 8 000 ticks per second: 5 000 ticks are 5 000 frames
    spt, n, n_fft = shape.spt, 5000, 256
    edges = edges_for(n_fft, 31)
    ws, ss, smn, amp, g = io_graph(shape.sample_rate, shape.ticks_per_second, n)
    taps = [Tap(amp, 0, 2, n_fft, edges), Tap(smn, 0, 1, n_fft, edges)]   # 10 000 pairs against 4 096 blocks
    set_taps(g, taps, n_fft, edges)
    g.write_source(ss, wide(1, n * 2 * spt), n); g.write_source(smn, wide(2, n * spt), n)
    g.run_ticks(0, n)
    check_run(g, taps, n, f"{n} ticks")


def test_runs_cut_by_scheduled_updates():
    sr, n, spt, n_fft = 48000, 16, 800, 2048
    edges = edges_for(n_fft, 31)
    ws, ss, smn, amp, g = io_graph(sr, 60, n)
    taps = [Tap(amp, 0, 2, n_fft, edges), Tap(smn, 0, 1, n_fft, edges)]
    set_taps(g, taps, n_fft, edges)
    for r in range(2):
        g.write_source(ss, wide(50 + r, n * 2 * spt), n); g.write_source(smn, wide(60 + r, n * spt), n)
        g.schedule_params(amp, 3, abi.AmplifierParams(0.25, 0.0))
        g.schedule_params(amp, 9 + r, abi.AmplifierParams(2.0, 0.0))
        g.run_ticks(r * n, n)
        check_run(g, taps, n, f"cut run {r}")


@pytest.mark.parametrize("mode", ["flag", "auto", "auto-off"])
def test_strips_master_and_cue_in_every_tail_mode_with_meters(mode, monkeypatch):
    """Runs go out in pairs: taps on the Master and the Cue go behind the held-back Mixer bank, taps on strips read that run's buffer parity.
    Meters are set on the same ports; a third graph with the meters alone shows that the spectra leave their records alone."""
    sr, spt, n, n_runs, n_strips, n_fft = 48000, 800, 16, 8, 64, 2048
    edges = edges_for(n_fft, 31)
    if mode == "auto-off":
        monkeypatch.setenv("MX_OVERLAP_AUTO", "0")
    flags = abi.FLAG_OVERLAP_TAIL if mode == "flag" else 0
    ws, mix, srcs, trigs = strips(n_strips, sr)
    plain = ws.build(max_ticks_per_run=n, flags=flags)    # the same desk without taps
    only_m = ws.build(max_ticks_per_run=n, flags=flags)   # ... with the meters alone
    g = ws.build(max_ticks_per_run=n, flags=flags)
    amps = [mix + 6 * (k + 1) for k in (0, 1, 17, 63)]
    where = [(mix, 0, 2), (amps[0], 0, 2), (mix, 1, 2), (srcs[5], 0, 1)] + [(a, 0, 2) for a in amps[1:]]
    taps = [Tap(nd, p, ch, n_fft, edges) for nd, p, ch in where]
    meters = [MeterModel(ch, 2, 0.75) for _, _, ch in where]
    set_taps(g, taps, n_fft, edges)
    for gr in (g, only_m):
        gr.set_meters([(nd, p) for nd, p, _ in where], abi.MeterParams(2, 0.75))
    noise = [synth.noise(k, n_runs * n * spt) * np.float32(8.0) for k in range(n_strips)]
    for r in range(n_runs):
        for gr in (plain, only_m, g):
            for k, tr in enumerate(trigs):
                gr.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                gr.write_source(s, noise[k][r * n * spt:(r + 1) * n * spt], n)
            gr.run_ticks(r * n, n)
        data = [t.port_data(plain, n) for t in taps]
        want_m = [m.run(d, n) for m, d in zip(meters, data)]
        if r % 2 == 0:   # not read: the next run is queued behind it first; the models take the desk's ports from the plain graph
            for t, d in zip(taps, data):
                t.model.run(d, n)
            continue
        for nd, p, ch in where:
            want = plain.read_output(nd, p, n, ch == 2).view(np.uint32)
            assert np.array_equal(g.read_output(nd, p, n, ch == 2).view(np.uint32), want), f"taps changed port ({nd}, {p})"
        check_run(g, taps, n, f"{mode} run {r}", port_source=plain)
        got_m = g.read_meters(0, n)
        assert got_m.tobytes() == only_m.read_meters(0, n).tobytes(), "the meter records are what they are without spectra"
        for i in range(len(where)):
            assert meter_records_equal(got_m[:, i], want_m[i]).all()
    assert (g.tail_stream() is not None) == (mode != "auto-off")   # the taps do not end the automatic mode
    if mode != "auto-off":
        gated, at_once = g.debug_tail_releases()
        assert gated > 0


def from_bits(b):
    return np.array([b], np.uint32).view(np.float32)[0]


def test_subnormal_large_and_non_finite_samples():
    sr, spt, n, n_fft = 48000, 800, 4, 1024
    edges = edges_for(n_fft, 31)
    ws, ss, smn, amp, g = io_graph(sr, 60, n)
    taps = [Tap(ss, 0, 2, n_fft, edges), Tap(smn, 0, 1, n_fft, edges), Tap(amp, 0, 2, n_fft, edges)]
    set_taps(g, taps, n_fft, edges)
    rng = np.random.default_rng(9)
    # subnormals: samples of a few thousand ulps of 2^-149, and normal samples so small that the window makes them subnormal
    xs = (rng.integers(-5000, 5000, n * 2 * spt).astype(np.float32) * from_bits(1)).astype(np.float32)
    xm = (synth.noise(3, n * spt) * np.float32(2.0 ** -120)).astype(np.float32)
    assert xs.any() and (np.abs(xs[xs != 0]) < from_bits(0x00800000)).all()
    g.write_source(ss, xs, n); g.write_source(smn, xm, n); g.run_ticks(0, n)
    got = check_run(g, taps, n, "subnormal")
    assert not np.isnan(got).any()
    # large finite samples: 1e30 squares to 1e60 in the f64 powers and overflows the f32 record to +Inf in the loud bands
    g.write_source(ss, synth.noise(4, n * 2 * spt) * np.float32(1e30), n); g.write_source(smn, synth.noise(5, n * spt) * np.float32(1e15), n)
    g.run_ticks(n, n)
    got = check_run(g, taps, n, "large")
    assert np.isinf(got[:, 0]).any() and np.isfinite(got[:, 1, 0]).all() and got[:, 1, 0].max() > 1e20
    # NaN and Inf in the stream: any NaN equals any NaN
    x = synth.noise(6, n * 2 * spt); x[[5, 2 * spt + 7]] = np.nan; x[3 * 2 * spt + 100] = np.inf
    g.write_source(ss, x, n); g.write_source(smn, synth.noise(7, n * spt), n)
    g.run_ticks(2 * n, n)
    got = check_run(g, taps, n, "non-finite")
    assert np.isnan(got[:, 0]).any() and np.isfinite(got[:, 1, 0]).all()


def test_refusals():
    ws = Workspace(48000, 60)
    ss = ws.source_stereo()
    vm = ws.video_mixer(a=None, b=None, fader=1.0)
    ws2, mix, srcs, trigs = strips(2, 48000)
    eq = mix + 4
    assert ws2.nodes[eq][0] == abi.KIND_EQ_THREE
    g = ws.build(max_ticks_per_run=4)
    g2 = ws2.build(max_ticks_per_run=4)
    good = edges_for(1024, 31)

    def code(gr, ports, n_fft=1024, edges=good, n_bands=None):
        e = np.ascontiguousarray(edges, np.uint16)
        pa = (abi.PortRef * len(ports))(*[abi.PortRef(n, p) for n, p in ports])
        pr = abi.SpectrumParams(n_fft, e.size - 1 if n_bands is None else n_bands, e.ctypes.data_as(abi.C.POINTER(abi.C.c_uint16)))
        rc = abi.lib.mx_graph_set_spectra(gr._h, pa, len(ports), abi.C.byref(pr))
        return rc, (abi.lib.mx_last_error() or b"").decode()

    assert code(g, [(vm, 0)])[0] == abi.MX_ERR_TYPE
    assert code(g, [(len(ws.nodes), 0)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 1)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 0), (ss, 0)])[0] == abi.MX_ERR_INVALID
    for n_fft in (0, 128, 1000, 8192, 1 << 31):
        assert code(g, [(ss, 0)], n_fft=n_fft)[0] == abi.MX_ERR_INVALID, n_fft
    assert code(g, [(ss, 0)], n_bands=0)[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 0)], edges=np.arange(130))[0] == abi.MX_ERR_INVALID           # 129 bands
    assert code(g, [(ss, 0)], edges=[0, 5, 5, 9])[0] == abi.MX_ERR_INVALID             # not strictly ascending
    assert code(g, [(ss, 0)], edges=[0, 9, 5])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 0)], edges=[0, 514])[0] == abi.MX_ERR_INVALID                 # beyond n_fft / 2 + 1
    assert code(g, [(ss, 0)], edges=[0, 513])[0] == abi.MX_OK
    pa = (abi.PortRef * 1)(abi.PortRef(ss, 0))
    assert abi.lib.mx_graph_set_spectra(g._h, pa, 1, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_set_spectra(g._h, pa, 1, abi.C.byref(abi.SpectrumParams(1024, 1, None))) == abi.MX_ERR_INVALID
    c, msg = code(g2, [(eq, 0)])
    with pytest.raises(abi.MxError) as e:
        g2.read_output(eq, 0, 1, True)
    assert c == abi.MX_ERR_INVALID and msg in str(e.value)
    g.set_spectra([])
    with pytest.raises(abi.MxError):
        g.read_spectra(0, 1)   # no taps
    g.set_spectra([(ss, 0)], 1024, good)
    with pytest.raises(abi.MxError):
        g.read_spectra(0, 1)   # no run since the taps were set
    g.write_source(ss, wide(1, 4 * 1600), 4)
    g.run_ticks(0, 3)
    first = g.read_spectra(0, 3)
    assert code(g, [(ss, 0)], n_fft=100)[0] == abi.MX_ERR_INVALID   # refused: the set and its records stay as they were
    assert g.read_spectra(0, 3).tobytes() == first.tobytes()
    for at, cnt in ((0, 4), (3, 1), (2, 2)):
        with pytest.raises(abi.MxError):
            g.read_spectra(at, cnt)   # beyond the last run
    out = np.zeros(3 * 2 * 31, np.float32)
    assert abi.lib.mx_graph_read_spectra(g._h, 0, 3, out.ctypes.data, out.size - 1) == abi.MX_ERR_INVALID   # cap too small
    assert abi.lib.mx_graph_read_spectra(g._h, 0, 3, out.ctypes.data, out.size) == abi.MX_OK
    assert out.tobytes() == first.tobytes()


def test_profile_run_keeps_18_kinds_and_counts_spectra_in_the_total():
    n_fft = 4096
    edges = edges_for(n_fft, 31)
    ws, ss, smn, amp, g = io_graph(48000, 60, 8)
    g.write_source(ss, wide(1, 8 * 1600), 8); g.write_source(smn, wide(2, 8 * 800), 8)
    _, bare = g.profile_run(0, 8); _, bare = g.profile_run(8, 8)
    taps = [Tap(amp, 0, 2, n_fft, edges), Tap(smn, 0, 1, n_fft, edges)]
    set_taps(g, taps, n_fft, edges)
    for r in range(2):
        by_kind, total = g.profile_run(16 + 8 * r, 8)
        assert total > 0 and set(by_kind) <= set(abi.KIND_NAMES[:abi.PROFILE_KINDS])
        info, us = g.performance_info(len(ws.nodes))
        tick_us = total * 1000.0 / 8
        assert abs(sum(us) + info.engine_us - tick_us) <= len(ws.nodes) + 2
        assert total > sum(by_kind.values())   # the taps' launches are in the total, in no kind
    print(f"profile: 8 ticks without taps {bare:.4f} ms, with 2 taps of n_fft {n_fft} {total:.4f} ms")
    assert g.read_spectra(0, 8).shape == (8, 2, 2, 31)
