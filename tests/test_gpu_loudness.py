"""Loudness taps on the device against tests/loudness_model.py, bit for bit (any NaN equals any NaN).  The model is fed what the graph itself
wrote on each tapped port (read back with read_output), so what is tested here is the measurement; the ports have their own parity tests."""
import numpy as np
import pytest

import loudness_model as lm
import spectrum_model as sm
import synth
from meter_model import MeterModel
from meter_model import records_equal as meter_records_equal
from mixlab_amd import abi, ingest, video
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import strips
from test_gpu_spectrum import io_graph, wide
from tick_shapes import by_id

pytestmark = pytest.mark.gpu


class Tap:
    """one tap and its model; `rate` is the port's (up, down) domain, channels what read_output returns per frame"""

    def __init__(self, node, port, channels, sr, spt, m=24, s=180, rate=(1, 1)):
        self.node, self.port, self.channels, self.rate = node, port, channels, rate
        self.args = (channels, sr * rate[0] / rate[1], spt * rate[0] // rate[1], m, s)
        self.reset()

    def reset(self):
        self.model = lm.LoudnessModel(*self.args)

    def port_data(self, g, n_ticks):
        return g.read_output(self.node, self.port, n_ticks, self.channels == 2, rate=self.rate)


def set_taps(g, taps, m=24, s=180):
    g.set_loudness([(t.node, t.port) for t in taps], m, s)
    for t in taps:
        t.reset()


def check_run(g, taps, n_ticks, what, port_source=None):
    """the last run's records of every tap against its model fed the port's samples (read from `port_source`, default g)"""
    got = g.read_loudness(0, n_ticks)
    assert got.shape == (n_ticks, len(taps))
    for i, t in enumerate(taps):
        want = t.model.run(t.port_data(port_source or g, n_ticks), n_ticks)
        assert lm.records_equal(got[:, i], want), f"{what}: tap {i} ({t.node}, {t.port}): {lm.first_difference(got[:, i], want)}"
    return got


@pytest.mark.parametrize("shape_id", ["44k1", "48k", "44k1_100", "48k_1000", "8k_8000", "5k4"])
def test_mono_and_stereo_ports_at_several_rates_and_tick_lengths(shape_id):
    shape = by_id(shape_id)
    spt, sr = shape.spt, shape.sample_rate
    n_ticks = 37 if spt > 100 else 150   # more than one block of 32 (stereo) ticks; the short ticks also beyond 64 and past the 11-frame history
    ws, ss, smn, amp, g = io_graph(sr, shape.ticks_per_second, n_ticks)
    for m, s in ((24, 180), (3, 1)):
        taps = [Tap(amp, 0, 2, sr, spt, m, s), Tap(smn, 0, 1, sr, spt, m, s), Tap(ss, 0, 2, sr, spt, m, s)]
        set_taps(g, taps, m, s)   # every set starts from silence again
        for r in range(2):        # state, window and frame history carry across runs
            g.write_source(ss, wide(10 * r + 1, n_ticks * 2 * spt), n_ticks)
            g.write_source(smn, wide(10 * r + 2, n_ticks * spt), n_ticks)
            g.run_ticks(r * n_ticks, n_ticks)
            got = check_run(g, taps, n_ticks, f"{shape.id} M {m} S {s} run {r}")
            assert (got["frames"] == spt).all() and (got["channels"][:, 1] == 1).all() and (got["channels"][:, 0] == 2).all()
            assert not got["ksq"][:, 1, 1].any() and not got["true_peak"][:, 1, 1].any()   # a mono port's [1] is 0
        assert g.read_loudness(n_ticks - 1, 1).tobytes() == got[n_ticks - 1:].tobytes()   # a window of the last run is the matching slice


@pytest.mark.parametrize("sr,spt", [(44100, 735), (48000, 800)])
def test_one_run_one_tick_runs_uneven_runs_and_a_cut_run_agree(sr, spt):
    n = 70
    xs, xm = wide(1, n * 2 * spt), wide(2, n * spt)
    records = []
    for cuts in ([n], [1] * n, [3, 1, 33, 2, 30, 1], "cut"):
        cut = cuts == "cut"
        if cut:
            cuts = [n]
        assert sum(cuts) == n
        ws, ss, smn, amp, g = io_graph(sr, 60, max(cuts))
        taps = [Tap(amp, 0, 2, sr, spt, 24, 40), Tap(smn, 0, 1, sr, spt, 24, 40)]
        set_taps(g, taps, 24, 40)
        out, at = [], 0
        for c in cuts:
            g.write_source(ss, xs[at * 2 * spt:(at + c) * 2 * spt], c); g.write_source(smn, xm[at * spt:(at + c) * spt], c)
            if cut:   # the same parameters again: the run is cut into spans at ticks 5 and 41, the samples are what they were
                g.schedule_params(amp, 5, abi.AmplifierParams(1.5, 0.0)); g.schedule_params(amp, 41, abi.AmplifierParams(1.5, 0.0))
            g.run_ticks(at, c)
            out.append(check_run(g, taps, c, f"{sr} runs {cuts[:3]}.. at {at}"))
            at += c
        records.append(np.concatenate(out))
    for k in (1, 2, 3):
        assert records[0].tobytes() == records[k].tobytes() or all(lm.records_equal(records[0][:, i], records[k][:, i]) for i in range(2)), k
    # a second set resets every tap: the same first ticks read as they did from silence
    set_taps(g, taps, 24, 40)
    g.write_source(ss, xs[:4 * 2 * spt], 4); g.write_source(smn, xm[:4 * spt], 4); g.run_ticks(n, 4)
    got = check_run(g, taps, 4, "after a second set")
    assert all(lm.records_equal(got[:, i], records[0][:4, i]) for i in range(2))


def test_dup_stored_strip_ports_equal_the_unfused_graph():
    sr, n = 48000, 6
    ws, mix, srcs, trigs = strips(8, sr)
    amps = [mix + 6 * (k + 1) for k in range(8)]
    fused, plain = ws.build(max_ticks_per_run=n), ws.build(max_ticks_per_run=n, flags=abi.FLAG_NO_FUSE)
    with pytest.raises(abi.MxError):
        fused.output_device_ptr(amps[0], 0)   # stored one float per frame
    mk = lambda: [Tap(a, 0, 2, sr, 800) for a in amps] + [Tap(mix, 0, 2, sr, 800), Tap(mix, 1, 2, sr, 800)]
    tf, tp = mk(), mk()
    set_taps(fused, tf); set_taps(plain, tp)
    for r, nr in enumerate((n, 1, n)):   # a one-tick run between two longer ones
        for g in (fused, plain):
            for k, tr in enumerate(trigs):
                g.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                g.write_source(s, synth.noise(k + 10 * r, nr * 800) * np.float32(6.0), nr)
            g.run_ticks(r * n, nr)
        a = check_run(fused, tf, nr, f"fused run {r}")
        b = check_run(plain, tp, nr, f"unfused run {r}")
        assert all(lm.records_equal(a[:, i], b[:, i]) for i in range(len(tf))), "a dup-stored port reads as the unfused graph's stereo port"
        assert a["ksq"][:, 0, 0].tobytes() == a["ksq"][:, 0, 1].tobytes() and a["true_peak"][:, 0, 0].tobytes() == a["true_peak"][:, 0, 1].tobytes()
        assert (a["channels"] == 2).all()


def test_resample_output_has_its_own_rate():
    sr, n = 44100, 5
    ws = Workspace(sr, 60)
    src = ws.source_stereo()
    rs = ws.resample(160, 147, np.full((160, 4), 0.4))
    ws.connect(src, 0, rs, 0)
    g = ws.build(max_ticks_per_run=n)
    taps = [Tap(rs, 0, 2, sr, 735, rate=(160, 147)), Tap(src, 0, 2, sr, 735)]   # 48 kHz / 800 frames and 44.1 kHz / 735 frames per tick
    assert taps[0].args[1:3] == (48000.0, 800)
    set_taps(g, taps)
    for r in range(3):
        g.write_source(src, wide(r, n * 2 * 735), n)
        g.run_ticks(r * n, n)
        got = check_run(g, taps, n, f"resampled run {r}")
        assert (got["frames"][:, 0] == 800).all() and (got["frames"][:, 1] == 735).all()


@pytest.mark.parametrize("mode", ["flag", "auto", "auto-off"])
def test_master_and_cue_in_every_tail_mode_with_meters_and_spectra(mode, monkeypatch):
    """Runs go out in pairs: taps on the Master and the Cue go behind the held-back Mixer bank, taps on strips read that run's buffer
    parity.  Meters and spectrum taps sit on the same ports, each against its own model; the graph without taps gives every port."""
    sr, spt, n, n_runs, n_strips, n_fft = 48000, 800, 16, 8, 64, 1024
    edges = abi.log_band_edges(n_fft, 31, 20.0, 20000.0, 48000.0)
    if mode == "auto-off":
        monkeypatch.setenv("MX_OVERLAP_AUTO", "0")
    flags = abi.FLAG_OVERLAP_TAIL if mode == "flag" else 0
    ws, mix, srcs, trigs = strips(n_strips, sr)
    plain = ws.build(max_ticks_per_run=n, flags=flags)    # the same desk without taps
    g = ws.build(max_ticks_per_run=n, flags=flags)
    amps = [mix + 6 * (k + 1) for k in (0, 1, 17, 63)]
    where = [(mix, 0, 2), (amps[0], 0, 2), (mix, 1, 2), (srcs[5], 0, 1)] + [(a, 0, 2) for a in amps[1:]]
    taps = [Tap(nd, p, ch, sr, spt) for nd, p, ch in where]
    meters = [MeterModel(ch, 2, 0.75) for _, _, ch in where]
    spectra = [sm.SpectrumModel(ch, n_fft, edges) for _, _, ch in where]
    set_taps(g, taps)
    g.set_meters([(nd, p) for nd, p, _ in where], abi.MeterParams(2, 0.75))
    g.set_spectra([(nd, p) for nd, p, _ in where], n_fft, edges)
    noise = [synth.noise(k, n_runs * n * spt) * np.float32(8.0) for k in range(n_strips)]
    for r in range(n_runs):
        for gr in (plain, g):
            for k, tr in enumerate(trigs):
                gr.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                gr.write_source(s, noise[k][r * n * spt:(r + 1) * n * spt], n)
            gr.run_ticks(r * n, n)
        data = [t.port_data(plain, n) for t in taps]
        want_m = [m.run(d, n) for m, d in zip(meters, data)]
        want_s = [m.run(d, n) for m, d in zip(spectra, data)]
        if r % 2 == 0:   # not read: the next run is queued behind it first; the models take the desk's ports from the plain graph
            for t, d in zip(taps, data):
                t.model.run(d, n)
            continue
        for nd, p, ch in where:
            want = plain.read_output(nd, p, n, ch == 2).view(np.uint32)
            assert np.array_equal(g.read_output(nd, p, n, ch == 2).view(np.uint32), want), f"taps changed port ({nd}, {p})"
        check_run(g, taps, n, f"{mode} run {r}", port_source=plain)
        got_m, got_s = g.read_meters(0, n), g.read_spectra(0, n)
        for i in range(len(where)):
            assert meter_records_equal(got_m[:, i], want_m[i]).all(), f"meters of tap {i}"
            assert sm.records_equal(got_s[:, i], want_s[i]).all(), f"spectra of tap {i}"
    assert (g.tail_stream() is not None) == (mode != "auto-off")   # the taps do not end the automatic mode
    if mode != "auto-off":
        gated, at_once = g.debug_tail_releases()
        assert gated > 0


def test_taps_change_no_sample_and_no_picture():
    """a mixed audio + video graph and a strip desk, with and without loudness taps: every audio port, the Monitor's pictures and audio,
    the RGBA sink and the downloaded composite"""
    import oracle_video as ov
    from test_gpu_video_scopes import sink_graph
    N, spt = 6, 735
    sizes = [(320, 180), (212, 120), (320, 180)]
    hosts = [ov.HostFrame(w, h).fill(k, seed=21) for k, (w, h) in enumerate(sizes)]
    audio = synth.noise(9, N * 2 * spt)
    results = []
    for tapped in (False, True):
        ws, srcs, m0, m1, rgba, au, amp, mon = sink_graph()
        g = ws.build(max_ticks_per_run=N)
        dev = [video.DFrame(f.w, f.h).upload(*f.visible()) for f in hosts]
        for s, d in zip(srcs, dev):
            video.graph_set_video_source(g, s, d, dur=(1, 60), off=(0, 1), repeat=True)
        if tapped:
            g.set_loudness([(amp, 0), (au, 0)])
        g.write_source(au, audio, N)
        g.run_ticks(0, N)
        res = {"rgba": video.graph_rgba_output(g, rgba).copy(), "audio": g.read_output(amp, 0, N, True).copy(), "source": g.read_output(au, 0, N, True).copy(),
               "mon_audio": ingest.graph_read_monitor_audio_i16(g, mon, N, spt).copy()}
        for k in range(N):
            _ts, vid = ingest.graph_read_monitor_tick(g, mon, k)
            res[f"mon{k}"] = np.concatenate([p.ravel() for p in vid[0].download()])
        res["prog"] = np.concatenate([p.ravel() for p in video.graph_video_output(g, m1, 0).download()])
        if tapped:
            assert g.read_loudness(0, N).shape == (N, 2)
        results.append(res)
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]), f"{k} differs with taps set"
    # the desk: every strip's Amplifier, the Master and the Cue
    ws, mix, srcs, trigs = strips(8, 48000)
    ports = [(mix + 6 * (k + 1), 0) for k in range(8)] + [(mix, 0), (mix, 1)]
    outs = []
    for tapped in (False, True):
        g = ws.build(max_ticks_per_run=4)
        if tapped:
            g.set_loudness(ports)
        per_run = []
        for r in range(3):
            for k, s in enumerate(srcs):
                g.write_source(s, synth.noise(k + 5 * r, 4 * 800), 4)
            g.run_ticks(4 * r, 4)
            per_run.append(np.concatenate([g.read_output(nd, p, 4, True) for nd, p in ports]))
        outs.append(np.concatenate(per_run))
    assert outs[0].tobytes() == outs[1].tobytes()


def test_non_finite_subnormal_and_large_samples():
    sr, spt, n = 48000, 800, 4
    ws, ss, smn, amp, g = io_graph(sr, 60, n)
    taps = [Tap(ss, 0, 2, sr, spt, 2, 3), Tap(smn, 0, 1, sr, spt, 2, 3), Tap(amp, 0, 2, sr, spt, 2, 3)]
    set_taps(g, taps, 2, 3)
    rng = np.random.default_rng(9)
    tiny = np.array([1], np.uint32).view(np.float32)[0]
    xs = (rng.integers(-5000, 5000, n * 2 * spt).astype(np.float32) * tiny).astype(np.float32)   # subnormal samples
    g.write_source(ss, xs, n); g.write_source(smn, synth.noise(3, n * spt) * np.float32(2.0 ** -120), n); g.run_ticks(0, n)
    got = check_run(g, taps, n, "subnormal")
    assert got["true_peak"][:, 0].any() and not np.isnan(got["ksq"]).any()
    g.write_source(ss, synth.noise(4, n * 2 * spt) * np.float32(1e30), n); g.write_source(smn, synth.noise(5, n * spt) * np.float32(1e15), n)
    g.run_ticks(n, n)
    got = check_run(g, taps, n, "large")
    assert np.isfinite(got["ksq"]).all() and got["ksq"][:, 0].max() > 1e60
    x = synth.noise(6, n * 2 * spt); x[[5, 2 * spt + 7]] = np.nan; x[3 * 2 * spt + 100] = np.inf
    g.write_source(ss, x, n); g.write_source(smn, synth.noise(7, n * spt), n)
    g.run_ticks(2 * n, n)
    got = check_run(g, taps, n, "non-finite")
    assert np.isnan(got["ksq"][:, 0]).any() and np.isnan(got["true_peak"][:, 0]).any() and np.isnan(got["momentary_sq"][:, 0]).any()
    assert np.isfinite(got["ksq"][:, 1, 0]).all()   # the mono source next to it is untouched
    # the filter never forgets a NaN: the next run still reads NaN, as the model does
    g.write_source(ss, synth.noise(8, n * 2 * spt), n); g.write_source(smn, synth.noise(9, n * spt), n); g.run_ticks(3 * n, n)
    got = check_run(g, taps, n, "after a NaN")
    assert np.isnan(got["ksq"][:, 0]).all()


def test_refusals():
    ws = Workspace(48000, 60)
    ss = ws.source_stereo()
    vm = ws.video_mixer(a=None, b=None, fader=1.0)
    ws2, mix, srcs, trigs = strips(2, 48000)
    eq = mix + 4
    assert ws2.nodes[eq][0] == abi.KIND_EQ_THREE
    g = ws.build(max_ticks_per_run=4)
    g2 = ws2.build(max_ticks_per_run=4)

    def code(gr, ports, m=24, s=180):
        pa = (abi.PortRef * len(ports))(*[abi.PortRef(n, p) for n, p in ports])
        rc = abi.lib.mx_graph_set_loudness(gr._h, pa, len(ports), abi.C.byref(abi.LoudnessParams(m, s)))
        return rc, (abi.lib.mx_last_error() or b"").decode()

    assert code(g, [(vm, 0)])[0] == abi.MX_ERR_TYPE
    assert code(g, [(len(ws.nodes), 0)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 1)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 0), (ss, 0)])[0] == abi.MX_ERR_INVALID
    for m, s in ((0, 180), (1025, 180), (24, 0), (24, 1025), (1 << 31, 1)):
        assert code(g, [(ss, 0)], m, s)[0] == abi.MX_ERR_INVALID, (m, s)
    assert code(g, [(ss, 0)], 1024, 1024)[0] == abi.MX_OK and code(g, [(ss, 0)], 1, 1)[0] == abi.MX_OK
    pa = (abi.PortRef * 1)(abi.PortRef(ss, 0))
    assert abi.lib.mx_graph_set_loudness(g._h, pa, 1, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_set_loudness(g._h, None, 1, abi.C.byref(abi.LoudnessParams(24, 180))) == abi.MX_ERR_INVALID
    c, msg = code(g2, [(eq, 0)])
    with pytest.raises(abi.MxError) as e:
        g2.read_output(eq, 0, 1, True)
    assert c == abi.MX_ERR_INVALID and msg in str(e.value)   # a port the fusion did not materialise
    low = Workspace(3000, 60); ls = low.source_mono(); gl = low.build(max_ticks_per_run=2)
    assert code(gl, [(ls, 0)])[0] == abi.MX_ERR_INVALID      # a rate below twice the shelf frequency
    g.set_loudness([])
    with pytest.raises(abi.MxError):
        g.read_loudness(0, 1)   # no taps
    g.set_loudness([(ss, 0)])
    with pytest.raises(abi.MxError):
        g.read_loudness(0, 1)   # no run since the taps were set
    g.write_source(ss, wide(1, 4 * 1600), 4)
    g.run_ticks(0, 3)
    first = g.read_loudness(0, 3)
    assert code(g, [(ss, 0)], 0, 0)[0] == abi.MX_ERR_INVALID   # refused: the set and its records stay as they were
    assert g.read_loudness(0, 3).tobytes() == first.tobytes()
    for at, cnt in ((0, 4), (3, 1), (2, 2)):
        with pytest.raises(abi.MxError):
            g.read_loudness(at, cnt)   # beyond the last run
    out = np.zeros(3, abi.LOUDNESS_TICK_DTYPE)
    assert abi.lib.mx_graph_read_loudness(g._h, 0, 3, out.ctypes.data, 2) == abi.MX_ERR_INVALID   # cap too small
    assert abi.lib.mx_graph_read_loudness(g._h, 0, 3, out.ctypes.data, 3) == abi.MX_OK
    assert out.tobytes() == first.tobytes()


def test_adopt_state_carries_no_taps_and_profile_counts_them_in_the_total_only():
    ws, ss, smn, amp, g = io_graph(48000, 60, 8)
    g.write_source(ss, wide(1, 8 * 1600), 8); g.write_source(smn, wide(2, 8 * 800), 8)
    g.set_loudness([(amp, 0), (smn, 0)])
    for r in range(2):
        by_kind, total = g.profile_run(8 * r, 8)
        assert total > 0 and set(by_kind) <= set(abi.KIND_NAMES[:abi.PROFILE_KINDS])
        assert total > sum(by_kind.values())   # the taps' launches are in the total, in no kind
    assert g.read_loudness(0, 8).shape == (8, 2)
    g2 = ws.build(max_ticks_per_run=8)
    g2.adopt_state(g, list(range(len(ws.nodes))))
    g2.write_source(ss, wide(1, 8 * 1600), 8); g2.write_source(smn, wide(2, 8 * 800), 8); g2.run_ticks(16, 8)
    with pytest.raises(abi.MxError):
        g2.read_loudness(0, 1)
