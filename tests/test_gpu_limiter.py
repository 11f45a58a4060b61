"""Limiter taps on the device against tests/limiter_model.py, bit for bit: the limited copy, its i16 form and the per-tick records.  The
model is fed what the graph itself wrote on each tapped port (read back with read_output), so what is tested here is the limiter; the
ports have their own parity tests."""
import numpy as np
import pytest

import limiter_model as lm
import synth
from mixlab_amd import abi, ingest, video
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import strips
from test_gpu_spectrum import io_graph, wide
from tick_shapes import by_id

pytestmark = pytest.mark.gpu
F32 = np.float32
TILE = abi.LIMITER_TILE


class Tap:
    """one tap and its model; `rate` is the port's (up, down) domain"""

    def __init__(self, node, port, channels, rate=(1, 1)):
        self.node, self.port, self.channels, self.rate = node, port, channels, rate
        self.model = None

    def port_data(self, g, n_ticks):
        return g.read_output(self.node, self.port, n_ticks, self.channels == 2, rate=self.rate)


def set_taps(g, taps, ceiling, lookahead):
    g.set_limiters([(t.node, t.port) for t in taps], ceiling, lookahead)
    for t in taps:
        t.model = lm.LimiterModel(ceiling, lookahead, t.channels)


def check_run(g, taps, n_ticks, what, port_source=None):
    """the last run's copies (f32 and i16) and records of every tap against its model fed the port's samples (read from `port_source`,
    default g); returns (the copies, the records)"""
    got = g.read_limiters(0, n_ticks)
    assert got.shape == (n_ticks, len(taps))
    copies = []
    for i, t in enumerate(taps):
        want_y, want = t.model.run(t.port_data(port_source or g, n_ticks), n_ticks)
        y = g.read_limited(i, 0, n_ticks)
        diff = np.flatnonzero(y.view(np.uint32) != want_y.view(np.uint32)) if y.shape == want_y.shape else None
        assert diff is not None and diff.size == 0, \
            f"{what}: tap {i} ({t.node}, {t.port}): {0 if diff is None else diff.size} samples differ, first at {None if diff is None else diff[:4]}: " \
            f"{None if diff is None else (y[diff[:4]], want_y[diff[:4]])}"
        assert lm.records_equal(got[:, i], want), f"{what}: tap {i} ({t.node}, {t.port}): {lm.first_difference(got[:, i], want)}"
        assert np.array_equal(g.read_limited(i, 0, n_ticks, i16=True), lm.to_i16(want_y)), f"{what}: tap {i}: the i16 form"
        assert ((y.view(np.uint32) & 0x7fffffff) <= t.model.c.view(np.uint32)).all()
        copies.append(y)
    return copies, got


def programme(seed, frames, channels):
    """loud noise over a wide dynamic range with silent and quiet stretches (the transparent branch), and a few non-finite samples"""
    rng = np.random.default_rng(seed)
    x = (wide(seed, frames * channels) * F32(3.0)).reshape(frames, channels)
    for _ in range(4):
        at = int(rng.integers(0, max(1, frames - frames // 8)))
        x[at:at + frames // 8] *= F32(rng.choice([0.0, 0.01]))
    bad = rng.choice(frames * channels, 5, replace=False)
    x.reshape(-1)[bad] = np.array([np.inf, -np.inf, np.nan, 1e6, -3e38], F32)
    return x.reshape(-1)


@pytest.mark.parametrize("D", [0, 1, 7, 64, 512])
@pytest.mark.parametrize("shape_id", ["44k1", "48k", "8k_8000"])
def test_mono_and_stereo_ports_at_several_tick_lengths_and_lookaheads(shape_id, D):
    shape = by_id(shape_id)
    spt = shape.spt
    n_ticks = 5 if spt > 100 else 2500   # both cross the kernel's tile; 2500 one-frame ticks share two tiles
    ws, ss, smn, amp, g = io_graph(shape.sample_rate, shape.ticks_per_second, n_ticks)
    taps = [Tap(amp, 0, 2), Tap(smn, 0, 1), Tap(ss, 0, 2)]
    set_taps(g, taps, 0.5, D)
    for r in range(2):   # the frame history carries across runs
        g.write_source(ss, programme(10 * r + 1, n_ticks * spt, 2), n_ticks)
        g.write_source(smn, programme(10 * r + 2, n_ticks * spt, 1), n_ticks)
        g.run_ticks(r * n_ticks, n_ticks)
        _, got = check_run(g, taps, n_ticks, f"{shape.id} D {D} run {r}")
        assert (got["frames"] == spt).all() and got["channels"][0].tolist() == [2, 1, 2]
        assert got["limited"].sum() > 0 and got["nonfinite"].sum() > 0
    assert g.read_limiters(n_ticks - 1, 1).tobytes() == got[n_ticks - 1:].tobytes()   # a window of the last run is the matching slice
    assert g.read_limited(1, n_ticks - 1, 1).tobytes() == g.read_limited(1, 0, n_ticks)[(n_ticks - 1) * spt:].tobytes()


@pytest.mark.parametrize("D", [0, 1, 7, 64, 512])
def test_a_peak_on_every_boundary_and_d_and_2d_frames_before_it(D):
    """Single peaks in a quiet programme: on the last and the first frame of a tick, of a run and of the kernel's tile (counted from the
    run's first frame), and D and 2 D frames before each of those -- where the hold, the smoothing and the delayed output each reach
    across the boundary."""
    sr, spt, n_ticks, n_runs = 48000, 800, 4, 3   # a run is 3200 frames: one tile boundary inside it
    run_frames = n_ticks * spt
    ws, ss, smn, amp, g = io_graph(sr, 60, n_ticks)
    taps = [Tap(ss, 0, 2), Tap(smn, 0, 1)]
    set_taps(g, taps, 0.5, D)
    total = n_runs * run_frames
    xs = (synth.noise(3, total * 2) * F32(0.2)).astype(F32)
    xm = (synth.noise(4, total) * F32(0.2)).astype(F32)
    bounds = [spt, 3 * spt, run_frames, 2 * run_frames, TILE, run_frames + TILE, 2 * run_frames + TILE, total]
    at = sorted({b - 1 - back for b in bounds for back in (0, D, 2 * D)} | {b - back for b in bounds for back in (0, D, 2 * D)})
    at = [p for p in at if 0 <= p < total]
    for k, p in enumerate(at):
        xs[2 * p + (k & 1)] = F32(3.0 if k % 3 else -2.5)
        xm[p] = F32(-4.0 if k % 3 else 1.25)
    limited = 0
    for r in range(n_runs):
        g.write_source(ss, xs[r * run_frames * 2:(r + 1) * run_frames * 2], n_ticks)
        g.write_source(smn, xm[r * run_frames:(r + 1) * run_frames], n_ticks)
        g.run_ticks(r * n_ticks, n_ticks)
        _, got = check_run(g, taps, n_ticks, f"D {D} run {r}")
        limited += int(got["limited"].sum())
    assert limited > 0 and float(got["peak_out"].max()) <= 0.5


@pytest.mark.parametrize("sr,spt,D", [(48000, 800, 512), (44100, 735, 64), (8000, 1, 64)])
def test_one_run_one_tick_runs_runs_of_two_and_a_cut_run_agree(sr, spt, D):
    """2 D frames of history against one-tick runs of 800 frames (D 512) and of one frame (D 64): the history is shifted, not replaced"""
    n = 64
    tps = sr // spt
    xs = programme(1, n * spt, 2)
    results = []
    for cuts in ([n], [1] * n, [2] * (n // 2), "cut"):
        cut = cuts == "cut"
        if cut:
            cuts = [n]
        ws, ss, smn, amp, g = io_graph(sr, tps, max(cuts))
        taps = [Tap(amp, 0, 2), Tap(ss, 0, 2)]
        set_taps(g, taps, 0.25, D)
        ys, recs, at = [[], []], [], 0
        for c in cuts:
            g.write_source(ss, xs[at * 2 * spt:(at + c) * 2 * spt], c)
            if cut:   # the same parameters again: the run is cut into spans at ticks 5 and 41, the samples are what they were
                g.schedule_params(amp, 5, abi.AmplifierParams(1.5, 0.0)); g.schedule_params(amp, 41, abi.AmplifierParams(1.5, 0.0))
            g.run_ticks(at, c)
            y, rec = check_run(g, taps, c, f"{sr} D {D} runs {cuts[:3]}.. at {at}")
            ys[0].append(y[0]); ys[1].append(y[1]); recs.append(rec)
            at += c
        results.append((np.concatenate(ys[0]), np.concatenate(ys[1]), np.concatenate(recs)))
    for k in (1, 2, 3):
        for a, b in zip(results[0], results[k]):
            assert a.tobytes() == b.tobytes(), k
    # a second set resets every tap: the same first ticks read as they did from silence
    set_taps(g, taps, 0.25, D)
    g.write_source(ss, xs[:4 * 2 * spt], 4); g.run_ticks(n, 4)
    y, rec = check_run(g, taps, 4, "after a second set")
    assert y[0].tobytes() == results[0][0][:4 * 2 * spt].tobytes() and rec.tobytes() == results[0][2][:4].tobytes()


def test_device_bound_source_and_a_descriptor_reupload_keep_the_stream():
    """A source bound to a device buffer (another graph's port).  Binding it again rebuilds every tap descriptor and the room for the
    copies -- the path a changed call length takes, which only the per-module interface (no graph handle) can reach -- and what the taps
    carry comes through: the model runs on as one stream.  The limited copy's device pointer feeds a third graph."""
    sr, n, D = 44100, 3, 240
    feed_ws = Workspace(sr, 60); feed = feed_ws.source_stereo(); fg = feed_ws.build(max_ticks_per_run=n)
    ws2 = Workspace(sr, 60); bsrc = ws2.source_stereo(); amp = ws2.amplifier(0.5, 0.0); ws2.connect(bsrc, 0, amp, 0)
    g2 = ws2.build(max_ticks_per_run=n)
    taps = [Tap(bsrc, 0, 2)]
    set_taps(g2, taps, 0.5, D)   # before the bind: the descriptors follow it
    ptr = fg.output_device_ptr(feed, 0)[0]
    g2.bind_source_device(bsrc, ptr)
    ws3 = Workspace(sr, 60); csrc = ws3.source_stereo(); camp = ws3.amplifier(1.0, 0.0); ws3.connect(csrc, 0, camp, 0)
    g3 = ws3.build(max_ticks_per_run=n)
    for r in range(4):
        if r == 2:
            g2.bind_source_device(bsrc, ptr)
        fg.write_source(feed, programme(20 + r, n * 735, 2), n)
        g2.run_ticks(r * n, n)
        y, _ = check_run(g2, taps, n, f"bound run {r}")
    dev, stride = g2.limited_device_ptr(0)
    assert stride == 2 * 735 and dev % 4 == 0   # one tap: its ticks lie back to back
    assert dev % 16 == 0   # the first tap's copy starts the allocation
    g3.bind_source_device(csrc, dev)
    g2.sync(); g3.run_ticks(0, n)
    assert g3.read_output(csrc, 0, n, True).tobytes() == y[0].tobytes()
    with pytest.raises(abi.MxError):
        g2.limited_device_ptr(1)


def test_dup_stored_strip_ports_equal_the_unfused_graph():
    sr, n = 48000, 6
    ws, mix, srcs, trigs = strips(8, sr)
    amps = [mix + 6 * (k + 1) for k in range(8)]
    fused, plain = ws.build(max_ticks_per_run=n), ws.build(max_ticks_per_run=n, flags=abi.FLAG_NO_FUSE)
    with pytest.raises(abi.MxError):
        fused.output_device_ptr(amps[0], 0)   # stored one float per frame
    mk = lambda: [Tap(a, 0, 2) for a in amps] + [Tap(mix, 0, 2), Tap(mix, 1, 2)]
    tf, tp = mk(), mk()
    set_taps(fused, tf, 0.5, 64); set_taps(plain, tp, 0.5, 64)
    for r, nr in enumerate((n, 1, n)):   # a one-tick run between two longer ones
        for g in (fused, plain):
            for k, tr in enumerate(trigs):
                g.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                g.write_source(s, synth.noise(k + 10 * r, nr * 800) * F32(6.0), nr)
            g.run_ticks(r * n, nr)
        ya, a = check_run(fused, tf, nr, f"fused run {r}")
        yb, b = check_run(plain, tp, nr, f"unfused run {r}")
        assert a.tobytes() == b.tobytes() and all(p.tobytes() == q.tobytes() for p, q in zip(ya, yb)), "a dup-stored port reads as the unfused graph's stereo port"
        assert (a["channels"] == 2).all() and np.array_equal(ya[0][0::2], ya[0][1::2])   # interleaved stereo, L == R


def test_resample_output_has_its_own_rate():
    sr, n = 44100, 5
    ws = Workspace(sr, 60)
    src = ws.source_stereo()
    rs = ws.resample(160, 147, np.full((160, 4), 0.4))
    ws.connect(src, 0, rs, 0)
    g = ws.build(max_ticks_per_run=n)
    taps = [Tap(rs, 0, 2, rate=(160, 147)), Tap(src, 0, 2)]   # 800 and 735 frames per tick: the copies of a tick are 1600 + 1470 floats
    set_taps(g, taps, 0.5, 240)
    for r in range(3):
        g.write_source(src, wide(r, n * 2 * 735) * F32(2.0), n)
        g.run_ticks(r * n, n)
        y, got = check_run(g, taps, n, f"resampled run {r}")
        assert (got["frames"][:, 0] == 800).all() and (got["frames"][:, 1] == 735).all()
        assert y[0].size == n * 1600 and y[1].size == n * 1470
    assert g.limited_device_ptr(1)[1] == 1600 + 1470 and g.limited_device_ptr(1)[0] - g.limited_device_ptr(0)[0] == 4 * 1600


@pytest.mark.parametrize("mode", ["flag", "auto"])
def test_master_and_cue_behind_the_held_back_mixer_bank(mode):
    """Runs go out in pairs: taps on the Master and the Cue go behind the held-back Mixer bank on the second stream (both buffer parities,
    deferred launch), taps on strips read that run's buffer parity.  The graph without taps gives every port."""
    sr, spt, n, n_runs, n_strips = 48000, 800, 16, 8, 64
    flags = abi.FLAG_OVERLAP_TAIL if mode == "flag" else 0
    ws, mix, srcs, trigs = strips(n_strips, sr)
    plain = ws.build(max_ticks_per_run=n, flags=flags)    # the same desk without taps
    g = ws.build(max_ticks_per_run=n, flags=flags)
    amps = [mix + 6 * (k + 1) for k in (0, 17, 63)]
    where = [(mix, 0), (amps[0], 0), (mix, 1)] + [(a, 0) for a in amps[1:]]
    taps = [Tap(nd, p, 2) for nd, p in where]
    set_taps(g, taps, 0.25, 240)
    noise = [synth.noise(k, n_runs * n * spt) * F32(8.0) for k in range(n_strips)]
    for r in range(n_runs):
        for gr in (plain, g):
            for k, tr in enumerate(trigs):
                gr.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                gr.write_source(s, noise[k][r * n * spt:(r + 1) * n * spt], n)
            gr.run_ticks(r * n, n)
        if r % 2 == 0:   # not read: the next run is queued behind it first; the models take the desk's ports from the plain graph
            for t in taps:
                t.model.run(t.port_data(plain, n), n)
            continue
        for nd, p in where:
            want = plain.read_output(nd, p, n, True).view(np.uint32)
            assert np.array_equal(g.read_output(nd, p, n, True).view(np.uint32), want), f"taps changed port ({nd}, {p})"
        _, got = check_run(g, taps, n, f"{mode} run {r}", port_source=plain)
        assert got["limited"][:, 0].sum() > 0
    assert g.tail_stream() is not None   # the taps do not end the automatic mode
    gated, at_once = g.debug_tail_releases()
    assert gated > 0


def test_the_other_five_tap_sets_and_every_port_are_undisturbed():
    """a mixed audio + video graph with the five other tap sets, and with limiter taps as well: every output and every other set's records
    are the same in both, and the limiter's are the model's"""
    import oracle_video as ov
    from test_gpu_video_scopes import sink_graph
    N, spt, n_fft = 6, 735, 256
    edges = abi.log_band_edges(n_fft, 8, 100.0, 10000.0, 44100.0)
    sizes = [(320, 180), (212, 120), (320, 180)]
    hosts = [ov.HostFrame(w, h).fill(k, seed=21) for k, (w, h) in enumerate(sizes)]
    results = []
    for with_limiters in (False, True):
        ws, srcs, m0, m1, rgba, au, amp, mon = sink_graph()
        g = ws.build(max_ticks_per_run=N)
        dev = [video.DFrame(f.w, f.h).upload(*f.visible()) for f in hosts]
        for s, d in zip(srcs, dev):
            video.graph_set_video_source(g, s, d, dur=(1, 60), off=(0, 1), repeat=True)
        ports = [(amp, 0), (au, 0)]
        g.set_meters(ports, abi.MeterParams(2, 0.75)); g.set_spectra(ports, n_fft, edges); g.set_loudness(ports, 3, 5)
        g.set_stereo(ports, 4, 64, 1, 4)
        g.set_video_scopes([(m1, 0), (m0, 0)], wave_cols=64, vectorscope=True, hop=2)
        taps = [Tap(nd, p, 2) for nd, p in ports]
        if with_limiters:
            set_taps(g, taps, 0.5, 64)
        res = {}
        for r in range(2):
            g.write_source(au, synth.noise(9 + r, N * 2 * spt) * F32(2.0), N)
            g.run_ticks(r * N, N)
            res[f"rgba{r}"] = video.graph_rgba_output(g, rgba).copy()
            res[f"audio{r}"] = g.read_output(amp, 0, N, True).copy(); res[f"source{r}"] = g.read_output(au, 0, N, True).copy()
            res[f"mon_audio{r}"] = ingest.graph_read_monitor_audio_i16(g, mon, N, spt).copy()
            res[f"prog{r}"] = np.concatenate([p.ravel() for p in video.graph_video_output(g, m1, 0).download()])
            res[f"T meters{r}"] = g.read_meters(0, N).copy(); res[f"T spectra{r}"] = g.read_spectra(0, N).copy()
            res[f"T loudness{r}"] = g.read_loudness(0, N).copy(); res[f"T stereo{r}"] = g.read_stereo(0, N).copy()
            res[f"T gonio{r}"] = np.concatenate([np.concatenate([x["gon"].ravel(), [x["tick_in_run"], x["frames"]]]) for e in g.read_goniometers() for x in e])
            sc = g.read_video_scopes()
            res[f"T scopes{r}"] = np.concatenate([np.concatenate([x["hist"].ravel(), x["wave"].ravel(), x["vec"].ravel(), [x["tick_in_run"]]]) for e in sc for x in e])
            if with_limiters:
                _, got = check_run(g, taps, N, f"six sets, run {r}")
                assert got["limited"].sum() > 0
        results.append(res)
    for k in results[0]:
        assert results[0][k].tobytes() == results[1][k].tobytes(), f"{k} differs with limiter taps set"


def test_refusals():
    ws = Workspace(48000, 60)
    ss, smn = ws.source_stereo(), ws.source_mono()
    vm = ws.video_mixer(a=None, b=None, fader=1.0)
    ws2, mix, srcs, trigs = strips(2, 48000)
    pan = mix + 5
    assert ws2.nodes[pan][0] == abi.KIND_STEREO_PANNER
    g = ws.build(max_ticks_per_run=4)
    g2 = ws2.build(max_ticks_per_run=4)

    def code(gr, ports, c=0.5, D=64):
        pa = (abi.PortRef * len(ports))(*[abi.PortRef(n, p) for n, p in ports])
        rc = abi.lib.mx_graph_set_limiters(gr._h, pa, len(ports), abi.C.byref(abi.LimiterParams(c, D)))
        return rc, (abi.lib.mx_last_error() or b"").decode()

    assert code(g, [(vm, 0)])[0] == abi.MX_ERR_TYPE
    assert code(g, [(len(ws.nodes), 0)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 1)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 0), (smn, 0), (ss, 0)])[0] == abi.MX_ERR_INVALID   # a duplicate
    for c, D in ((1.0000001, 64), (0.0, 64), (2.0 ** -21, 64), (-0.5, 64), (float("nan"), 64), (float("inf"), 64), (0.5, 513), (0.5, 1 << 31)):
        assert code(g, [(ss, 0)], c, D)[0] == abi.MX_ERR_INVALID, (c, D)
    assert code(g, [(ss, 0)], 1.0, 512)[0] == abi.MX_OK and code(g, [(ss, 0), (smn, 0)], 2.0 ** -20, 0)[0] == abi.MX_OK
    pa = (abi.PortRef * 1)(abi.PortRef(ss, 0))
    assert abi.lib.mx_graph_set_limiters(g._h, pa, 1, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_set_limiters(g._h, None, 1, abi.C.byref(abi.LimiterParams(0.5, 4))) == abi.MX_ERR_INVALID
    c, msg = code(g2, [(pan, 0)])
    with pytest.raises(abi.MxError) as e:
        g2.read_output(pan, 0, 1, True)
    assert c == abi.MX_ERR_INVALID and msg in str(e.value)   # a port the fusion did not materialise
    g.set_limiters([])
    for call in (lambda: g.read_limiters(0, 1), lambda: g.read_limited(0, 0, 1), lambda: g.limited_device_ptr(0)):
        with pytest.raises(abi.MxError):
            call()   # no taps
    g.set_limiters([(ss, 0), (smn, 0)], 0.5, 7)
    for call in (lambda: g.read_limiters(0, 1), lambda: g.read_limited(0, 0, 1)):
        with pytest.raises(abi.MxError):
            call()   # no run since the taps were set
    g.write_source(ss, wide(1, 4 * 1600) * F32(4.0), 4)
    g.run_ticks(0, 3)
    first, y0 = g.read_limiters(0, 3), g.read_limited(0, 0, 3)
    assert code(g, [(ss, 0)], 1.5, 7)[0] == abi.MX_ERR_INVALID   # refused: the set, its records and its copies stay as they were
    assert g.read_limiters(0, 3).tobytes() == first.tobytes() and g.read_limited(0, 0, 3).tobytes() == y0.tobytes()
    for at, cnt in ((0, 4), (3, 1), (2, 2)):
        with pytest.raises(abi.MxError):
            g.read_limiters(at, cnt)   # beyond the last run
        with pytest.raises(abi.MxError):
            g.read_limited(1, at, cnt)
    with pytest.raises(abi.MxError):
        g.read_limited(2, 0, 1)   # tap out of range
    out, cnt = np.zeros(3 * 1600, F32), abi.C.c_size_t(0)
    assert abi.lib.mx_graph_read_limited(g._h, 0, 0, 3, out.ctypes.data, 3 * 1600 - 1, abi.C.byref(cnt)) == abi.MX_ERR_INVALID   # cap too small
    assert cnt.value == 3 * 1600
    assert abi.lib.mx_graph_read_limited(g._h, 0, 0, 3, out.ctypes.data, 3 * 1600, None) == abi.MX_OK and out.tobytes() == y0.tobytes()
    assert abi.lib.mx_graph_read_limited(g._h, 1, 1, 2, None, 0, abi.C.byref(cnt)) == abi.MX_OK and cnt.value == 2 * 800   # the count alone
    rec = np.zeros(6, abi.LIMITER_TICK_DTYPE)
    assert abi.lib.mx_graph_read_limiters(g._h, 0, 3, rec.ctypes.data, 5) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_read_limiters(g._h, 0, 3, rec.ctypes.data, 6) == abi.MX_OK and rec.tobytes() == first.tobytes()


def test_adopt_state_carries_no_taps_and_profile_counts_them_in_the_total_only():
    ws, ss, smn, amp, g = io_graph(48000, 60, 8)
    g.write_source(ss, wide(1, 8 * 1600), 8); g.write_source(smn, wide(2, 8 * 800), 8)
    g.set_limiters([(amp, 0), (ss, 0)], 0.5, 64)
    for r in range(2):
        by_kind, total = g.profile_run(8 * r, 8)
        assert total > 0 and set(by_kind) <= set(abi.KIND_NAMES[:abi.PROFILE_KINDS])
        assert total > sum(by_kind.values())   # the taps' launches are in the total, in no kind
    assert g.read_limiters(0, 8).shape == (8, 2)
    g2 = ws.build(max_ticks_per_run=8)
    g2.adopt_state(g, list(range(len(ws.nodes))))
    g2.write_source(ss, wide(1, 8 * 1600), 8); g2.write_source(smn, wide(2, 8 * 800), 8); g2.run_ticks(16, 8)
    with pytest.raises(abi.MxError):
        g2.read_limiters(0, 1)
