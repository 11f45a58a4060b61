"""Stereo field taps on the device against tests/stereo_model.py, bit for bit (any NaN equals any NaN; every count equal).  The model is fed
what the graph itself wrote on each tapped port (read back with read_output), so what is tested here is the measurement; the ports have
their own parity tests."""
import numpy as np
import pytest

import stereo_model as stm
import synth
from mixlab_amd import abi, ingest, video
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import strips
from test_gpu_spectrum import io_graph, wide
from tick_shapes import by_id, far_first_tick

pytestmark = pytest.mark.gpu


class Tap:
    """one tap and its model; `rate` is the port's (up, down) domain"""

    def __init__(self, node, port, rate=(1, 1)):
        self.node, self.port, self.rate = node, port, rate
        self.model = None

    def port_data(self, g, n_ticks):
        return g.read_output(self.node, self.port, n_ticks, True, rate=self.rate)


def set_taps(g, taps, window=180, grid=0, zoom=0, hop=1):
    g.set_stereo([(t.node, t.port) for t in taps], window, grid, zoom, hop)
    for t in taps:
        t.model = stm.StereoModel(window, grid, zoom, hop)


def check_run(g, taps, n_ticks, what, port_source=None):
    """the last run's records and goniometer emissions of every tap against its model fed the port's samples (read from `port_source`,
    default g); returns (records, emissions)"""
    got = g.read_stereo(0, n_ticks)
    assert got.shape == (n_ticks, len(taps))
    grid = taps[0].model.grid
    got_em = g.read_goniometers() if grid else []
    for i, t in enumerate(taps):
        want, want_em = t.model.run(t.port_data(port_source or g, n_ticks), n_ticks)
        assert stm.records_equal(got[:, i], want), f"{what}: tap {i} ({t.node}, {t.port}): {stm.first_difference(got[:, i], want)}"
        if grid:
            assert len(got_em) == len(want_em), f"{what}: {len(got_em)} emissions, the model has {len(want_em)}"
            for e, (a, b) in enumerate(zip(got_em, want_em)):
                assert stm.gonio_equal(a[i], b), f"{what}: tap {i}, emission {e}: header {[(k, a[i][k], b[k]) for k in b if k != 'gon' and a[i][k] != b[k]]}, " \
                                                 f"{int((a[i]['gon'] != b['gon']).sum())} cells differ"
    return got, got_em


@pytest.mark.parametrize("shape_id", ["44k1", "48k", "44k1_100", "48k_1000", "8k_8000", "5k4"])
def test_stereo_ports_at_several_rates_and_tick_lengths(shape_id):
    shape = by_id(shape_id)
    spt, sr = shape.spt, shape.sample_rate
    n_ticks = 37 if spt > 100 else 150
    ws, ss, smn, amp, g = io_graph(sr, shape.ticks_per_second, n_ticks)
    for window, grid, zoom, hop in ((24, 64, 0, 5), (3, 128, 2, 1), (1024, 0, 0, 0), (1, 128, 8, 1000)):
        taps = [Tap(amp, 0), Tap(ss, 0)]
        set_taps(g, taps, window, grid, zoom, hop)   # every set starts from silence again, c = 0
        for r in range(2):                           # window history, c and the grids carry across runs
            g.write_source(ss, wide(10 * r + 1, n_ticks * 2 * spt), n_ticks)
            g.write_source(smn, wide(10 * r + 2, n_ticks * spt), n_ticks)
            g.run_ticks(r * n_ticks, n_ticks)
            got, em = check_run(g, taps, n_ticks, f"{shape.id} W {window} G {grid} Z {zoom} H {hop} run {r}")
            assert (got["frames"] == spt).all() and not got["nonfinite"].any()
            if grid:
                assert len(em) == ((r + 1) * n_ticks) // hop - (r * n_ticks) // hop
                assert all(int(x["gon"].sum()) == x["frames"] == hop * spt for e in em for x in e)
        assert g.read_stereo(n_ticks - 1, 1).tobytes() == got[n_ticks - 1:].tobytes()   # a window of the last run is the matching slice


@pytest.mark.parametrize("hop", [7, 40, 1])
@pytest.mark.parametrize("sr,spt", [(44100, 735), (48000, 800)])
def test_one_run_one_tick_runs_uneven_runs_and_a_cut_run_agree(sr, spt, hop):
    n = 70
    xs = wide(1, n * 2 * spt)
    records, emissions = [], []
    for cuts in ([n], [1] * n, [3, 1, 33, 2, 30, 1], "cut"):   # hop 7 and 40 straddle run boundaries; 40 is longer than every run of the third
        cut = cuts == "cut"
        if cut:
            cuts = [n]
        assert sum(cuts) == n
        ws, ss, smn, amp, g = io_graph(sr, 60, max(cuts))
        taps = [Tap(amp, 0), Tap(ss, 0)]
        set_taps(g, taps, 40, 64, 1, hop)
        out, ems, at = [], [], 0
        for c in cuts:
            g.write_source(ss, xs[at * 2 * spt:(at + c) * 2 * spt], c)
            if cut:   # the same parameters again: the run is cut into spans at ticks 5 and 41, the samples are what they were
                g.schedule_params(amp, 5, abi.AmplifierParams(1.5, 0.0)); g.schedule_params(amp, 41, abi.AmplifierParams(1.5, 0.0))
            g.run_ticks(at, c)
            rec, em = check_run(g, taps, c, f"{sr} hop {hop} runs {cuts[:3]}.. at {at}")
            out.append(rec)
            ems += [[dict(x, tick_in_run=x["tick_in_run"] + at) for x in e] for e in em]
            at += c
        records.append(np.concatenate(out)); emissions.append(ems)
    for k in (1, 2, 3):
        assert records[0].tobytes() == records[k].tobytes(), k
        assert len(emissions[k]) == len(emissions[0]) == n // hop
        assert all(stm.gonio_equal(a, b) for ea, eb in zip(emissions[0], emissions[k]) for a, b in zip(ea, eb)), k
    assert [e[0]["tick_in_run"] for e in emissions[0]] == list(range(hop - 1, n, hop))
    # a second set resets every tap and c: the same first ticks read as they did from silence
    set_taps(g, taps, 40, 64, 1, hop)
    g.write_source(ss, xs[:4 * 2 * spt], 4); g.run_ticks(n, 4)
    got, _ = check_run(g, taps, 4, "after a second set")
    assert got.tobytes() == records[0][:4].tobytes()


def test_hop_beyond_every_run_emits_when_the_counter_gets_there():
    sr, spt = 48000, 800
    ws, ss, smn, amp, g = io_graph(sr, 60, 4)
    taps = [Tap(ss, 0)]
    set_taps(g, taps, 8, 128, 0, 10)
    counts = []
    for r in range(5):   # ticks 0 .. 19 in runs of 4: emissions at ticks 9 and 19 -- tick 1 of run 2 and tick 3 of run 4
        g.write_source(ss, wide(r, 4 * 2 * spt), 4); g.run_ticks(4 * r, 4)
        _, em = check_run(g, taps, 4, f"run {r}")
        counts.append([e[0]["tick_in_run"] for e in em])
        assert all(e[0]["frames"] == 10 * spt for e in em)
    assert counts == [[], [], [1], [], [3]]


def test_dup_stored_strip_ports_equal_the_unfused_graph():
    sr, n = 48000, 6
    ws, mix, srcs, trigs = strips(8, sr)
    amps = [mix + 6 * (k + 1) for k in range(8)]
    fused, plain = ws.build(max_ticks_per_run=n), ws.build(max_ticks_per_run=n, flags=abi.FLAG_NO_FUSE)
    with pytest.raises(abi.MxError):
        fused.output_device_ptr(amps[0], 0)   # stored one float per frame
    mk = lambda: [Tap(a, 0) for a in amps] + [Tap(mix, 0), Tap(mix, 1)]
    tf, tp = mk(), mk()
    set_taps(fused, tf, 5, 64, 0, 4); set_taps(plain, tp, 5, 64, 0, 4)
    for r, nr in enumerate((n, 1, n)):   # a one-tick run between two longer ones
        for g in (fused, plain):
            for k, tr in enumerate(trigs):
                g.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                g.write_source(s, synth.noise(k + 10 * r, nr * 800) * np.float32(6.0), nr)
            g.run_ticks(r * n, nr)
        a, ea = check_run(fused, tf, nr, f"fused run {r}")
        b, eb = check_run(plain, tp, nr, f"unfused run {r}")
        assert a.tobytes() == b.tobytes(), "a dup-stored port reads as the unfused graph's stereo port"
        assert len(ea) == len(eb) and all(stm.gonio_equal(x, y) for p, q in zip(ea, eb) for x, y in zip(p, q))
        assert a["sum_ll"][:, 0].tobytes() == a["sum_rr"][:, 0].tobytes() == a["sum_lr"][:, 0].tobytes()   # L == R
        for e in ea:   # L == R: everything in column grid / 2
            assert int(e[0]["gon"][:, 32].sum()) == e[0]["frames"]


def test_resample_output_has_its_own_rate():
    sr, n = 44100, 5
    ws = Workspace(sr, 60)
    src = ws.source_stereo()
    rs = ws.resample(160, 147, np.full((160, 4), 0.4))
    ws.connect(src, 0, rs, 0)
    g = ws.build(max_ticks_per_run=n)
    taps = [Tap(rs, 0, rate=(160, 147)), Tap(src, 0)]   # 800 and 735 frames per tick
    set_taps(g, taps, 7, 64, 0, 3)
    for r in range(3):
        g.write_source(src, wide(r, n * 2 * 735), n)
        g.run_ticks(r * n, n)
        got, em = check_run(g, taps, n, f"resampled run {r}")
        assert (got["frames"][:, 0] == 800).all() and (got["frames"][:, 1] == 735).all()
        assert all(e[0]["frames"] == 3 * 800 and e[1]["frames"] == 3 * 735 for e in em)


@pytest.mark.parametrize("mode", ["flag", "auto", "auto-off"])
def test_master_and_cue_in_every_tail_mode_with_the_meters_sums(mode, monkeypatch):
    """Runs go out in pairs: taps on the Master and the Cue go behind the held-back Mixer bank, taps on strips read that run's buffer
    parity.  Meters sit on the same ports: sum_ll and sum_rr are their sum_sq, bit for bit.  The graph without taps gives every port."""
    sr, spt, n, n_runs, n_strips = 48000, 800, 16, 8, 64
    if mode == "auto-off":
        monkeypatch.setenv("MX_OVERLAP_AUTO", "0")
    flags = abi.FLAG_OVERLAP_TAIL if mode == "flag" else 0
    ws, mix, srcs, trigs = strips(n_strips, sr)
    plain = ws.build(max_ticks_per_run=n, flags=flags)    # the same desk without taps
    g = ws.build(max_ticks_per_run=n, flags=flags)
    amps = [mix + 6 * (k + 1) for k in (0, 1, 17, 63)]
    where = [(mix, 0), (amps[0], 0), (mix, 1)] + [(a, 0) for a in amps[1:]]
    taps = [Tap(nd, p) for nd, p in where]
    set_taps(g, taps, 24, 64, 0, 24)   # hop 24 against runs of 16: emissions in runs 1, 2, 4, 5, 7
    g.set_meters(where, abi.MeterParams(2, 0.75))
    noise = [synth.noise(k, n_runs * n * spt) * np.float32(8.0) for k in range(n_strips)]
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
        got, em = check_run(g, taps, n, f"{mode} run {r}", port_source=plain)
        assert len(em) == ((r + 1) * n) // 24 - (r * n) // 24
        m = g.read_meters(0, n)
        assert m["sum_sq"][:, :, 0].tobytes() == got["sum_ll"].tobytes() and m["sum_sq"][:, :, 1].tobytes() == got["sum_rr"].tobytes()
    assert (g.tail_stream() is not None) == (mode != "auto-off")   # the taps do not end the automatic mode
    if mode != "auto-off":
        gated, at_once = g.debug_tail_releases()
        assert gated > 0


def check_all_five_tap_sets_together(first_tick):
    """a mixed audio + video graph without taps, with the four earlier tap sets, and with stereo taps as well: every output is the same in
    all three, the earlier sets' records are the same with and without stereo taps, and the stereo records are the model's"""
    import oracle_video as ov
    from test_gpu_video_scopes import sink_graph
    N, spt, n_fft = 6, 735, 256
    edges = abi.log_band_edges(n_fft, 8, 100.0, 10000.0, 44100.0)
    sizes = [(320, 180), (212, 120), (320, 180)]
    hosts = [ov.HostFrame(w, h).fill(k, seed=21) for k, (w, h) in enumerate(sizes)]
    results = []
    for level in (0, 1, 2):
        ws, srcs, m0, m1, rgba, au, amp, mon = sink_graph()
        g = ws.build(max_ticks_per_run=N)
        dev = [video.DFrame(f.w, f.h).upload(*f.visible()) for f in hosts]
        for s, d in zip(srcs, dev):
            video.graph_set_video_source(g, s, d, dur=(1, 60), off=(0, 1), repeat=True)
        ports = [(amp, 0), (au, 0)]
        if level >= 1:
            g.set_meters(ports, abi.MeterParams(2, 0.75)); g.set_spectra(ports, n_fft, edges); g.set_loudness(ports, 3, 5)
            g.set_video_scopes([(m1, 0), (m0, 0)], wave_cols=64, vectorscope=True, hop=2)
        taps = [Tap(nd, p) for nd, p in ports]
        if level == 2:
            set_taps(g, taps, 4, 128, 1, 4)
        res = {}
        for r in range(2):
            g.write_source(au, synth.noise(9 + r, N * 2 * spt), N)
            g.run_ticks(first_tick + r * N, N)
            res[f"rgba{r}"] = video.graph_rgba_output(g, rgba).copy()
            res[f"audio{r}"] = g.read_output(amp, 0, N, True).copy(); res[f"source{r}"] = g.read_output(au, 0, N, True).copy()
            res[f"mon_audio{r}"] = ingest.graph_read_monitor_audio_i16(g, mon, N, spt).copy()
            for k in range(N):
                _ts, vid = ingest.graph_read_monitor_tick(g, mon, k)
                res[f"mon{r}_{k}"] = np.concatenate([p.ravel() for p in vid[0].download()])
            res[f"prog{r}"] = np.concatenate([p.ravel() for p in video.graph_video_output(g, m1, 0).download()])
            if level >= 1:
                res[f"T meters{r}"] = g.read_meters(0, N).copy(); res[f"T spectra{r}"] = g.read_spectra(0, N).copy()
                res[f"T loudness{r}"] = g.read_loudness(0, N).copy()
                sc = g.read_video_scopes()
                res[f"T scopes{r}"] = np.concatenate([np.concatenate([x["hist"].ravel(), x["wave"].ravel(), x["vec"].ravel(), [x["tick_in_run"]]]) for e in sc for x in e])
            if level == 2:
                _, em = check_run(g, taps, N, f"five sets, run {r}")
                assert [e[0]["tick_in_run"] for e in em] == ([3] if r == 0 else [1, 5])
        results.append(res)
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]) and np.array_equal(results[0][k], results[2][k]), f"{k} differs with taps set"
    for k in results[1]:
        assert results[1][k].tobytes() == results[2][k].tobytes(), f"{k} differs with stereo taps set beside the other four"
    # the desk: every strip's Amplifier, the Master and the Cue
    ws, mix, srcs, trigs = strips(8, 48000)
    ports = [(mix + 6 * (k + 1), 0) for k in range(8)] + [(mix, 0), (mix, 1)]
    outs = []
    for tapped in (False, True):
        g = ws.build(max_ticks_per_run=4)
        if tapped:
            g.set_stereo(ports, 24, 64, 0, 3)
        per_run = []
        for r in range(3):
            for k, s in enumerate(srcs):
                g.write_source(s, synth.noise(k + 5 * r, 4 * 800), 4)
            g.run_ticks(first_tick + 4 * r, 4)
            per_run.append(np.concatenate([g.read_output(nd, p, 4, True) for nd, p in ports]))
        outs.append(np.concatenate(per_run))
    assert outs[0].tobytes() == outs[1].tobytes()


def test_all_five_tap_sets_together_and_no_sample_or_picture_changes():
    check_all_five_tap_sets_together(0)


def test_all_five_tap_sets_together_from_the_2p40_epoch():
    """The same fixed graphs with the clock started at sample time 2^40: the records and the goniometer emissions equal the models' as they
    do from tick 0 (the taps count ticks since they were set, never absolute time), and no sample or picture changes with taps set."""
    check_all_five_tap_sets_together(far_first_tick("at_2p40", 735, 12))


def test_every_audio_tap_set_through_the_end_of_the_automatic_tail_mode():
    """The automatic second-stream mode ends (a stream-ordered consumer takes the Master's raw pointer) while meters, spectrum, loudness,
    stereo and limiter taps are set: every set's descriptors are rebuilt for one stream and one buffer per port, and what the taps carry --
    a hold longer than a run, the spectrum history, the loudness and stereo windows, the goniometer grid and its counter, the limiter's
    look-ahead history and where each limited copy lies -- comes through.  The twin desk without taps, driven identically, gives every port."""
    import test_gpu_limiter as tlim
    import test_gpu_loudness as tl
    import test_gpu_meters as tm
    import test_gpu_spectrum as ts
    sr, spt, n, n_strips, n_fft = 48000, 800, 16, 64, 1024
    edges = abi.log_band_edges(n_fft, 31, 20.0, 20000.0, 48000.0)
    ws, mix, srcs, trigs = strips(n_strips, sr)
    plain = ws.build(max_ticks_per_run=n)    # the same desk without taps
    g = ws.build(max_ticks_per_run=n)
    where = [(mix, 0), (mix, 1), (mix + 6, 0), (mix + 6 * 64, 0)]   # Master, Cue, the Amplifiers of strips 0 and 63
    sets = [(tm, [tm.Tap(nd, p, 2, hold_ticks=40) for nd, p in where]), (ts, [ts.Tap(nd, p, 2, n_fft, edges) for nd, p in where]),
            (tl, [tl.Tap(nd, p, 2, sr, spt) for nd, p in where]), (tlim, [tlim.Tap(nd, p, 2) for nd, p in where])]
    stereo = [Tap(nd, p) for nd, p in where]
    tm.set_taps(g, sets[0][1]); ts.set_taps(g, sets[1][1], n_fft, edges); tl.set_taps(g, sets[2][1]); tlim.set_taps(g, sets[3][1], 0.5, 64)
    set_taps(g, stereo, 24, 64, 0, 24)   # hop 24 against runs of 16: the grid of ticks 48 .. 63 is carried through the mode's end
    noise = [synth.noise(k, 6 * n * spt) * np.float32(8.0) for k in range(n_strips)]
    n_emitted = 0
    for r in range(6):
        if r == 4:   # the mode ends, in both desks
            assert g.tail_stream() is not None and plain.tail_stream() is not None
            g.output_device_ptr(mix, 0); plain.output_device_ptr(mix, 0)
            assert g.tail_stream() is None and plain.tail_stream() is None
        for gr in (plain, g):
            for k, tr in enumerate(trigs):
                gr.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                gr.write_source(s, noise[k][r * n * spt:(r + 1) * n * spt], n)
            gr.run_ticks(r * n, n)
        if r in (0, 2):   # not read: the next run is queued behind it first; the models take the desk's ports from the plain graph
            for t in [t for _, taps in sets for t in taps] + stereo:
                t.model.run(t.port_data(plain, n), n)
            continue
        for nd, p in where:
            want = plain.read_output(nd, p, n, True).view(np.uint32)
            assert np.array_equal(g.read_output(nd, p, n, True).view(np.uint32), want), f"run {r}: taps changed port ({nd}, {p})"
        for mod, taps in sets:
            mod.check_run(g, taps, n, f"{mod.__name__} run {r}", port_source=plain)
        _, em = check_run(g, stereo, n, f"stereo run {r}", port_source=plain)
        assert len(em) == ((r + 1) * n) // 24 - (r * n) // 24
        n_emitted += len(em)
        if r == 1:
            assert g.tail_stream() is not None   # the mode is on: what follows does end it
    assert n_emitted == 3  # runs 1, 4 and 5 (run 2's emission was not read)


def test_non_finite_subnormal_and_large_samples():
    sr, spt, n = 48000, 800, 4
    ws, ss, smn, amp, g = io_graph(sr, 60, n)
    taps = [Tap(ss, 0), Tap(amp, 0)]
    set_taps(g, taps, 2, 128, 8, 2)
    rng = np.random.default_rng(9)
    tiny = np.array([1], np.uint32).view(np.float32)[0]
    xs = (rng.integers(-5000, 5000, n * 2 * spt).astype(np.float32) * tiny).astype(np.float32)   # subnormal samples: a negative one lies in cell -1
    g.write_source(ss, xs, n); g.run_ticks(0, n)
    got, em = check_run(g, taps, n, "subnormal")
    assert got["sum_ll"][:, 0].any() and len(em) == 2 and np.count_nonzero(em[0][0]["gon"]) == 4
    g.write_source(ss, synth.noise(4, n * 2 * spt) * np.float32(3e38), n)   # finite L, R whose sum or difference overflows: the edge cells
    g.run_ticks(n, n)
    got, em = check_run(g, taps, n, "large")
    assert not got["nonfinite"][:, 0].any() and np.isfinite(got["sum_ll"][:, 0]).all() and got["sum_ll"][:, 0].max() > 1e70
    assert all(e[0]["skipped"] == 0 and e[0]["frames"] == 2 * spt for e in em)
    assert got["nonfinite"][:, 1].all()   # the Amplifier's 1.5 x overflows some of them: its port holds Inf
    x = synth.noise(6, n * 2 * spt); x[[5, 2 * spt + 6, 2 * spt + 7]] = np.nan; x[3 * 2 * spt + 100] = np.inf; x[3 * 2 * spt + 301] = -np.inf
    g.write_source(ss, x, n)
    g.run_ticks(2 * n, n)
    got, em = check_run(g, taps, n, "non-finite")
    assert got["nonfinite"][:, 0].tolist() == [1, 1, 0, 2] and [e[0]["skipped"] for e in em] == [2, 2]
    assert np.isnan(got["sum_rr"][0, 0]) and np.isnan(got["win_lr"][1, 0]) and np.isfinite(got["sum_ll"][2, 0])
    # a window is summed afresh: two ticks later the NaN has left it
    g.write_source(ss, synth.noise(8, n * 2 * spt), n); g.run_ticks(3 * n, n)
    got, em = check_run(g, taps, n, "after a NaN")
    assert not np.isfinite(got["win_ll"][0, 0]) and np.isfinite(got["win_ll"][1:, 0]).all() and np.isfinite(got["win_rr"][1:, 0]).all()


def test_refusals():
    ws = Workspace(48000, 60)
    ss, smn = ws.source_stereo(), ws.source_mono()
    vm = ws.video_mixer(a=None, b=None, fader=1.0)
    ws2, mix, srcs, trigs = strips(2, 48000)
    eq, pan = mix + 4, mix + 5
    assert ws2.nodes[eq][0] == abi.KIND_EQ_THREE and ws2.nodes[pan][0] == abi.KIND_STEREO_PANNER
    g = ws.build(max_ticks_per_run=4)
    g2 = ws2.build(max_ticks_per_run=4)

    def code(gr, ports, w=24, grid=64, zoom=0, hop=1):
        pa = (abi.PortRef * len(ports))(*[abi.PortRef(n, p) for n, p in ports])
        rc = abi.lib.mx_graph_set_stereo(gr._h, pa, len(ports), abi.C.byref(abi.StereoParams(w, grid, zoom, hop)))
        return rc, (abi.lib.mx_last_error() or b"").decode()

    assert code(g, [(vm, 0)])[0] == abi.MX_ERR_TYPE
    assert code(g, [(smn, 0)])[0] == abi.MX_ERR_TYPE
    assert code(g, [(len(ws.nodes), 0)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 1)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 0), (ss, 0)])[0] == abi.MX_ERR_INVALID
    for w, grid, zoom, hop in ((0, 64, 0, 1), (1025, 64, 0, 1), (1 << 31, 0, 0, 1), (24, 32, 0, 1), (24, 65, 0, 1), (24, 256, 0, 1), (24, 64, 9, 1),
                               (24, 0, 9, 1), (24, 64, 0, 0), (24, 128, 0, 0)):
        assert code(g, [(ss, 0)], w, grid, zoom, hop)[0] == abi.MX_ERR_INVALID, (w, grid, zoom, hop)
    assert code(g, [(ss, 0)], 1024, 128, 8, 1 << 31)[0] == abi.MX_OK and code(g, [(ss, 0)], 1, 0, 0, 0)[0] == abi.MX_OK   # hop is ignored with grid 0
    pa = (abi.PortRef * 1)(abi.PortRef(ss, 0))
    assert abi.lib.mx_graph_set_stereo(g._h, pa, 1, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_set_stereo(g._h, None, 1, abi.C.byref(abi.StereoParams(24, 64, 0, 1))) == abi.MX_ERR_INVALID
    assert code(g2, [(eq, 0)])[0] == abi.MX_ERR_TYPE        # mono (and not materialised: the type is tested first)
    c, msg = code(g2, [(pan, 0)])
    with pytest.raises(abi.MxError) as e:
        g2.read_output(pan, 0, 1, True)
    assert c == abi.MX_ERR_INVALID and msg in str(e.value)   # a stereo port the fusion did not materialise
    # goniometer records of one run beyond 4 GiB: 70 000 ticks x 65 568 bytes at hop 1; at hop 64 they are 72 MB
    big = Workspace(48000, 48000); bs = big.source_stereo(); gb = big.build(max_ticks_per_run=70000)
    assert code(gb, [(bs, 0)], 24, 128, 0, 1)[0] == abi.MX_ERR_NOMEM
    assert code(gb, [(bs, 0)], 24, 128, 0, 64)[0] == abi.MX_OK
    g.set_stereo([])
    with pytest.raises(abi.MxError):
        g.read_stereo(0, 1)   # no taps
    with pytest.raises(abi.MxError):
        g.read_goniometers()
    g.set_stereo([(ss, 0)], 24, 64, 0, 2)
    with pytest.raises(abi.MxError):
        g.read_stereo(0, 1)   # no run since the taps were set
    with pytest.raises(abi.MxError):
        g.read_goniometers()
    g.write_source(ss, wide(1, 4 * 1600), 4)
    g.run_ticks(0, 3)
    first, first_em = g.read_stereo(0, 3), g.read_goniometers()
    assert len(first_em) == 1 and first_em[0][0]["tick_in_run"] == 1
    assert code(g, [(ss, 0)], 0, 64, 0, 1)[0] == abi.MX_ERR_INVALID   # refused: the set and its records stay as they were
    assert g.read_stereo(0, 3).tobytes() == first.tobytes() and stm.gonio_equal(g.read_goniometers()[0][0], first_em[0][0])
    for at, cnt in ((0, 4), (3, 1), (2, 2)):
        with pytest.raises(abi.MxError):
            g.read_stereo(at, cnt)   # beyond the last run
    out = np.zeros(3, abi.STEREO_TICK_DTYPE)
    assert abi.lib.mx_graph_read_stereo(g._h, 0, 3, out.ctypes.data, 2) == abi.MX_ERR_INVALID   # cap too small
    assert abi.lib.mx_graph_read_stereo(g._h, 0, 3, out.ctypes.data, 3) == abi.MX_OK
    assert out.tobytes() == first.tobytes()
    raw, got = np.zeros(16416, np.uint8), abi.C.c_uint32(7)
    assert abi.lib.mx_graph_read_goniometers(g._h, raw.ctypes.data, 16415, abi.C.byref(got)) == abi.MX_ERR_INVALID   # cap_bytes too small
    assert abi.lib.mx_graph_read_goniometers(g._h, raw.ctypes.data, 16416, abi.C.byref(got)) == abi.MX_OK and got.value == 1
    g.run_ticks(3, 1)   # c = 4: tick 0 of this run emits; then a run that emits nothing reads as 0 records
    assert [e[0]["tick_in_run"] for e in g.read_goniometers()] == [0]
    g.run_ticks(4, 1)
    assert abi.lib.mx_graph_read_goniometers(g._h, None, 0, abi.C.byref(got)) == abi.MX_OK and got.value == 0


def test_grid_0_allocates_and_launches_no_goniometer():
    ws, ss, smn, amp, g = io_graph(48000, 60, 4)
    taps = [Tap(ss, 0), Tap(amp, 0)]
    set_taps(g, taps, 3, 0, 0, 0)
    g.write_source(ss, wide(1, 4 * 1600), 4); g.run_ticks(0, 4)
    check_run(g, taps, 4, "grid 0")
    with pytest.raises(abi.MxError) as e:
        g.read_goniometers()
    assert e.value.code == abi.MX_ERR_INVALID and "grid = 0" in str(e.value)


def test_adopt_state_carries_no_taps_and_profile_counts_them_in_the_total_only():
    ws, ss, smn, amp, g = io_graph(48000, 60, 8)
    g.write_source(ss, wide(1, 8 * 1600), 8); g.write_source(smn, wide(2, 8 * 800), 8)
    g.set_stereo([(amp, 0), (ss, 0)], 24, 64, 0, 4)
    for r in range(2):
        by_kind, total = g.profile_run(8 * r, 8)
        assert total > 0 and set(by_kind) <= set(abi.KIND_NAMES[:abi.PROFILE_KINDS])
        assert total > sum(by_kind.values())   # the taps' launches are in the total, in no kind
    assert g.read_stereo(0, 8).shape == (8, 2) and len(g.read_goniometers()) == 2
    g2 = ws.build(max_ticks_per_run=8)
    g2.adopt_state(g, list(range(len(ws.nodes))))
    g2.write_source(ss, wide(1, 8 * 1600), 8); g2.write_source(smn, wide(2, 8 * 800), 8); g2.run_ticks(16, 8)
    with pytest.raises(abi.MxError):
        g2.read_stereo(0, 1)
