"""MX_KIND_OUTPUT_DEVICE on the device against tests/output_device_model.py, bit for bit: the floats every tick would push into the cpal ring
and the per-tick Clip / Lag records.  The model is fed what the graph itself produced on the node's input port (read back separately), so
what is tested here is the node; the ports upstream have their own parity tests."""
import threading

import numpy as np
import pytest

import synth
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from output_device_model import OutputDeviceModel
from test_gpu_audio_parity import strips
from tick_shapes import SHAPES

pytestmark = pytest.mark.gpu


def odp(channels, left=None, right=None):
    return abi.OutputDeviceParams(channels, -1 if left is None else left, -1 if right is None else right, 0)


def loud_noise(seed, n_ticks, spt):
    """stereo noise, every third tick quiet: clips come and go, so the statuses move"""
    x = synth.noise(seed, n_ticks * 2 * spt).reshape(n_ticks, 2 * spt).astype(np.float32)
    x[::3] *= np.float32(0.25)
    return x.reshape(-1)


def amp_graph(sr, tps, channels, left, right, max_ticks, flags=0):
    ws = Workspace(sr, tps)
    src = ws.source_stereo()
    amp = ws.amplifier(1.5, 0.0)   # gain > 1: clips
    od = ws.output_device(channels, left, right)
    ws.connect(src, 0, amp, 0)
    ws.connect(amp, 0, od, 0)
    return ws, src, amp, od, ws.build(max_ticks_per_run=max_ticks, flags=flags)


def check_run(g, od, model, port_stereo, t0, spt, n_ticks, what, rate=(1, 1)):
    """one run's hand-off and records against the model fed the same input"""
    f = len(port_stereo) // (2 * n_ticks)
    want, recs = model.run(t0, spt, [port_stereo[k * 2 * f:(k + 1) * 2 * f] for k in range(n_ticks)])
    got, ticks = g.read_audio_out(od, 0, n_ticks)
    assert got.size == want.size, f"{what}: {got.size} floats, want {want.size}"
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"{what}: hand-off differs at {np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:5]}"
    mine = [tuple(int(v) for v in t) for t in ticks.tolist()]
    assert mine == recs, f"{what}: records differ at tick {next(k for k in range(n_ticks) if mine[k] != recs[k])}"
    return got, ticks


@pytest.mark.parametrize("shape", SHAPES, ids=[s.id for s in SHAPES])
@pytest.mark.parametrize("channels", [1, 2, 6, 8, 256])
@pytest.mark.parametrize("n_ticks", [1, 7])
def test_hand_off_and_records_at_every_tick_shape(shape, channels, n_ticks):
    sr, spt = shape.sample_rate, shape.spt
    left, right = (0, 0) if channels == 1 else (channels - 1, channels // 2)
    ws, src, amp, od, g = amp_graph(sr, shape.ticks_per_second, channels, left, right, n_ticks)
    model = OutputDeviceModel(sr, channels, left, right)
    for r in range(3):   # state carried across runs
        x = loud_noise(7 * r + channels, n_ticks, spt)
        g.write_source(src, x, n_ticks)
        g.run_ticks(r * n_ticks, n_ticks)
        check_run(g, od, model, g.read_output(amp, 0, n_ticks, True), r * n_ticks * spt, spt, n_ticks, f"run {r}")


@pytest.mark.parametrize("sr,tps,channels,n_ticks", [pytest.param(sr, 60, c, n, id=f"{c}-{n}-{sr}") for (c, n) in ((2, 64), (8, 64), (256, 64), (2, 2048))
                                                      for sr in (44100, 48000)]
                         + [pytest.param(8000, 8000, c, 5000, id=f"{c}-5000-8k_8000") for c in (2, 256)])
def test_long_submissions(sr, tps, channels, n_ticks):
    spt = sr // tps
    ws, src, amp, od, g = amp_graph(sr, tps, channels, 1, 0, n_ticks)
    model = OutputDeviceModel(sr, channels, 1, 0)
    for r in range(2):
        x = loud_noise(r, n_ticks, spt)
        if n_ticks > 2048:   # quiet but for ticks [1000, 1200): at 8000 ticks/s Clip goes None -> Active -> Recent inside the run
            x[:1000 * 2 * spt] *= np.float32(0.01)
            x[1200 * 2 * spt:] *= np.float32(0.01)
        g.write_source(src, x, n_ticks)
        g.run_ticks(r * n_ticks, n_ticks)
        got, ticks = check_run(g, od, model, g.read_output(amp, 0, n_ticks, True), r * n_ticks * spt, spt, n_ticks, f"run {r}")
        if n_ticks > 2048 and r == 0:
            assert set(ticks["clip_status"].tolist()) == {0, 1, 2}
    # a window of the last run is the matching slice of the whole
    whole, wt = g.read_audio_out(od, 0, n_ticks)
    part, pt = g.read_audio_out(od, 5, 9)
    per = spt * channels
    assert np.array_equal(part, whole[5 * per:14 * per]) and np.array_equal(pt, wt[5:14])


def test_scheduled_updates_state_across_runs_and_adopt_state():
    sr, spt, n = 48000, 800, 16
    ws, src, amp, od, g = amp_graph(sr, 60, 2, 0, 1, n)
    model = OutputDeviceModel(sr, 2, 0, 1)
    events = [(3, (2, 1, 0)), (5, (2, 1, 9)), (6, (2, 1, 9)), (8, (0, 0, 1)), (10, (6, 4, 5)), (12, (6, 4, 5)), (13, (4, 3, None))]
    t = 0
    for r in range(2):
        x = loud_noise(40 + r, n, spt)
        g.write_source(src, x, n)
        for tick, p in events:
            g.schedule_params(od, tick, odp(*p))
        g.run_ticks(r * n, n)
        port = g.read_output(amp, 0, n, True)
        want, recs = [], []
        for k in range(n):
            for tick, p in events:
                if tick == k:
                    model.update(*p)
            w, rec = model.run_tick(t, port[k * 2 * spt:(k + 1) * 2 * spt])
            want.append(w); recs.append(rec); t += spt
        got, ticks = g.read_audio_out(od, 0, n)
        want = np.concatenate(want)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"run {r}"
        assert [tuple(int(v) for v in q) for q in ticks.tolist()] == recs, f"run {r}"
        if r == 0:
            assert [int(q) for q in ticks["channels"]] == [2] * 8 + [0] * 2 + [6] * 3 + [4] * 3
        events = [(0, (2, 0, 1)), (4, (8, 7, 6))]
    # a topology edit: the module persists (scratch, times, statuses, a pending lag note)
    g.audio_out_lag(od)
    model.note_lag()
    g2 = ws.build(max_ticks_per_run=n)
    g2.adopt_state(g, list(range(len(ws.nodes))))
    g.close()
    x = loud_noise(50, n, spt)
    g2.write_source(src, x, n)
    g2.run_ticks(2 * n, n)
    check_run(g2, od, model, g2.read_output(amp, 0, n, True), 2 * n * spt, spt, n, "after adopt_state")


def test_lag_notes_between_runs_and_from_another_thread():
    sr, spt, n = 44100, 735, 8
    ws, src, amp, od, g = amp_graph(sr, 60, 2, 0, 1, n)
    model = OutputDeviceModel(sr, 2, 0, 1)
    quiet = np.zeros(n * 2 * spt, np.float32)
    g.write_source(src, quiet, n)
    for r in range(4):
        if r in (1, 2):
            g.audio_out_lag(od); g.audio_out_lag(od)   # two notes before one run: one event
            model.note_lag()
        g.run_ticks(r * n, n)
        check_run(g, od, model, quiet, r * n * spt, spt, n, f"run {r}")
    # a note from the callback thread while a run is being queued: that run or the next one takes it, exactly once
    before = model.__dict__.copy()
    done = threading.Event()
    th = threading.Thread(target=lambda: (g.audio_out_lag(od), done.set()))
    th.start()
    g.run_ticks(4 * n, n)
    th.join(); assert done.is_set()
    a = g.read_audio_out(od, 0, n)[1]
    g.run_ticks(5 * n, n)
    b = g.read_audio_out(od, 0, n)[1]
    got = [tuple(int(v) for v in q) for q in a.tolist()] + [tuple(int(v) for v in q) for q in b.tolist()]
    outcomes = []
    for first in (True, False):
        m = OutputDeviceModel(sr, 2, 0, 1); m.__dict__.update({k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in before.items()})
        if first:
            m.note_lag()
        recs = m.run(4 * n * spt, spt, [quiet[:2 * spt]] * n)[1]
        if not first:
            m.note_lag()
        recs += m.run(5 * n * spt, spt, [quiet[:2 * spt]] * n)[1]
        outcomes.append(recs)
    assert got in outcomes


def test_disconnected_dup_stored_and_resampled_inputs():
    sr, spt, n = 44100, 735, 6
    # Disconnected: reads the stereo zero buffer (io.rs:45-47)
    ws = Workspace(sr, 60)
    od = ws.output_device(3, 2, 0)
    g = ws.build(max_ticks_per_run=n)
    model = OutputDeviceModel(sr, 3, 2, 0)
    g.run_ticks(0, n)
    check_run(g, od, model, np.zeros(n * 2 * spt, np.float32), 0, spt, n, "disconnected")
    # a strip's Amplifier read by the Mixer and the OutputDevice only: stored one float per frame, expanded by the node
    ws, mix, srcs, trigs = strips(4, sr)
    amp0 = mix + 6
    assert ws.nodes[amp0][0] == abi.KIND_AMPLIFIER
    od = ws.output_device(4, 3, 1)
    ws.connect(amp0, 0, od, 0)
    g = ws.build(max_ticks_per_run=n)
    with pytest.raises(abi.MxError):
        g.output_device_ptr(amp0, 0)   # stored one float per frame (no public pointer)
    model = OutputDeviceModel(sr, 4, 3, 1)
    for r in range(2):
        for k, s in enumerate(srcs):
            g.write_source(s, synth.noise(k + 10 * r, n * spt) * np.float32(4.0), n)
        for tr in trigs:
            g.update_params(tr, abi.TriggerParams(1))
        g.run_ticks(r * n, n)
        check_run(g, od, model, g.read_output(amp0, 0, n, True), r * n * spt, spt, n, f"dup-stored run {r}")
    # behind a 44.1 -> 48 kHz Resample: 800 frames per tick of the port's own domain, the clock stays the graph's
    ws = Workspace(sr, 60)
    src = ws.source_stereo()
    rs = ws.resample(160, 147, np.full((160, 4), 0.4))
    od = ws.output_device(2, 1, 0)
    ws.connect(src, 0, rs, 0); ws.connect(rs, 0, od, 0)
    g = ws.build(max_ticks_per_run=n)
    model = OutputDeviceModel(sr, 2, 1, 0)
    for r in range(2):
        g.write_source(src, loud_noise(r, n, spt), n)
        g.run_ticks(r * n, n)
        port = g.read_output(rs, 0, n, True, rate=(160, 147))
        assert port.size == n * 2 * 800
        check_run(g, od, model, port, r * n * spt, spt, n, f"resampled run {r}")


@pytest.mark.parametrize("mode", ["flag", "auto", "auto-off"])
def test_master_of_an_overlapped_graph_in_every_tail_mode(mode, monkeypatch):
    """Runs go out in pairs: the node behind run k's Master is held back with the Mixer bank until run k + 1 is queued"""
    sr, spt, n, n_runs, n_strips = 48000, 800, 16, 4, 64
    if mode == "auto-off":
        monkeypatch.setenv("MX_OVERLAP_AUTO", "0")
    flags = abi.FLAG_OVERLAP_TAIL if mode == "flag" else 0
    ws, mix, srcs, trigs = strips(n_strips, sr)
    plain = ws.build(max_ticks_per_run=n, flags=flags)   # the same desk without the node
    od = ws.output_device(2, 0, 1)
    ws.connect(mix, 0, od, 0)
    g = ws.build(max_ticks_per_run=n, flags=flags)
    model = OutputDeviceModel(sr, 2, 0, 1)
    noise = [synth.noise(k, n_runs * n * spt) * np.float32(8.0) for k in range(n_strips)]
    for r in range(n_runs):
        for gr in (plain, g):
            for k, tr in enumerate(trigs):
                gr.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                gr.write_source(s, noise[k][r * n * spt:(r + 1) * n * spt], n)
        plain.run_ticks(r * n, n)
        pm, pc = plain.read_output(mix, 0, n, True), plain.read_output(mix, 1, n, True)
        if r == 2:
            g.audio_out_lag(od); model.note_lag()
        g.run_ticks(r * n, n)
        if r % 2 == 0:   # not read: the next run is queued behind it first
            model.run(r * n * spt, spt, [pm[k * 2 * spt:(k + 1) * 2 * spt] for k in range(n)])
            continue
        master = g.read_output(mix, 0, n, True)
        assert np.array_equal(master.view(np.uint32), pm.view(np.uint32)), "the node changed the Master"
        assert np.array_equal(g.read_output(mix, 1, n, True).view(np.uint32), pc.view(np.uint32)), "the node changed the Cue"
        check_run(g, od, model, master, r * n * spt, spt, n, f"{mode} run {r}")
    assert (g.tail_stream() is not None) == (mode != "auto-off")   # the node does not end the automatic mode
    if mode != "auto-off":
        gated, at_once = g.debug_tail_releases()
        assert gated > 0


def test_invalid_windows_and_params_are_refused():
    ws, src, amp, od, g = amp_graph(48000, 60, 2, 0, 1, 4)
    g.run_ticks(0, 4)
    for first, n in ((0, 5), (4, 1), (3, 2)):
        with pytest.raises(abi.MxError) as e:
            g.read_audio_out(od, first, n)
        assert e.value.code == abi.MX_ERR_INVALID
    with pytest.raises(abi.MxError) as e:
        g.read_audio_out(amp, 0, 1)
    assert e.value.code == abi.MX_ERR_INVALID
    for bad in (odp(257, 0, 1), abi.OutputDeviceParams(2, -2, 0, 0), abi.OutputDeviceParams(2, 0, -7, 0)):
        with pytest.raises(abi.MxError) as e:
            g.update_params(od, bad)
        assert e.value.code == abi.MX_ERR_INVALID
        with pytest.raises(abi.MxError) as e:
            g.schedule_params(od, 1, bad)
        assert e.value.code == abi.MX_ERR_INVALID
        ws2 = Workspace(48000, 60)
        ws2.add(abi.KIND_OUTPUT_DEVICE, bad)
        with pytest.raises(abi.MxError) as e:
            ws2.build()
        assert e.value.code == abi.MX_ERR_INVALID
    g.update_params(od, odp(256, 255, 0))   # the limits themselves are accepted
    g.run_ticks(4, 4)
    assert g.read_audio_out(od, 0, 4)[0].size == 4 * 800 * 256


def _stale(got, ticks, spt, channel):
    """the samples a tick's hand-off holds at `channel` of every frame, tick by tick (channel count from the records)"""
    out, off = [], 0
    for c in ticks["channels"].tolist():
        out.append(got[off:off + spt * c][channel::c] if c > channel else np.zeros(0, np.float32))
        off += spt * c
    return out


def test_persistent_scratch_across_channel_changes_runs_and_adopt_state():
    """Channel counts change while the assignment stays: nothing is zeroed, so every unassigned position of the hand-off shows what an
    earlier, narrower or wider layout left in the scratch (output_device.rs:184-210) -- within a run (spans), across runs, through
    growth beyond any earlier count and through a topology edit."""
    sr, spt, n = 48000, 800, 12
    ws, src, amp, od, g = amp_graph(sr, 60, 2, 0, 1, n)
    model = OutputDeviceModel(sr, 2, 0, 1)
    t = 0

    def run(graph, sched, before=None, seed=0):
        nonlocal t
        x = loud_noise(60 + seed, n, spt)
        graph.write_source(src, x, n)
        if before is not None:
            graph.update_params(od, odp(*before)); model.update(*before)
        for tick, p in sched:
            graph.schedule_params(od, tick, odp(*p))
        graph.run_ticks(t // spt, n)
        port = graph.read_output(amp, 0, n, True)
        want, recs = [], []
        for k in range(n):
            for tick, p in sched:
                if tick == k:
                    model.update(*p)
            w, rec = model.run_tick(t, port[k * 2 * spt:(k + 1) * 2 * spt])
            want.append(w); recs.append(rec); t += spt
        got, ticks = graph.read_audio_out(od, 0, n)
        want = np.concatenate(want)
        assert got.size == want.size and np.array_equal(got.view(np.uint32), want.view(np.uint32)), f"hand-off of run at t {t}"
        assert [tuple(int(v) for v in q) for q in ticks.tolist()] == recs
        return got, ticks

    # within one run: 2 -> 4 -> 2 -> 4 channels at ticks 3, 6, 9, same assignment
    got, ticks = run(g, [(3, (4, 0, 1)), (6, (2, 0, 1)), (9, (4, 0, 1))])
    st = _stale(got, ticks, spt, 2)
    assert np.any(st[3] != 0) and np.any(st[9] != 0)       # channel 2 of a 4-channel tick: frame-1 samples of the 2-channel layout
    # across runs: back to 2, then 6 (beyond any earlier count, by an update between runs) and 8 (by a schedule inside a run)
    run(g, [(4, (2, 0, 1))], seed=1)
    got, ticks = run(g, [(5, (8, 0, 1))], before=(6, 0, 1), seed=2)
    assert all(np.any(s != 0) for s in _stale(got, ticks, spt, 3))
    # a topology edit carries the scratch; then more channels than the old graph ever had, same assignment
    g2 = ws.build(max_ticks_per_run=n)
    g2.adopt_state(g, list(range(len(ws.nodes))))
    g.close()
    got, ticks = run(g2, [(2, (4, 0, 1)), (7, (12, 0, 1))], seed=3)
    assert np.any(_stale(got, ticks, spt, 5)[7] != 0)


def test_a_tick_count_that_goes_back_reads_as_the_model_does():
    """The node assumes a forward-moving clock (mixlab_gpu.h); a host that restarts its tick count behind a recorded clip sees a negative
    distance, Active until the clock has passed the clip by 100 ms -- the same as the numpy model's arithmetic"""
    sr, spt, n = 44100, 735, 8
    ws, src, amp, od, g = amp_graph(sr, 60, 2, 0, 1, n)
    model = OutputDeviceModel(sr, 2, 0, 1)
    for first in (1000, 0, 3):
        x = loud_noise(first, n, spt) * np.float32(1.0 if first == 1000 else 0.1)   # clips at 1000 only
        g.write_source(src, x, n)
        g.run_ticks(first, n)
        check_run(g, od, model, g.read_output(amp, 0, n, True), first * spt, spt, n, f"first tick {first}")


@pytest.mark.parametrize("with_video", [False, True])
def test_profiled_runs_account_the_node(with_video):
    """performance_info gives the node its launches' time; with a video section on the same stream the node goes after it, and every
    account stays inside the tick"""
    ws = Workspace(48000, 60)
    src = ws.source_stereo(); amp = ws.amplifier(1.5, 0.0); od = ws.output_device(6, 0, 1)
    ws.connect(src, 0, amp, 0); ws.connect(amp, 0, od, 0)
    if with_video:
        ws.video_mixer(a=None, b=None, fader=1.0)
    g = ws.build(max_ticks_per_run=8)
    g.write_source(src, loud_noise(1, 8, 800), 8)
    for r in range(2):
        by_kind, total = g.profile_run(8 * r, 8)
        info, us = g.performance_info(len(ws.nodes))
        tick_us = total * 1000.0 / 8
        assert total > 0 and 0 < us[od] <= tick_us + 1
        assert abs(sum(us) + info.engine_us - tick_us) <= len(ws.nodes) + 2
