"""Video scope taps on the device (mx_video_scope, mx_graph_set_video_scopes / mx_graph_read_video_scopes) against the numpy model of the
header's text (tests/video_scope_model.py).  Every comparison is ==: the records are integer counts."""
import ctypes as C

import numpy as np
import pytest

import oracle_video as ov
import synth
import video_scope_model as vm
from mixlab_amd import abi, ingest, video
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu

SIZES = [(64, 36), (1000, 562), (1280, 720), (1918, 1078), (1920, 1080)]
PATTERNS = ["blank", "noise", "ramp", "all255", "checker", "yuva"]


def picture(pattern, w, h):
    pw, ph = w >> 1, h >> 1
    rng = np.random.default_rng(w * 7 + h)
    if pattern == "blank":
        return vm.blank(w, h)
    if pattern in ("noise", "yuva"):
        return tuple(rng.integers(0, 256, s, dtype=np.uint8) for s in ((h, w), (ph, pw), (ph, pw)))
    if pattern == "ramp":
        return vm.ramp(w, h)
    if pattern == "all255":
        return tuple(np.full(s, 255, np.uint8) for s in ((h, w), (ph, pw), (ph, pw)))
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx = np.mgrid[0:ph, 0:pw]
    return (np.where((xx + yy) & 1, 235, 16).astype(np.uint8), np.where((cx // 3 + cy) & 1, 240, 16).astype(np.uint8),
            np.where((cx + cy // 2) & 1, 17, 239).astype(np.uint8))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_frame_against_the_model(size, pattern):
    w, h = size
    y, u, v = picture(pattern, w, h)
    fmt = video.PIXFMT_YUVA420P if pattern == "yuva" else video.PIXFMT_YUV420P
    d = video.DFrame(w, h, fmt=fmt).upload(y, u, v)
    if pattern == "yuva":   # the coverage plane is ignored: fill it with something that would show
        d.upload_alpha(np.random.default_rng(1).integers(0, 256, (h, w), dtype=np.uint8))
    for cols in vm.WAVE_COLS:
        for vec in (False, True):
            got = video.scope(d, cols, vec)
            want = vm.record((fmt, w, h, (y, u, v)), 0, cols, vec)
            assert vm.same(got, want), f"wave_cols {cols} vectorscope {vec}: {vm.first_difference(got, want)}"
    if pattern == "blank":   # the closed form, straight from the device
        got = video.scope(d, 256, True)
        assert got["hist"][0][0] == w * h and got["hist"][1][128] == got["hist"][2][128] == got["vec"][64][64] == (w >> 1) * (h >> 1)


def test_a_fresh_device_frame_is_the_blank_frame_and_a_record_buffer_is_reused():
    d = video.DFrame(322, 182)            # mx_dframe_create: Y = 0, U = V = 0x80, nothing uploaded
    buf = video.DeviceBuffer(abi.video_scope_record_bytes(128, True))
    want = vm.record((0, 322, 182, vm.blank(322, 182)), 0, 128, True)
    for _ in range(3):                    # the record starts from zero every call, whatever the buffer held
        video.scope(d, 128, True, out=buf, download=False)
        got = abi.parse_video_scope_records(buf.download(), 128, True)[0]
        assert vm.same(got, want), vm.first_difference(got, want)


@pytest.mark.parametrize("fmt,bpp", [(video.PIXFMT_RGB24, 3), (video.PIXFMT_BGRA, 4)])
def test_a_packed_rgb_frame_is_present_but_not_counted(fmt, bpp):
    pix = np.random.default_rng(3).integers(0, 256, (36, 64, bpp), dtype=np.uint8)
    d = video.DFrame(64, 36, fmt=fmt).upload_packed(pix)
    got = video.scope(d, 64, True)
    want = vm.record((fmt, 64, 36, None), 0, 64, True)
    assert got["counted"] == 0 and got["present"] == 1 and vm.same(got, want), vm.first_difference(got, want)
    d2 = video.DFrame(64, 36, fmt=video.PIXFMT_NV12)
    got = video.scope(d2, 0, False)
    assert (got["present"], got["counted"], got["pixfmt"], got["width"], got["height"]) == (1, 0, video.PIXFMT_NV12, 64, 36) and not got["hist"].any()


# ---- graph taps ----
SR, SPT, T = 44100, 735, 40
LAYERS = [((320, 180), 0), ((212, 120), 0), ((160, 120), 2)]   # layer 2 is yuv444p: the B output of the last mixer is a clone of it -- present, not counted


def tapped_cascade():
    """three sources -> two VideoMixers in cascade -> RGBA sink (so both program outputs are symbolic chains until something needs pixels)"""
    ws = Workspace(SR, 60)
    srcs = [ws.source_video() for _ in LAYERS]
    m0 = ws.video_mixer(a=0, b=1, fader=0.25)
    ws.connect(srcs[0], 0, m0, 0); ws.connect(srcs[1], 0, m0, 1)
    m1 = ws.video_mixer(a=0, b=1, fader=0.6)
    ws.connect(m0, 0, m1, 0); ws.connect(srcs[2], 0, m1, 1)
    rgba = ws.video_to_rgba(None)
    ws.connect(m1, 0, rgba, 0)
    return ws, srcs, m0, m1, rgba


def host_frame(hf):
    fmt = {0: vm.PIXFMT_YUV420P}.get(hf.fmt, hf.fmt)
    return (fmt, hf.w, hf.h, tuple(hf.visible()) if hf.fmt == 0 else None)


FADER_MOVES = {7: 0.9, 19: 0.0, 20: 1.0, 33: 0.4}          # tick -> m1's fader from that tick on (scheduled updates: the run is cut there)
LAYER1_TICKS = [0, 1, 5, 6, 7, 8, 20, 21, 22, 30, 39]       # the ticks source 1 delivers a frame on; it lives two ticks


@pytest.mark.parametrize("hop", [1, 3, 64])
@pytest.mark.parametrize("cols,vec", [(256, True), (64, False)])
def test_taps_in_a_mixer_cascade_follow_the_oracle_tick_by_tick(hop, cols, vec):
    ws, srcs, m0, m1, rgba = tapped_cascade()
    g = ws.build(max_ticks_per_run=T)
    taps = [(m1, 0), (m1, 1), (m1, 2), (srcs[1], 0), (m0, 0), (srcs[2], 0)]
    g.set_video_scopes(taps, wave_cols=cols, vectorscope=vec, hop=hop)
    hosts = [[ov.HostFrame(w, h, fmt).fill(k + 3 * j, seed=11 + j) for j in range(3)] for k, ((w, h), fmt) in enumerate(LAYERS)]
    dev = [[video.DFrame(f.w, f.h, fmt=f.fmt).upload(*f.visible()) for f in fs] for fs in hosts]
    video.graph_set_video_source_ring(g, srcs[0], dev[0], dur=(1, 60), off=(0, 1))     # a new picture every tick
    video.graph_set_video_source_ring(g, srcs[2], dev[2], dur=(1, 60), off=(0, 1))
    for t in LAYER1_TICKS:
        ingest.graph_queue_video_source(g, srcs[1], t, dev[1][t % 3], dur=(2, 60), off=(0, 1))
    for t, f in FADER_MOVES.items():
        g.schedule_params(m1, t, video.VideoMixerParams(0, 1, f))
    g.run_ticks(0, T)
    got = g.read_video_scopes()
    # the oracle, tick by tick
    o0, o1 = ov.OracleVideoMixer(a=0, b=1, fader=0.25), ov.OracleVideoMixer(a=0, b=1, fader=0.6)
    want, n_absent, n_uncounted = [], 0, 0
    for t in range(T):
        if t in FADER_MOVES:
            o1.update(a=0, b=1, fader=FADER_MOVES[t])
        l0, l2 = hosts[0][t % 3], hosts[2][t % 3]
        l1 = hosts[1][t % 3] if t in LAYER1_TICKS else None
        p0 = o0.run_tick(t * SPT, [(l0, (1, 60), (0, 1)), (l1, (2, 60), (0, 1)) if l1 else None, None, None])
        p1 = o1.run_tick(t * SPT, [(p0, (1, 60), (0, 1)), (l2, (1, 60), (0, 1)), None, None])
        if t % hop:
            continue
        frames = [host_frame(p1), host_frame(p0), host_frame(l2), host_frame(l1) if l1 else None, host_frame(p0), host_frame(l2)]
        n_absent += frames[3] is None
        n_uncounted += 2
        want.append([vm.record(f, t, cols, vec) for f in frames])
    assert len(got) == len(want) == -(-T // hop)
    for rg, rw in zip(got, want):
        assert len(rg) == len(taps)
        for k, (a, b) in enumerate(zip(rg, rw)):
            assert vm.same(a, b), f"hop {hop} tick {b['tick_in_run']} tap {k}: {vm.first_difference(a, b)}"
    if hop == 1:
        assert n_absent > 10 and n_uncounted > 10          # both special record kinds were exercised
    # the pictures themselves are the oracle's (the tap materialised symbolic frames: same bytes)
    prog = video.graph_video_output(g, m1, 0)
    for p, (a, b) in enumerate(zip(prog.download(), p1.visible())):
        assert np.array_equal(a, b), f"plane {p} of the composite"
    assert np.array_equal(video.graph_rgba_output(g, rgba), ov.to_rgba(p1, None))
    if hop == 64:   # longer than the run: the next run records nothing until c comes round (c = 40 .. 79: tick 24 of the run is c = 64)
        g.run_ticks(T, T)
        nxt = g.read_video_scopes()
        assert len(nxt) == 1 and nxt[0][0]["tick_in_run"] == 24 and nxt[0][0]["present"] == 1
        g.run_ticks(2 * T, 20)                              # c = 80 .. 99: nothing
        assert g.read_video_scopes() == []


def test_the_hop_counter_is_carried_across_runs_and_reset_by_a_new_set():
    ws = Workspace(SR, 60)
    s = ws.source_video(); m = ws.video_mixer(a=0, b=None, fader=1.0)
    ws.connect(s, 0, m, 0)
    g = ws.build(max_ticks_per_run=8)
    hf = ov.HostFrame(64, 48).fill(1, seed=2)
    d = video.DFrame(64, 48).upload(*hf.visible())
    video.graph_set_video_source(g, s, d, dur=(1, 60), off=(0, 1), repeat=True)
    g.set_video_scopes([(m, 0)], wave_cols=64, vectorscope=True, hop=3)
    want = vm.record((0, 64, 48, tuple(hf.visible())), 0, 64, True)
    ticks = lambda: [r[0]["tick_in_run"] for r in g.read_video_scopes()]
    g.run_ticks(0, 5); assert ticks() == [0, 3]             # c = 0 .. 4
    g.run_ticks(5, 5); assert ticks() == [1, 4]             # c = 5 .. 9: 6 and 9
    g.run_ticks(10, 1); assert ticks() == []                # c = 10
    g.run_ticks(11, 8); assert ticks() == [1, 4, 7]         # c = 11 .. 18: 12, 15, 18
    for r in g.read_video_scopes():
        assert vm.same(r[0], {**want, "tick_in_run": r[0]["tick_in_run"]})
    g.set_video_scopes([(m, 0), (s, 0)], wave_cols=0, vectorscope=False, hop=3)   # a new set: c = 0 again
    with pytest.raises(abi.MxError) as ei:
        g.read_video_scopes()                               # no run since the taps were set
    assert ei.value.code == abi.MX_ERR_INVALID
    g.run_ticks(19, 4)
    recs = g.read_video_scopes()
    assert [r[0]["tick_in_run"] for r in recs] == [0, 3] and all(len(r) == 2 for r in recs)
    w0 = vm.record((0, 64, 48, tuple(hf.visible())), 3, 0, False)
    assert vm.same(recs[1][0], w0) and vm.same(recs[1][1], w0)
    g.set_video_scopes([])
    g.run_ticks(23, 2)
    with pytest.raises(abi.MxError):
        g.read_video_scopes()


def sink_graph():
    ws = Workspace(SR, 60)
    srcs = [ws.source_video() for _ in range(3)]
    m0 = ws.video_mixer(a=0, b=1, fader=0.3); ws.connect(srcs[0], 0, m0, 0); ws.connect(srcs[1], 0, m0, 1)
    m1 = ws.video_mixer(a=0, b=1, fader=0.7); ws.connect(m0, 0, m1, 0); ws.connect(srcs[2], 0, m1, 1)
    rgba = ws.video_to_rgba([3900, 150, 46, 4096, 60, 3980, 56, -2048, 20, 120, 3956, 0]); ws.connect(m1, 0, rgba, 0)
    au = ws.source_stereo(); amp = ws.amplifier(0.8, 0.0); ws.connect(au, 0, amp, 0)
    mon = ws.monitor(160, 100); ws.connect(m1, 0, mon, 0); ws.connect(amp, 0, mon, 1)
    return ws, srcs, m0, m1, rgba, au, amp, mon


def test_taps_change_no_picture_and_no_sample():
    """the same mixed audio + video graph with and without taps: RGBA sink, Monitor pictures, the downloaded composite and the audio ports"""
    N = 6
    sizes = [(320, 180), (212, 120), (320, 180)]
    hosts = [ov.HostFrame(w, h).fill(k, seed=21) for k, (w, h) in enumerate(sizes)]
    audio = synth.noise(9, N * 2 * SPT)
    results = []
    for tapped in (False, True):
        ws, srcs, m0, m1, rgba, au, amp, mon = sink_graph()
        g = ws.build(max_ticks_per_run=N)
        dev = [video.DFrame(f.w, f.h).upload(*f.visible()) for f in hosts]
        for s, d in zip(srcs, dev):
            video.graph_set_video_source(g, s, d, dur=(1, 60), off=(0, 1), repeat=True)
        if tapped:
            g.set_video_scopes([(m1, 0), (m0, 0), (srcs[1], 0), (m1, 2)], wave_cols=128, vectorscope=True, hop=2)
        g.write_source(au, audio, N)
        g.run_ticks(0, N)
        res = {"rgba": video.graph_rgba_output(g, rgba).copy(), "audio": g.read_output(amp, 0, N, True).copy(),
               "mon_audio": ingest.graph_read_monitor_audio_i16(g, mon, N, SPT).copy()}
        for k in range(N):
            _ts, vid = ingest.graph_read_monitor_tick(g, mon, k)
            res[f"mon{k}"] = np.concatenate([p.ravel() for p in vid[0].download()])
        res["prog"] = np.concatenate([p.ravel() for p in video.graph_video_output(g, m1, 0).download()])
        if tapped:
            recs = g.read_video_scopes()
            assert [r[0]["tick_in_run"] for r in recs] == [0, 2, 4] and all(x["counted"] == 1 for r in recs for x in r)
            assert all(int(r[0]["hist"][0].sum()) == 320 * 180 for r in recs)
        results.append(res)
    assert results[0].keys() == results[1].keys()
    for k in results[0]:
        assert np.array_equal(results[0][k], results[1][k]), f"{k} differs with taps set"


def test_every_error_path():
    ws, srcs, m0, m1, rgba, au, amp, mon = sink_graph()
    g = ws.build(max_ticks_per_run=2048)
    P = abi.VideoScopeParams

    def set_raw(ports, params, n=None):
        pa = (abi.PortRef * max(1, len(ports)))(*[abi.PortRef(a, b) for a, b in ports])
        return abi.lib.mx_graph_set_video_scopes(g._h, pa, len(ports) if n is None else n, C.byref(params) if params is not None else None)

    ok = P(64, 1, 1)
    assert set_raw([(amp, 0)], ok) == abi.MX_ERR_TYPE                      # an audio port
    assert set_raw([(au, 0)], ok) == abi.MX_ERR_TYPE
    assert set_raw([(999, 0)], ok) == abi.MX_ERR_INVALID                   # node out of range
    assert set_raw([(m1, 3)], ok) == abi.MX_ERR_INVALID                    # port out of range
    assert set_raw([(rgba, 0)], ok) == abi.MX_ERR_INVALID                  # a sink has no output port
    assert set_raw([(m1, 0), (m0, 0), (m1, 0)], ok) == abi.MX_ERR_INVALID  # duplicate
    for bad in (1, 32, 100, 512):
        assert set_raw([(m1, 0)], P(bad, 0, 1)) == abi.MX_ERR_INVALID      # wave_cols outside the list
    assert set_raw([(m1, 0)], P(64, 0, 0)) == abi.MX_ERR_INVALID           # hop = 0
    assert b"hop" in abi.lib.mx_last_error()
    assert set_raw([(m1, 0)], None) == abi.MX_ERR_INVALID                  # params NULL with taps
    assert abi.lib.mx_graph_set_video_scopes(g._h, None, 1, C.byref(ok)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_set_video_scopes(None, None, 0, None) == abi.MX_ERR_INVALID
    n = C.c_uint32()
    assert abi.lib.mx_graph_read_video_scopes(g._h, None, 0, C.byref(n)) == abi.MX_ERR_INVALID   # no taps
    # 2048 ticks x 7 taps x 330 784 bytes > 4 GiB at hop 1: refused, the message names the remedy, nothing is set
    seven = [(srcs[0], 0), (srcs[1], 0), (srcs[2], 0), (m0, 0), (m0, 1), (m1, 0), (m1, 1)]
    assert set_raw(seven, P(256, 1, 1)) == abi.MX_ERR_NOMEM
    assert b"hop" in abi.lib.mx_last_error()
    assert abi.lib.mx_graph_read_video_scopes(g._h, None, 0, C.byref(n)) == abi.MX_ERR_INVALID
    assert set_raw(seven, P(256, 1, 64)) == abi.MX_OK                      # the same taps at hop 64: 32 ticks of room
    assert abi.lib.mx_graph_read_video_scopes(g._h, None, 0, C.byref(n)) == abi.MX_ERR_INVALID   # no run since they were set
    d = video.DFrame(64, 36)
    video.graph_set_video_source(g, srcs[0], d, repeat=True)
    g.run_ticks(0, 2)
    rb = abi.video_scope_record_bytes(256, True)
    buf = np.zeros(7 * rb, np.uint8)
    assert abi.lib.mx_graph_read_video_scopes(g._h, buf.ctypes.data_as(C.c_void_p), 7 * rb - 1, C.byref(n)) == abi.MX_ERR_INVALID   # cap too small
    assert abi.lib.mx_graph_read_video_scopes(g._h, None, 7 * rb, C.byref(n)) == abi.MX_ERR_INVALID                                   # dst NULL
    assert abi.lib.mx_graph_read_video_scopes(g._h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)) == abi.MX_OK and n.value == 7
    recs = abi.parse_video_scope_records(buf, 256, True)
    assert [r["present"] for r in recs] == [1, 0, 0, 1, 1, 1, 1]           # source 0, m0's program and its A clone, m1's program and its A clone
    # a failed set leaves the taps as they were
    assert set_raw([(amp, 0)], ok) == abi.MX_ERR_TYPE
    assert abi.lib.mx_graph_read_video_scopes(g._h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)) == abi.MX_OK and n.value == 7
    # mx_graph_adopt_state carries no taps
    ws2 = sink_graph()[0]
    g2 = ws2.build(max_ticks_per_run=4)
    g2.adopt_state(g, list(range(len(ws2.nodes))))
    assert abi.lib.mx_graph_read_video_scopes(g2._h, buf.ctypes.data_as(C.c_void_p), buf.size, C.byref(n)) == abi.MX_ERR_INVALID
    # the pixel-path form
    rec = video.DeviceBuffer(rb)
    assert abi.lib.mx_video_scope(None, C.byref(ok), rec.ptr, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_video_scope(d._h, None, rec.ptr, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_video_scope(d._h, C.byref(ok), None, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_video_scope(d._h, C.byref(P(96, 0, 1)), rec.ptr, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_video_scope(d._h, C.byref(ok), C.c_void_p(rec.ptr.value + 2), None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_video_scope(d._h, C.byref(P(64, 1, 0)), rec.ptr, None) == abi.MX_OK      # hop is ignored here
    video.sync()
