"""Tonality taps on the device against tests/tonality_model.py, byte for byte: every record a run emits, header and sums.  The model is fed
what the graph itself wrote on each tapped port (read back with read_output), so what is tested here is the measurement; the ports have
their own parity tests.  The shapes are tests/tonality_cases.py's."""
import numpy as np
import pytest

import synth
import tonality_cases as tc
import tonality_model as tm
from mixlab_amd import abi
from mixlab_amd.workspace import Workspace
from test_gpu_audio_parity import strips
from test_gpu_spectrum import io_graph, wide

pytestmark = pytest.mark.gpu
F32 = np.float32


class Tap:
    """one tap and its model; `rate` is the port's (up, down) domain"""

    def __init__(self, node, port, channels, rate=(1, 1)):
        self.node, self.port, self.channels, self.rate = node, port, channels, rate
        self.model = None

    def port_data(self, g, n_ticks):
        return g.read_output(self.node, self.port, n_ticks, self.channels == 2, rate=self.rate)


def set_taps(g, taps, sr, D, Hc, O, f_lo_mhz, emit):
    g.set_tonality([(t.node, t.port) for t in taps], D, Hc, O, f_lo_mhz, emit)
    for t in taps:
        t.model = tm.TonalityModel(sr * t.rate[0] / t.rate[1], D, Hc, O, f_lo_mhz, emit, t.channels)


def check_run(g, taps, n_ticks, what, port_source=None):
    """the last run's records of every tap against its model fed the port's samples (read from `port_source`, default g); returns the
    records as a list over emissions of lists over taps of bytes"""
    got = g.read_tonality()
    want = [t.model.run(t.port_data(port_source or g, n_ticks), n_ticks) for t in taps]
    assert len(got) == len(want[0]), f"{what}: {len(got)} emissions, the model has {len(want[0])}"
    for e, row in enumerate(got):
        assert len(row) == len(taps)
        for i, t in enumerate(taps):
            if row[i]["raw"] != want[i][e]:
                a, b = row[i], tm.parse_record(want[i][e])
                head = [(k, a[k], b[k]) for k in ("tick_in_run", "hops", "nonfinite", "decim", "hop_frames", "octaves", "f_lo_mhz", "reserved") if a[k] != b[k]]
                bad = np.flatnonzero(a["cq"] != b["cq"])
                raise AssertionError(f"{what}: tap {i} ({t.node}, {t.port}), emission {e}: header {head}; {bad.size} bins differ, first {bad[:4]}: "
                                     f"{a['cq'][bad[:4]]} vs {b['cq'][bad[:4]]}")
    return [[r["raw"] for r in row] for row in got]


def feed(g, ss, smn, n_ticks, spt, seed):
    g.write_source(ss, tc.hostile(seed, n_ticks * spt, 2), n_ticks)
    g.write_source(smn, tc.hostile(seed + 1, n_ticks * spt, 1), n_ticks)


@pytest.mark.parametrize("case_id", [c.id for c in tc.CASES])
def test_shared_cases_in_runs_of_1_3_7_64_ticks_and_in_one_piece(case_id):
    """every shared case on a stereo port, a mono port and a stereo port behind an Amplifier, however the ticks are grouped into runs;
    +-Inf, NaN, subnormals, +-2 and sums that overflow are in every stream"""
    c = tc.by_id(case_id)
    xs, xm = tc.hostile(3, c.n_ticks * c.F, 2), tc.hostile(4, c.n_ticks * c.F, 1)
    results = []
    for run in (c.n_ticks, 1, 3, 7, 64):
        ws, ss, smn, amp, g = io_graph(c.rate, c.rate // c.F, min(run, c.n_ticks))
        taps = [Tap(amp, 0, 2), Tap(smn, 0, 1), Tap(ss, 0, 2)] if c.F > 1 else [Tap(smn, 0, 1), Tap(ss, 0, 2)]
        set_taps(g, taps, c.rate, c.D, c.Hc, c.O, c.f_lo_mhz, c.emit)
        out, at = [], 0
        while at < c.n_ticks:
            k = min(run, c.n_ticks - at)
            g.write_source(ss, xs[at * 2 * c.F:(at + k) * 2 * c.F], k); g.write_source(smn, xm[at * c.F:(at + k) * c.F], k)
            g.run_ticks(at, k)
            for row in check_run(g, taps, k, f"{c.id} runs of {run} at {at}"):
                out.append([(at + tm.parse_record(b)["tick_in_run"], b[4:]) for b in row])
            at += k
        results.append(out)
    for k in range(1, len(results)):
        assert results[k] == results[0], k
    assert [row[0][0] for row in results[0]] == list(range(c.emit - 1, c.n_ticks, c.emit))
    recs = [tm.parse_record(b"\0\0\0\0" + b) for row in results[0] for _, b in row]
    assert sum(r["nonfinite"] for r in recs) > 0 and any(r["cq"].any() for r in recs)
    assert sum(r["hops"] for r in recs[::len(taps)]) == -(-(c.n_ticks // c.emit * c.emit * c.F) // c.D) // c.Hc
    if c.id == "one_frame":   # many ticks pass with no complete hop: those emissions are all zero
        early = recs[:72 * len(taps)]
        assert all(r["hops"] == 0 and not r["cq"].any() for r in early)
    # setting again resets every tap and c: the same first ticks read as they did from silence
    set_taps(g, taps, c.rate, c.D, c.Hc, c.O, c.f_lo_mhz, c.emit)
    k = min(64, c.n_ticks)
    g.write_source(ss, xs[:k * 2 * c.F], k); g.write_source(smn, xm[:k * c.F], k); g.run_ticks(c.n_ticks, k)
    again = check_run(g, taps, k, "after a second set")
    assert [[b[4:] for b in row] for row in again] == [[b for _, b in row] for row in results[0][:k // c.emit]]


def test_two_rate_domains_in_one_set_behind_a_resampler():
    sr, n = 44100, 6
    ws = Workspace(sr, 60)
    src = ws.source_stereo()
    rs = ws.resample(160, 147, np.full((160, 4), 0.4))
    ws.connect(src, 0, rs, 0)
    g = ws.build(max_ticks_per_run=n)
    taps = [Tap(rs, 0, 2, rate=(160, 147)), Tap(src, 0, 2)]   # 48 kHz / 800 frames and 44.1 kHz / 735 frames per tick: two table sets
    set_taps(g, taps, sr, 4, 128, 2, 440000, 2)
    assert taps[0].model.N != taps[1].model.N
    seen = []
    for r in range(3):
        g.write_source(src, wide(r, n * 2 * 735) * F32(2.0), n)
        g.run_ticks(r * n, n)
        seen += check_run(g, taps, n, f"resampled run {r}")
    last = [tm.parse_record(b) for b in seen[-1]]
    assert len(seen) == 9 and all(r["cq"].any() for r in last) and sum(tm.parse_record(row[0])["hops"] for row in seen) == 3 * n * 800 // 4 // 128


def test_device_bound_source_and_a_descriptor_reupload_keep_the_stream():
    """A source bound to a device buffer (another graph's port).  Binding it again rebuilds every tap descriptor mid-stream, and what the taps
    carry comes through: stream position, both histories, sums, counts and the counter; the model runs on as one stream."""
    sr, n = 44100, 5
    feed_ws = Workspace(sr, 60); src = feed_ws.source_stereo(); fg = feed_ws.build(max_ticks_per_run=n)
    ws2 = Workspace(sr, 60); bsrc = ws2.source_stereo(); amp = ws2.amplifier(0.5, 0.0); ws2.connect(bsrc, 0, amp, 0)
    g2 = ws2.build(max_ticks_per_run=n)
    taps = [Tap(bsrc, 0, 2), Tap(amp, 0, 2)]
    set_taps(g2, taps, sr, 4, 128, 2, 440000, 3)   # before the bind: the descriptors follow it
    ptr = fg.output_device_ptr(src, 0)[0]
    g2.bind_source_device(bsrc, ptr)
    emitted = 0
    for r in range(6):   # 30 ticks of 735 frames: 43 hops
        if r in (2, 5):
            g2.bind_source_device(bsrc, ptr)
        fg.write_source(src, tc.hostile(20 + r, n * 735, 2), n)
        g2.run_ticks(r * n, n)
        emitted += len(check_run(g2, taps, n, f"bound run {r}"))
    assert emitted == 6 * n // 3


def test_dup_stored_strip_ports_equal_the_unfused_graph():
    sr, n = 48000, 6
    ws, mix, srcs, trigs = strips(8, sr)
    amps = [mix + 6 * (k + 1) for k in range(8)]
    fused, plain = ws.build(max_ticks_per_run=n), ws.build(max_ticks_per_run=n, flags=abi.FLAG_NO_FUSE)
    with pytest.raises(abi.MxError):
        fused.output_device_ptr(amps[0], 0)   # stored one float per frame
    mk = lambda: [Tap(a, 0, 2) for a in amps] + [Tap(mix, 0, 2), Tap(mix, 1, 2)]
    tf, tp = mk(), mk()
    set_taps(fused, tf, sr, 4, 128, 2, 440000, 2); set_taps(plain, tp, sr, 4, 128, 2, 440000, 2)
    for r, nr in enumerate((n, 1, n, n)):   # a one-tick run between longer ones
        for g in (fused, plain):
            for k, tr in enumerate(trigs):
                g.update_params(tr, abi.TriggerParams(1 if (k + r) % 3 else 0))
            for k, s in enumerate(srcs):
                g.write_source(s, synth.noise(k + 10 * r, nr * 800) * F32(6.0), nr)
            g.run_ticks(r * n, nr)
        a = check_run(fused, tf, nr, f"fused run {r}")
        b = check_run(plain, tp, nr, f"unfused run {r}")
        assert a == b, "a dup-stored port reads as the unfused graph's stereo port"
    assert any(tm.parse_record(x)["cq"].any() for x in a[-1])


def test_master_and_cue_behind_the_held_back_mixer_bank_with_every_other_tap_set():
    """The second-stream mode on: runs go out in pairs, taps on the Master and the Cue go behind the held-back Mixer bank on the second
    stream (both buffer parities, deferred launch), taps on strips read that run's buffer parity.  The six other audio tap sets sit on the
    same ports; their records are those of the same desk without tonality taps, and every port is what the desk without taps gives."""
    sr, spt, n, n_runs, n_strips = 48000, 800, 8, 6, 32
    ws, mix, srcs, trigs = strips(n_strips, sr)
    amps = [mix + 6 * (k + 1) for k in (0, 17, 31)]
    where = [(mix, 0), (amps[0], 0), (mix, 1)] + [(a, 0) for a in amps[1:]]
    edges = abi.log_band_edges(256, 8, 100.0, 10000.0, sr)

    def others(gr):
        gr.set_meters(where, abi.MeterParams(2, 0.75)); gr.set_spectra(where, 256, edges); gr.set_loudness(where, 3, 5)
        gr.set_stereo(where, 4, 64, 1, 4); gr.set_limiters(where, 0.25, 64); gr.set_tempo(where, 128, 64, 32, 3)

    plain = ws.build(max_ticks_per_run=n, flags=abi.FLAG_OVERLAP_TAIL)    # the same desk without taps
    six = ws.build(max_ticks_per_run=n, flags=abi.FLAG_OVERLAP_TAIL); others(six)
    g = ws.build(max_ticks_per_run=n, flags=abi.FLAG_OVERLAP_TAIL); others(g)
    taps = [Tap(nd, p, 2) for nd, p in where]
    set_taps(g, taps, sr, 4, 128, 2, 440000, 3)
    noise = [synth.noise(k, n_runs * n * spt) * F32(8.0) for k in range(n_strips)]
    for r in range(n_runs):
        for gr in (plain, six, g):
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
        rows = check_run(g, taps, n, f"run {r}", port_source=plain)
        assert tm.parse_record(rows[-1][0])["cq"].any()
        for name, read in (("meters", lambda x: x.read_meters(0, n)), ("spectra", lambda x: x.read_spectra(0, n)), ("loudness", lambda x: x.read_loudness(0, n)),
                           ("stereo", lambda x: x.read_stereo(0, n)), ("limiters", lambda x: x.read_limiters(0, n)), ("limited", lambda x: x.read_limited(0, 0, n)),
                           ("tempo", lambda x: np.frombuffer(b"".join(rec["raw"] for row in x.read_tempo() for rec in row), np.uint8))):
            assert read(g).tobytes() == read(six).tobytes(), f"{name} differ with tonality taps set"
    assert g.tail_stream() is not None   # the taps do not end the second-stream mode


def test_a_pure_tone_on_the_master_peaks_at_its_bin_and_reads_its_pitch_class():
    sr, spt, n = 48000, 800, 40   # 32 000 frames: 4000 decimated, 7 hops of 512
    ws = Workspace(sr, 60)
    mix = ws.mixer([(0.0, 1.0, False)])
    src = ws.source_stereo()
    ws.connect(src, 0, mix, 0)
    g = ws.build(max_ticks_per_run=n)
    g.set_tonality([(mix, 0)], 8, 512, 5, 65406, n)
    b = 33                                                  # A4: bin 33 above C2
    f = 65.406 * 2.0 ** (b / 12.0)
    x = (0.4 * np.sin(2 * np.pi * f * np.arange(n * spt) / sr)).astype(F32)
    g.write_source(src, np.repeat(x, 2), n)
    g.run_ticks(0, n)
    rows = g.read_tonality()
    assert len(rows) == 1 and rows[0][0]["hops"] == n * spt // 8 // 512
    model = tm.TonalityModel(sr, 8, 512, 5, 65406, n, 2)
    assert rows[0][0]["raw"] == model.run(g.read_output(mix, 0, n, True), n)[0]
    assert int(np.argmax(rows[0][0]["cq"] / np.array(model.N))) == b
    # What the fold must show follows from the window.  A Hann kernel of Q = 17 periods answers a tone x of its own transform bins away
    # with |sinc(x) / (1 - x^2)| of its peak, and a semitone is 17 (1 - 2^(-1/12)) = 0.954 such bins seen from the bin above and
    # 17 (2^(1/12) - 1) = 1.011 seen from the bin below: 0.535 and 0.491 of the peak, against 0.031 and 0.012 two semitones off.  So the
    # tone's class holds less than half (1 / (1 + 0.535 + 0.491) = 0.494 at the most), B flat follows, then A flat, then all the rest.
    leak = lambda x: abs(np.sinc(x) / (1.0 - x * x))
    up, down = leak(17.0 * (1.0 - 2.0 ** (-1 / 12.0))), leak(17.0 * (2.0 ** (1 / 12.0) - 1.0))
    assert 1.0 > up > down > leak(17.0 * (1.0 - 2.0 ** (-2 / 12.0))) > leak(17.0 * (2.0 ** (2 / 12.0) - 1.0))
    ch = abi.tonality_chroma(rows[0], sr)
    print("chroma", ch, "expected neighbours", down, up)
    assert int(np.argmax(ch)) == 9 and ch[9] < 1.0 / (1.0 + up + down)
    assert ch[9] > ch[10] > ch[8] > np.delete(ch, [8, 9, 10]).max()


def test_refusals_profile_and_adopt_state():
    ws = Workspace(48000, 60)
    ss, smn = ws.source_stereo(), ws.source_mono()
    vm = ws.video_mixer(a=None, b=None, fader=1.0)
    ws2, mix, srcs, trigs = strips(2, 48000)
    pan = mix + 5
    assert ws2.nodes[pan][0] == abi.KIND_STEREO_PANNER
    g = ws.build(max_ticks_per_run=4)
    g2 = ws2.build(max_ticks_per_run=4)
    ok = (4, 128, 2, 440000, 1)

    def code(gr, ports, par=ok):
        pa = (abi.PortRef * len(ports))(*[abi.PortRef(n, p) for n, p in ports])
        rc = abi.lib.mx_graph_set_tonality(gr._h, pa, len(ports), abi.C.byref(abi.TonalityParams(*par)))
        return rc, (abi.lib.mx_last_error() or b"").decode()

    assert code(g, [(vm, 0)])[0] == abi.MX_ERR_TYPE
    assert code(g, [(len(ws.nodes), 0)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 1)])[0] == abi.MX_ERR_INVALID
    assert code(g, [(ss, 0), (smn, 0), (ss, 0)])[0] == abi.MX_ERR_INVALID   # a duplicate
    for par in ((2, 128, 2, 440000, 1), (16, 128, 2, 440000, 1), (4, 64, 2, 440000, 1), (4, 1024, 2, 440000, 1), (4, 128, 1, 440000, 1), (4, 128, 7, 440000, 1),
                (4, 128, 2, 0, 1), (4, 128, 2, 440000, 0),
                (4, 128, 2, 99000, 1),      # N_0 = ceil(17 x 12000 / 99) = 2061
                (8, 128, 6, 65406, 1)):     # the top bin, 3951 Hz, above 0.45 x 6000 Hz
        assert code(g, [(ss, 0)], par)[0] == abi.MX_ERR_INVALID, par
    assert code(g, [(ss, 0)], (4, 512, 5, 130813, 1))[0] == abi.MX_OK and code(g, [(ss, 0), (smn, 0)], (8, 128, 5, 65406, 1 << 31))[0] == abi.MX_OK
    pa = (abi.PortRef * 1)(abi.PortRef(ss, 0))
    assert abi.lib.mx_graph_set_tonality(g._h, pa, 1, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_set_tonality(g._h, None, 1, abi.C.byref(abi.TonalityParams(*ok))) == abi.MX_ERR_INVALID
    c, msg = code(g2, [(pan, 0)])
    with pytest.raises(abi.MxError) as e:
        g2.read_output(pan, 0, 1, True)
    assert c == abi.MX_ERR_INVALID and msg in str(e.value)   # a port the fusion did not materialise
    big = Workspace(8000, 8000); bs = big.source_mono()
    gb = big.build(max_ticks_per_run=(1 << 23) + 8)   # one-frame ticks; more than 2^23 emissions of 512 bytes: beyond 4 GiB
    assert code(gb, [(bs, 0)], (4, 128, 5, 20000, 1))[0] == abi.MX_ERR_NOMEM
    assert code(gb, [(bs, 0)], (4, 128, 5, 20000, 64))[0] == abi.MX_OK
    g.set_tonality([])
    with pytest.raises(abi.MxError):
        g.read_tonality()   # no taps
    g.set_tonality([(ss, 0), (smn, 0)], 4, 128, 2, 440000, 2)
    with pytest.raises(abi.MxError):
        g.read_tonality()   # no run since the taps were set
    g.write_source(ss, wide(1, 4 * 1600) * F32(4.0), 4)
    g.run_ticks(0, 4)
    first = [[r["raw"] for r in row] for row in g.read_tonality()]
    assert len(first) == 2 and tm.parse_record(first[1][0])["cq"].any()
    assert code(g, [(ss, 0)], (4, 128, 7, 440000, 2))[0] == abi.MX_ERR_INVALID   # refused: the set and its records stay as they were
    assert [[r["raw"] for r in row] for row in g.read_tonality()] == first
    rb = 32 + 96 * 2
    raw, got = np.zeros(4 * rb, np.uint8), abi.C.c_uint32()
    assert abi.lib.mx_graph_read_tonality(g._h, raw.ctypes.data, 4 * rb - 1, abi.C.byref(got)) == abi.MX_ERR_INVALID   # cap too small
    assert abi.lib.mx_graph_read_tonality(g._h, None, 4 * rb, abi.C.byref(got)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_graph_read_tonality(g._h, raw.ctypes.data, 4 * rb, None) == abi.MX_OK and raw.tobytes() == b"".join(b for row in first for b in row)
    # the launches are in the profile's total, in no kind; adopt_state carries no taps
    by_kind, total = g.profile_run(4, 4)
    assert total > sum(by_kind.values()) and set(by_kind) <= set(abi.KIND_NAMES[:abi.PROFILE_KINDS])
    g3 = ws.build(max_ticks_per_run=4)
    g3.adopt_state(g, list(range(len(ws.nodes))))
    g3.run_ticks(8, 4)
    with pytest.raises(abi.MxError):
        g3.read_tonality()
