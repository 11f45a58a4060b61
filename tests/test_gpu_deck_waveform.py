"""The deck's waveform picture on the device (include/mixlab_gpu.h "WAVEFORM"): every byte of the three planes mx_deck_render_waveform writes,
stride padding included, against the Python model (tests/deck_waveform_model.py) over the shared cases (tests/deck_waveform_cases.py); the strips' forms; the host
restatement over the device's own records; the ordering against the analysis it reads and the one that replaces it; two decks on one stream; the refusals, each of
which leaves *out, the analysis and the deck as they were; that playing is untouched; and the frame as a view of the multiviewer."""
import ctypes as C

import numpy as np
import pytest

import deck_cases as dc
import deck_waveform_cases as wc
import deck_waveform_model as wm
import video_multiview_model as mm
from mixlab_amd import abi, deck, video
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu


def loaded(case):
    tr = wc.track(case)
    d = deck.Deck(tr.shape[0])
    d.load(tr)
    return d


def whole_planes(f):
    """the frame's three planes as they lie in device memory, stride padding included"""
    video.sync(f.stream)
    ptrs, strides = f.device_planes()
    out = []
    for k in range(3):
        rows = f.height >> (1 if k else 0)
        got = np.empty(strides[k] * rows, np.uint8)
        abi.check(abi.lib.mx_device_download(got.ctypes.data_as(C.c_void_p), C.c_void_p(ptrs[k]), got.size, None))
        out.append(got.reshape(rows, strides[k]))
    return out


def assert_picture(f, want, what):
    """every byte of the frame's planes: `want` in the visible area, Y 0 and chroma 0x80 in the stride padding"""
    assert f.fmt == video.PIXFMT_YUV420P and not f.has_alpha() and (f.width, f.height) == (want[0].shape[1], want[0].shape[0])
    for name, g, w in zip("YUV", whole_planes(f), wm.padded(want, f.width, f.height)):
        assert g.shape == w.shape, f"{what}: plane {name} is {g.shape} with its stride, want {w.shape}"
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: plane {name} differs at {bad[:4].tolist()} ({len(bad)} bytes), got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}"


@pytest.mark.parametrize("case", wc.CASES, ids=lambda c: c.name)
def test_the_picture_its_padding_and_the_counts_equal_the_model(case):
    d = loaded(case)
    d.analyse(wc.abi_analysis(case.settings))
    p = wc.abi_wave(case.wave)
    f = d.render_waveform(p)                      # no host wait between the analysis and the render
    counts = deck.debug_last_waveform()
    assert_picture(f, wc.truth(case), case.name)
    assert counts == wm.forms(case.wave, case.settings.column, d.n_frames), case.name
    # ... and the host restatement over the device's own records gives the device's picture
    host = deck.waveform_host(d.read_columns(), case.settings.column, d.n_frames, p)
    for name, g, w in zip("YUV", f.download(), host):
        assert np.array_equal(g, w), f"{case.name}: plane {name} of the device against mx_deck_waveform_host"
    d.close()


def test_every_form_ran():
    total = {}
    for case in wc.CASES:
        for k, v in wm.forms(case.wave, case.settings.column, wc.track(case).shape[0]).items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total   # (the counts themselves are held against the device's case by case, above)


def test_a_render_is_ordered_behind_its_analysis_and_ahead_of_the_one_that_regrows_the_buffer():
    small, large = wc.BY_NAME["C = 512"], wc.BY_NAME["130 x 34"]
    tr = wc.track(large)
    n = tr.shape[0]
    cols512 = wc.am.analyse(tr, small.settings)[0]
    want1 = wm.render(cols512, 512, n, small.wave)
    d = deck.Deck(n)
    d.load(tr)
    d.analyse(wc.abi_analysis(small.settings))          # 12 records
    f1 = d.render_waveform(wc.abi_wave(small.wave))     # nothing has waited for the analysis
    d.analyse(wc.abi_analysis(large.settings))          # 94 records: the buffer is regrown under the render in flight
    f2 = d.render_waveform(wc.abi_wave(large.wave))
    d.analyse(wc.abi_analysis(large.settings))          # ... and rewritten in place under the second
    assert_picture(f1, want1, "the first picture, downloaded after the buffer went")
    assert_picture(f2, wc.truth(large), "the second picture")
    assert np.array_equal(d.read_columns(), wc.columns(large))
    d.close()


def test_two_decks_rendered_back_to_back_on_one_stream():
    a, b = wc.BY_NAME["66 x 18"], wc.BY_NAME["envelope of an all-negative track"]
    da, db = loaded(a), loaded(b)
    da.analyse(wc.abi_analysis(a.settings)); db.analyse(wc.abi_analysis(b.settings))
    fa, fb = da.render_waveform(wc.abi_wave(a.wave)), db.render_waveform(wc.abi_wave(b.wave))
    fa2 = da.render_waveform(wc.abi_wave(a.wave))
    assert_picture(fb, wc.truth(b), "deck b")
    assert_picture(fa, wc.truth(a), "deck a")
    assert_picture(fa2, wc.truth(a), "deck a again")
    da.close(); db.close()


def test_refusals_leave_out_the_analysis_and_the_deck_as_they_were():
    case = wc.BY_NAME["64 x 16"]
    d = loaded(case)
    good = wc.abi_wave(case.wave)
    mark = 0x5A5A5A5A

    def refused(p):
        out = C.c_void_p(mark)
        assert abi.lib.mx_deck_render_waveform(d._h, C.byref(p), C.byref(out), None) == abi.MX_ERR_INVALID
        assert out.value == mark

    refused(good)                                      # no analysis yet
    d.analyse(wc.abi_analysis(case.settings))
    for field, value in (("w", 63), ("h", 2), ("frames_per_px", 0), ("style", 2), ("n_grids", 17), ("_pad", 1)):
        bad = wc.abi_wave(case.wave)
        setattr(bad, field, value)
        refused(bad)
        assert_picture(d.render_waveform(good), wc.truth(case), f"after a refused {field}")
    assert np.array_equal(d.read_columns(), wc.columns(case))
    d.analyse(None)                                    # the results go: nothing to render
    refused(good)
    d.analyse(wc.abi_analysis(case.settings))
    assert_picture(d.render_waveform(good), wc.truth(case), "analysed again")
    d.close()


def test_playing_is_untouched_by_renders_between_loads_and_feeds():
    """output bits, tick records and mx_deck_state of a deck fed into a small graph, with and without analyse and render calls in between"""
    spt, n_ticks = 257, 4
    case = wc.BY_NAME["130 x 34"]
    tr = wc.track(case)
    ws = Workspace(*dc.rate_of(spt))
    src = ws.source_stereo()
    mix = ws.mixer([(0.0, 1.0, False)])
    ws.connect(src, 0, mix, 0)
    g = ws.build(max_ticks_per_run=n_ticks)
    runs, clock = [], 0
    for with_render in (False, True):
        d = deck.Deck(tr.shape[0])
        d.load(tr[:4000])
        if with_render:
            d.analyse(wc.abi_analysis(case.settings))
            d.render_waveform(wc.abi_wave(case.wave))
        d.load(tr[4000:], 4000)
        d.set(deck.params(step_q32=dc.frames(1.08), flags=abi.DECK_PLAY)); d.seek(dc.frames(100.5))
        out, pictures = [], []
        for _ in range(3):
            if with_render:
                d.analyse(wc.abi_analysis(case.settings))
                pictures.append(d.render_waveform(wc.abi_wave(case.wave)))
            deck.feed([d], [src], g, n_ticks)
            g.run_ticks(clock, n_ticks)
            clock += n_ticks
            h = d.state()
            out.append((g.read_output(src, 0, n_ticks, True).view(np.uint32).tolist(),
                        [(t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank) for t in d.read_ticks(0, n_ticks)],
                        (h.pos_q32, h.step_q32, h.params.step_q32, h.params.flags, h.last_looping)))
        for k, f in enumerate(pictures):
            assert_picture(f, wc.truth(case), f"the picture beside feed {k}")
        runs.append(out)
        d.close()
    assert runs[0] == runs[1]
    g.close()


def test_the_frame_is_a_view_of_the_multiviewer_beside_a_plain_picture():
    case = wc.BY_NAME["66 x 18"]
    d = loaded(case)
    d.analyse(wc.abi_analysis(case.settings))
    f = d.render_waveform(wc.abi_wave(case.wave))
    plain = mm.noise_src(34, 18, 7)
    dev = video.DFrame(plain.w, plain.h).upload(plain.y, plain.u, plain.v)
    p = mm.MvP(130, 74, (mm.View(2, 2, 70, 22, 2, mm.RED, 0), mm.View(80, 30, 44, 30, 2, mm.GREEN, 1)))
    params = video.MultiviewParams(p.canvas_w, p.canvas_h, [video.MultiviewView(v.x, v.y, v.w, v.h, v.border, v.colour, v.fit) for v in p.views], bg=p.bg, hop=1)
    out, shown = video.multiview([f, dev], params)
    assert shown == 3
    Y, U, V = wc.truth(case)
    want = mm.multiview_model([mm.Src(case.wave.w, case.wave.h, Y, U, V), plain], p)
    for name, g, w in zip("YUV", out.download(), want):
        assert np.array_equal(g, w), f"canvas plane {name}"
    d.close()
