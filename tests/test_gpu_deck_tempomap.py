"""The deck's tempo map on the device (include/mixlab_gpu.h "TEMPO MAP"): every comb record, every tooth weight and the form counts
mx_deck_analyse_tempomap leaves, against the model (tests/deck_tempomap_model.py) over the shared cases (tests/deck_tempomap_cases.py), byte for byte; every kernel form;
loading in pieces; a second analysis that grows the buffer and one that keeps it; windows; the refusals, each of which leaves deck and result as they were; the six
analyses of a deck back to back; two decks; Deck.map_tempo against the model; the property of the CPU suite on the device's own map; that playing is untouched; and the
warp run of the CPU suite scheduled feed by feed and played on the device."""
import ctypes as C

import numpy as np
import pytest

import deck_analysis_cases as ac
import deck_analysis_model as am
import deck_bars_cases as bc
import deck_bars_model as bm
import deck_cases as dc
import deck_finegrid_model as fm
import deck_loudkey_cases as lk
import deck_model as dm
import deck_tempomap_cases as tc
import deck_tempomap_model as tm
import loudness_model as lm
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu


def c_settings(s):
    return deck.tempomap(s.hop, s.n_periods, s.period0, s.dperiod, s.window, s.stride)


def want_bytes(recs) -> bytes:
    return np.array(tc.flat(recs), abi.DECK_COMB_DTYPE).tobytes()


def loaded(tr, pieces=None):
    d = deck.Deck(tr.shape[0])
    if pieces is None:
        d.load(tr)
    else:
        for a, b in pieces:
            d.load(tr[a:b], a)
    return d


def assert_equal(d, recs, w, label=""):
    got = d.read_tempomap()
    want = tc.flat(recs)
    assert got.tobytes() == want_bytes(recs), (label, [(k, tuple(a), b) for k, (a, b) in enumerate(zip(got.tolist(), want)) if tuple(a) != b][:4])
    got_w = d.read_tempomap_onsets()
    assert got_w.dtype == np.uint32 and got_w.tobytes() == w.astype(np.uint32).tobytes(), (label, np.flatnonzero(got_w != w)[:4])


def assert_result(d, case, label=""):
    assert_equal(d, *tc.truth(case), label=(case.name, label))


def seg_tuples(segs) -> list:
    return [tm.Segment(*(int(x) for x in g)) for g in segs]


# ---- the records, weights and forms over the shared cases ----
@pytest.mark.parametrize("case", tc.CASES, ids=lambda c: c.name)
def test_records_weights_and_forms_equal_the_model(case):
    d = loaded(tc.track(case))
    d.analyse_tempomap(c_settings(case.settings))
    forms = deck.debug_last_tempomap()
    assert_result(d, case)
    d.close()
    assert forms == tc.forms(case), case.name


def test_every_kernel_form_is_among_the_cases_and_one_past_2_20_records_is_refused():
    total = {}
    for c in tc.CASES:
        for k, v in tc.forms(c).items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total
    # ... and the shapes inside them: a group of candidates that is not full, more than one group, phases at and one above the lanes of a pass, many passes
    n = sorted({c.settings.n_periods for c in tc.CASES})
    assert n[0] == 1 and any(x % abi.DECK_TEMPOMAP_GROUP for x in n) and any(x > abi.DECK_TEMPOMAP_GROUP for x in n) and any(x % abi.DECK_TEMPOMAP_GROUP == 0 for x in n)
    ph = {tm.phases(c.settings.period0 + j * c.settings.dperiod) for c in tc.CASES for j in range(c.settings.n_periods)}
    assert {tm.LANES, tm.LANES + 1} <= ph and max(ph) > 8 * tm.LANES
    n_frames, s = tc.ONE_PAST
    d = loaded(np.zeros((n_frames, 2), np.int16))
    with pytest.raises(abi.MxError) as err:
        d.analyse_tempomap(c_settings(s))
    assert err.value.code == abi.MX_ERR_INVALID and "windows x n_periods" in str(err.value)
    d.close()


def test_a_track_loaded_in_pieces_gives_the_same_result():
    case = tc.BY_NAME["dperiod 1, 40 periods"]
    d = loaded(tc.track(case), pieces=[(7000, 20000), (0, 33), (33, 7000)])
    d.analyse_tempomap(c_settings(case.settings))
    assert_result(d, case)
    d.close()


def test_a_second_analysis_that_grows_the_buffer_one_that_keeps_it_and_windows():
    """few records at h = 64 first, then many at h = 16 on the same deck (the buffer grows), then the first again (kept, and w moves inside it), then other settings"""
    tr = tc.bumpy(20000, "tm second analysis", 700)
    small, big, other = tm.Settings(64, 4, 9 * tm.Q16 + 5, 3001, 40, 30), tm.Settings(16, 11, 30 * tm.Q16 + 77, 999, 90, 13), tm.Settings(64, 2, 5 * tm.Q16, 40000, 12, 12)
    want = {s: tm.analyse(tr, s) for s in (small, big, other)}
    d = loaded(tr)
    d.analyse_tempomap(c_settings(small)); assert_equal(d, *want[small], "first")
    d.analyse_tempomap(c_settings(big)); assert_equal(d, *want[big], "grown")
    recs, w = tc.flat(want[big][0]), want[big][1]
    n_rec = len(recs)
    assert n_rec == tm.windows(1250, 90, 13) * 11
    for at, cnt in ((0, 1), (9, 4), (n_rec - 1, 1), (n_rec, 0), (1, n_rec - 1)):
        assert d.read_tempomap(at, cnt).tobytes() == np.array(recs[at:at + cnt], abi.DECK_COMB_DTYPE).tobytes(), (at, cnt)
    n = len(w)
    for at, cnt in ((0, 1), (255, 3), (n - 1, 1), (n, 0), (700, n - 700)):
        assert np.array_equal(d.read_tempomap_onsets(at, cnt), w[at:at + cnt]), (at, cnt)
    d.analyse_tempomap(c_settings(small)); assert_equal(d, *want[small], "kept")
    d.analyse_tempomap(c_settings(other)); d.analyse_tempomap(c_settings(big)); assert_equal(d, *want[big], "two in a row without a read")
    d.load(np.zeros((100, 2), np.int16), 50)                # a later load does not invalidate the snapshot
    assert_equal(d, *want[big], "after a load")
    d.analyse_tempomap(c_settings(other))                   # ... and a new analysis sees it
    assert_equal(d, *tm.analyse(np.concatenate([tr[:50], np.zeros((100, 2), np.int16), tr[150:]]), other), "a new analysis")
    d.close()


def test_refusals_leave_the_previous_result_and_the_deck_usable():
    case = tc.BY_NAME["one silent window between loud ones"]

    def refused(fn):
        with pytest.raises(abi.MxError) as err:
            fn()
        assert err.value.code == abi.MX_ERR_INVALID, err.value

    d = loaded(tc.track(case))
    refused(lambda: d.read_tempomap(0, 1))      # no analysis yet
    refused(lambda: d.read_tempomap_onsets(0, 1))
    d.analyse_tempomap(c_settings(case.settings))
    N = tm.hops(len(tc.track(case)), case.settings.hop)
    n_rec = 5 * case.settings.n_periods
    for field, value in (("hop", 8), ("hop", 96), ("n_periods", 0), ("n_periods", 1025), ("dperiod_q16", 0), ("period0_q16", tm.PERIOD_MIN - 1), ("period0_q16", tm.PERIOD_MAX),
                         ("window_hops", 19), ("window_hops", 16385), ("stride_hops", 0), ("stride_hops", 61), ("_pad", 1)):
        bad = c_settings(case.settings)
        setattr(bad, field, value)
        refused(lambda: d.analyse_tempomap(bad))
        assert_result(d, case, f"after a refused {field}")
    refused(lambda: d.read_tempomap(0, n_rec + 1))      # windows past the end
    refused(lambda: d.read_tempomap(n_rec + 1, 0))
    refused(lambda: d.read_tempomap_onsets(1, N))
    refused(lambda: d.read_tempomap_onsets(N + 1, 0))
    buf = np.zeros(n_rec, abi.DECK_COMB_DTYPE)
    assert abi.lib.mx_deck_read_tempomap(d._h, 0, n_rec, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_tempomap_onsets(d._h, 0, 6, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_tempomap(None, 0, n_rec, buf.ctypes.data_as(C.c_void_p)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_analyse_tempomap(None, C.byref(c_settings(case.settings))) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_tempomap(d._h, 0, n_rec, buf.ctypes.data_as(C.c_void_p)) == abi.MX_OK and buf.tobytes() == want_bytes(tc.truth(case)[0])
    refused(lambda: d.read_finegrid(0, 1))      # the other analyses were never made on this deck
    refused(lambda: d.read_columns(0, 1))
    d.analyse_tempomap(None)                    # NULL frees
    refused(lambda: d.read_tempomap(0, 1))
    refused(lambda: d.read_tempomap_onsets(0, 1))
    d.analyse_tempomap(None)
    d.analyse_tempomap(c_settings(case.settings))
    assert_result(d, case, "analysed again")
    d.close()


def test_the_six_analyses_back_to_back_on_one_deck_and_a_second_deck_beside_it():
    """no read between the analyses: one stream orders them, and the six results do not share memory -- the fine grid's w and the tempo map's least of all"""
    t = lk.TON_BY_NAME["20 hops of noise, G = 7: a short last segment"]
    tr = lk.track(t)
    l = lk.LOUD_BY_NAME["noise, 1000 frames"]._replace(name=t.name, n_frames=t.n_frames)   # (a noise track is seeded by its name and length)
    a = ac.BY_NAME["noise, 10 000 frames at C = 64"]
    f = fm.Settings(16, 9, 11 * fm.Q16 + 9, 777, first_hop=2)
    b = bm.Settings(bc.q32(333.3), bc.q32(2050.5), *bc.T9, M=3, Q=2, w_bar=1, w_phrase=2, lead=17)      # (a track of 10 240 frames: four beats)
    m = tm.Settings(32, 13, 9 * tm.Q16 + 3, 555, 50, 17)                                                   # (another hop than the fine grid's)
    assert bm.check(b, len(tr)) is None and tm.check(m, len(tr)) is None
    want_cols, want_R = am.analyse(tr, a.settings)
    want_recs, want_w = fm.analyse(tr, f)
    want_beats, want_H, _ = bm.analyse(tr, b)
    want_map = tm.analyse(tr, m)
    other = tc.BY_NAME["256 and 257 phases"]
    d, d2 = loaded(tr), loaded(tc.track(other))
    d.analyse_tempomap(c_settings(m)); d.analyse_bars(bc.c_settings(b)); d.analyse_finegrid(deck.finegrid(f.hop, f.n_periods, f.period0, f.dperiod, f.first_hop, f.max_beats))
    d2.analyse_tempomap(c_settings(other.settings))
    d.analyse_tonality(lk.c_tonality(t)); d.analyse(deck.analysis(a.settings.column, a.settings.max_lag, a.settings.lo, a.settings.hi)); d.analyse_loudness(lk.c_loudness(l))
    assert_result(d2, other, "deck 2")
    assert lm.records_equal(d.read_loudness(), lk.loud_records(l))
    assert d.read_columns().tobytes() == want_cols.tobytes() and np.array_equal(d.read_autocorr(), want_R)
    assert b"".join(r["raw"] for r in d.read_tonality()) == b"".join(lk.ton_records(t))
    assert d.read_finegrid().tobytes() == np.array(want_recs, abi.DECK_COMB_DTYPE).tobytes() and np.array_equal(d.read_fine_onsets(), want_w)
    assert d.read_bars().tobytes() == want_beats.tobytes() and np.array_equal(d.read_bar_folds(), want_H)
    assert_equal(d, *want_map, "deck 1")
    d.close(); d2.close()


# ---- Deck.map_tempo, and the property on the device's own map ----
@pytest.mark.parametrize("dr", tc.DRIFTS, ids=lambda d: d.name)
def test_map_tempo_equals_the_model_and_sits_on_the_clicks(dr):
    want_segs, s, recs, idx, pick = tc.drift_map(dr)
    d = loaded(tc.drift_track(dr))
    segs = d.map_tempo(abi.DeckBeats(pick.grid.first, pick.grid.period), tc.HOP, tc.WINDOW_BEATS, tc.STRIDE_BEATS, tc.WIDTH)
    assert seg_tuples(segs) == want_segs
    assert d.read_tempomap().tobytes() == want_bytes(recs)                                   # the deck holds the search's records
    forms = deck.debug_last_tempomap()
    assert forms == tm.forms(tc.N_FRAMES, s) and forms["wgs_staged"]
    per_window = d.map_tempo(abi.DeckBeats(pick.grid.first, pick.grid.period), tc.HOP, tc.WINDOW_BEATS, tc.STRIDE_BEATS, tc.WIDTH, penalty=0)
    assert seg_tuples(per_window) == tm.segments(recs, s, tc.N_FRAMES, tm.path([[r[0] for r in row] for row in recs], 0))
    beats = deck.tempomap_beats(segs, tc.N_FRAMES << 32)
    assert beats == tm.beats(want_segs, tc.N_FRAMES << 32)
    miss = tc.misses(dr, [b for b, _v in beats])
    assert max(miss) <= 2 + int(np.ceil(dr.dp_per_beat * (tc.WINDOW_BEATS / 2) ** 2 / 2 / tc.HOP)), miss   # the CPU suite's bound, derived there
    assert len(d.map_tempo(abi.DeckBeats(), tc.HOP)) == 0                                    # a grid without a period
    d.close()
    quiet = loaded(np.zeros((20000, 2), np.int16))
    segs = quiet.map_tempo(abi.DeckBeats(0, 2000 << 32), tc.HOP, tc.WINDOW_BEATS, tc.STRIDE_BEATS)
    assert len(segs) > 1 and not segs["period_q32"].any() and (segs["flags"] == abi.DECK_TEMPO_EMPTY).all()
    quiet.close()


def test_playing_is_untouched_by_tempo_map_calls_between_loads_and_feeds():
    """output bits, tick records and mx_deck_state of a deck fed into a small graph, with and without the new calls in between"""
    spt, n_ticks = 257, 4
    case = tc.BY_NAME["dperiod 1, 40 periods"]
    tr = tc.track(case)
    ws = Workspace(*dc.rate_of(spt))
    src = ws.source_stereo()
    mix = ws.mixer([(0.0, 1.0, False)])
    ws.connect(src, 0, mix, 0)
    g = ws.build(max_ticks_per_run=n_ticks)
    runs, clock = [], 0
    for with_calls in (False, True):
        d = deck.Deck(tr.shape[0])
        d.load(tr[:6000])
        if with_calls:
            d.analyse_tempomap(c_settings(case.settings))
        d.load(tr[6000:], 6000)
        d.set(deck.params(step_q32=dc.frames(1.08), flags=abi.DECK_PLAY)); d.seek(dc.frames(100.5))
        out = []
        for _ in range(3):
            if with_calls:
                d.analyse_tempomap(c_settings(case.settings))
            deck.feed([d], [src], g, n_ticks)
            g.run_ticks(clock, n_ticks)
            clock += n_ticks
            h = d.state()
            out.append((g.read_output(src, 0, n_ticks, True).view(np.uint32).tolist(),
                        [(k.pos_q32, k.step_q32, k.dstep_q32, k.loop_in, k.loop_len, k.flags, k.bank) for k in d.read_ticks(0, n_ticks)],
                        (h.pos_q32, h.step_q32, h.params.step_q32, h.params.flags, h.last_looping)))
        if with_calls:
            assert_result(d, case, "beside the feeds")
        runs.append(out)
        d.close()
    assert runs[0] == runs[1]
    g.close()


def test_the_warp_run_plays_on_the_device_as_the_deck_model_says():
    """the ramp track mapped on the device, scheduled with Deck.schedule_warp (mx_deck_schedule) before each feed of 8 ticks, bit for bit what the deck model plays under
    the model's own warp events"""
    dr = tc.DRIFT_BY_NAME["ramp"]
    want_segs, _s, _recs, _idx, pick = tc.drift_map(dr)
    tables = np.stack([deck.deck_tables(b) for b in range(4)])
    want_out, want_ticks, want_changes = tc.warp_run(dr, want_segs, tables)
    ws = Workspace(*dc.rate_of(tc.WARP_SPT))
    src = ws.source_stereo()
    mix = ws.mixer([(0.0, 1.0, False)])
    ws.connect(src, 0, mix, 0)
    g = ws.build(max_ticks_per_run=tc.WARP_FEED)
    d = loaded(tc.drift_track(dr))
    segs = d.map_tempo(abi.DeckBeats(pick.grid.first, pick.grid.period), tc.HOP, tc.WINDOW_BEATS, tc.STRIDE_BEATS, tc.WIDTH)
    got, ticks, changes = [], [], []
    for first in range(0, tc.WARP_TICKS, tc.WARP_FEED):
        ev = d.schedule_warp(segs, tc.WARP_OUT_PERIOD, tc.WARP_FEED, tc.WARP_SPT, *((deck.params(flags=abi.DECK_PLAY), 0) if first == 0 else ()))
        changes += [(first + k, seg, st) for k, seg, st in ev]
        deck.feed([d], [src], g, tc.WARP_FEED)
        g.run_ticks(first, tc.WARP_FEED)
        got.append(g.read_output(src, 0, tc.WARP_FEED, True))
        ticks += [dm.Tick(k.pos_q32, k.step_q32, k.dstep_q32, k.loop_in, k.loop_len, k.flags, k.bank) for k in d.read_ticks(0, tc.WARP_FEED)]
    assert changes == want_changes and len(changes) >= 4
    assert ticks == want_ticks
    assert np.array_equal(np.concatenate(got).view(np.uint32), want_out.view(np.uint32))
    d.close()
    g.close()
