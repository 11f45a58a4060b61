"""The deck's bars and phrases on the device (include/mixlab_gpu.h "BARS"): every beat record, the folds and the form counts
mx_deck_analyse_bars leaves, against the model (tests/deck_bars_model.py) over the shared cases (tests/deck_bars_cases.py), byte for byte; every kernel form; loading in
pieces; a second and third analysis; windows; the refusals, each of which leaves deck and result as they were; the five analyses of a deck back to back; two decks;
that playing is untouched; Deck.analyse -> beatgrid -> refine_grid -> find_bars against the composed models; and two decks synced on their bars grids, played."""
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
import loudness_model as lm
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu


def loaded(tr, pieces=None):
    d = deck.Deck(tr.shape[0])
    if pieces is None:
        d.load(tr)
    else:
        for a, b in pieces:
            d.load(tr[a:b], a)
    return d


def assert_equal(d, recs, H, label=""):
    got = d.read_bars()
    assert got.tobytes() == recs.tobytes(), (label, [k for k in range(min(len(got), len(recs))) if got[k] != recs[k]][:4], len(got), len(recs))
    got_H = d.read_bar_folds()
    assert got_H.dtype == np.uint64 and [int(v) for v in got_H] == list(H), label


def assert_result(d, case, label=""):
    recs, H, _n0 = bc.truth(case)
    assert_equal(d, recs, H, (case.name, label))


# ---- the records, folds and forms over the shared cases ----
@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name[:60])
def test_records_folds_and_forms_equal_the_model(case):
    d = loaded(bc.track(case))
    d.analyse_bars(bc.c_settings(case.settings))
    forms = deck.debug_last_bars()
    assert_result(d, case)
    d.close()
    assert forms == bc.forms(case), case.name


def test_every_kernel_form_is_among_the_cases():
    total = {}
    for c in bc.CASES:
        for k, v in bc.forms(c).items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total
    # ... and the shapes inside them: one case with halves of one tile only, one with both forms side by side, one where nothing is defined; novelty blocks that are
    # full and part-full; windows of one pair a lane pass (W = 1), of less than a pass, and of several passes (W = 64: 16 384 pairs)
    f = [bc.forms(c) for c in bc.CASES]
    assert any(x["wgs_half_tiled"] == 0 for x in f) and any(x["wgs_half_one_tile"] and x["wgs_half_tiled"] for x in f) and any(x["novelties_defined"] == 0 for x in f)
    assert {len(bc.truth(c)[0]) % abi.DECK_BARS_BLOCK for c in bc.CASES} == {0, 1, 2, 3}
    widths = {w for c in bc.CASES for w in (c.settings.w_bar, c.settings.w_phrase)}
    assert {1, 2, 3, 4, 5, 8, 32, 64} <= widths
    assert {c.settings.K for c in bc.CASES} >= {1, 9, 63, 127}


def test_a_track_loaded_in_pieces_gives_the_same_result():
    case = bc.BY_NAME["period 5000.7: several tiles a half, odd beats"]
    d = loaded(bc.track(case), pieces=[(70000, 95019), (0, 33), (33, 70000)])
    d.analyse_bars(bc.c_settings(case.settings))
    assert_result(d, case)
    d.close()


def test_a_second_and_third_analysis_and_windows():
    tr = bc.bumpy(2300 * 30, "second analysis", 1700)
    one = bm.Settings(bc.q32(400.0), bc.q32(2300.7), *bc.T9, w_bar=2, w_phrase=5)
    two = bm.Settings(bc.q32(900.0), bc.q32(4100.1), *bc.T63, M=3, Q=2, w_bar=1, w_phrase=3, lead=0)
    three = one._replace(max_beats=11)
    want = {s: bm.analyse(tr, s) for s in (one, two, three)}
    d = loaded(tr)

    def same(s, label):
        assert_equal(d, want[s][0], want[s][1], label)

    d.analyse_bars(bc.c_settings(one)); same(one, "first")
    d.analyse_bars(bc.c_settings(one)); same(one, "again")
    d.analyse_bars(bc.c_settings(two)); same(two, "other settings")
    recs = want[two][0]
    n = len(recs)
    for at, cnt in ((0, 1), (2, 4), (n - 1, 1), (n, 0), (1, n - 1)):
        assert d.read_bars(at, cnt).tobytes() == recs[at:at + cnt].tobytes(), (at, cnt)
    assert [int(v) for v in d.read_bar_folds(cap=bm.MAX_FOLDS)] == list(want[two][1])     # more room than M + M Q
    d.analyse_bars(bc.c_settings(three)); same(three, "cut")
    d.analyse_bars(bc.c_settings(one)); same(one, "a third time")
    d.load(np.zeros((3000, 2), np.int16), 5000)                 # a later load does not invalidate the snapshot
    same(one, "after a load")
    d.analyse_bars(bc.c_settings(one))                          # ... and a new analysis sees it
    recs, H, _ = bm.analyse(np.concatenate([tr[:5000], np.zeros((3000, 2), np.int16), tr[8000:]]), one)
    assert_equal(d, recs, H, "the new track")
    d.close()


def test_refusals_leave_the_previous_result_and_the_deck_usable():
    case = bc.BY_NAME["lead 4096"]

    def refused(fn):
        with pytest.raises(abi.MxError) as err:
            fn()
        assert err.value.code == abi.MX_ERR_INVALID, err.value

    d = loaded(bc.track(case))
    refused(lambda: d.read_bars(0, 1))          # no analysis yet
    refused(lambda: d.read_bar_folds(cap=136))
    d.analyse_bars(bc.c_settings(case.settings))
    n = len(bc.truth(case)[0])
    for change in ({"period": bm.PERIOD_MIN - 1}, {"period": bm.PERIOD_MAX + 1}, {"first": bm.FAR + 1}, {"lead": 4097}, {"taps": 8}, {"M": 1}, {"M": 9}, {"Q": 0}, {"Q": 17},
                   {"w_bar": 0}, {"w_phrase": 65}, {"tail": ((1,), ())}, {"hi": (16384, 0, -16384)}, {"period": bm.PERIOD_MAX}, {"period": 40000 << 32, "lead": 0}):
        bad = case.settings._replace(**change)
        assert bm.check(bad, len(bc.track(case))) is not None, change
        refused(lambda: d.analyse_bars(bc.c_settings(bad)))
        assert_result(d, case, f"after a refused {change}")
    refused(lambda: d.read_bars(0, n + 1))      # windows past the end
    refused(lambda: d.read_bars(n + 1, 0))
    refused(lambda: d.read_bar_folds(cap=19))   # M + M Q is 20
    buf = np.zeros(n, abi.DECK_BEAT_DTYPE)
    H = np.zeros(20, np.uint64)
    assert abi.lib.mx_deck_read_bars(d._h, 0, n, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_bar_folds(d._h, None, 20) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_bars(None, 0, n, buf.ctypes.data_as(C.c_void_p)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_bar_folds(None, H.ctypes.data_as(C.c_void_p), 20) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_analyse_bars(None, C.byref(bc.c_settings(case.settings))) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_bars(d._h, 0, n, buf.ctypes.data_as(C.c_void_p)) == abi.MX_OK and buf.tobytes() == bc.truth(case)[0].tobytes()
    refused(lambda: d.read_finegrid(0, 1))      # the other analyses were never made on this deck
    d.analyse_bars(None)                        # NULL frees
    refused(lambda: d.read_bars(0, 1))
    refused(lambda: d.read_bar_folds(cap=136))
    d.analyse_bars(None)
    d.analyse_bars(bc.c_settings(case.settings))
    assert_result(d, case, "analysed again")
    d.close()


def test_the_five_analyses_back_to_back_on_one_deck_and_a_second_deck_beside_it():
    """no read between the analyses: one stream orders them, and the five results do not share memory"""
    t = lk.TON_BY_NAME["20 hops of noise, G = 7: a short last segment"]
    tr = lk.track(t)
    l = lk.LOUD_BY_NAME["noise, 1000 frames"]._replace(name=t.name, n_frames=t.n_frames)   # (a noise track is seeded by its name and length)
    a = ac.BY_NAME["noise, 10 000 frames at C = 64"]
    f = fm.Settings(16, 9, 11 * fm.Q16 + 9, 777, first_hop=2)
    b = bm.Settings(bc.q32(333.3), bc.q32(2050.5), *bc.T9, M=3, Q=2, w_bar=1, w_phrase=2, lead=17)      # (a track of 10 240 frames: four beats)
    assert bm.check(b, len(tr)) is None and bm.beats(b, len(tr))[1] == 4
    want_cols, want_R = am.analyse(tr, a.settings)
    want_recs, want_w = fm.analyse(tr, f)
    want_beats, want_H, _ = bm.analyse(tr, b)
    other = bc.BY_NAME["M = 3, Q = 1"]
    d, d2 = loaded(tr), loaded(bc.track(other))
    d.analyse_bars(bc.c_settings(b)); d.analyse_finegrid(deck.finegrid(f.hop, f.n_periods, f.period0, f.dperiod, f.first_hop, f.max_beats)); d.analyse_tonality(lk.c_tonality(t))
    d2.analyse_bars(bc.c_settings(other.settings))
    d.analyse(deck.analysis(a.settings.column, a.settings.max_lag, a.settings.lo, a.settings.hi)); d.analyse_loudness(lk.c_loudness(l))
    assert_result(d2, other, "deck 2")
    assert lm.records_equal(d.read_loudness(), lk.loud_records(l))
    assert d.read_columns().tobytes() == want_cols.tobytes() and np.array_equal(d.read_autocorr(), want_R)
    assert b"".join(r["raw"] for r in d.read_tonality()) == b"".join(lk.ton_records(t))
    assert d.read_finegrid().tobytes() == np.array(want_recs, abi.DECK_COMB_DTYPE).tobytes() and np.array_equal(d.read_fine_onsets(), want_w)
    assert_equal(d, want_beats, want_H, "deck 1")
    d.close(); d2.close()


def test_playing_is_untouched_by_bars_calls_between_loads_and_feeds():
    """output bits, tick records and mx_deck_state of a deck fed into a small graph, with and without the new calls in between"""
    spt, n_ticks = 257, 4
    case = bc.BY_NAME["period 2049.37: every half a tile and a frame or two"]
    tr = bc.track(case)
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
            d.analyse_bars(bc.c_settings(case.settings))
        d.load(tr[6000:], 6000)
        d.set(deck.params(step_q32=dc.frames(1.08), flags=abi.DECK_PLAY)); d.seek(dc.frames(100.5))
        out = []
        for _ in range(3):
            if with_calls:
                d.analyse_bars(bc.c_settings(case.settings))
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


# ---- end to end ----
def device_chain(d, sec):
    """Deck.analyse -> mx_deck_beatgrid -> Deck.refine_grid -> Deck.find_bars, the host's side of the story on the device's own analyses"""
    a = deck.analysis_bands(rate=bc.RATE, column=bc.E2E_COLUMN, max_lag=bc.E2E_LAG)
    d.analyse(a)
    coarse = deck.beatgrid(d.read_columns(), d.read_autocorr(), a.column, bc.RATE, *bc.E2E_BPM)
    fine = d.refine_grid(coarse, a.column, bc.RATE, bc.E2E_HOP)
    return coarse, fine, d.find_bars(fine, a)


def test_analyse_beatgrid_refine_and_find_bars_equal_the_composed_models_and_find_the_downbeats():
    sec, e = bc.END_TO_END, bc.end_to_end()
    d = loaded(bc.section_track(sec))
    coarse, fine, p = device_chain(d, sec)
    assert (coarse.bpm, coarse.period_columns, coarse.first_beat_frame) == (e["coarse"].bpm, e["coarse"].period_columns, e["coarse"].first_beat_frame)
    assert (fine.grid.first_q32, fine.grid.period_q32, fine.score) == (e["fine"].grid.first, e["fine"].grid.period, e["fine"].score)
    assert bc.m_pick(p) == e["pick"]
    assert_equal(d, e["records"], e["folds"], "the deck holds the records find_bars read")
    misses = bc.downbeat_misses(sec, bm.Beats(p.bars.first_q32, p.bars.period_q32))
    print(f"bar phase {p.bar_phase}, phrase phase {p.phrase_phase}; downbeat misses: largest {max(misses):.1f} frames; bound {2 * bc.E2E_HOP}")
    assert (p.bar_phase, p.phrase_phase) == bc.section_truth(sec, e["n0"]) and max(misses) <= 2 * bc.E2E_HOP
    assert d.find_bars(abi.DeckFinePick()).bar_sum == 0 and d.find_bars(abi.DeckBeats(0, 0)).bar_sum == 0      # a pick, or a grid, without a period
    assert_equal(d, e["records"], e["folds"], "... which launches nothing")
    assert bc.m_pick(d.find_bars(fine.grid, deck.analysis_bands(rate=bc.RATE, column=bc.E2E_COLUMN, max_lag=bc.E2E_LAG), w_phrase=8, beats_per_bar=4)) == e["pick"]   # by keywords, on the grid
    d.close()
    quiet = loaded(np.zeros((30000, 2), np.int16))
    assert bc.m_pick(quiet.find_bars(abi.DeckBeats(0, 2400 << 32))) == bm.Pick()           # a silent track: every vector is zero, and so is the pick
    quiet.close()


def test_a_follower_synced_on_the_bars_grids_plays_as_the_deck_model_says_downbeat_on_downbeat():
    pair = bc.bar_sync_pair()
    secs = (bc.BAR_SYNC_LEADER, bc.BAR_SYNC_FOLLOWER)
    tracks = [bc.section_track(s) for s in secs]
    decks = [loaded(tr) for tr in tracks]
    picks = [device_chain(d, s)[2] for d, s in zip(decks, secs)]
    assert [bc.m_pick(p) for p in picks] == [pair["leader"]["pick"], pair["follower"]["pick"]]
    step, seek, _ = deck.deck_sync(picks[0].bars, bc.BAR_SYNC_LEADER_POS, dm.ONE, picks[1].bars, bc.BAR_SYNC_FOLLOWER_POS)
    assert (step, seek) == pair["sync"][:2]
    gaps, bound = bc.bar_sync_gaps(step, seek)
    print(f"{len(gaps)} downbeats; largest gap {max(gaps):.1f} output frames; bound {bound:.1f}")
    assert bound == 2 * bc.E2E_HOP and len(gaps) >= 12 and max(gaps) <= bound      # the two constructed downbeats coincide, to the end of the shorter track
    # ... and the device plays exactly that: both decks against the deck model, bit for bit
    tables = np.stack([deck.deck_tables(b) for b in range(4)])
    starts = [(dm.ONE, bc.BAR_SYNC_LEADER_POS), (step, seek)]
    want = []
    for tr, (st, pos) in zip(tracks, starts):
        m = dm.DeckModel(tr, tables)
        m.schedule(0, dm.Params(st, flags=dm.PLAY), pos)
        want.append(m.feed(bc.BAR_SYNC_TICKS, bc.BAR_SYNC_SPT)[0])
    ws = Workspace(*dc.rate_of(bc.BAR_SYNC_SPT))
    srcs = [ws.source_stereo(), ws.source_stereo()]
    mix = ws.mixer([(0.0, 1.0, False)] * 2)
    for k, s in enumerate(srcs):
        ws.connect(s, 0, mix, k)
    g = ws.build(max_ticks_per_run=bc.BAR_SYNC_FEED)
    for d, (st, pos) in zip(decks, starts):
        d.schedule(0, deck.params(step_q32=st, flags=abi.DECK_PLAY), pos)
    got = [[], []]
    for first in range(0, bc.BAR_SYNC_TICKS, bc.BAR_SYNC_FEED):
        deck.feed(decks, srcs, g, bc.BAR_SYNC_FEED)
        g.run_ticks(first, bc.BAR_SYNC_FEED)
        for k, s in enumerate(srcs):
            got[k].append(g.read_output(s, 0, bc.BAR_SYNC_FEED, True))
    for k in range(2):
        assert np.array_equal(np.concatenate(got[k]).view(np.uint32), want[k].view(np.uint32)), ("leader", "follower")[k]
    # ... in which both decks sound a kick where the leader's downbeats fall: loud within 150 output frames after each, on the leader and on the follower
    n_out = bc.BAR_SYNC_SPT * bc.BAR_SYNC_TICKS
    downs = [round((f * 2.0 ** 32 - bc.BAR_SYNC_LEADER_POS) / dm.ONE) for f in bc.downbeat_frames(bc.BAR_SYNC_LEADER)]
    downs = [x for x in downs if -1 <= x < n_out - 300]
    assert len(downs) >= 2
    for x in downs:
        for k in range(2):
            y = np.abs(want[k].reshape(-1, 2)[max(0, x - 150):x + 150]).max()
            assert y > 0.1, (x, ("leader", "follower")[k], y)      # (a kick peaks at 0.2; between kicks the tracks stay below 0.01)
    for d in decks:
        d.close()
    g.close()
