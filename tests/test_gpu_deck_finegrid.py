"""The deck's fine beat grid on the device (include/mixlab_gpu.h "FINE GRID"): every comb record, every tooth weight and the form counts
mx_deck_analyse_finegrid leaves, against the model (tests/deck_finegrid_model.py) over the shared cases (tests/deck_finegrid_cases.py), byte for byte; every kernel
form; loading in pieces; a second and third analysis; windows; the refusals, each of which leaves deck and result as they were; the four analyses of a deck back to
back; two decks; Deck.refine_grid against the model's two stages; that playing is untouched; and the synced pair of the CPU suite played on the device."""
import ctypes as C

import numpy as np
import pytest

import deck_analysis_cases as ac
import deck_analysis_model as am
import deck_cases as dc
import deck_finegrid_cases as fc
import deck_finegrid_model as fm
import deck_loudkey_cases as lk
import deck_model as dm
import loudness_model as lm
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu


def c_settings(s):
    return deck.finegrid(s.hop, s.n_periods, s.period0, s.dperiod, s.first_hop, s.max_beats)


def want_bytes(recs) -> bytes:
    return np.array(recs, abi.DECK_COMB_DTYPE).tobytes()


def loaded(tr, pieces=None):
    d = deck.Deck(tr.shape[0])
    if pieces is None:
        d.load(tr)
    else:
        for a, b in pieces:
            d.load(tr[a:b], a)
    return d


def assert_result(d, case, label=""):
    recs, w = fc.truth(case)
    got = d.read_finegrid()
    assert got.tobytes() == want_bytes(recs), (case.name, label, [k for k, (a, b) in enumerate(zip(got.tolist(), recs)) if tuple(a) != b][:4])
    got_w = d.read_fine_onsets()
    assert got_w.dtype == np.uint32 and got_w.tobytes() == w.astype(np.uint32).tobytes(), (case.name, label, np.flatnonzero(got_w != w)[:4])


# ---- the records, weights and forms over the shared cases ----
@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: c.name)
def test_records_weights_and_forms_equal_the_model(case):
    d = loaded(fc.track(case))
    d.analyse_finegrid(c_settings(case.settings))
    forms = deck.debug_last_finegrid()
    assert_result(d, case)
    d.close()
    assert forms == fc.forms(case), case.name


def test_every_kernel_form_is_among_the_cases():
    total = {}
    for c in fc.CASES:
        for k, v in fc.forms(c).items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total
    # ... and the shapes inside them: phases at, one below and one above the lanes of a pass; three and four passes; more than one onset workgroup, whose halo hops lie
    # in a neighbour's tile; a last onset workgroup that is not full
    ph = sorted({fm.phases(c.settings.period0 + j * c.settings.dperiod) for c in fc.CASES for j in range(c.settings.n_periods)})
    assert {abi.DECK_FINEGRID_LANES, abi.DECK_FINEGRID_LANES + 1} <= set(ph) and any(2 * abi.DECK_FINEGRID_LANES < p <= 3 * abi.DECK_FINEGRID_LANES for p in ph) \
        and any(p > 3 * abi.DECK_FINEGRID_LANES for p in ph)
    assert any(fc.forms(c)["wgs_onset"] > 1 and fm.count(len(fc.track(c)), c.settings.hop) % 256 for c in fc.CASES)


def test_a_track_loaded_in_pieces_gives_the_same_result():
    case = fc.BY_NAME["an irregular fractional period"]
    d = loaded(fc.track(case), pieces=[(7000, 9000), (0, 33), (33, 7000)])
    d.analyse_finegrid(c_settings(case.settings))
    assert_result(d, case)
    d.close()


def test_a_second_and_third_analysis_and_windows():
    """h = 64 first (N = 313), then h = 16 on the same deck (N = 1250: the buffer grows), then h = 64 again (kept), then other settings at the same hop"""
    tr = fc.bumpy(20000, "second analysis", 700)
    small, big, other = fm.Settings(64, 4, 9 * fm.Q16 + 5, 3001), fm.Settings(16, 7, 30 * fm.Q16 + 77, 999, first_hop=3), fm.Settings(64, 2, 5 * fm.Q16, 40000, max_beats=9)
    want = {s: fm.analyse(tr, s) for s in (small, big, other)}
    d = loaded(tr)

    def same(s, label):
        recs, w = want[s]
        assert d.read_finegrid().tobytes() == want_bytes(recs) and np.array_equal(d.read_fine_onsets(), w), label

    d.analyse_finegrid(c_settings(small)); same(small, "first")
    d.analyse_finegrid(c_settings(big)); same(big, "grown")
    recs, w = want[big]
    for at, cnt in ((0, 1), (2, 4), (6, 1), (7, 0), (1, 6)):
        assert d.read_finegrid(at, cnt).tobytes() == want_bytes(recs[at:at + cnt]), (at, cnt)
    n = len(w)
    for at, cnt in ((0, 1), (255, 3), (n - 1, 1), (n, 0), (700, n - 700)):
        assert np.array_equal(d.read_fine_onsets(at, cnt), w[at:at + cnt]), (at, cnt)
    d.analyse_finegrid(hop=small.hop, n_periods=small.n_periods, period0_q16=small.period0, dperiod_q16=small.dperiod); same(small, "kept")   # by keywords
    d.analyse_finegrid(c_settings(other)); same(other, "other settings")
    d.load(np.zeros((100, 2), np.int16), 50)                # a later load does not invalidate the snapshot
    same(other, "after a load")
    d.analyse_finegrid(c_settings(other))                   # ... and a new analysis sees it
    recs, w = fm.analyse(np.concatenate([tr[:50], np.zeros((100, 2), np.int16), tr[150:]]), other)
    assert d.read_finegrid().tobytes() == want_bytes(recs) and np.array_equal(d.read_fine_onsets(), w)
    d.close()


def test_refusals_leave_the_previous_result_and_the_deck_usable():
    case = fc.BY_NAME["first_hop 37"]

    def refused(fn):
        with pytest.raises(abi.MxError) as err:
            fn()
        assert err.value.code == abi.MX_ERR_INVALID, err.value

    d = loaded(fc.track(case))
    refused(lambda: d.read_finegrid(0, 1))      # no analysis yet
    refused(lambda: d.read_fine_onsets(0, 1))
    d.analyse_finegrid(c_settings(case.settings))
    N = fm.count(len(fc.track(case)), case.settings.hop)
    for field, value in (("hop", 8), ("hop", 96), ("n_periods", 0), ("n_periods", 8193), ("dperiod_q16", 0), ("period0_q16", fm.PERIOD_MIN - 1), ("period0_q16", fm.PERIOD_MAX),
                         ("first_hop", N), ("max_beats", 1), ("_pad", 1)):
        bad = c_settings(case.settings)
        setattr(bad, field, value)
        refused(lambda: d.analyse_finegrid(bad))
        assert_result(d, case, f"after a refused {field}")
    for call in (lambda: d.analyse_finegrid(), lambda: d.analyse_finegrid(c_settings(case.settings), hop=16), lambda: d.analyse_finegrid(None, hop=16)):
        with pytest.raises(TypeError):          # neither settings nor keywords, or both: there are no defaults, and a bare call does not free the result
            call()
        assert_result(d, case, "after a call without or with too many arguments")
    refused(lambda: d.read_finegrid(0, 7))      # windows past the end
    refused(lambda: d.read_finegrid(7, 0))
    refused(lambda: d.read_fine_onsets(1, N))
    refused(lambda: d.read_fine_onsets(N + 1, 0))
    buf = np.zeros(6, abi.DECK_COMB_DTYPE)
    assert abi.lib.mx_deck_read_finegrid(d._h, 0, 6, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_fine_onsets(d._h, 0, 6, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_finegrid(None, 0, 6, buf.ctypes.data_as(C.c_void_p)) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_analyse_finegrid(None, C.byref(c_settings(case.settings))) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_finegrid(d._h, 0, 6, buf.ctypes.data_as(C.c_void_p)) == abi.MX_OK and buf.tobytes() == want_bytes(fc.truth(case)[0])
    refused(lambda: d.read_columns(0, 1))       # the other analyses were never made on this deck
    d.analyse_finegrid(None)                    # NULL frees
    refused(lambda: d.read_finegrid(0, 1))
    refused(lambda: d.read_fine_onsets(0, 1))
    d.analyse_finegrid(None)
    d.analyse_finegrid(c_settings(case.settings))
    assert_result(d, case, "analysed again")
    d.close()


def test_the_four_analyses_back_to_back_on_one_deck_and_a_second_deck_beside_it():
    """no read between the analyses: one stream orders them, and the four results do not share memory"""
    t = lk.TON_BY_NAME["20 hops of noise, G = 7: a short last segment"]
    tr = lk.track(t)
    l = lk.LOUD_BY_NAME["noise, 1000 frames"]._replace(name=t.name, n_frames=t.n_frames)   # (a noise track is seeded by its name and length)
    a = ac.BY_NAME["noise, 10 000 frames at C = 64"]
    f = fm.Settings(16, 9, 11 * fm.Q16 + 9, 777, first_hop=2)
    want_cols, want_R = am.analyse(tr, a.settings)
    want_recs, want_w = fm.analyse(tr, f)
    other = fc.BY_NAME["256 and 257 phases"]
    d, d2 = loaded(tr), loaded(fc.track(other))
    d.analyse_finegrid(c_settings(f)); d.analyse_tonality(lk.c_tonality(t)); d2.analyse_finegrid(c_settings(other.settings))
    d.analyse(deck.analysis(a.settings.column, a.settings.max_lag, a.settings.lo, a.settings.hi)); d.analyse_loudness(lk.c_loudness(l))
    assert_result(d2, other, "deck 2")
    assert lm.records_equal(d.read_loudness(), lk.loud_records(l))
    assert d.read_columns().tobytes() == want_cols.tobytes() and np.array_equal(d.read_autocorr(), want_R)
    assert b"".join(r["raw"] for r in d.read_tonality()) == b"".join(lk.ton_records(t))
    assert d.read_finegrid().tobytes() == want_bytes(want_recs) and np.array_equal(d.read_fine_onsets(), want_w)
    d.close(); d2.close()


@pytest.mark.parametrize("clicks,case", fc.CLICK_CASES[:2], ids=lambda v: getattr(v, "name", None))
def test_refine_grid_equals_the_models_two_stages(clicks, case):
    tr = fc.track(case)
    want, _one, two = fm.refine(tr, fc.coarse_columns(clicks), fc.COLUMN, fc.RATE, clicks.hop)
    d = loaded(tr)
    p = d.refine_grid(abi.DeckGrid(0.0, fc.coarse_columns(clicks), 0.0, 0, 0, 0), fc.COLUMN, fc.RATE, clicks.hop)
    assert fm.Pick(fm.Beats(p.grid.first_q32, p.grid.period_q32), p.score, p.bpm, p.index, p.n_beats) == want
    assert d.read_finegrid().tobytes() == want_bytes(fm.analyse(tr, two)[0])        # the deck holds stage two's records
    assert d.refine_grid(abi.DeckGrid(), fc.COLUMN, fc.RATE, clicks.hop).score == 0    # a grid without a period
    d.close()
    quiet = loaded(np.zeros((5000, 2), np.int16))
    assert quiet.refine_grid(abi.DeckGrid(0.0, 46.0, 0.0, 0, 0, 0), 512, fc.RATE).score == 0
    quiet.close()


def test_playing_is_untouched_by_fine_grid_calls_between_loads_and_feeds():
    """output bits, tick records and mx_deck_state of a deck fed into a small graph, with and without the new calls in between"""
    spt, n_ticks = 257, 4
    case = fc.BY_NAME["an irregular fractional period"]
    tr = fc.track(case)
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
            d.analyse_finegrid(c_settings(case.settings))
        d.load(tr[6000:], 6000)
        d.set(deck.params(step_q32=dc.frames(1.08), flags=abi.DECK_PLAY)); d.seek(dc.frames(100.5))
        out = []
        for _ in range(3):
            if with_calls:
                d.analyse_finegrid(c_settings(case.settings))
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


def test_the_synced_pair_plays_on_the_device_as_the_deck_model_says():
    pair = fc.sync_pair()
    step, seek, _delta = pair["sync"]
    tables = np.stack([deck.deck_tables(b) for b in range(4)])
    names = [f"click track {c.period} / {c.t0} / h {c.hop}" for c in (fc.SYNC_LEADER, fc.SYNC_FOLLOWER)]
    tracks = [fc.track(fc.BY_NAME[n]) for n in names]
    starts = [(dm.ONE, fc.SYNC_LEADER_POS), (step, seek)]
    want = []
    for tr, (st, pos) in zip(tracks, starts):
        m = dm.DeckModel(tr, tables)
        m.schedule(0, dm.Params(st, flags=dm.PLAY), pos)
        want.append(m.feed(fc.SYNC_TICKS, fc.SYNC_SPT)[0])
    ws = Workspace(*dc.rate_of(fc.SYNC_SPT))
    srcs = [ws.source_stereo(), ws.source_stereo()]
    mix = ws.mixer([(0.0, 1.0, False)] * 2)
    for k, s in enumerate(srcs):
        ws.connect(s, 0, mix, k)
    g = ws.build(max_ticks_per_run=fc.SYNC_FEED)
    decks = [loaded(tr) for tr in tracks]
    # the host's side of the story, on the device's own analyses: refine both, sync, schedule
    picks = [d.refine_grid(abi.DeckGrid(0.0, fc.coarse_columns(c), 0.0, 0, 0, 0), fc.COLUMN, fc.RATE, c.hop) for d, c in zip(decks, (fc.SYNC_LEADER, fc.SYNC_FOLLOWER))]
    assert deck.deck_sync(picks[0].grid, fc.SYNC_LEADER_POS, dm.ONE, picks[1].grid, fc.SYNC_FOLLOWER_POS)[:2] == (step, seek)
    for d, (st, pos) in zip(decks, starts):
        d.schedule(0, deck.params(step_q32=st, flags=abi.DECK_PLAY), pos)
    got = [[], []]
    for first in range(0, fc.SYNC_TICKS, fc.SYNC_FEED):
        deck.feed(decks, srcs, g, fc.SYNC_FEED)
        g.run_ticks(first, fc.SYNC_FEED)
        for k, s in enumerate(srcs):
            got[k].append(g.read_output(s, 0, fc.SYNC_FEED, True))
    for k in range(2):
        assert np.array_equal(np.concatenate(got[k]).view(np.uint32), want[k].view(np.uint32)), ("leader", "follower")[k]
    for d in decks:
        d.close()
    g.close()
