"""The deck's track analysis on the device (include/mixlab_gpu.h "ANALYSIS"): every column record and the autocorrelation mx_deck_analyse
leaves in device memory against the Python model (tests/deck_analysis_model.py), integer for integer, over the shared cases (tests/deck_analysis_cases.py); every
kernel form; loading in pieces; a second analysis; windows; the errors, each of which leaves deck and analysis as they were; and that playing is untouched."""
import numpy as np
import pytest

import deck_analysis_cases as ac
import deck_analysis_model as am
import deck_cases as dc
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu


def c_settings(s):
    return deck.analysis(s.column, s.max_lag, s.lo, s.hi)


def analysed(case, pieces=None):
    """the case on the device: (columns, R, debug counts)"""
    tr = ac.track(case)
    d = deck.Deck(tr.shape[0])
    if pieces is None:
        d.load(tr)
    else:
        for a, b in pieces:
            d.load(tr[a:b], a)
    d.analyse(c_settings(case.settings))
    counts = deck.debug_last_analysis()
    cols, R = d.read_columns(), d.read_autocorr()
    d.close()
    return cols, R, counts


def assert_records(got, want, label):
    for name in want.dtype.names:
        if not np.array_equal(got[name], want[name]):
            bad = np.flatnonzero((got[name] != want[name]).reshape(len(want), -1).any(axis=1))
            raise AssertionError(f"{label}: {name} differs in {bad.size} of {len(want)} columns, first {bad[0]}: got {got[name][bad[0]]}, want {want[name][bad[0]]}")
    assert got.tobytes() == want.tobytes(), label


@pytest.mark.parametrize("case", ac.CASES, ids=lambda c: c.name)
def test_columns_autocorrelation_and_counts_equal_the_model(case):
    cols, R, counts = analysed(case)
    want_cols, want_R, want_grid = ac.truth(case)
    assert len(cols) == len(want_cols) == deck.column_count(ac.track(case).shape[0], case.settings.column)
    assert_records(cols, want_cols, case.name)
    assert np.array_equal(R, want_R), (case.name, np.flatnonzero(R != want_R)[:4])
    assert counts == ac.forms(case), case.name
    g = deck.beatgrid(cols, R, case.settings.column, ac.RATE, ac.BPM_LO, ac.BPM_HI)
    got = np.array([g.bpm, g.period_columns, g.confidence]).view(np.uint64).tolist() + [g.first_beat_frame, g.lag, g.phase_column]
    assert got == np.array(want_grid[:3]).view(np.uint64).tolist() + list(want_grid[3:]), case.name


def test_every_kernel_form_ran():
    total = {}
    for name in ("noise, 10 000 frames at C = 64", "noise, 3 * 4096 + 17 frames at C = 4096", "noise, 5 frames under a 126-frame halo", "noise, 2500 frames at C = 1024"):
        for k, v in analysed(ac.BY_NAME[name])[2].items():
            total[k] = total.get(k, 0) + v
    assert all(v > 0 for v in total.values()), total
    assert total == {"wgs_several_columns": 10, "wgs_tiled_column": 4, "short_track": 1, "wgs_one_column": 3}


def test_a_track_loaded_in_pieces_gives_the_same_records():
    case = ac.BY_NAME["noise, 10 000 frames at C = 64"]
    cols, R, _ = analysed(case, pieces=[(7000, 10000), (0, 33), (33, 7000)])
    assert_records(cols, ac.truth(case)[0], "in pieces")
    assert np.array_equal(R, ac.truth(case)[1])


def test_a_second_analysis_replaces_the_first_and_windows_read_what_they_name():
    a, b = ac.BY_NAME["noise, 10 000 frames at C = 64"], ac.BY_NAME["noise, 3 * 4096 + 17 frames at C = 4096"]
    tr = ac.track(a)
    want, want_R, _ = ac.truth(a)
    s2 = b.settings                      # other settings over the same track: 3 wide columns, 16 lags
    cols2, R2 = am.analyse(tr, s2)
    d = deck.Deck(tr.shape[0])
    d.load(tr)
    d.analyse(c_settings(s2))
    assert_records(d.read_columns(), cols2, "first")
    assert np.array_equal(d.read_autocorr(), R2) and len(d.read_autocorr()) == s2.max_lag
    d.analyse(c_settings(a.settings))    # more columns: the buffer grows
    assert_records(d.read_columns(), want, "second")
    assert np.array_equal(d.read_autocorr(), want_R)
    for first, n in ((0, 1), (5, 7), (len(want) - 1, 1), (len(want), 0), (3, len(want) - 3)):
        assert_records(d.read_columns(first, n), want[first:first + n], f"window {first} + {n}")
    d.analyse(c_settings(s2))            # fewer again: the buffer is kept
    assert_records(d.read_columns(), cols2, "third")
    assert np.array_equal(d.read_autocorr(), R2)
    # a later load does not invalidate the snapshot
    d.load(np.zeros((100, 2), np.int16), 50)
    assert_records(d.read_columns(), cols2, "after a load")
    d.close()


def test_errors_leave_the_previous_analysis_and_the_deck_usable():
    case = ac.BY_NAME["noise, C + 1 frames"]
    tr = ac.track(case)
    want, want_R, _ = ac.truth(case)
    d = deck.Deck(tr.shape[0])
    d.load(tr)

    def refused(fn):
        with pytest.raises(abi.MxError) as err:
            fn()
        assert err.value.code == abi.MX_ERR_INVALID, err.value

    refused(lambda: d.read_columns(0, 1))            # no analysis yet
    refused(lambda: d.read_autocorr(1024))
    good = c_settings(case.settings)
    d.analyse(good)
    for field, value in (("column", 500), ("taps", 64), ("max_lag", 15), ("_pad", 1)):
        bad = c_settings(case.settings)
        setattr(bad, field, value)
        refused(lambda: d.analyse(bad))
        assert_records(d.read_columns(), want, f"after a refused {field}")
    refused(lambda: d.read_columns(0, len(want) + 1))     # a window past N
    refused(lambda: d.read_columns(len(want) + 1, 0))
    refused(lambda: d.read_autocorr(case.settings.max_lag - 1))   # a small cap
    assert np.array_equal(d.read_autocorr(1024), want_R)
    assert_records(d.read_columns(), want, "after the refused reads")
    d.analyse(None)                                        # NULL frees
    refused(lambda: d.read_columns(0, 1))
    refused(lambda: d.read_autocorr(1024))
    d.analyse(None)
    d.analyse(good)
    assert_records(d.read_columns(), want, "analysed again")
    d.close()


def test_two_decks_analysed_back_to_back_without_a_read_in_between():
    a, b = ac.BY_NAME["click track"], ac.BY_NAME["noise, 70 000 frames at max_lag 1024, C = 64"]
    da, db = deck.Deck(ac.track(a).shape[0]), deck.Deck(ac.track(b).shape[0])
    da.load(ac.track(a)); db.load(ac.track(b))
    da.analyse(c_settings(a.settings)); db.analyse(c_settings(b.settings))
    assert_records(db.read_columns(), ac.truth(b)[0], "deck b")
    assert_records(da.read_columns(), ac.truth(a)[0], "deck a")
    assert np.array_equal(da.read_autocorr(), ac.truth(a)[1]) and np.array_equal(db.read_autocorr(), ac.truth(b)[1])
    da.close(); db.close()


def test_playing_is_untouched_by_an_analysis_between_loads_and_feeds():
    """output bits, tick records and mx_deck_state of a deck fed into a small graph, with and without analyse calls in between"""
    spt, n_ticks = 257, 4
    case = ac.BY_NAME["noise, 10 000 frames at C = 64"]
    tr = ac.track(case)
    ws = Workspace(*dc.rate_of(spt))
    src = ws.source_stereo()
    mix = ws.mixer([(0.0, 1.0, False)])
    ws.connect(src, 0, mix, 0)
    g = ws.build(max_ticks_per_run=n_ticks)
    runs, clock = [], 0
    for with_analysis in (False, True):
        d = deck.Deck(tr.shape[0])
        d.load(tr[:6000])
        if with_analysis:
            d.analyse(c_settings(case.settings))
        d.load(tr[6000:], 6000)
        d.set(deck.params(step_q32=dc.frames(1.08), flags=abi.DECK_PLAY)); d.seek(dc.frames(100.5))
        out = []
        for _ in range(3):
            if with_analysis:
                d.analyse(c_settings(case.settings))
            deck.feed([d], [src], g, n_ticks)
            g.run_ticks(clock, n_ticks)
            clock += n_ticks
            h = d.state()
            out.append((g.read_output(src, 0, n_ticks, True).view(np.uint32).tolist(),
                        [(t.pos_q32, t.step_q32, t.dstep_q32, t.loop_in, t.loop_len, t.flags, t.bank) for t in d.read_ticks(0, n_ticks)],
                        (h.pos_q32, h.step_q32, h.params.step_q32, h.params.flags, h.last_looping)))
        if with_analysis:
            assert_records(d.read_columns(), ac.truth(case)[0], "the analysis beside the feeds")
        runs.append(out)
        d.close()
    assert runs[0] == runs[1]
    g.close()
