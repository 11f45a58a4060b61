"""The deck's four whole-track analyses as four objects on one deck (DESIGN.md section 0.17 "the shared protocol"): one track, one load stream.  All four queued back
to back and read in the reverse order; two of them freed beside two that stay; tonality analysed again with the tables it had and with others under a buffer that
stays (the table cache, and the wait that only new tables ask for); a refused setting on each; and mx_deck_debug_last_* of each against a lone analysis with the same
settings.  Every result is compared with what the analysis' own test compares it with: the models of the case modules, each run once."""
import numpy as np
import pytest

import deck_analysis_cases as ac
import deck_finegrid_model as fm
import deck_loudkey_cases as lk
import loudness_model as lm
from mixlab_amd import abi, deck

pytestmark = pytest.mark.gpu

A = ac.BY_NAME["noise, 10 000 frames at C = 64"]
N_FRAMES = 10000
# the smallest settings of the case modules: 2 octaves in segments of one hop (20 segments here); blocks of 64 frames (157); hops of 64 frames (157), 3 candidate periods
T = lk.TON_BY_NAME["20 hops of noise, G = 1"]._replace(n_frames=N_FRAMES)
T_SAME_TABLES = T._replace(G=2)                                # what shapes the tables stays: 10 segments
T_OTHER_TABLES = T._replace(G=2, O=3, f_lo_mhz=110000)         # other tables, and records that still fit the buffer of T: only the tables make the deck wait
L = lk.LOUD_BY_NAME["noise, 1000 frames"]._replace(n_frames=N_FRAMES)
F = fm.Settings(64, 3, round(21.7 * fm.Q16), 4000)


def c_columns():
    s = A.settings
    return deck.analysis(s.column, s.max_lag, s.lo, s.hi)


def c_finegrid():
    return deck.finegrid(F.hop, F.n_periods, F.period0, F.dperiod, F.first_hop, F.max_beats)


ANALYSES = {   # name: (analyse, the C settings, mx_deck_debug_last_* of it)
    "columns": (deck.Deck.analyse, c_columns, deck.debug_last_analysis),
    "tonality": (deck.Deck.analyse_tonality, lambda: lk.c_tonality(T), deck.debug_last_tonality),
    "loudness": (deck.Deck.analyse_loudness, lambda: lk.c_loudness(L), deck.debug_last_loudness),
    "finegrid": (deck.Deck.analyse_finegrid, c_finegrid, deck.debug_last_finegrid),
}


def refused(fn):
    with pytest.raises(abi.MxError) as err:
        fn()
    assert err.value.code == abi.MX_ERR_INVALID, err.value


def lone_counts(tr, analyse, settings, debug_last) -> dict:
    """mx_deck_debug_last_* after this one analysis on a deck of its own"""
    d = deck.Deck(len(tr))
    d.load(tr)
    analyse(d, settings)
    out = debug_last()
    d.close()
    return out


def test_four_analyses_share_one_deck():
    tr = ac.track(A)
    assert len(tr) == N_FRAMES
    want_cols, want_R, _ = ac.truth(A)
    want_ton = {c: b"".join(lk.ton_records(c, tr=tr)) for c in (T, T_SAME_TABLES, T_OTHER_TABLES)}
    want_loud = lk.loud_records(L, tr=tr)
    fine_recs, want_w = fm.analyse(tr, F)
    want_fine = np.array(fine_recs, abi.DECK_COMB_DTYPE).tobytes()
    lone = {name: lone_counts(tr, analyse, settings(), debug_last) for name, (analyse, settings, debug_last) in ANALYSES.items()}
    lone_other_tables = lone_counts(tr, deck.Deck.analyse_tonality, lk.c_tonality(T_OTHER_TABLES), deck.debug_last_tonality)
    assert lone["tonality"] == lk.ton_forms(T) and lone_other_tables == lk.ton_forms(T_OTHER_TABLES) and lone["tonality"] != lone_other_tables

    def columns_are(d, label):
        assert d.read_autocorr().tobytes() == want_R.tobytes(), label
        assert d.read_columns().tobytes() == want_cols.tobytes(), label

    def tonality_is(d, case, label):
        assert b"".join(r["raw"] for r in d.read_tonality()) == want_ton[case], label

    def loudness_is(d, label):
        got = d.read_loudness()
        assert len(got) == len(want_loud) and lm.records_equal(got, want_loud), (label, lm.first_difference(got, want_loud))

    def finegrid_is(d, label):
        assert d.read_fine_onsets().tobytes() == want_w.astype(np.uint32).tobytes(), label
        assert d.read_finegrid().tobytes() == want_fine, label

    d = deck.Deck(N_FRAMES)
    d.load(tr)

    # all four queued back to back, read in the reverse order
    for analyse, settings, _ in ANALYSES.values():
        analyse(d, settings())
    finegrid_is(d, "back to back"); loudness_is(d, "back to back"); tonality_is(d, T, "back to back"); columns_are(d, "back to back")
    assert {name: debug_last() for name, (_, _, debug_last) in ANALYSES.items()} == lone

    # two freed beside two that stay
    d.analyse_tonality(None); d.analyse(None)
    loudness_is(d, "beside two freed"); finegrid_is(d, "beside two freed")
    refused(lambda: d.read_tonality(0, 1)); refused(lambda: d.read_columns(0, 1)); refused(lambda: d.read_autocorr(1024))

    # tonality again: new tables after the free, then the same tables for other segments, then other tables under a buffer that stays
    d.analyse_tonality(lk.c_tonality(T))
    d.analyse_tonality(lk.c_tonality(T_SAME_TABLES))
    tonality_is(d, T_SAME_TABLES, "the tables kept")
    d.analyse_tonality(lk.c_tonality(T_OTHER_TABLES))
    tonality_is(d, T_OTHER_TABLES, "other tables")
    loudness_is(d, "beside tonality again"); finegrid_is(d, "beside tonality again")
    refused(lambda: d.read_columns(0, 1))
    d.analyse(c_columns())
    columns_are(d, "analysed again")

    # a refused setting on any one leaves all four as they were
    for name, (analyse, settings, _) in ANALYSES.items():
        bad = settings()
        bad._pad = 1
        refused(lambda: analyse(d, bad))
        label = f"after {name} refused _pad = 1"
        columns_are(d, label); tonality_is(d, T_OTHER_TABLES, label); loudness_is(d, label); finegrid_is(d, label)

    assert {name: debug_last() for name, (_, _, debug_last) in ANALYSES.items()} == dict(lone, tonality=lone_other_tables)
    d.close()
