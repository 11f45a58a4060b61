"""The deck's whole-track tonality and loudness on the device (include/mixlab_gpu.h "KEY AND LOUDNESS"): every record mx_deck_analyse_tonality
and mx_deck_analyse_loudness leave in device memory against the TAPS' models (tests/tonality_model.py, tests/loudness_model.py) over the shared cases
(tests/deck_loudkey_cases.py), byte for byte; every kernel form; loading in pieces; a second analysis; windows; the refusals, each of which leaves deck and results
as they were; the three analyses of a deck back to back; two decks; that playing is untouched; and the two cross-checks that tie the pass to the taps themselves:
a deck played at unity into a graph whose loudness / tonality tap reads the same records."""
import ctypes as C

import numpy as np
import pytest

import deck_analysis_cases as ac
import deck_analysis_model as am
import deck_cases as dc
import deck_loudkey_cases as lk
import loudness_model as lm
from mixlab_amd import abi, deck
from mixlab_amd.workspace import Workspace

pytestmark = pytest.mark.gpu


def raw(recs) -> bytes:
    return b"".join(r["raw"] for r in recs)


def loaded(tr, pieces=None):
    d = deck.Deck(tr.shape[0])
    if pieces is None:
        d.load(tr)
    else:
        for a, b in pieces:
            d.load(tr[a:b], a)
    return d


def assert_loud(got, want, label):
    assert len(got) == len(want), label
    assert lm.records_equal(got, want), (label, lm.first_difference(got, want))


# ---- the records, counts and forms over the shared cases ----
@pytest.mark.parametrize("case", lk.TON_CASES, ids=lambda c: c.name)
def test_tonality_records_counts_and_forms_equal_the_model(case):
    d = loaded(lk.track(case))
    d.analyse_tonality(lk.c_tonality(case))
    forms = deck.debug_last_tonality()
    recs = d.read_tonality()
    d.close()
    assert len(recs) == lk.ton_segments(case) == deck.tonality_count(case.n_frames, lk.c_tonality(case))
    want = lk.ton_truth(case)
    rb = 32 + 96 * case.O
    for g, r in enumerate(recs):
        assert r["raw"] == want[g * rb:(g + 1) * rb], (case.name, g, r["hops"], np.flatnonzero(r["cq"] != np.frombuffer(want, "<u8", 12 * case.O, g * rb + 32))[:4])
    assert forms == lk.ton_forms(case), case.name


@pytest.mark.parametrize("case", lk.LOUD_CASES, ids=lambda c: c.name)
def test_loudness_records_counts_and_forms_equal_the_model(case):
    d = loaded(lk.track(case))
    d.analyse_loudness(lk.c_loudness(case))
    forms = deck.debug_last_loudness()
    recs = d.read_loudness()
    d.close()
    assert len(recs) == lk.loud_blocks(case) == deck.loudness_count(case.n_frames, case.F)
    assert_loud(recs, lk.loud_truth(case), case.name)
    assert forms == lk.loud_forms(case), case.name


def test_every_kernel_form_is_among_the_cases():
    for forms, cases in ((lk.ton_forms, lk.TON_CASES), (lk.loud_forms, lk.LOUD_CASES)):
        total = {}
        for c in cases:
            for k, v in forms(c).items():
                total[k] = total.get(k, 0) + v
        assert all(v > 0 for v in total.values()), total
    # ... and the shapes inside them: a segment of fewer, exactly and more than 8 hops; a peak wave that straddles two blocks (an F that is no multiple of 64) and
    # one that does not; a walk workgroup of fewer than 32 blocks and more than one of them
    assert {c.G % 8 == 0 for c in lk.TON_CASES} == {True, False} and any(c.G > 8 and c.G % 8 for c in lk.TON_CASES)
    assert any(c.F % 64 for c in lk.LOUD_CASES) and any(lk.loud_blocks(c) > 64 for c in lk.LOUD_CASES)


def test_a_track_loaded_in_pieces_gives_the_same_records():
    t, l = lk.TON_BY_NAME["20 hops of noise, G = 7: a short last segment"], lk.LOUD_BY_NAME["71 blocks: 64 * 70 + 5 frames"]
    d = loaded(lk.track(t), pieces=[(7000, 10240), (0, 33), (33, 7000)])
    d.analyse_tonality(lk.c_tonality(t))
    assert raw(d.read_tonality()) == lk.ton_truth(t)
    d.close()
    d = loaded(lk.track(l), pieces=[(3000, l.n_frames), (0, 65), (65, 3000)])
    d.analyse_loudness(lk.c_loudness(l))
    assert_loud(d.read_loudness(), lk.loud_truth(l), "in pieces")
    d.close()


def test_a_second_analysis_replaces_the_first_and_windows_read_what_they_name():
    # tonality: one record (small), then twenty (the buffer grows), then one again (kept); the settings of the tables stay, then change
    small, big = lk.TON_BY_NAME["20 hops of noise, G = 65536: one record"], lk.TON_BY_NAME["20 hops of noise, G = 1"]
    tr = lk.track(big)
    third = small._replace(name="other tables", O=3, f_lo_mhz=110000, G=5)
    want_third = b"".join(lk.ton_records(third._replace(name=big.name)))   # (the track is seeded by the name)
    d = loaded(tr)
    d.analyse_tonality(lk.c_tonality(big._replace(G=4)))   # 5 records
    first = raw(d.read_tonality())
    assert first == b"".join(lk.ton_records(big._replace(G=4)))
    d.analyse_tonality(lk.c_tonality(big))                 # 20
    assert raw(d.read_tonality()) == lk.ton_truth(big)
    rb, n = 224, 20
    for at, cnt in ((0, 1), (5, 7), (n - 1, 1), (n, 0), (3, n - 3)):
        assert raw(d.read_tonality(at, cnt)) == lk.ton_truth(big)[at * rb:(at + cnt) * rb], (at, cnt)
    d.analyse_tonality(lk.c_tonality(big._replace(G=4)))   # fewer again: the buffer is kept
    assert raw(d.read_tonality()) == first
    d.analyse_tonality(lk.c_tonality(third))               # other kernels: a new table set
    assert raw(d.read_tonality()) == want_third
    d.load(np.zeros((100, 2), np.int16), 50)                # a later load does not invalidate the snapshot
    assert raw(d.read_tonality()) == want_third
    d.close()
    # loudness: 3 blocks of 512 frames, then 23 of 64, then 3 again
    few, many = lk.LOUD_BY_NAME["noise, 1000 frames"]._replace(F=512), lk.LOUD_BY_NAME["noise, 1000 frames"]._replace(F=64, n_frames=1450)
    tr = lk.track(many)
    want_few = lk.loud_records(few._replace(n_frames=1450))
    want_many = lk.loud_records(many)
    d = loaded(tr)
    d.analyse_loudness(lk.c_loudness(few))
    assert_loud(d.read_loudness(), want_few, "first")
    d.analyse_loudness(lk.c_loudness(many))
    assert_loud(d.read_loudness(), want_many, "second")
    n = len(want_many)
    for at, cnt in ((0, 1), (5, 7), (n - 1, 1), (n, 0), (3, n - 3)):
        assert_loud(d.read_loudness(at, cnt), want_many[at:at + cnt], f"window {at} + {cnt}")
    d.analyse_loudness(lk.c_loudness(few))
    assert_loud(d.read_loudness(), want_few, "third")
    d.load(np.zeros((100, 2), np.int16), 50)
    assert_loud(d.read_loudness(), want_few, "after a load")
    d.close()


def test_refusals_leave_the_previous_result_and_the_deck_usable():
    t, l = lk.TON_BY_NAME["F + 1 frames, G = 3"], lk.LOUD_BY_NAME["65 frames"]
    tr_t, tr_l = lk.track(t), lk.track(l)

    def refused(fn):
        with pytest.raises(abi.MxError) as err:
            fn()
        assert err.value.code == abi.MX_ERR_INVALID, err.value

    d = loaded(tr_t)
    refused(lambda: d.read_tonality(0, 1))     # no analysis yet
    refused(lambda: d.read_loudness(0, 1))
    d.analyse_tonality(lk.c_tonality(t))
    want = lk.ton_truth(t)
    for field, value in (("decim", 5), ("hop_frames", 100), ("octaves", 7), ("f_lo_mhz", 0), ("f_lo_mhz", 440000), ("f_lo_mhz", 16000), ("segment_hops", 0),
                         ("segment_hops", 65537), ("rate", float("nan")), ("rate", 0.0), ("_pad", 1)):
        bad = lk.c_tonality(t)
        setattr(bad, field, value)
        refused(lambda: d.analyse_tonality(bad))
        assert raw(d.read_tonality()) == want, field
    refused(lambda: d.read_tonality(0, 3))     # a window past n_seg
    refused(lambda: d.read_tonality(3, 0))
    buf = np.zeros(448, np.uint8)
    assert abi.lib.mx_deck_read_tonality(d._h, 0, 2, buf.ctypes.data_as(C.c_void_p), 447) == abi.MX_ERR_INVALID   # a cap too small
    assert abi.lib.mx_deck_read_tonality(d._h, 0, 2, None, 448) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_tonality(None, 0, 2, buf.ctypes.data_as(C.c_void_p), 448) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_tonality(d._h, 0, 2, buf.ctypes.data_as(C.c_void_p), 448) == abi.MX_OK and buf.tobytes() == want
    d.analyse_tonality(None)                   # NULL frees
    refused(lambda: d.read_tonality(0, 1))
    d.analyse_tonality(None)
    d.analyse_tonality(lk.c_tonality(t))
    assert raw(d.read_tonality()) == want
    d.close()

    d = loaded(tr_l)
    d.analyse_loudness(lk.c_loudness(l))
    want = lk.loud_truth(l)
    for field, value in (("block_frames", 63), ("block_frames", 65537), ("momentary_blocks", 0), ("momentary_blocks", 1025), ("short_blocks", 0),
                         ("short_blocks", 1025), ("rate", 3000.0), ("rate", float("inf")), ("_pad", 1)):
        bad = lk.c_loudness(l)
        setattr(bad, field, value)
        refused(lambda: d.analyse_loudness(bad))
        assert_loud(d.read_loudness(), want, f"after a refused {field}")
    refused(lambda: d.read_loudness(0, 3))
    refused(lambda: d.read_loudness(3, 0))
    assert abi.lib.mx_deck_read_loudness(d._h, 0, 2, None) == abi.MX_ERR_INVALID
    assert abi.lib.mx_deck_read_loudness(None, 0, 2, None) == abi.MX_ERR_INVALID
    refused(lambda: d.read_tonality(0, 1))     # the other analysis was never made on this deck
    d.analyse_loudness(None)
    refused(lambda: d.read_loudness(0, 1))
    d.analyse_loudness(None)
    d.analyse_loudness(lk.c_loudness(l))
    assert_loud(d.read_loudness(), want, "analysed again")
    d.close()


def test_the_three_analyses_back_to_back_on_one_deck_and_two_decks():
    """no read between the analyses: one stream orders them, and the three results do not share memory"""
    t = lk.TON_BY_NAME["20 hops of noise, G = 7: a short last segment"]
    tr = lk.track(t)
    l = lk.LOUD_BY_NAME["noise, 1000 frames"]._replace(name=t.name, n_frames=t.n_frames)   # (a noise track is seeded by its name and length)
    a = ac.BY_NAME["noise, 10 000 frames at C = 64"]
    want_cols, want_R = am.analyse(tr, a.settings)
    t2, l2 = lk.TON_BY_NAME["odd negative s throughout"], lk.LOUD_BY_NAME["F = 4800 over 3.5 blocks"]
    d, d2, d3 = loaded(tr), loaded(lk.track(t2)), loaded(lk.track(l2))
    d.analyse_tonality(lk.c_tonality(t)); d.analyse(deck.analysis(a.settings.column, a.settings.max_lag, a.settings.lo, a.settings.hi)); d.analyse_loudness(lk.c_loudness(l))
    d2.analyse_tonality(lk.c_tonality(t2)); d3.analyse_loudness(lk.c_loudness(l2))
    assert_loud(d3.read_loudness(), lk.loud_truth(l2), "deck 3")
    assert raw(d2.read_tonality()) == lk.ton_truth(t2)
    assert_loud(d.read_loudness(), lk.loud_records(l), "deck 1")
    assert d.read_columns().tobytes() == want_cols.tobytes() and np.array_equal(d.read_autocorr(), want_R)
    assert raw(d.read_tonality()) == b"".join(lk.ton_records(t))
    k, conf, name = d.key(t.rate)
    assert (k, conf) == abi.tonality_key(abi.tonality_chroma(lk.ton_records(t), t.rate)) and name == (deck.camelot(k) if k >= 0 else "")
    for x in (d, d2, d3):
        x.close()


def test_playing_is_untouched_by_the_new_calls_between_loads_and_feeds():
    """output bits, tick records and mx_deck_state of a deck fed into a small graph, with and without the new calls in between"""
    spt, n_ticks = 257, 4
    t = lk.TON_BY_NAME["20 hops of noise, G = 7: a short last segment"]
    l = lk.LOUD_BY_NAME["noise, 1000 frames"]._replace(name=t.name, n_frames=t.n_frames)
    tr = lk.track(t)
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
            d.analyse_tonality(lk.c_tonality(t)); d.analyse_loudness(lk.c_loudness(l))
        d.load(tr[6000:], 6000)
        d.set(deck.params(step_q32=dc.frames(1.08), flags=abi.DECK_PLAY)); d.seek(dc.frames(100.5))
        out = []
        for _ in range(3):
            if with_calls:
                d.analyse_loudness(lk.c_loudness(l)); d.analyse_tonality(lk.c_tonality(t))
            deck.feed([d], [src], g, n_ticks)
            g.run_ticks(clock, n_ticks)
            clock += n_ticks
            h = d.state()
            out.append((g.read_output(src, 0, n_ticks, True).view(np.uint32).tolist(),
                        [(k.pos_q32, k.step_q32, k.dstep_q32, k.loop_in, k.loop_len, k.flags, k.bank) for k in d.read_ticks(0, n_ticks)],
                        (h.pos_q32, h.step_q32, h.params.step_q32, h.params.flags, h.last_looping)))
        if with_calls:
            assert raw(d.read_tonality()) == lk.ton_truth(t)
            assert_loud(d.read_loudness(), lk.loud_records(l), "beside the feeds")
        runs.append(out)
        d.close()
    assert runs[0] == runs[1]
    g.close()


# ---- the pass and the taps ----
def played_at_unity(tr, spt, n_ticks, set_taps, read_taps):
    """a deck at unity from frame 0 into a SOURCE_STEREO of a graph of spt frames per tick, run for n_ticks ticks in two runs of unequal length"""
    ws = Workspace(spt * 60, 60)
    src = ws.source_stereo()
    first = max(1, n_ticks // 3)
    g = ws.build(max_ticks_per_run=n_ticks)
    set_taps(g, src)
    d = loaded(tr)
    d.set(deck.params(step_q32=deck.ONE, flags=abi.DECK_PLAY))
    got, clock = [], 0
    for n in (first, n_ticks - first):
        if not n:
            continue
        deck.feed([d], [src], g, n)
        g.run_ticks(clock, n)
        clock += n
        got.append(read_taps(g, n))
    return d, g, got


@pytest.mark.parametrize("spt,n_frames", [(64, 64 * 70 + 5), (480, 480 * 9 + 17)])
def test_a_loudness_tap_on_the_deck_played_at_unity_reads_the_same_records(spt, n_frames):
    case = lk.LoudCase(f"tap cross-check at {spt}", n_frames, "noise", spt * 60.0, spt, 4, 30)
    tr, nb = lk.track(case), lk.loud_blocks(case)
    d, g, got = played_at_unity(tr, spt, nb, lambda g, src: g.set_loudness([(src, 0)], case.M, case.S), lambda g, n: g.read_loudness(0, n)[:, 0])
    tap = np.concatenate(got)
    d.analyse_loudness(lk.c_loudness(case))
    mine = d.read_loudness()
    assert len(tap) == len(mine) == nb
    assert_loud(mine, tap, "deck against tap")
    assert_loud(mine, lk.loud_records(case), "deck against model")
    d.close(); g.close()


def test_a_tonality_tap_on_the_deck_played_at_unity_emits_the_same_records():
    spt, n_seg = 512, 9
    case = lk.TonCase("tap cross-check", spt * n_seg, "noise", spt * 60.0, 4, 128, 2, 440000, 1)
    tr = lk.track(case)
    d, g, got = played_at_unity(tr, spt, n_seg, lambda g, src: g.set_tonality([(src, 0)], case.D, case.Hc, case.O, case.f_lo_mhz, 1),
                                lambda g, n: [e[0] for e in g.read_tonality()])
    tap = [r for run in got for r in run]
    d.analyse_tonality(lk.c_tonality(case))
    mine = d.read_tonality()
    assert len(tap) == len(mine) == n_seg
    for k, (a, b) in enumerate(zip(mine, tap)):
        assert a["raw"][4:] == b["raw"][4:], k     # word 0 is the segment here, the tick in its run there
        assert a["tick_in_run"] == k
    assert raw(mine) == b"".join(lk.ton_records(case))
    d.close(); g.close()
