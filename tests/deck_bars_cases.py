"""The shared cases of the deck's bars and phrases (tests/test_cpu_deck_bars.py, tests/test_gpu_deck_bars.py): a track, the settings, and the model's result, which is
computed once per case and shared.  Tracks are generated from seeds; nothing is read from disk.  No track is longer than 400 000 frames.

SECTION_TRACKS are the synthetic arrangements the rule was tried on: a kick on every beat, a snare on every bar's third beat, sections of 16 beats that add a high or a
mid layer, and a pick-up of a few beats that makes both true phases non-zero.  CASES are the smallest shapes at which the kernels can go wrong."""
from __future__ import annotations

import zlib
from typing import Callable, NamedTuple

import numpy as np

import deck_analysis_model as am
import deck_bars_model as bm
from deck_bars_model import Settings

RATE = 48000.0
ONE = 1 << 32
T63 = (tuple(am.band_taps(RATE, 200.0, 63)[0]), tuple(am.band_taps(RATE, 2500.0, 63)[0]))
T127 = (tuple(am.band_taps(RATE, 200.0, 127)[0]), tuple(am.band_taps(RATE, 2500.0, 127)[0]))
T9 = (tuple(am.band_taps(RATE, 1500.0, 9)[0]), tuple(am.band_taps(RATE, 6000.0, 9)[0]))


def _rng(name: str):
    return np.random.default_rng(zlib.crc32(name.encode()))


def q32(frames: float) -> int:
    return round(frames * ONE)


def noise(n: int, name: str, amp: int = 32767) -> np.ndarray:
    return _rng(name).integers(-amp - 1, amp + 1, (n, 2)).astype(np.int16)


def constant(n: int, value: int) -> np.ndarray:
    return np.full((n, 2), value, np.int16)


def bumpy(n: int, name: str, every: int) -> np.ndarray:
    """noise whose level changes every `every` frames: beat vectors that differ all along the track"""
    t = noise(n, name, 400).astype(np.int64)
    gain = _rng(name + " gain").integers(1, 60, n // every + 1)
    return (t * gain[np.arange(n) // every][:, None]).astype(np.int16)


# ---- the section tracks ----
class Section(NamedTuple):
    period: float      # frames
    pickup: int        # beats before the first section
    first: int         # the first beat's frame
    types: str         # the sections' layers in turn: A none, B a high layer on the second half-beat, C a mid layer
    lead: int
    sections: int = 6
    sec_beats: int = 16

    @property
    def name(self):
        return f"sections {self.period} / pick-up {self.pickup} / {self.types}"


SECTION_TRACKS = [Section(2400.3, 2, 1000, "ABC", 128), Section(2217.7, 5, 3000, "ABAC", 128), Section(3001.5, 11, 700, "ABC", 64), Section(2400.3, 2, 1000, "AB", 0),
                  Section(2400.3, 7, 5000, "ABC", 128)]
END_TO_END = Section(2400.3, 3, 1500, "ABC", 128, sections=4)   # the track of the end-to-end tests: 67 beats, 162 000 frames


def section_track(c: Section) -> np.ndarray:
    rng = _rng(c.name)
    nb = c.pickup + c.sections * c.sec_beats + 3
    n = int(c.first + nb * c.period) + 500
    L = np.zeros(n)
    t = np.arange(300)
    kick = 12000 * np.sin(2 * np.pi * 150 * t / RATE) * np.exp(-t / 120)
    half, full = int(c.period // 2), int(c.period)
    for k in range(nb):
        s = int(round(c.first + k * c.period))
        L[s:s + 300] += kick
        sec = (k - c.pickup) // c.sec_beats if k >= c.pickup else -1
        ty = c.types[sec % len(c.types)] if 0 <= sec < c.sections else "A"
        if ty == "B":
            L[s + half:s + full] += rng.integers(-3000, 3001, full - half) * np.where(np.arange(full - half) % 2, 1, -1)
        if ty == "C":
            L[s:s + full] += 4000 * np.sin(2 * np.pi * 1000 * np.arange(full) / RATE)
        if k >= c.pickup and (k - c.pickup) % 4 == 2:
            L[s:s + 200] += rng.integers(-6000, 6001, 200)
    L += rng.integers(-50, 51, n)
    x = np.clip(np.rint(L), -32768, 32767).astype(np.int16)
    return np.stack([x, x], axis=1)


def section_settings(c: Section) -> Settings:
    """the constructed grid itself, with the header's recommended tables and M = 4, Q = 4, W = 4 and 8"""
    return Settings(c.first * ONE, int(c.period * ONE), *T63, lead=c.lead)


def section_truth(c: Section, n0: int):
    """(bar phase, phrase phase) as constructed, for a grid whose beat 0 is the grid's line n0 and whose line 0 is the track's first beat"""
    return (c.pickup - n0) % 4, (c.pickup - n0) % 16


def downbeat_frames(c: Section) -> list[float]:
    nb = c.pickup + c.sections * c.sec_beats
    return [c.first + k * c.period for k in range(c.pickup, nb, 4)]


# ---- the shapes ----
class Case(NamedTuple):
    name: str
    build: Callable[[], np.ndarray]
    settings: Settings


def _exact_end(period: int, n_beats: int, lead: int) -> int:
    """the frame at which beat n_beats - 1 of a grid with first_q32 = lead 2^32 ends"""
    return ((lead * ONE + n_beats * period) >> 32) - lead


P5000 = q32(5000.7)
CASES = [
    Case("period exactly 2048: every half one tile", lambda: bumpy(2048 * 21 + 700, "p2048", 1500), Settings(300 * ONE, 2048 * ONE, *T63)),
    Case("period 2049.37: every half a tile and a frame or two", lambda: bumpy(2049 * 22, "p2049", 1700), Settings(q32(150.25), q32(2049.37), *T63)),
    Case("period 5000.7: several tiles a half, odd beats", lambda: bumpy(5001 * 19, "p5000", 2100), Settings(q32(700.5), P5000, *T63, w_bar=2, w_phrase=3)),
    Case("K = 1", lambda: bumpy(2300 * 14, "k1", 900), Settings(q32(555.5), q32(2300.01), w_bar=2, w_phrase=5)),
    Case("K = 127, lead 0, a line on frame 0 and the last beat ending exactly at n_frames: the halo reaches before the track and past it",
         lambda: noise(_exact_end(q32(2100.6), 13, 0), "k127", 20000), Settings(0, q32(2100.6), *T127, lead=0, w_bar=2, w_phrase=3)),
    Case("the last beat one frame short of n_frames' reach", lambda: noise(_exact_end(q32(2100.6), 13, 0) - 1, "k127", 20000),
         Settings(0, q32(2100.6), *T127, lead=0, w_bar=2, w_phrase=3)),
    Case("lead 4096", lambda: bumpy(2500 * 17, "lead4096", 1300), Settings(q32(5000.0), q32(2500.5), *T9, lead=4096, w_bar=3, w_phrase=4)),
    Case("a negative first_q32", lambda: bumpy(2222 * 18, "negative", 1000), Settings(-q32(7 * 2222.4 + 900.0), q32(2222.4), *T9, M=4, Q=2)),
    Case("first_q32 several periods into the track: n0 < 0", lambda: bumpy(2222 * 18, "into", 1000), Settings(q32(5 * 2222.4 + 1300.0), q32(2222.4), *T9, M=4, Q=2)),
    Case("max_beats cutting the track", lambda: bumpy(2100 * 30, "cut", 1900), Settings(q32(400.0), q32(2100.25), *T9, max_beats=13)),
    Case("W = 1 and W = 64 over 141 beats", lambda: bumpy(2048 * 141 + 512, "w64", 5000), Settings(q32(300.0), 2048 * ONE + 12345, w_bar=1, w_phrase=64)),
    Case("2 W above n_beats: every N is 0 and the pick all zero", lambda: bumpy(2100 * 9, "few", 700), Settings(q32(300.0), q32(2100.5), *T9, w_bar=5, w_phrase=8)),
    Case("M = 3, Q = 1", lambda: bumpy(2100 * 25, "waltz", 1500), Settings(q32(300.0), q32(2100.5), *T9, M=3, Q=1, w_bar=3, w_phrase=3)),
    Case("M = 8, Q = 16", lambda: bumpy(2048 * 140, "long phrases", 3000), Settings(q32(300.0), q32(2048.9), *T9, M=8, Q=16, w_bar=8, w_phrase=32)),
    Case("a noise track", lambda: noise(2400 * 20, "noise"), Settings(q32(100.0), q32(2400.3), *T63)),
    Case("a constant track", lambda: constant(2400 * 20, -32768), Settings(q32(100.0), q32(2400.3), *T63)),
    Case("the best phrase phase of all lies off the bar phase", lambda: bumpy(2100 * 40, "off the bar 0", 1234), Settings(q32(300.0), q32(2100.5), *T9, M=4, Q=2, w_bar=2, w_phrase=3)),
] + [Case(c.name, (lambda c=c: section_track(c)), section_settings(c)) for c in SECTION_TRACKS]
BY_NAME = {c.name: c for c in CASES}
SECTION_CASES = [(c, BY_NAME[c.name]) for c in SECTION_TRACKS]

# the case whose compared values each misreading of the model changes
MISREADING_CASE = {
    "half_rounded_up": "period 5000.7: several tiles a half, odd beats",
    "lead_added": "lead 4096",
    "n0_strict": "K = 127, lead 0, a line on frame 0 and the last beat ending exactly at n_frames: the halo reaches before the track and past it",
    "partial_last_beat": "K = 1",
    "unordered_within": "M = 3, Q = 1",
    "phrase_free_of_bar": "the best phrase phase of all lies off the bar phase",
    "novelty_one_further": "period 2049.37: every half a tile and a frame or two",
    "fold_by_grid_index": "first_q32 several periods into the track: n0 < 0",
}

_tracks, _truth = {}, {}


def track(case: Case) -> np.ndarray:
    if case.name not in _tracks:
        _tracks[case.name] = case.build()
        _tracks[case.name].setflags(write=False)
    return _tracks[case.name]


def truth(case: Case):
    """(records as bm.BEAT_DTYPE[n_beats], the folds as a list, n0) of the model, computed once"""
    if case.name not in _truth:
        recs, H, n0 = bm.analyse(track(case), case.settings)
        recs.setflags(write=False)
        _truth[case.name] = (recs, tuple(H), n0)
    return _truth[case.name]


def forms(case: Case) -> dict:
    return bm.forms(track(case).shape[0], case.settings)


def c_settings(s: Settings):
    """the settings as the library's struct, bad values and all"""
    from mixlab_amd import abi
    c = abi.DeckBars()
    c.grid = abi.DeckBeats(s.first, s.period)
    c.lead, c.taps, c.beats_per_bar, c.bars_per_phrase, c.w_bar, c.w_phrase, c.max_beats = s.lead, s.K, s.M, s.Q, s.w_bar, s.w_phrase, s.max_beats
    for dst, t, tail in ((c.lo, s.lo, s.tail[0]), (c.hi, s.hi, s.tail[1])):
        for k, v in enumerate(tuple(t) + tuple(tail)):
            dst[k] = int(v)
    return c


def m_pick(p) -> bm.Pick:
    """the library's mx_deck_bar_pick as the model's"""
    return bm.Pick(bm.Beats(p.bars.first_q32, p.bars.period_q32), bm.Beats(p.phrases.first_q32, p.phrases.period_q32), p.bar_phase, p.phrase_phase, p.bar_best, p.bar_sum,
                   p.phrase_best, p.phrase_sum)


# ---- pick and next line: random draws, ties and range edges included ----
def pick_draws(n: int = 300):
    """(folds, settings): small integers so that ties are common, some all zero, some with H_bar all zero and H_phrase not"""
    rng = _rng("pick draws")
    out = []
    for k in range(n):
        M, Q = int(rng.integers(2, 9)), int(rng.integers(1, 17))
        top = int(rng.choice([1, 2, 3, 1 << 40]))
        H = [int(v) for v in rng.integers(0, top + 1, M + M * Q)]
        if k % 17 == 0:
            H[:M] = [0] * M
        if k % 23 == 0:
            H = [0] * len(H)
        first = int(rng.integers(-1 << 62, (1 << 62) + 1)) if k % 5 == 0 else int(rng.integers(-1 << 40, 1 << 46))
        period = int(rng.choice([bm.PERIOD_MIN, bm.PERIOD_MAX, int(rng.integers(bm.PERIOD_MIN, bm.PERIOD_MAX + 1))]))
        out.append((H, Settings(first, period, lead=int(rng.choice([0, 1, 128, 4096])), M=M, Q=Q)))
    return out


def next_draws(n: int = 400):
    """(grid, pos): periods from 1 to 2^56, positions before and behind the first line, on a line and one off it, and the edges of the range"""
    rng = _rng("next draws")
    out = [(bm.Beats(-bm.FAR, 1), bm.FAR), (bm.Beats(-bm.FAR, 2), bm.FAR), (bm.Beats(bm.FAR, 1 << 56), -bm.FAR), (bm.Beats(bm.FAR, 1), bm.FAR),
           (bm.Beats(0, (1 << 56) + 1), 0), (bm.Beats(0, 0), 0), (bm.Beats(0, -3), 0), (bm.Beats(bm.FAR + 1, 5), 0), (bm.Beats(0, 5), -bm.FAR - 1), (bm.Beats(5, 10), -6),
           (bm.Beats(5, 10), 5), (bm.Beats(5, 10), 6), (bm.Beats(5, 10), -5), (bm.Beats(5, 10), -15), (bm.Beats(5, 10), -16)]
    while len(out) < n:
        P = int(rng.choice([1, 3, int(rng.integers(1, 1 << 20)), int(rng.integers(1 << 40, (1 << 56) + 1))]))
        first = int(rng.integers(-1 << 62, (1 << 62) + 1)) if rng.random() < 0.3 else int(rng.integers(-1 << 50, 1 << 50))
        k = int(rng.integers(-1000, 1000))
        pos = first + k * P + int(rng.choice([0, 1, -1, int(rng.integers(0, P))]))
        out.append((bm.Beats(first, P), max(-bm.FAR - 1, min(bm.FAR + 1, pos))))
    return out


# ---- end to end: analyse -> beat grid -> fine grid -> bars, on the four models ----
E2E_HOP, E2E_COLUMN, E2E_LAG, E2E_BPM = 64, 64, 256, (800.0, 2000.0)    # (a beat of 2400 frames at 48 kHz is 1200 BPM: a test's tempo, short so that tracks stay small)
_chains = {}


def chain(sec: Section) -> dict:
    """the composed models on a section track, computed once: coarse grid, fine pick, bars settings, records, folds, n0, pick"""
    import deck_finegrid_model as fm
    if sec.name not in _chains:
        tr = section_track(sec)
        a = am.settings_bands(rate=RATE, column=E2E_COLUMN, max_lag=E2E_LAG)
        cols, R = am.analyse(tr, a)
        coarse = am.beatgrid(cols["onset"], R, a.max_lag, a.column, RATE, *E2E_BPM)
        fine = fm.refine(tr, coarse.period_columns, a.column, RATE, E2E_HOP)[0]
        s = Settings(fine.grid.first, fine.grid.period, a.lo, a.hi)
        recs, H, n0 = bm.analyse(tr, s)
        recs.setflags(write=False)
        _chains[sec.name] = {"coarse": coarse, "fine": fine, "settings": s, "records": recs, "folds": H, "n0": n0, "pick": bm.pick(H, s)}
    return _chains[sec.name]


def end_to_end() -> dict:
    return chain(END_TO_END)


def downbeat_misses(sec: Section, bars: bm.Beats) -> list[float]:
    """per constructed downbeat, the distance in frames to the nearest line of a bars grid"""
    P, first = bars.period / 2.0 ** 32, bars.first / 2.0 ** 32
    return [abs((f - first + P / 2) % P - P / 2) for f in downbeat_frames(sec)]


# ---- two decks in time on their bars ----
BAR_SYNC_LEADER, BAR_SYNC_FOLLOWER = END_TO_END, Section(2217.7, 6, 900, "ACB", 128, sections=4)
BAR_SYNC_SPT, BAR_SYNC_TICKS, BAR_SYNC_FEED = 800, 24, 8
# the leader stands on its first downbeat, the follower two beats behind one of its own: the nearest beat is a "3"
BAR_SYNC_LEADER_POS = round(BAR_SYNC_LEADER.first + BAR_SYNC_LEADER.pickup * BAR_SYNC_LEADER.period) << 32
BAR_SYNC_FOLLOWER_POS = round(BAR_SYNC_FOLLOWER.first + (BAR_SYNC_FOLLOWER.pickup + 2) * BAR_SYNC_FOLLOWER.period) << 32
_bar_pair = {}


def bar_sync_pair() -> dict:
    import deck_finegrid_model as fm
    if not _bar_pair:
        _bar_pair["leader"], _bar_pair["follower"] = chain(BAR_SYNC_LEADER), chain(BAR_SYNC_FOLLOWER)
        _bar_pair["sync"] = fm.sync(fm.Beats(*_bar_pair["leader"]["pick"].bars), BAR_SYNC_LEADER_POS, ONE, fm.Beats(*_bar_pair["follower"]["pick"].bars), BAR_SYNC_FOLLOWER_POS)
    return _bar_pair


def bar_sync_gaps(step: int, seek: int):
    """(per constructed leader downbeat from the leader's position on that has follower downbeats on both sides, the distance in output frames to the nearest constructed
    follower downbeat; the bound on it: the end-to-end test's own, two fine hops, in output frames).  Track frame f of a deck that stands at `pos` and moves by `step`
    sounds at output frame (f 2^32 - pos) / step.  Each track's constructed downbeats lie on the same side of its bars grid's lines -- a line is a tooth's centre, the
    kick's first frame a hop or so before it -- so the two offsets cancel in the gap to within their difference, and what is left is held to the bound of one."""
    lead_out = [(f * 2.0 ** 32 - BAR_SYNC_LEADER_POS) / ONE for f in downbeat_frames(BAR_SYNC_LEADER)]
    follow_out = [(f * 2.0 ** 32 - seek) / step for f in downbeat_frames(BAR_SYNC_FOLLOWER)]
    gaps = [min(abs(x - y) for y in follow_out) for x in lead_out if x >= 0 and follow_out[0] <= x <= follow_out[-1]]
    return gaps, 2 * E2E_HOP
