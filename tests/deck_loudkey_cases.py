"""The shared cases of the deck's whole-track tonality and loudness (include/mixlab_gpu.h "KEY AND LOUDNESS"; tests/test_cpu_deck_loudkey.py,
tests/test_gpu_deck_loudkey.py): tracks, settings, and what the independent models of the TAPS (tests/tonality_model.py, tests/loudness_model.py) give for them,
each computed once.  The models are fed the zero-padded track as (float)sample / 32768 in ticks of one segment (emit_ticks = 1) or one block: the header says the
records equal theirs byte for byte.  `mis` switches in ONE deliberate misreading of the text.

The smallest shapes at which the kernels can still go wrong: a track of one frame, lengths around a hop's last input frame and around a segment, segments of fewer,
exactly and more than the 8 hops a constant-Q workgroup takes, blocks around one, more than the 32 blocks of a walk workgroup, windows longer than the track."""
from __future__ import annotations

import zlib
from collections import namedtuple

import numpy as np

import loudness_model as lm
import tonality_model as tm

TonCase = namedtuple("TonCase", "name n_frames kind rate D Hc O f_lo_mhz G")
LoudCase = namedtuple("LoudCase", "name n_frames kind rate F M S")

TON_MISREADINGS = ("shift_q", "last_segment_dropped", "padded_hops_not_counted", "late_hop")
LOUD_MISREADINGS = ("over_32767", "last_block_short", "run_in_not_carried", "history_cut_at_m")


def _ton(name, n, kind="noise", G=1, rate=8000.0, D=4, Hc=128, O=2, f_lo_mhz=220000):
    return TonCase(name, n, kind, rate, D, Hc, O, f_lo_mhz, G)


def _loud(name, n, kind="noise", F=64, M=4, S=30, rate=48000.0):
    return LoudCase(name, n, kind, rate, F, M, S)


# D 4, Hc 128, O 2 at 8 kHz from 220 Hz, not the 440 Hz first thought of: two octaves from 440 Hz end at 440 * 2^(23/12 + 1/24) = 1710 Hz, beyond 900 = 0.45 fs_d, and
# mx_tonality_tables refuses that; from 220 Hz they end at 855 Hz, and N_0 = ceil(17 * 2000 / 220) = 155 <= 2048 (test_cpu_deck_loudkey.py checks both settings with
# mx_tonality_tables).  A hop is 512 frames; (Hc - 1) D = 508 is the first hop's last input frame.
TON_CASES = (
    _ton("1 frame", 1),
    _ton("508 frames: the first hop's last input frame absent", 508),
    _ton("509 frames: ... present", 509),
    _ton("F - 1 frames, G = 1", 511), _ton("F frames, G = 1", 512), _ton("F + 1 frames, G = 1", 513),
    _ton("F - 1 frames, G = 3", 1535, G=3), _ton("F frames, G = 3", 1536, G=3), _ton("F + 1 frames, G = 3", 1537, G=3),
    _ton("20 hops of noise, G = 1", 10240),
    _ton("20 hops of noise, G = 7: a short last segment", 10240, G=7),
    _ton("20 hops of noise, G = 8: full constant-Q workgroups", 10240, G=8),
    _ton("20 hops of noise, G = 12: a full and a partial workgroup per segment", 10240, G=12),
    _ton("20 hops of noise, G = 65536: one record", 10240, G=65536),
    _ton("every sample -32768", 3000, "floor", G=3),
    _ton("full-scale alternating square", 3000, "square", G=3),
    _ton("odd negative s throughout", 3000, "odd_negative", G=3),
    _ton("silence", 3000, "silence", G=3),
    _ton("D 8, Hc 512, O 5 from C2 at 48 kHz, 40 000 frames", 40000, G=4, rate=48000.0, D=8, Hc=512, O=5, f_lo_mhz=65406),
)
LOUD_CASES = (
    _loud("1 frame", 1), _loud("63 frames", 63), _loud("64 frames", 64), _loud("65 frames", 65),
    _loud("71 blocks: 64 * 70 + 5 frames", 64 * 70 + 5),
    _loud("71 blocks, windows 1 and 1024", 64 * 70 + 5, M=1, S=1024),
    _loud("F = 4800 over 3.5 blocks", 16800, F=4800),
    _loud("full-scale alternating square", 1000, "square"),
    _loud("every sample -32768", 1000, "floor"),
    _loud("silence", 1000, "silence"),
    _loud("noise, 1000 frames", 1000),
    _loud("noise, F = 100: a wave of the peak kernel spans two blocks", 1000, F=100),
    _loud("44.1 kHz", 700, rate=44100.0),
)
TON_BY_NAME = {c.name: c for c in TON_CASES}
LOUD_BY_NAME = {c.name: c for c in LOUD_CASES}


def track(case) -> np.ndarray:
    """int16 (n_frames, 2), seeded by the case's name"""
    n = case.n_frames
    if case.kind == "silence":
        return np.zeros((n, 2), np.int16)
    if case.kind == "floor":
        return np.full((n, 2), -32768, np.int16)
    if case.kind == "square":   # +32767, -32767, ... on both channels: the interpolator overshoots between the samples
        return np.repeat(np.where(np.arange(n) & 1, -32767, 32767).astype(np.int16)[:, None], 2, axis=1)
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    if case.kind == "odd_negative":   # s = l + r odd and negative in every frame: s / 4 truncates toward zero, s >> 2 floors
        l = rng.integers(-16000, 0, size=n)
        r = -rng.integers(0, 8000, size=n) * 2 - 1 - (l & 1)   # of the parity that makes l + r odd
        t = np.stack([l, r], axis=1)
        assert ((t.sum(axis=1) & 1) == 1).all() and (t.sum(axis=1) < 0).all()
        return t.astype(np.int16)
    t = rng.integers(-32768, 32768, size=(n, 2), dtype=np.int64).astype(np.int16)
    t[rng.integers(0, n, size=max(1, n // 64))] = (-32768, 32767)
    return t


def padded(tr: np.ndarray, frames: int) -> np.ndarray:
    out = np.zeros((frames, 2), np.int16)
    out[:min(frames, len(tr))] = tr[:frames]
    return out


# ---- tonality ----
def ton_segments(case) -> int:
    return -(-case.n_frames // (case.G * case.Hc * case.D))


def ton_forms(case) -> dict:
    """mx_deck_debug_last_tonality for the case (mixlab_amd/csrc/mx_k_deck_tonality.hip launch_deck_tonality)"""
    n = ton_segments(case)
    return {"wgs_decimate": -(-n * case.G * case.Hc // 512), "wgs_cq_full": n * (case.G // 8), "wgs_cq_part": n if case.G % 8 else 0,
            "wgs_head": -(-n * (4 + 12 * case.O) // 256)}


def _ton_model(case, variant=None):
    return tm.TonalityModel(case.rate, case.D, case.Hc, case.O, case.f_lo_mhz, emit_ticks=1, channels=2, variant=variant)


def _ton_floats(case, tr, frames, mis):
    x = padded(tr, frames).astype(np.int64)
    if mis == "shift_q":   # q = s >> 2: a left channel of (s >> 2) / 8192 beside a silent right one quantises to exactly that
        return np.stack([((x[:, 0] + x[:, 1]) >> 2).astype(np.float32) / np.float32(8192.0), np.zeros(frames, np.float32)], axis=1)
    return x.astype(np.float32) / np.float32(32768.0)


def ton_records(case, mis=None, tr=None) -> list:
    """the records as bytes, one per segment, from the taps' model; tr: another track of case.n_frames than the case's own"""
    tr = track(case) if tr is None else tr
    F, n_seg = case.G * case.Hc * case.D, ton_segments(case)
    hop = case.Hc * case.D
    # every hop whose kernels can see a frame of the track: the FIR reaches 8 D - 1 frames back and the longest kernel 2047 decimated frames; behind that q, d, S and
    # M are all 0, so a segment's later hops add nothing
    live_hops = min(n_seg * case.G, -(-(case.n_frames + 8 * case.D + 2048 * case.D) // hop) + 1)
    direct = mis in (None, "shift_q", "late_hop", "last_segment_dropped") and n_seg * F <= 1 << 20
    if direct:   # the header's statement itself: ticks of F frames, emit_ticks = 1
        m = _ton_model(case, "late_hop" if mis == "late_hop" else None)
        recs = m.run(_ton_floats(case, tr, n_seg * F, mis), n_seg)
    else:        # the same model hop by hop (ticks of Hc D frames), the hops of a segment summed here: how a segment of 2^25 frames is fed in a test's time
        m = _ton_model(case)
        per_hop = [tm.parse_record(r) for r in m.run(_ton_floats(case, tr, live_hops * hop, mis), live_hops)]
        recs = []
        for g in range(n_seg):
            C, hops = np.zeros(12 * case.O, np.uint64), case.G
            for h in range(g * case.G, min((g + 1) * case.G, live_hops)):
                if mis == "padded_hops_not_counted" and ((h + 1) * case.Hc - 1) * case.D >= case.n_frames:
                    continue
                C += per_hop[h]["cq"]
            if mis == "padded_hops_not_counted":
                hops = sum(1 for h in range(g * case.G, (g + 1) * case.G) if ((h + 1) * case.Hc - 1) * case.D < case.n_frames)
            head = np.array([g, hops, 0, case.D, case.Hc, case.O, case.f_lo_mhz, 0], np.uint32)
            recs.append(head.tobytes() + C.tobytes())
    if mis == "last_segment_dropped":
        recs = recs[:case.n_frames // F]
    return [bytes(r) for r in recs]


_ton_truth = {}


def ton_truth(case) -> bytes:
    """all the records back to back, segment index in word 0"""
    if case.name not in _ton_truth:
        recs = ton_records(case)
        out = b""
        for g, r in enumerate(recs):   # (the model's word 0 is the tick in its run: here the one run starts at segment 0)
            assert np.frombuffer(r, np.uint32, 2).tolist() == [g, case.G]
            out += r
        _ton_truth[case.name] = out
    return _ton_truth[case.name]


def c_tonality(case):
    from mixlab_amd import deck
    return deck.tonality(case.rate, case.D, case.Hc, case.O, case.f_lo_mhz, case.G)


# ---- loudness ----
def loud_blocks(case) -> int:
    return -(-case.n_frames // case.F)


def loud_forms(case) -> dict:
    """mx_deck_debug_last_loudness for the case (mixlab_amd/csrc/mx_k_deck_loudness.hip launch_deck_loudness)"""
    n = loud_blocks(case)
    return {"wgs_peak": -(-n * case.F // 1024), "wgs_walk": -(-n // 32), "scan_steps": n, "wgs_window": -(-n // 256)}


def loud_records(case, mis=None, tr=None) -> np.ndarray:
    """... from the taps' model; tr: another track of case.n_frames than the case's own"""
    tr, n = track(case) if tr is None else tr, loud_blocks(case)
    x = padded(tr, n * case.F).astype(np.float32) / np.float32(32767.0 if mis == "over_32767" else 32768.0)
    m = lm.LoudnessModel(2, case.rate, case.F, case.M, case.S)
    if mis in ("run_in_not_carried", "history_cut_at_m"):   # block by block (the model's records do not depend on the grouping), forgetting in between
        out = []
        for k in range(n):
            if mis == "run_in_not_carried":
                m.x_hist[:] = 0
            else:
                m.e_hist[:lm.HIST_TICKS - (case.M - 1)] = 0
            out.append(m.run(x[k * case.F:(k + 1) * case.F], 1))
        recs = np.concatenate(out)
    else:
        recs = m.run(x, n)
    if mis == "last_block_short":
        recs["frames"][-1] = case.n_frames - (n - 1) * case.F
    return recs


_loud_truth = {}


def loud_truth(case) -> np.ndarray:
    if case.name not in _loud_truth:
        _loud_truth[case.name] = loud_records(case)
        _loud_truth[case.name].setflags(write=False)
    return _loud_truth[case.name]


def c_loudness(case):
    from mixlab_amd import deck
    return deck.loudness(case.rate, case.F, case.M, case.S)
