"""The cases of tests/test_cpu_fir_model.py (oracle == model, every misreading caught) and tests/test_gpu_fir_model.py (device == model): the
smallest shapes that reach each branch of launch_fir and launch_resample (mx_k_fir.hip), with a Python restatement of those two launchers'
choice, the model's own runs and the graph both sides build.  Importable without a GPU.

Every member of a case is one node behind a stereo source of its own, all on one dependency level.  The engine forms one launch group per
(level, kind, OUTPUT RATE DOMAIN) -- up / down reduced -- so Resample nodes share a launch only where their ratios are equal: 160/147 and 320/294
do, 160/147 and 2/1 do not.  `groups()` restates that; the "mixed" cases say which of their members really meet in one launch.

"n" channels means one per compute unit (multi_processor_count): with it the phase-stationary kernel gets 5 blocks per channel and the staged
kernel at most 8, whatever the chip.  The CPU tests run the same cases with N_CPU channels (the arithmetic of a channel does not depend on its
neighbours) and check the branch table for 256 compute units.

44.1 kHz, 735 frames per tick.  The grid-stride repeat of k_fir (a block's second tile) needs over 2 M frames per channel and is left out.
"""
from __future__ import annotations

from dataclasses import dataclass
from fractions import Fraction
from math import gcd

import numpy as np

import fir_model as fm
import synth

SPT = 735
N_CPU = 6
F32 = np.float32
FAR_2P32 = 5_368_708                      # tick: 800 outputs per tick put output time 2^32 into the second tick of the run (input time stays below)
FAR_2P40 = -(-(1 << 40) // 800)           # the first tick whose output time is at or past 2^40


@dataclass(frozen=True)
class Case:
    id: str
    kind: str                 # "fir" | "resample"
    members: tuple            # fir: (K, ...); resample: ((up, down, P, channels), ...), channels an int, "n" or "2n"
    ticks: int                # per submission
    runs: int
    why: str
    kernels: tuple            # the kernels launch_fir / launch_resample pick for it at 256 compute units
    walks: int = 0            # a block of the first launch walks at least this many 256-output groups (0: not what the case is for)
    first_tick: int = 0
    connected: bool = True
    fma_exact: bool = False   # small enough for the exact Fraction FMA


# ------------------------------------------------------------------------------------------------
# launch_fir / launch_resample restated (mx_k_fir.hip): kernel, blocks per channel, the most 256-output groups a block walks
# ------------------------------------------------------------------------------------------------
FIR_LDS_LIMIT = 64 * 1024


def fir_lds_plan(max_taps: int, frames: int):
    per = 8 if frames >= 8192 and max_taps <= 1024 else 4
    wn = 256 * per + max_taps + per
    return per, ((max_taps + 1) & ~1) * 8 + (wn + wn // per + 2) * 16


def fir_launch(max_taps: int, frames: int):
    per, lds = fir_lds_plan(max_taps, frames)
    if lds > FIR_LDS_LIMIT:
        return "k_fir_plain", min(1024, -(-frames // 256)), 1
    return f"k_fir<{per}>", min(1024, -(-frames // (256 * per))), 1


def resample_launch(nodes, out_frames: int, cus: int):
    """nodes: the (up, down, P) of every node of ONE launch group"""
    n = len(nodes)
    common = lambda vals: vals[0] if len(set(vals)) == 1 else 0
    c_up, c_down, c_p = common([u for u, _d, _p in nodes]), common([d for _u, d, _p in nodes]), common([p for _u, _d, p in nodes])
    tab = max(u * p for u, _d, p in nodes)
    win = max(255 * d // u + 2 + p for u, d, p in nodes)
    groups = -(-out_frames // 256)
    if c_up == 160 and c_p == 16 and c_down and 255 * c_down // 160 + 2 + 16 <= 256:
        per_ch = max(1, (cus * 8) // n) // 5 * 5 or 5
        per_ch = min(per_ch, -(-groups // 5) * 5)
        return "k_resample_ps<160,16>", per_ch, -(-groups // per_ch)
    lds = tab * 8 + ((win + 1) & ~1) * 16
    if lds <= 60 * 1024:
        resident = cus * max(1, min(8, (160 * 1024) // max(lds, 1)))
        per_ch = max(1, min(groups, max(1, resident // n)))
        return ("k_resample<160>" if c_up == 160 else "k_resample<0>"), per_ch, -(-groups // per_ch)
    return "k_resample_gather", min(1024, groups), 1


# Noise does not tell two f64 summation orders apart: they differ by a few 2^-53 relative, and an f32 rounding boundary lies that close to one sample
# in 10^8.  The tie cases put the sum ON a boundary.  With h0 = 1 + 2^-24 (half-way between the f32 neighbours 1 and 1 + 2^-23) over a stretch of 1.0:
#   TIE_ORDER  (h0, s, s), s = 0.75 * 2^-53: ascending, h0 + s rounds back to h0 twice and the f32 tie goes to even, 1.0; descending, s + s = 1.5 * 2^-53
#              passes half an f64 ULP of h0 and the sum rounds up to 1 + 2^-23
#   TIE_FMA    (h0, h1) over x[n] = 1, x[n-1] = 1 + 2^-23, h1 the smallest double whose EXACT product with x[n-1] exceeds 2^-53 while the rounded
#              product is 2^-53: separately, h0 + 2^-53 is an f64 tie and goes to even (h0, then 1.0); fused, the sum rounds up (1 + 2^-23)
TIE_H0, TIE_S, TIE_X1 = 1.0 + 2.0 ** -24, 0.75 * 2.0 ** -53, 1.0 + 2.0 ** -23
TIE_H1 = float(np.nextafter(np.nextafter(2.0 ** -53 / TIE_X1, 0.0), 0.0))
while Fraction(TIE_H1) * Fraction(TIE_X1) <= Fraction(1, 1 << 53):
    TIE_H1 = float(np.nextafter(TIE_H1, 1.0))
assert TIE_H1 * TIE_X1 == 2.0 ** -53
TIE_ORDER, TIE_FMA = (TIE_H0, TIE_S, TIE_S), (TIE_H0, TIE_H1)

_K_LAST_TILED = max(k for k in range(1400, 1700) if fir_lds_plan(k, SPT)[1] <= FIR_LDS_LIMIT)      # 1605 for a one-tick run: its plan is exactly 65 536 bytes

FIR = [
    Case("F1a", "fir", (1, 7, 8), 12, 3, "k_fir<8>: K < PER, K = PER; own K differs from max_taps; 8820 = 4 * 2048 + 628, 628 = 78 * 8 + 4: one lane stores 4 of its 8 outputs", ("k_fir<8>",)),
    Case("F1b", "fir", (9, 128, 131), 12, 3, "k_fir<8>: K a multiple of PER and not (the remainder loop that rotates by moving)", ("k_fir<8>",)),
    Case("F1c", "fir", (3, 300, 1024), 12, 3, "k_fir<8> at its largest window (max_taps = 1024)", ("k_fir<8>",)),
    Case("F2", "fir", (1025,), 12, 3, "k_fir<4> over 9 tiles: the first K past k_fir<8>", ("k_fir<4>",)),
    Case("F2s", "fir", (5, 9), 1, 2, "k_fir<4> on a short run (735 frames), small enough for the exact FMA", ("k_fir<4>",), fma_exact=True),
    Case("F3", "fir", (2048, 6000, 16384), 1, 3, "the plain path: history longer than a run, k_fir_history_chunked moving old history in place; K at the accepted limit", ("k_fir_plain",)),
    Case("F3t", "fir", (_K_LAST_TILED,), 1, 3, "the longest filter the tiled kernel still takes (the last plan at or under 64 KiB)", ("k_fir<4>",)),
    Case("F3p", "fir", (_K_LAST_TILED + 1, 5), 1, 3, "the shortest filter on the plain path, and a 5-tap neighbour of the same launch drawn into it", ("k_fir_plain",)),
    Case("F5", "fir", (3, 2), 1, 2, "the tie taps TIE_ORDER and TIE_FMA: the summation order and a fused step each move an f32", ("k_fir<4>",), fma_exact=True),
    Case("F4", "fir", (16,), 2, 2, "a disconnected input: every output bit is +0.0", ("k_fir<4>",), connected=False),
]

RESAMPLE = [
    Case("R1_T4", "resample", ((160, 147, 16, "n"),), 4, 3, "k_resample_ps across groups: 3200 outputs, 12.5 groups, blocks walk 3/3/3/2/2", ("k_resample_ps<160,16>",), walks=3),
    Case("R1_T13", "resample", ((160, 147, 16, "n"),), 13, 3, "k_resample_ps: 10 400 outputs, 40.6 groups, 8-9 per block (pre, pre2, f0 += in_step)", ("k_resample_ps<160,16>",), walks=8),
    Case("R2", "resample", ((160, 140, 16, 2), (160, 120, 16, 2)), 4, 3, "k_resample_ps with gcd(up, down) > 1: a launch group each (8/7 and 4/3)", ("k_resample_ps<160,16>", "k_resample_ps<160,16>")),
    Case("R3a", "resample", ((160, 147, 15, "n"),), 13, 3, "k_resample<160> with blocks walking 5-6 groups", ("k_resample<160>",), walks=5),
    Case("R3b", "resample", ((160, 147, 15, "n/2"), (160, 147, 17, "n/2")), 13, 3, "k_resample<160>, taps per phase differing inside the launch", ("k_resample<160>",), walks=5),
    Case("R3c", "resample", ((8, 7, 12, "n"),), 13, 3, "k_resample<0> with blocks walking 5-6 groups", ("k_resample<0>",), walks=5),
    Case("R4a", "resample", ((1, 3, 23, "n"),), 13, 3, "win_cap > 256: the staging loop of more than one frame per lane; 13 groups over 8 blocks", ("k_resample<0>",)),
    Case("R4w", "resample", ((1, 3, 23, "2n"),), 13, 3, "the same with twice the channels: 4 blocks per channel walk 3-4 groups", ("k_resample<0>",), walks=3),
    Case("R4b", "resample", ((1, 1, 1000, 1),), 1, 3, "history spanning two earlier runs (999 frames of 735-frame runs), window 1257", ("k_resample<0>",)),
    Case("R5a", "resample", ((160, 147, 48, 2),), 4, 3, "k_resample_gather: 61 440 bytes of table", ("k_resample_gather",)),
    Case("R5b", "resample", ((1, 1, 4096, 1),), 1, 3, "k_resample_gather at the accepted limit; in_frames < H in k_resample_history", ("k_resample_gather",)),
    Case("R5m", "resample", ((160, 147, 16, 1), (2, 1, 5, 1), (160, 147, 48, 1), (320, 294, 5, 1)), 2, 3,
         "a launch pushed into k_resample_gather by one member (160/147 P 16 and 320/294 P 5 beside P 48); 2/1 is a launch of its own", ("k_resample_gather", "k_resample<0>")),
    Case("R6", "resample", ((160, 147, 16, 1), (2, 1, 5, 1), (1, 3, 23, 1), (4, 5, 9, 1)), 2, 3, "four ratios on one level: four launches, one ratio each", ("k_resample<0>", "k_resample<0>", "k_resample<0>", "k_resample_ps<160,16>")),
    Case("R6m", "resample", ((160, 147, 20, 2), (320, 294, 12, 2)), 4, 3, "one staged launch with common_up = 0: the largest window (P 20: 256) and the largest table (320 x 12) from different members",
         ("k_resample<0>",)),
    Case("R6s", "resample", ((2, 1, 5, 1), (4, 2, 3, 1)), 1, 2, "a mixed staged launch small enough for the exact FMA", ("k_resample<0>",), fma_exact=True),
    Case("R9", "resample", ((1, 1, 3, 1), (1, 1, 2, 1)), 1, 2, "the tie taps TIE_ORDER and TIE_FMA as one-phase tables", ("k_resample<0>",), fma_exact=True),
    Case("R7a_2p32", "resample", ((160, 147, 16, 8),), 4, 1, "k_resample_ps: output time crosses 2^32 inside the run", ("k_resample_ps<160,16>",), first_tick=FAR_2P32),
    Case("R7b_2p32", "resample", ((160, 147, 15, 8),), 4, 1, "k_resample<160>: output time crosses 2^32 inside the run", ("k_resample<160>",), first_tick=FAR_2P32),
    Case("R7c_2p32", "resample", ((160, 147, 48, 2),), 4, 1, "k_resample_gather: output time crosses 2^32 inside the run", ("k_resample_gather",), first_tick=FAR_2P32),
    Case("R7a_2p40", "resample", ((160, 147, 16, 8),), 4, 1, "k_resample_ps from output time 2^40", ("k_resample_ps<160,16>",), first_tick=FAR_2P40),
    Case("R7b_2p40", "resample", ((160, 147, 15, 8),), 4, 1, "k_resample<160> from output time 2^40", ("k_resample<160>",), first_tick=FAR_2P40),
    Case("R7c_2p40", "resample", ((160, 147, 48, 2),), 4, 1, "k_resample_gather from output time 2^40", ("k_resample_gather",), first_tick=FAR_2P40),
    Case("R8", "resample", ((160, 147, 16, 1), (1, 3, 23, 1)), 2, 2, "a disconnected input: every output bit is +0.0", ("k_resample<0>", "k_resample_ps<160,16>"), connected=False),
]



def channels(count, n: int) -> int:
    return {"n": n, "2n": 2 * n, "n/2": max(1, n // 2)}.get(count, count)


def nodes_of(case: Case, n: int):
    """[(member index, channel index inside the member)] in the order the graph is built"""
    if case.kind == "fir":
        return [(i, 0) for i in range(len(case.members))]
    return [(i, c) for i, (_u, _d, _p, cnt) in enumerate(case.members) for c in range(channels(cnt, n))]


def groups(case: Case, n: int):
    """the launch groups of the case's level, in launch order: lists of member indices (one entry per node)"""
    if case.kind == "fir":
        return [[i for i, _c in nodes_of(case, n)]]
    key = lambda i: (lambda u, d: ((u // gcd(u, d)) << 32) | (d // gcd(u, d)))(*case.members[i][:2])
    out = {}
    for i, _c in nodes_of(case, n):
        out.setdefault(key(i), []).append(i)
    return [out[k] for k in sorted(out)]


def launches(case: Case, cus: int):
    """[(kernel, blocks per channel, most groups a block walks)] per launch group, for n = cus channels"""
    res = []
    for grp in groups(case, cus):
        if case.kind == "fir":
            res.append(fir_launch(max(case.members[i] for i in grp), case.ticks * SPT))
        else:
            u, d = case.members[grp[0]][:2]
            res.append(resample_launch([case.members[i][:3] for i in grp], case.ticks * SPT * u // d, cus))
    return res


CASES = FIR + RESAMPLE
BY_ID = {c.id: c for c in CASES}
BRANCHES = ("k_fir<4>", "k_fir<8>", "k_fir_plain", "k_resample_ps<160,16>", "k_resample<160>", "k_resample<0>", "k_resample_gather")


# ------------------------------------------------------------------------------------------------
# parameters, inputs, the model's runs
# ------------------------------------------------------------------------------------------------
def _seed(case: Case) -> int:
    return 9000 + 97 * CASES.index(case)


def fir_taps(case: Case, i: int) -> np.ndarray:
    K = case.members[i]
    if case.id == "F5":
        return np.array((TIE_ORDER, TIE_FMA)[i])
    return synth.uniform(_seed(case) + i, K, -1.0, 1.0) * np.exp(-3.0 * np.arange(K) / K) * 0.35      # the last tap still carries 5 % of the first


def table(case: Case, i: int, c: int) -> np.ndarray:
    up, _down, P, _cnt = case.members[i]
    if case.id == "R9":
        return np.array((TIE_ORDER, TIE_FMA)[i]).reshape(1, P)
    return synth.uniform(_seed(case) + 1000 * i + c, up * P, -1.0, 1.0).reshape(up, P)


def source(case: Case, i: int, c: int) -> np.ndarray:
    """(runs * ticks * SPT, 2) f32: noise with a few values whose bits an arithmetic shortcut would lose"""
    x = synth.noise(_seed(case) + 5000 + 1000 * i + c, 2 * case.runs * case.ticks * SPT).reshape(-1, 2).copy()
    x[3] = (-0.0, F32(1e-42)); x[100] = (1.0, -1.0); x[200:230] = 0.0
    x[300:340] = 1.0; x[340:380:2] = F32(TIE_X1); x[341:380:2] = 1.0          # what the tie cases (F5, R9) need; noise to the others
    x[SPT - 1] = (F32(2.0 ** -126), F32(-0.999999940395))
    return x


def rate(case: Case, i: int):
    return (1, 1) if case.kind == "fir" else case.members[i][:2]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def assert_same_bits(got, want, what):
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    assert got.size == want.size, f"{what}: {got.size} samples, expected {want.size}"
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} samples differ, first at {bad[0]}: {got[bad[0]]!r} != {want[bad[0]]!r}"


def assert_within_one_ulp(got, want, what):
    """the contracted order's promise: 1 ULP of the exact order, 2^-40 absolute at a zero crossing -- no sample beyond"""
    got, want = np.asarray(got, F32).reshape(-1), np.asarray(want, F32).reshape(-1)
    assert got.size == want.size, what
    d = synth.ulp_diff(got, want)
    bad = (d > 1) & (np.abs(got.astype(np.float64) - want.astype(np.float64)) > 2.0 ** -40)
    assert not bad.any(), f"{what}: {int(bad.sum())} samples beyond 1 ULP, first {int(np.flatnonzero(bad)[0])}"
    return d


_MODEL = {}


def model(case: Case, n: int, order: str = "exact", mis=None):
    """{(member, channel): (runs * out_frames, 2) f32}: every submission's output, history carried by the model itself"""
    key = (case.id, n, order, mis)
    if key in _MODEL:
        return _MODEL[key]
    out = {}
    frames = case.ticks * SPT
    for i, member in enumerate(case.members):
        if case.kind == "fir":
            taps, hist, ys = fir_taps(case, i), np.zeros((member - 1, 2), F32), []
            x = source(case, i, 0)
            for r in range(case.runs):
                y, hist = fm.fir(taps, hist, x[r * frames:(r + 1) * frames] if case.connected else None, frames, order, mis)
                ys.append(y)
            out[i, 0] = np.concatenate(ys)
            continue
        up, down, P, cnt = member
        C = channels(cnt, n)
        tabs = np.stack([table(case, i, c) for c in range(C)])
        x = np.stack([source(case, i, c) for c in range(C)])
        hist, ys = np.zeros((C, P - 1, 2), F32), []
        for r in range(case.runs):
            t0 = (case.first_tick + r * case.ticks) * SPT                       # the engine: in_base = t0 * 1 / 1, out_base = t0 * up / down (reduced)
            y, hist = fm.resample(tabs, up, down, hist, t0, t0 * up // down, x[:, r * frames:(r + 1) * frames] if case.connected else None,
                                  frames * up // down, frames, order, mis)
            ys.append(y)
        y = np.concatenate(ys, axis=1)
        for c in range(C):
            out[i, c] = y[c]
    if mis is None:
        _MODEL[key] = out
    return out


def workspace(case: Case, n: int):
    """-> (Workspace, [(member, channel, source node or None, node)])"""
    from mixlab_amd.workspace import Workspace
    ws = Workspace(44100, 60)
    nodes = []
    for i, c in nodes_of(case, n):
        node = ws.fir(fir_taps(case, i)) if case.kind == "fir" else ws.resample(*case.members[i][:2], table(case, i, c))
        src = None
        if case.connected:
            src = ws.source_stereo()
            ws.connect(src, 0, node, 0)
        nodes.append((i, c, src, node))
    return ws, nodes
