"""Fir and Resample without a GPU: the C oracle against the independent numpy model (tests/fir_model.py, written from DESIGN.md section 7 alone), the
model against scipy and against exact rational sums, the case table against the launchers' branches, and every deliberate misreading caught.

(a) oracle.fir_run / oracle.resample_run, history carried from submission to submission, equal the model on every bit of every case of
    tests/fir_cases.py (N_CPU channels where a case says "n"); OracleGraph does on the cases with more than one member, tick by tick; the oracle's
    contract mode equals the model's contracted order where the exact FMA is affordable (the fma_exact cases), and stays within 1 ULP of the
    uncontracted model everywhere else;
(b) the model reproduces tests/golden/fir_resample_scipy.npz in the existing test's terms (1 ULP, 2^-40 absolute at a zero crossing, < 5e-3 of the
    samples differing);
(c) the model's f64 accumulator is within a bound derived by counting roundings of the exact sum (test_the_model_is_within_the_derived_bound...);
(d) for 256 compute units every branch of launch_fir / launch_resample is drawn by a case, and the cases that are there for blocks walking
    several groups give a block at least that many;
(e) each of fir_model.MISREADINGS changes a bit of a named case.
"""
from fractions import Fraction

import numpy as np
import pytest

import fir_cases as fc
import fir_model as fm
import oracle
import synth

from fir_cases import assert_same_bits, assert_within_one_ulp, bits

F32 = np.float32
N = fc.N_CPU


def by_id(cases):
    return pytest.mark.parametrize("case", cases, ids=[c.id for c in cases])


def oracle_runs(case, n):
    """{(member, channel): samples}: the per-module oracle calls, history carried by the caller as the ABI's hist buffer"""
    out = {}
    frames = case.ticks * fc.SPT
    silence = np.zeros(2 * frames, F32)
    for i, c in fc.nodes_of(case, n):
        x = fc.source(case, i, c).reshape(-1) if case.connected else None
        ys = []
        if case.kind == "fir":
            taps = fc.fir_taps(case, i)
            hist = np.zeros(2 * max(1, taps.size - 1), F32)
            for r in range(case.runs):
                ys.append(oracle.fir_run(taps, hist, x[r * 2 * frames:(r + 1) * 2 * frames] if case.connected else silence))
        else:
            up, down, P, _cnt = case.members[i]
            tab = fc.table(case, i, c)
            hist = np.zeros(2 * max(1, P - 1), F32)
            for r in range(case.runs):
                t0 = (case.first_tick + r * case.ticks) * fc.SPT
                ys.append(oracle.resample_run(tab, up, down, hist, t0, t0 * up // down, x[r * 2 * frames:(r + 1) * 2 * frames] if case.connected else silence,
                                              frames * up // down))
        out[i, c] = np.concatenate(ys)
    return out


# ------------------------------------------------------------------------------------------------
# (a) oracle == model
# ------------------------------------------------------------------------------------------------
@by_id(fc.CASES)
def test_the_oracle_modules_equal_the_model(case):
    want = fc.model(case, N)
    got = oracle_runs(case, N)
    assert set(got) == set(want)
    for key in want:
        assert_same_bits(got[key], want[key], f"{case.id} member {key[0]} channel {key[1]}")
        if not case.connected:
            assert not bits(got[key]).any(), f"{case.id}: a disconnected input must give +0.0 in every bit"


@by_id([c for c in fc.CASES if len(c.members) > 1 or not c.connected])
def test_the_oracle_graph_equals_the_model(case):
    want = fc.model(case, N)
    ws, nodes = fc.workspace(case, N)
    og = oracle.OracleGraph(ws)
    got = {(i, c): [] for i, c, _s, _n in nodes}
    src = {(i, c): fc.source(case, i, c).reshape(-1) for i, c, s, _n in nodes if s is not None}
    for t in range(case.runs * case.ticks):
        for i, c, s, _n in nodes:
            if s is not None:
                og.set_source(s, src[i, c][t * 2 * fc.SPT:(t + 1) * 2 * fc.SPT])
        og.run_tick(case.first_tick + t)
        for i, c, _s, node in nodes:
            got[i, c].append(og.output(node, 0))
    for key in want:
        assert_same_bits(np.concatenate(got[key]), want[key], f"{case.id} member {key[0]} channel {key[1]}")


@by_id(fc.CASES)
def test_the_oracle_contract_mode_against_the_model(case):
    """bit for bit where the model has an exact FMA; elsewhere within 1 ULP of the uncontracted model"""
    with oracle.fp_contract():
        got = oracle_runs(case, N)
    if fm.HAVE_FAST_FMA or case.fma_exact:
        want = fc.model(case, N, "contracted")
        for key in want:
            assert_same_bits(got[key], want[key], f"{case.id} contracted, member {key[0]} channel {key[1]}")
    want = fc.model(case, N)
    for key in want:
        assert_within_one_ulp(got[key], want[key], f"{case.id} contracted against the exact order, member {key[0]} channel {key[1]}")


def test_the_exact_fma_is_fused():
    a, b = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30               # a * b = 1 - 2^-60: rounds to 1.0 as a product of its own
    assert a * b - 1.0 == 0.0 and fm.fma(a, b, -1.0) == -(2.0 ** -60)
    assert fm.fma(0.1, 10.0, -1.0) == float(Fraction(0.1) * 10 - 1)
    assert str(fm.fma(-0.0, 1.0, 0.0)) == "0.0" and str(fm.fma(-0.0, 1.0, -0.0)) == "-0.0"


# ------------------------------------------------------------------------------------------------
# (b) model vs scipy
# ------------------------------------------------------------------------------------------------
def test_the_model_agrees_with_scipy_within_one_ulp():
    import pathlib
    z = np.load(pathlib.Path(__file__).parent / "golden" / "fir_resample_scipy.npz")
    x = np.ascontiguousarray(z["x"], F32)
    def close(got, want, what):
        d = assert_within_one_ulp(got, want, what)
        assert (d != 0).mean() < 5e-3, f"{what}: {(d != 0).mean():.4f} of the samples differ"
    K = z["fir_taps"].size
    y, _h = fm.fir(z["fir_taps"], np.zeros((K - 1, 2), F32), x)
    close(y, z["y_fir"], "model FIR vs scipy.signal.lfilter")
    for name in "abc":
        up, down, P = (int(v) for v in z[f"rs_{name}_ratio"])
        want = z[f"rs_{name}_y"]
        y, _h = fm.resample(z[f"rs_{name}_table"][None], up, down, np.zeros((1, P - 1, 2), F32), 0, 0, x[None], want.shape[0])
        close(y[0], want, f"model resampler {name} vs scipy.signal.upfirdn")


# ------------------------------------------------------------------------------------------------
# (c) model vs exact values
# ------------------------------------------------------------------------------------------------
# The accumulator after K ascending steps acc = fl(acc + fl(h_k x_k)), acc_0 = 0: with u = 2^-53 every product is h_k x_k (1 + d), |d| <= u (K
# roundings, one per term; f64(x) is exact), and term k then passes through the sums k, k + 1, .., K - 1, each (1 + e), |e| <= u -- the first sum,
# 0 + p_0, is exact, so there are K - 1 of them and no term meets more than K - 1.  A term therefore carries at most K factors (1 + d_i):
#     |acc - sum_k h_k x_k|  <=  ((1 + u)^K - 1) * sum_k |h_k x_k|  <=  K u / (1 - K u) * sum_k |h_k x_k|
# (no underflow: the products of these cases are far above 2^-1022).  Asserted with exact rationals; the largest fraction of the bound reached is printed
# (pytest -s -k derived_bound) and recorded in DESIGN.md section 7.
def _check_bound(what, acc64, terms_of):
    worst = 0.0
    for idx, got in acc64:
        terms = terms_of(idx)
        K = len(terms)
        exact, mag = sum(terms), sum(abs(t) for t in terms)
        bound = Fraction(K, 1 << 53) / (1 - Fraction(K, 1 << 53)) * mag
        err = abs(Fraction(float(got)) - exact)
        assert err <= bound, f"{what} {idx}: |model - exact| = {float(err):.3e} > {float(bound):.3e}"
        if bound:
            worst = max(worst, float(err / bound))
    print(f"\n{what}: largest fraction of the derived bound reached {worst:.4f}")
    return worst


def test_the_model_is_within_the_derived_bound_of_the_exact_sum_fir():
    case, i = fc.BY_ID["F1b"], 2                             # 131 taps
    taps, x = fc.fir_taps(case, i), fc.source(case, i, 0)[:fc.SPT]
    K = taps.size
    acc, _h = fm.fir(taps, np.zeros((K - 1, 2), F32), x, acc64=True)
    picks = [(n, ch) for n in list(range(0, 8)) + list(range(126, 140)) + list(range(600, 735, 9)) for ch in (0, 1)]
    terms = lambda p: [Fraction(float(taps[k])) * Fraction(float(x[p[0] - k, p[1]])) for k in range(K) if p[0] - k >= 0] + [Fraction(0)] * max(0, K - 1 - p[0])
    assert _check_bound("FIR F1b K = 131", [(p, acc[p]) for p in picks], terms) > 0.0


def test_the_model_is_within_the_derived_bound_of_the_exact_sum_resample():
    case = fc.BY_ID["R1_T4"]
    up, down, P, _cnt = case.members[0]
    tab, x = fc.table(case, 0, 0), fc.source(case, 0, 0)[:case.ticks * fc.SPT]
    acc, _h = fm.resample(tab[None], up, down, np.zeros((1, P - 1, 2), F32), 0, 0, x[None], 3200, acc64=True)
    picks = [(m, ch) for m in list(range(20, 60)) + list(range(3000, 3200, 7)) for ch in (0, 1)]
    def terms(p):
        n, ph = (p[0] * down) // up, (p[0] * down) % up
        return [Fraction(float(tab[ph, k])) * Fraction(float(x[n - k, p[1]])) for k in range(P)]
    assert _check_bound("Resample R1 160/147 P = 16", [(p, acc[0][p]) for p in picks], terms) > 0.0


# ------------------------------------------------------------------------------------------------
# (d) the case table reaches every branch
# ------------------------------------------------------------------------------------------------
def test_every_launcher_branch_is_drawn_by_a_case_at_256_compute_units():
    drawn = {}
    for case in fc.CASES:
        got = fc.launches(case, 256)
        assert sorted(k for k, _b, _w in got) == sorted(case.kernels), f"{case.id}: the launchers pick {got}, the table says {case.kernels}"
        for k, _b, _w in got:
            drawn.setdefault(k, []).append(case.id)
        if case.walks:
            assert len(got) == 1 and got[0][2] >= max(3, case.walks), f"{case.id}: a block walks {got[0][2]} groups, the case is there for {case.walks}"
    assert set(drawn) == set(fc.BRANCHES), f"not drawn: {set(fc.BRANCHES) - set(drawn)}"
    for kernel in ("k_resample_ps<160,16>", "k_resample<160>", "k_resample<0>"):
        assert any(fc.BY_ID[i].walks >= 3 and fc.BY_ID[i].kernels == (kernel,) for i in drawn[kernel]), f"{kernel}: no case walks several groups per block"
    # "n" channels keep the blocks per channel whatever the chip: 5 for the phase-stationary kernel, 8 for the staged one where its LDS allows 8 blocks
    for cus in (64, 228, 256, 304):
        assert fc.launches(fc.BY_ID["R1_T13"], cus)[0][1] == 5 and fc.launches(fc.BY_ID["R3c"], cus)[0][1] == 8
    # the switch of launch_fir sits where the tiled plan passes 64 KiB, on both tile sizes' side of it
    assert fc.fir_lds_plan(fc._K_LAST_TILED, fc.SPT)[1] <= fc.FIR_LDS_LIMIT < fc.fir_lds_plan(fc._K_LAST_TILED + 1, fc.SPT)[1]
    assert fc.fir_launch(128, 128 * fc.SPT)[0] == "k_fir<8>"                        # the benchmark's FIR leg never meets the plain kernel
    assert fc.fir_launch(16384, fc.SPT)[0] == "k_fir_plain" and fc.fir_lds_plan(16384, fc.SPT)[1] > 160 * 1024


def test_the_mixed_cases_meet_in_the_launches_they_name():
    assert [sorted(set(g)) for g in fc.groups(fc.BY_ID["R5m"], 256)] == [[1], [0, 2, 3]]      # 2/1 alone; 160/147 P 16, P 48 and 320/294 together
    assert [sorted(set(g)) for g in fc.groups(fc.BY_ID["R6m"], 256)] == [[0, 1]]
    assert len(fc.groups(fc.BY_ID["R6"], 256)) == 4 and len(fc.groups(fc.BY_ID["R2"], 256)) == 2


# ------------------------------------------------------------------------------------------------
# (e) every misreading changes a bit of a named case
# ------------------------------------------------------------------------------------------------
CAUGHT_BY = {
    "descending_taps": ("F5", "R9"),
    "f32_accumulation": ("F1b", "R1_T4"),
    "fma_in_exact_order": ("F5", "R9"),
    "round_per_tap": ("F1b", "R1_T4"),
    "phase_m_mod_up": ("R1_T4", "R2"),
    "n_rounded_up": ("R1_T4", "R3c"),
    "history_off_by_one": ("F1b", "R1_T4"),
    "history_dropped": ("F3", "R4b"),
    "table_transposed": ("R1_T4", "R6s"),
    "out_base_32bit": ("R7a_2p32", "R7b_2p40"),
    "history_lr_swapped": ("F1a", "R5b"),
}
assert set(CAUGHT_BY) == set(fm.MISREADINGS) and len(CAUGHT_BY) >= 10


@pytest.mark.parametrize("mis,case_id", [(m, c) for m, cs in CAUGHT_BY.items() for c in cs])
def test_every_misreading_changes_a_bit_of_a_named_case(mis, case_id):
    case = fc.BY_ID[case_id]
    n = 2                                                     # two channels are enough to see a bit change
    want, got = fc.model(case, n), fc.model(case, n, mis=mis)
    differ = sum(int(np.count_nonzero(bits(got[k]) != bits(want[k]))) for k in want)
    assert differ > 0, f"{mis} passes {case_id} unnoticed"
