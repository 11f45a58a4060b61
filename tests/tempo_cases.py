"""The shared cases of the tempo taps' tests: small parameter sets and hostile streams on which the model (tests/tempo_model.py), its slow
restatement and every deliberate misreading (tests/test_cpu_tempo.py) and the device (tests/test_gpu_tempo.py) are compared.  The shapes are the
smallest at which something can still go wrong: hops that straddle ticks, a hop that ends on a tick's last frame, ticks of one frame, L = W,
every hop length, more hops than W + L - 1 so that the window's far end holds onsets."""
import collections

import numpy as np

F32 = np.float32
Case = collections.namedtuple("Case", "id H W L emit F n_ticks channels")
CASES = [
    Case("straddle_50", 64, 64, 16, 1, 50, 220, 2),        # hops straddle ticks, an emission per tick
    Case("48k_800", 128, 128, 32, 3, 800, 40, 2),
    Case("44k1_735", 128, 96, 64, 3, 735, 40, 2),
    Case("odd_801_h256", 256, 256, 64, 5, 801, 110, 1),
    Case("l_equals_w", 64, 64, 64, 2, 800, 14, 2),         # 2 x 800 = 25 x 64: every second tick ends on a hop's last frame
    Case("one_frame", 64, 64, 16, 7, 1, 9000, 1),          # 63 of 64 ticks complete no hop; the first nine emissions come before any hop
]


def by_id(case_id):
    return next(c for c in CASES if c.id == case_id)


def hostile(seed, frames, channels):
    """seeded noise over a wide range with silent stretches and loud bursts (onsets), values above 4 and above 2^127 (finite L and R whose sum is
    not), +-Inf, NaN and subnormals, flat in the port's layout"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(frames * channels) * np.exp2(rng.integers(-9, 0, frames * channels))).astype(F32).reshape(frames, channels)
    at = 0
    while at < frames:                                      # stretches of a few hundred frames at very different levels
        n = int(rng.integers(40, 400))
        x[at:at + n] *= F32(rng.choice([0.0, 0.02, 0.3, 1.0, 3.0, 9.0]))
        at += n
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, min(24, flat.size // 4), replace=False)
    special = np.array([np.inf, -np.inf, np.nan, 4.0, -4.0, 4.0000005, 3.9999998, 2.0, 1e9, -3e38, 3.4e38, 100.0], F32)
    special = np.concatenate([special, np.array([1, 77, 0x7fffff, 0x80000001], np.uint32).view(F32), F32([-1e-41, 0.0, -0.0, 0.5, 2.0 ** -20, 2.0 ** -21, 1.9999999, 7.5])])
    flat[idx] = special[:idx.size]
    if channels == 2 and frames > 8:                        # finite L and R, L + R = +Inf; and Inf - Inf
        x[frames // 2] = F32(3e38); x[frames // 3] = (F32(np.inf), F32(-np.inf))
    return flat


def stream(case, seed=5):
    return hostile(seed, case.F * case.n_ticks, case.channels)
