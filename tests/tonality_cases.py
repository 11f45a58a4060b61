"""The shared cases of the tonality taps' tests: small parameter sets and hostile streams on which the model (tests/tonality_model.py), its
slow restatement and every deliberate misreading (tests/test_cpu_tonality.py) and the device (tests/test_gpu_tonality.py) are compared.  The
shapes are the smallest at which something can still go wrong: decimated frames and hops that straddle ticks, a hop whose last input frame is
a tick's last or the next tick's first, ticks of one frame, a kernel as long as the carried history, both decimations, every hop length."""
import collections

import numpy as np

F32 = np.float32
Case = collections.namedtuple("Case", "id rate D Hc O f_lo_mhz emit F n_ticks channels")
CASES = [
    Case("short_50", 48000, 4, 128, 2, 440000, 1, 50, 48, 2),          # N_0 = 464; 2400 frames: 600 decimated, 4 hops; an emission per tick
    Case("48k_800", 48000, 4, 128, 2, 440000, 3, 800, 12, 2),
    Case("44k1_735", 44100, 4, 256, 3, 220000, 2, 735, 12, 1),
    Case("odd_801", 48060, 8, 128, 2, 440000, 5, 801, 12, 2),
    Case("last_frame_509", 30540, 4, 128, 2, 440000, 1, 509, 5, 2),    # hop 0's last input frame, 127 x 4 = 508, is tick 0's last frame
    Case("first_frame_508", 30480, 4, 128, 2, 440000, 1, 508, 5, 1),   # ... is tick 1's first frame
    Case("long_kernel", 48000, 8, 512, 2, 50000, 4, 800, 24, 2),       # N_0 = 2040; hop 3 ends at decimated frame 2047 and reads back to frame 8
    Case("one_frame", 8000, 4, 128, 2, 100000, 7, 1, 600, 1),          # hop 0 is complete in tick 508: 72 emissions before any hop
]


def by_id(case_id):
    return next(c for c in CASES if c.id == case_id)


def hostile(seed, frames, channels):
    """seeded noise over a wide range with silent stretches and loud bursts, +-2 and its neighbours as the mid signal sees them (a mono x = 1, a
    stereo pair that sums to 2), values above 2^127 (finite L and R whose sum is not), +-Inf, NaN and subnormals, flat in the port's layout"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(frames * channels) * np.exp2(rng.integers(-9, 0, frames * channels))).astype(F32).reshape(frames, channels)
    at = 0
    while at < frames:                                      # stretches of a few hundred frames at very different levels
        n = int(rng.integers(40, 400))
        x[at:at + n] *= F32(rng.choice([0.0, 0.02, 0.3, 1.0, 3.0, 9.0]))
        at += n
    flat = x.reshape(-1)
    idx = rng.choice(flat.size, min(30, flat.size // 4), replace=False)
    special = np.array([np.inf, -np.inf, np.nan, 2.0, -2.0, 2.0000002, 1.9999999, -1.9999999, 1.0, -1.0, 1.0000001, 0.99999994, -0.99999994, 4.0, 1e9, -3e38,
                        3.4e38, 100.0], F32)
    special = np.concatenate([special, np.array([1, 77, 0x7fffff, 0x80000001], np.uint32).view(F32),
                              F32([-1e-41, 0.0, -0.0, 0.5, 2.0 ** -13, 2.0 ** -14, -(2.0 ** -14), 1.5 * 2.0 ** -13])])
    flat[idx] = special[:idx.size]
    if frames > 12:                                         # m = +-2 and its neighbours exactly, whatever the layout
        for k, m in enumerate(F32([2.0, -2.0, 2.0000002, 1.9999999, -2.0000002, -1.9999999])):
            x[5 + k] = m / F32(2.0)
    if channels == 2 and frames > 8:                        # finite L and R, L + R = +Inf; and Inf - Inf
        x[frames // 2] = F32(3e38); x[frames // 3] = (F32(np.inf), F32(-np.inf))
    return flat


def stream(case, seed=5):
    return hostile(seed, case.F * case.n_ticks, case.channels)
