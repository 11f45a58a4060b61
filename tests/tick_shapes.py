"""The tick shapes the graph ABI accepts beyond the two the reference runs at (44 100 and 48 000 Hz at 60 ticks/s).

mx_graph_opts takes any sample rate and tick rate whose quotient is whole (Graph::Graph refuses the rest).  The exact EqThree
path decides its chunk unit, warm-up and kernel form from the tick length, so each shape below is listed for the branch it
reaches.  The forms are what mx_graph_debug_eq_launch reports (abi.EQ_LAUNCH) for the first EqThree group of SHAPE_STRIPS
config-2 strips (tests/test_gpu_tick_shapes.py):

  fused     default flags, a submission of `long_ticks` ticks (the inline Envelope: EQM_AMP_ENV, mono store)
  unfused   MX_FLAG_NO_FUSE, the same submission (a plain EqThree)
  short     default flags, one tick

Importable without a GPU (tests/test_cpu_tick_shapes.py checks the table itself).
"""
from __future__ import annotations

from dataclasses import dataclass

SHAPE_STRIPS = 8


@dataclass(frozen=True)
class TickShape:
    id: str
    sample_rate: int
    ticks_per_second: int
    long_ticks: int        # ticks of a submission the planner speculates on (where it speculates at all)
    fused: str             # expected launch form of the long submission, fused strips
    unfused: str           # ... MX_FLAG_NO_FUSE
    short: str             # ... one tick, fused
    why: str

    @property
    def spt(self) -> int:
        return self.sample_rate // self.ticks_per_second


SHAPES = [
    TickShape("44k1", 44100, 60, 32, "ragged_tick", "tiled", "sequential", "735: today's 44.1 kHz control; 4-tick unit (2 940)"),
    TickShape("48k", 48000, 60, 16, "tiled", "tiled", "sequential", "800: today's 48 kHz control; whole-tick chunks"),
    TickShape("96k", 96000, 60, 16, "tiled", "tiled", "sequential", "1 600: aligned tiled kernel, 2 688-sample warm-up"),
    TickShape("192k", 192000, 60, 8, "tiled", "tiled", "sequential", "3 200: aligned tiled kernel, 5 376-sample warm-up"),
    TickShape("48k_40", 48000, 40, 16, "ragged_tick", "tiled", "sequential", "1 200 = 16 (mod 32): the RT kernel on ticks of whole 16-sample rows"),
    TickShape("88k2", 88200, 60, 32, "ragged_tick", "tiled", "sequential", "1 470 = 2 (mod 4): 2-tick chunk unit, RT kernel"),
    TickShape("44k1_100", 44100, 100, 32, "ragged_tick", "tiled", "sequential", "441, odd: 4-tick unit (1 764)"),
    TickShape("48k_1000", 48000, 1000, 128, "direct", "tiled", "sequential", "48 < 64, multiple of 16: direct kernel with an inline Envelope"),
    TickShape("42k_1000", 42000, 1000, 128, "direct", "tiled", "sequential", "42: 32 <= tick < 64, not a multiple of 16 (84-sample unit)"),
    TickShape("16k_1000", 16000, 1000, 128, "direct", "tiled", "sequential", "16: tick < 32"),
    TickShape("8k_8000", 8000, 8000, 2048, "direct", "tiled", "sequential", "1: one sample per tick"),
    TickShape("11k025_25", 11025, 25, 32, "ragged_tick", "tiled", "sequential", "441 at 11 025 Hz: high-band pole negative (p = -0.39)"),
    TickShape("6k", 6000, 60, 128, "ragged_tick", "tiled", "sequential", "100 at 6 kHz: p_hi = -0.975, forgets in 9 088 samples (3 072-sample warm-up)"),
    TickShape("5k4", 5400, 60, 128, "sequential", "sequential", "sequential", "90 at 5.4 kHz: p_hi = -1, never forgets: no speculation"),
    TickShape("44k1_1", 44100, 1, 3, "ragged_tick", "tiled", "direct", "44 100: a tick longer than any chunk (one tick: chunks inside the tick)"),
]

# Pairs Graph::Graph refuses with MX_ERR_INVALID: the tick is not a whole number of samples.
INVALID = [(22050, 60), (44100, 8), (48000, 7), (8000, 3), (30, 60), (44100, 88200)]


def by_id(shape_id: str) -> TickShape:
    return next(s for s in SHAPES if s.id == shape_id)


# The clock started far from zero (tests of absolute time: tests/test_gpu_far_clock.py and the `far` parametrisations elsewhere).
FAR_EPOCHS = ("below_2p31", "across_2p32", "at_2p40")


def far_first_tick(epoch: str, spt: int, n_ticks: int) -> int:
    """The first tick of a stretch of n_ticks ticks of spt samples that
      below_2p31   ends just below sample time 2^31 (every sample time still fits a signed 32-bit integer),
      across_2p32  holds sample time 2^32 in its tick of index n_ticks // 2 (at that tick's first sample where spt divides 2^32),
      at_2p40      starts at the first tick boundary at or after sample time 2^40."""
    if epoch == "below_2p31":
        return (1 << 31) // spt - n_ticks - 1
    if epoch == "across_2p32":
        return (1 << 32) // spt - n_ticks // 2
    assert epoch == "at_2p40"
    return -(-(1 << 40) // spt)
