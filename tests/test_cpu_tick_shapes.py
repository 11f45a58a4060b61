"""The tick-shape table (tests/tick_shapes.py) agrees with itself and with the GPU file that runs it: every valid pair divides,
every invalid one does not, ids are unique, and the forms are ones mx_graph_debug_eq_launch can report."""
from mixlab_amd import abi
from tick_shapes import INVALID, SHAPES


def test_valid_shapes_divide_and_invalid_ones_do_not():
    for s in SHAPES:
        assert s.sample_rate % s.ticks_per_second == 0 and s.spt >= 1, s
    for sr, tps in INVALID:
        assert sr % tps != 0, (sr, tps)
    assert (22050, 60) in INVALID


def test_shape_ids_unique_and_forms_known():
    assert len({s.id for s in SHAPES}) == len(SHAPES)
    assert len({(s.sample_rate, s.ticks_per_second) for s in SHAPES}) == len(SHAPES)
    forms = set(abi.EQ_LAUNCH.values())
    for s in SHAPES:
        assert {s.fused, s.unfused, s.short} <= forms, s
        assert s.long_ticks >= 1 and s.why


def test_the_two_reference_shapes_stay_controls():
    pairs = {(s.sample_rate, s.ticks_per_second) for s in SHAPES}
    assert {(44100, 60), (48000, 60)} <= pairs


def test_gpu_file_runs_every_shape_of_the_table():
    import test_gpu_tick_shapes as gpu
    assert [p.values[0] for p in gpu.SHAPE_PARAMS] == SHAPES
    assert [p.id for p in gpu.SHAPE_PARAMS] == [s.id for s in SHAPES]
