"""OutputDevice without a GPU: the test-side restatement (tests/output_device_model.py) against cases worked by hand from
src/module/output_device.rs, and the C ABI's declaration of the kind against abi.py and the library's exports."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np

from mixlab_amd import abi
from output_device_model import ACTIVE, NONE, RECENT, OutputDeviceModel, temporal_warning

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = (ROOT / "include" / "mixlab_gpu.h").read_text()


def st(pairs):
    return np.asarray(pairs, dtype=np.float32).reshape(-1)


def test_left_equal_right_routes_right_and_tests_both():
    m = OutputDeviceModel(44100, 2, left=1, right=1)
    pushed, rec = m.run_tick(0, st([(0.5, 0.25), (2.0, -0.75)]))
    assert pushed.tolist() == [0.0, 0.25, 0.0, -0.75]    # right wins; channel 0 keeps the zeroed scratch
    assert rec[0] == 1                                    # the left sample 2.0 was tested, though right overwrote it


def test_nan_and_unit_values_do_not_clip_but_the_next_float_does():
    m = OutputDeviceModel(48000, 2, left=0, right=1)
    _, rec = m.run_tick(0, st([(np.nan, 1.0), (-1.0, np.nan)]))
    assert rec == (0, NONE, NONE, 0, 2)
    above = np.nextafter(np.float32(1.0), np.float32(2.0))
    _, rec = m.run_tick(800, st([(0.0, above), (0.0, 0.0)]))
    assert rec == (1, ACTIVE, NONE, 1, 2)
    m2 = OutputDeviceModel(48000, 2, left=0, right=1)
    _, rec = m2.run_tick(0, st([(-above, 0.0)]))
    assert rec[0] == 1


def test_unassigned_input_is_not_tested():
    m = OutputDeviceModel(44100, 4, left=2, right=None)
    pushed, rec = m.run_tick(0, st([(0.5, 7.0), (0.25, -9.0)]))
    assert rec[0] == 0
    assert pushed.tolist() == [0, 0, 0.5, 0, 0, 0, 0.25, 0]


def test_two_to_four_channels_leaves_stale_samples():
    m = OutputDeviceModel(44100, 2, left=0, right=1)
    m.run_tick(0, st([(0.1, 0.2), (0.3, 0.4)]))          # scratch = [.1 .2 .3 .4]
    m.update(4, 0, 1)                                      # same assignment: not zeroed
    pushed, rec = m.run_tick(735, st([(0.5, 0.6), (0.7, 0.8)]))
    f = np.float32
    assert pushed.tolist() == [f(0.5), f(0.6), f(0.3), f(0.4), f(0.7), f(0.8), 0.0, 0.0]   # channels 2 and 3 of frame 0: the 2-channel frame 1
    assert rec[4] == 4


def test_repeated_out_of_range_request_zeroes_again():
    m = OutputDeviceModel(44100, 2, left=0, right=5)       # right filtered to None
    assert m.right is None
    m.run_tick(0, st([(0.5, 0.5)]))
    m.scratch[1] = 0.75                                    # stand-in for what an earlier layout left there
    m.update(2, 0, 5)                                      # stored None != requested 5: zeroed again
    assert m.scratch.tolist() == [0.0, 0.0]
    m.update(2, 0, None)
    m.scratch[:] = 0.5
    m.update(2, 0, None)                                   # same as stored: kept
    assert m.scratch.tolist() == [0.5, 0.5]


def test_no_stream_keeps_assignment_and_writes_nothing():
    m = OutputDeviceModel(44100, 2, left=1, right=0)
    m.update(0, 0, 0)
    assert (m.left, m.right) == (1, 0)
    pushed, rec = m.run_tick(0, st([(5.0, 5.0)]))
    assert pushed.size == 0 and rec == (0, NONE, NONE, 0, 0)
    m.update(6, 1, 0)                                      # same as stored: no zeroing
    assert (m.left, m.right) == (1, 0)


def test_status_boundaries_at_6_and_300_ticks():
    for rate, spt in ((44100, 735), (48000, 800)):
        assert temporal_warning(5 * spt, 0, rate) == ACTIVE
        assert temporal_warning(6 * spt, 0, rate) == RECENT   # exactly 100 ms: not Active
        assert temporal_warning(299 * spt, 0, rate) == RECENT
        assert temporal_warning(300 * spt, 0, rate) == NONE   # exactly 5 s
        m = OutputDeviceModel(rate, 2, left=0, right=1)
        recs = [m.run_tick(0, st([(1.5, 0.0)]))[1]]
        recs += [m.run_tick(k * spt, st([(0.0, 0.0)]))[1] for k in range(1, 302)]
        changed = [k for k, r in enumerate(recs) if r[3]]
        assert changed == [0, 6, 300]
        assert [recs[k][1] for k in (0, 5, 6, 299, 300)] == [ACTIVE, ACTIVE, RECENT, RECENT, NONE]


def test_lag_note_is_taken_by_the_next_tick():
    m = OutputDeviceModel(44100, 2, left=0, right=1)
    m.note_lag()
    _, r0 = m.run_tick(0, st([(0, 0)]))
    _, r1 = m.run_tick(735, st([(0, 0)]))
    assert r0[2] == ACTIVE and r0[3] == 1 and r1[2] == ACTIVE and r1[3] == 0 and not m.lag_flag


def test_header_declares_the_kind_struct_and_entry_points_as_abi_py_does():
    assert re.search(r"MX_KIND_OUTPUT_DEVICE\s*=\s*18\b", HEADER) and re.search(r"MX_KIND_COUNT\s*=\s*19\b", HEADER)
    assert re.search(r"#define\s+MX_PROFILE_KINDS\s+18\b", HEADER)
    assert abi.KIND_OUTPUT_DEVICE == 18 and abi.KIND_COUNT == 19 and len(abi.KIND_NAMES) == abi.KIND_COUNT and abi.PROFILE_KINDS == 18
    assert re.search(r"typedef struct \{ uint32_t channels; int32_t left, right; uint32_t _pad; \} mx_output_device_params;", HEADER)
    assert ctypes.sizeof(abi.OutputDeviceParams) == 16 and ctypes.sizeof(abi.AudioOutTick) == 8 and abi.AUDIO_OUT_TICK_DTYPE.itemsize == 8
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    for name in ("mx_graph_read_audio_out", "mx_graph_audio_out_lag"):
        assert re.search(rf"\b{name}\s*\(", HEADER)
        assert re.search(rf" T {name}$", out, flags=re.M)
        assert hasattr(abi.lib, name)


def test_per_module_path_refuses_the_kind():
    h = ctypes.c_void_p()
    p = abi.OutputDeviceParams(2, 0, 1, 0)
    rc = abi.lib.mx_module_create(abi.KIND_OUTPUT_DEVICE, ctypes.byref(p), ctypes.sizeof(p), ctypes.byref(h))
    assert rc == abi.MX_ERR_INVALID
