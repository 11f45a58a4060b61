"""The device's Fir and Resample kernels against the independent numpy model (tests/fir_model.py), directly: no oracle in between.

Every case of tests/fir_cases.py runs through a built graph, "n" channels being one per compute unit of the device, so the shapes -- not an
environment switch -- select k_fir<4>, k_fir<8>, k_fir_plain, k_resample_ps<160,16>, k_resample<160>, k_resample<0> and k_resample_gather, with blocks
walking several 256-output groups where a case says so (tests/test_cpu_fir_model.py checks the table against the launchers' restatement).  Every output port of every channel is compared with the model over all submissions of a case, so the
history a submission leaves is compared through the next one.

  default flags          bit for bit
  MX_FLAG_FP_CONTRACT    bit for bit where the model has an exact FMA (the fma_exact cases, or every case under an interpreter with math.fma); else
                         within 1 ULP of the uncontracted model (2^-40 absolute at a zero crossing), no sample beyond

The FIR cases also run through mx_module_run_tick, one module per member, state carried from call to call.  tests/test_cpu_fir_model.py shows that each
of fir_model.MISREADINGS changes a bit of one of these cases.  The grid-stride repeat of k_fir (over 2 M frames per channel) is left out.
"""
import struct

import numpy as np
import pytest

import fir_cases as fc
import fir_model as fm
from fir_cases import assert_same_bits, assert_within_one_ulp, bits
from mixlab_amd import abi

pytestmark = pytest.mark.gpu

F32 = np.float32
FLAGS = [pytest.param(0, id="exact"), pytest.param(abi.FLAG_FP_CONTRACT, id="contracted")]


@pytest.fixture(scope="module")
def n_cus():
    """multi_processor_count of device 0, asked of the HIP runtime the library itself has loaded (hipDeviceAttributeMultiprocessorCount = 63 in
    hip_runtime_api.h); launch_resample's own fallback, 256, where it cannot be asked"""
    import ctypes as C
    assert abi.lib.mx_device_count() > 0
    try:
        with open("/proc/self/maps") as maps:
            path = next(line.split()[-1] for line in maps if "libamdhip64.so" in line)
        hip, v = C.CDLL(path), C.c_int(0)
        if hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and 8 <= v.value <= 1024:
            return int(v.value)
    except (OSError, StopIteration, AttributeError):
        pass
    return 256


def compare(case, n, flags, key, got, what):
    if not flags:
        return assert_same_bits(got, fc.model(case, n)[key], what)
    if fm.HAVE_FAST_FMA or case.fma_exact:
        assert_same_bits(got, fc.model(case, n, "contracted")[key], what + ", contracted")
    assert_within_one_ulp(got, fc.model(case, n)[key], what + ", contracted against the exact order")


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("case", fc.CASES, ids=[c.id for c in fc.CASES])
def test_graph_equals_the_model(case, flags, n_cus):
    ws, nodes = fc.workspace(case, n_cus)
    g = ws.build(max_ticks_per_run=case.ticks, flags=flags)
    per_run = 2 * case.ticks * fc.SPT
    src = {(i, c): fc.source(case, i, c).reshape(-1) for i, c, s, _n in nodes if s is not None}
    got = {(i, c): [] for i, c, _s, _n in nodes}
    for r in range(case.runs):
        for i, c, s, _n in nodes:
            if s is not None:
                g.write_source(s, src[i, c][r * per_run:(r + 1) * per_run], case.ticks)
        g.run_ticks(case.first_tick + r * case.ticks, case.ticks)
        for i, c, _s, node in nodes:
            got[i, c].append(g.read_output(node, 0, case.ticks, True, rate=fc.rate(case, i)))
    g.close()
    for i, c, _s, _n in nodes:
        y = np.concatenate(got[i, c])
        compare(case, n_cus, flags, (i, c), y, f"{case.id} ({', '.join(case.kernels)}) member {i} channel {c}")
        if not case.connected:
            assert not bits(y).any(), f"{case.id}: a disconnected input must give +0.0 in every bit"


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("case", fc.FIR, ids=[c.id for c in fc.FIR])
def test_module_fir_equals_the_model(case, flags, n_cus):
    frames = case.ticks * fc.SPT
    for i, K in enumerate(case.members):
        m = abi.Module(abi.KIND_FIR, struct.pack("<II", K, 0) + fc.fir_taps(case, i).tobytes(), flags=flags)
        x = fc.source(case, i, 0).reshape(-1)
        got = np.empty(2 * frames * case.runs, F32)
        for r in range(case.runs):                                   # the history is carried from call to call
            sl = slice(r * 2 * frames, (r + 1) * 2 * frames)
            m.run_tick(r * frames, [(abi.MX_STEREO, x[sl]) if case.connected else (abi.MX_DISCONNECTED, None)], [(abi.MX_STEREO, got[sl])])
        m.close()
        compare(case, n_cus, flags, (i, 0), got, f"module FIR {case.id} member {i} (K = {K}: {fc.fir_launch(K, frames)[0]})")
