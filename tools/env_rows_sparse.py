"""bench.py's headline with SPARSE Envelope ramps (profiles/env_rows/README.md): every strip's gate opens at tick 100 and closes at tick 1100 of
each 2048-tick submission, so with the default Envelope 44 of a strip's 2048 ticks ramp (32 after the opening, 12 after the closing) -- two or
three of the 64 lanes of a wave at a time, the real-desk case in which the lockstep form taxes the whole wave-tick for one ramping lane.
Usage, from the repository root:  python tools/env_rows_sparse.py [bench.py's arguments].  It replaces benchlegs' gate schedule and runs bench.py."""
import ctypes as C
import os
import runpy
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import benchlegs.common as common  # noqa: E402

OPEN_AT, CLOSE_AT = 100, 1100


def gate_open(tick, k):
    return False


def gate_events(abi, trigs, first_strip, t0, n_ticks):
    p_open, p_closed = abi.TriggerParams(1), abi.TriggerParams(0)
    po, pc = C.addressof(p_open), C.addressof(p_closed)
    at = [(t, p) for (t, p) in ((OPEN_AT, po), (CLOSE_AT, pc)) if t < n_ticks]
    if not at:
        return None
    ev = np.zeros(len(trigs) * len(at), dtype=np.dtype([("node", "<u4"), ("tick_in_run", "<u4"), ("params", "<u8"), ("params_len", "<u8")], align=True))
    assert ev.dtype.itemsize == C.sizeof(abi.ParamEvent)
    ev["node"] = np.repeat(np.asarray(trigs, dtype=np.uint32), len(at))
    ev["tick_in_run"] = np.tile([t for t, _ in at], len(trigs)); ev["params"] = np.tile([p for _, p in at], len(trigs))
    ev["params_len"] = C.sizeof(abi.TriggerParams)
    return ev.ctypes.data_as(C.POINTER(abi.ParamEvent)), len(ev), (ev, p_open, p_closed)


common.gate_open = gate_open
common.gate_events = gate_events
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[1:]
runpy.run_path(os.path.join(ROOT, "bench.py"), run_name="__main__")
