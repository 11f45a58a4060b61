"""The compact stdout line of bench.py (benchlegs/line.py) -- CPU test: the full record of the round-5 default run (profiles/r05/bench_default_line.json, the 20.8 KB
line the driver could not parse) goes through compact() and comes out within the cap, strict JSON, with the contract's keys; a NaN anywhere is refused."""
import json
import pathlib
import sys

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def _full():
    full = json.loads((ROOT / "profiles" / "r05" / "bench_default_line.json").read_text())
    full["config"]["sample_rate"] = 48000
    full["config"]["ticks_policy"] = "one GPU"
    return full


def test_the_round_5_record_compacts_to_a_line_within_the_target():
    from benchlegs import line
    full = _full()
    assert len(json.dumps(full)) > 16384                       # what broke the driver's parse
    text = line.dumps_checked(line.compact(full, "bench_full.json"))
    assert "\n" not in text and len(text.encode()) <= line.LINE_TARGET
    got = json.loads(text)
    for key in line.CONTRACT + ("config", "roofline", "cpu_baseline", "headline_parity", "legs", "full"):
        assert key in got, key
    for key in ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "avg_launch_ms", "algorithmic_bytes_per_launch"):
        assert key in got["roofline"], key
    assert set(got["cpu_baseline"]) == {"value", "unit", "cores", "kind", "sample"}
    assert got["legs"]["video_fps"] > 0 and got["legs"]["fir_f64_frac"] > 0 and got["legs"]["model_speedup_8_fixed_ticks"] > 0


def test_a_nan_or_an_oversized_line_is_refused():
    from benchlegs import line
    full = _full()
    c = line.compact(full, "bench_full.json")
    c["value"] = float("nan")
    with pytest.raises(ValueError):
        line.dumps_checked(c)
    c["value"] = 1.0
    c["config"]["workload"] = "x" * 9000
    with pytest.raises(AssertionError):
        line.dumps_checked(c)
    text = line.dumps_within_cap(c)                           # what bench.py calls: a run never ends without its line -- the optional parts go first
    got = json.loads(text)
    assert len(text) <= line.LINE_HARD_CAP and all(k in got for k in line.CONTRACT + ("roofline", "cpu_baseline", "config")) and got["roofline"] == c["roofline"]


def test_a_plain_run_leaves_everything_beside_the_headline_to_full():
    """bench.py without --full: no oracle replay, no repeats, no secondary leg, no CPU baseline, no record file unless one is named; --full turns them back on."""
    import bench
    plain = bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1"])
    assert not plain.full and plain.full_out is None and plain.no_headline_parity and plain.no_cpu_baseline and plain.no_held_leg and plain.no_realtime
    assert plain.repeats == plain.video_frames == plain.fir_ticks == 0 and not plain.no_profile
    full = bench.parse_args(["--gpus", "1", "--steps", "2", "--warmup", "1", "--full"])
    assert full.full and full.full_out == str(ROOT / "bench_full.json")
    assert not (full.no_headline_parity or full.no_cpu_baseline or full.no_held_leg or full.no_realtime or full.no_profile)
    assert full.repeats == 4 and full.video_frames == 4096 and full.fir_ticks == 128


def test_bench_py_stays_a_thin_assembler():
    n = len((ROOT / "bench.py").read_text().splitlines())
    assert n <= 400, f"bench.py has {n} lines: legs belong in benchlegs/"


def test_dump_outputs_keeps_a_fixed_seeded_tick_sample_under_the_cap(tmp_path, monkeypatch):
    """bench.py --dump-outputs (benchlegs/dump.py): written whole while it fits, above the cap the same seeded ticks of every bus, listed in ticks.npy."""
    import numpy as np
    from benchlegs import dump

    rng = np.random.default_rng(5)
    bufs = {"master": rng.standard_normal((40, 8, 2), dtype=np.float32), "cue": rng.standard_normal((40, 8, 2), dtype=np.float32)}
    assert dump.write(tmp_path / "whole", bufs) == {"master": [40, 8, 2], "cue": [40, 8, 2]}
    assert np.array_equal(np.load(tmp_path / "whole" / "master.npy"), bufs["master"]) and not (tmp_path / "whole" / "ticks.npy").exists()
    monkeypatch.setattr(dump, "CAP_BYTES", 40 * 8 * 2 * 4)                  # room for half of the ticks
    for run in ("a", "b"):
        dump.write(tmp_path / run, bufs)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == ["cue.npy", "master.npy", "ticks.npy"] and sum((tmp_path / "a" / f).stat().st_size for f in files) <= dump.CAP_BYTES + 3 * 128   # (+ .npy headers)
    ticks = np.load(tmp_path / "a" / "ticks.npy")
    assert ticks.dtype == np.float64 and ticks.size == (2560 - 8 * 40) // 128 and np.all(np.diff(ticks) > 0)
    for name in ("master", "cue"):
        got = np.load(tmp_path / "a" / f"{name}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, bufs[name][ticks.astype(int)])
    assert all(np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)) for f in files)
