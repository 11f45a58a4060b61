"""Host-side proof obligation of the envelope kernel's exact-division shortcut (see
mixlab_amd/csrc/mx_env_math.hpp: ms_of_u32, seq_ms): checked exhaustively for every sample distance the
fast path accepts (dt < 2^32, i.e. > 24 h of audio) at every sample rate of the tick-shape table (tests/tick_shapes.py).
Distances of 2^32 and more take the true division: tests/test_gpu_far_clock.py."""
import pathlib
import subprocess

import pytest

from tick_shapes import SHAPES

HERE = pathlib.Path(__file__).resolve().parent / "helpers"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fastdiv") / "fastdiv_check"
    subprocess.run(["gcc", "-O2", "-mfma", "-fopenmp", "-ffp-contract=off", str(HERE / "fastdiv_check.c"), "-o", str(exe), "-lm"], check=True)
    return exe


@pytest.mark.parametrize("rate", sorted({s.sample_rate for s in SHAPES}))
def test_markstein_quotient_is_ieee_quotient_for_all_dt_below_2_32(checker, rate):
    out = subprocess.run([str(checker), str(rate), "0", str(1 << 32)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "0", out.stdout + out.stderr


def test_scaler_window_origin_f64_formula_equals_integer_tap_spec(tmp_path):
    exe = tmp_path / "tap_origin_check"
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-std=c11", str(HERE / "tap_origin_check.c"), "-o", str(exe), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "mismatches 0" in out.stdout, out.stdout + out.stderr


def test_square_oscillator_exact_sign_of_sine_agrees_with_libm_on_52_million_arguments(tmp_path):
    exe = tmp_path / "sin_sign_check"
    subprocess.run(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-std=gnu11", str(HERE / "sin_sign_check.c"), "-o", str(exe), "-lm"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("0 /"), out.stdout + out.stderr
