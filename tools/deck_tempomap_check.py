"""Build tools/deck_tempomap_check.cpp with the host's address and undefined-behaviour sanitizers and run it: the pure host functions of the deck's tempo map
(mx_deck_tempomap_check / _count / _span / _host / _path / _segments / _at / _step) at the corners where an index or a shift could go wrong.  A plain executable: no
device, no Python in the checked process.  The program and mixlab_amd/csrc/mx_deck_tempomap.cpp are compiled instrumented (hipcc -Xarch_host -fsanitize=...); what else
they refer to comes from libmixlab_gpu.so, which must have been built.  Usage: python tools/deck_tempomap_check.py [build dir]"""
import os
import pathlib
import shutil
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
PKG = ROOT / "mixlab_amd"


def main(build_dir) -> str:
    """the program's output; raises CalledProcessError when the build, the program or a sanitizer fails"""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = pathlib.Path(build_dir) / "deck_tempomap_check"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-std=c++17", "-g", "-O1", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                    "-fno-sanitize-recover=all", "-x", "hip", str(ROOT / "tools" / "deck_tempomap_check.cpp"), str(PKG / "csrc" / "mx_deck_tempomap.cpp"),
                    f"-L{PKG}", "-lmixlab_gpu", f"-Wl,-rpath,{PKG}", "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], check=True, capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1", "UBSAN_OPTIONS": "print_stacktrace=1"})
    return run.stdout


if __name__ == "__main__":
    if len(sys.argv) > 1:
        print(main(sys.argv[1]), end="")
    else:
        with tempfile.TemporaryDirectory() as d:
            print(main(d), end="")
