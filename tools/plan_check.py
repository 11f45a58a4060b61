"""Build tools/plan_check.cpp with the host compiler's address and undefined-behaviour sanitizers and run it on the 1024-strip bench
graph and on three full random graphs (tests/test_gpu_random_graphs.py's draws, written out as flat arrays).  A plain executable:
no device, no Python in the checked process.  Usage: python tools/plan_check.py [build dir]"""
import pathlib
import shutil
import struct
import subprocess
import sys
import tempfile

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

from mixlab_amd import abi  # noqa: E402
from test_gpu_random_graphs import FULL_SEEDS, MAX_RUN, random_graph  # noqa: E402
from tick_shapes import by_id  # noqa: E402


def write_graph(path, ws, max_ticks, flags=0):
    out = [struct.pack("<6I", ws.sample_rate, ws.ticks_per_second, max_ticks, flags, len(ws.nodes), len(ws.edges))]
    for kind, p in ws.nodes:
        blob = abi.params_bytes(p)
        out.append(struct.pack("<II", kind, len(blob)) + blob)
    out += [struct.pack("<4I", *e) for e in ws.edges]
    path.write_bytes(b"".join(out))


def main(build_dir):
    build_dir = pathlib.Path(build_dir)
    rocm = pathlib.Path(shutil.which("hipcc") or "/opt/rocm/bin/hipcc").resolve().parent.parent
    cxx = rocm / "llvm" / "bin" / "clang++"
    exe = build_dir / "plan_check"
    subprocess.run([str(cxx if cxx.exists() else "clang++"), "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__",
                    "-I", str(rocm / "include"), str(ROOT / "tools" / "plan_check.cpp"), str(ROOT / "mixlab_amd" / "csrc" / "mx_plan.cpp"), "-o", str(exe)], check=True)
    files = []
    for shape_id, seed in (FULL_SEEDS[0], FULL_SEEDS[25], FULL_SEEDS[50]):
        shape = by_id(shape_id)
        ws, _sources = random_graph(seed, shape.sample_rate, shape.ticks_per_second, full=True)
        files.append(build_dir / f"graph_{shape_id}_{seed}.bin")
        write_graph(files[-1], ws, MAX_RUN)
    subprocess.run([str(exe), *map(str, files)], check=True)


if __name__ == "__main__":
    if len(sys.argv) > 1:
        main(sys.argv[1])
    else:
        with tempfile.TemporaryDirectory() as d:
            main(d)
