"""CPU: csrc/triangulate_math.h -- the arithmetic the triangulation kernel compiles -- as a stand-alone program
(tests/cpp/triangulate_cpu.cpp, -ffp-contract=off) against the numpy restatement tests/triangulate_ref.py on every scene of the
GPU test: status identical for every pair, every accepted point within the GPU test's tolerance.  This is the proof, without
a device, that the Jacobi routine and the branch logic are right."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import triangulate_ref as tr

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++") or shutil.which("g++")
    assert cxx, "no compiler to build the program with"
    out = tmp_path_factory.mktemp("tri") / "triangulate_cpu"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "tests" / "cpp"), str(ROOT / "tests" / "cpp" / "triangulate_cpu.cpp"),
                    "-o", str(out)], check=True)
    return out


def test_cpu_build_of_the_kernel_arithmetic_equals_the_reference(exe, tmp_path):
    s = tr.s_tri()
    for id_, sc in tr.gpu_scenes():
        tr.write_scene(tmp_path / "scene.txt", sc)
        subprocess.run([str(exe), str(tmp_path / "scene.txt"), str(tmp_path / "out.txt")], check=True, capture_output=True)
        K, n1 = sc["K"], sc["n1"]
        status, x3d, rest = tr.read_result(tmp_path / "out.txt", K, n1)
        tr.compare(id_, tr.run(sc), status, x3d, np.array(rest[:K], np.int32), np.array(rest[K:], np.int32), s)
