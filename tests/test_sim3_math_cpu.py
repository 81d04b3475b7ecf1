"""CPU: csrc/sim3_math.h -- the arithmetic the Sim3 kernel compiles -- as a stand-alone program (tests/cpp/sim3_cpu.cpp,
-ffp-contract=off) against the numpy restatement tests/sim3_ref.py on every scene of the GPU test, under the GPU test's pass
condition.  This is the proof, without a device, that the Jacobi routine, the rotation and the inlier test are right."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sim3_ref as sr

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++") or shutil.which("g++")
    assert cxx, "no compiler to build the program with"
    out = tmp_path_factory.mktemp("sim3") / "sim3_cpu"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "tests" / "cpp"), str(ROOT / "tests" / "cpp" / "sim3_cpu.cpp"), "-o", str(out)], check=True)
    return out


def test_cpu_build_of_the_kernel_arithmetic_equals_the_reference(exe, tmp_path):
    s = sr.s_sim3()
    ill = guard = differ = 0
    for id_, sc in sr.gpu_scenes():
        sr.write_scene(tmp_path / "scene.txt", sc)
        subprocess.run([str(exe), str(tmp_path / "scene.txt"), str(tmp_path / "out.txt")], check=True, capture_output=True)
        r = sr.run(sc)
        n_inl, status, sim3, words, rest = sr.read_result(tmp_path / "out.txt", len(r["status"]))
        a, b, c = sr.compare(id_, sc, r, n_inl, status, sim3, words, np.array(rest, np.int32), s)
        ill += a; guard += b; differ += c
    print("not compared (ill-conditioned or degenerate):", ill, "guard-band decisions:", guard, "of which differ:", differ)
