"""CPU: csrc/initializer_reconstruct_math.h -- the arithmetic k_init_reconstruct.hip compiles -- as a stand-alone program
(tests/cpp/initializer_reconstruct_cpu.cpp, -ffp-contract=off) against the numpy restatement
tests/initializer_reconstruct_ref.py on every scene of the GPU test, under the GPU test's pass condition.  This is the proof,
without a device, that the 3 x 3 Jacobi SVD with its u_2 rule, Faugeras' and DecomposeE's formulas, CheckRT and the bisection
are right."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

import initializer_reconstruct_ref as rr

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++") or shutil.which("g++")
    assert cxx, "no compiler to build the program with"
    out = tmp_path_factory.mktemp("reconstruct") / "initializer_reconstruct_cpu"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "tests" / "cpp"), str(ROOT / "tests" / "cpp" / "initializer_reconstruct_cpu.cpp"), "-o", str(out)],
                   check=True)
    return out


def test_cpu_build_of_the_kernel_arithmetic_equals_the_reference(exe, tmp_path):
    worst = [0.0, 0.0, 0.0]
    for id_, sc, r in rr.scenes():
        rr.write_scene(tmp_path / "scene.txt", sc)
        subprocess.run([str(exe), str(tmp_path / "scene.txt"), str(tmp_path / "out.txt")], check=True, capture_output=True)
        out, _ = rr.read_result(tmp_path / "out.txt", sc)
        d = rr.compare(id_, sc, r, rr.split(sc, out))
        worst = [max(a, b) for a, b in zip(worst, d)]
    print("largest motion / point (relative) / cosine distances:", worst, "noise recorded:", rr.recorded())
