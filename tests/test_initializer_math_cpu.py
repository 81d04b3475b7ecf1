"""CPU: csrc/initializer_math.h -- the arithmetic the Initializer kernel compiles -- as a stand-alone program
(tests/cpp/initializer_cpu.cpp, -ffp-contract=off) against the numpy restatement tests/initializer_ref.py on every scene of the
GPU test, under the GPU test's pass condition.  This is the proof, without a device, that the one-sided Jacobi routine, the
rank-2 step, the inverse and the two scoring loops are right."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import initializer_ref as ir

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++") or shutil.which("g++")
    assert cxx, "no compiler to build the program with"
    out = tmp_path_factory.mktemp("initializer") / "initializer_cpu"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "tests" / "cpp"), str(ROOT / "tests" / "cpp" / "initializer_cpu.cpp"), "-o", str(out)], check=True)
    return out


def test_cpu_build_of_the_kernel_arithmetic_equals_the_reference(exe, tmp_path):
    s_model, s_score = ir.recorded()
    tol = (ir.allowance(s_model), ir.allowance(s_score))
    tot = dict(ill=0, guard=0, differ=0, d_model=0.0, d_score=0.0)
    for id_, sc in ir.gpu_scenes():
        ir.write_scene(tmp_path / "scene.txt", sc)
        subprocess.run([str(exe), str(tmp_path / "scene.txt"), str(tmp_path / "out.txt")], check=True, capture_output=True)
        r = ir.run(sc)
        score, status, n_inl, model, h12, words, rest = ir.read_result(tmp_path / "out.txt", len(r["status"]))
        c = ir.compare(id_, sc, r, score, status, n_inl, model, h12, words, np.array(rest, np.int32), tol)
        for k in ("ill", "guard", "differ"):
            tot[k] += c[k]
        tot["d_model"], tot["d_score"] = max(tot["d_model"], c["d_model"]), max(tot["d_score"], c["d_score"])
    print("not compared (ill-conditioned or degenerate):", tot["ill"], "guard-band decisions:", tot["guard"], "of which differ:",
          tot["differ"], "largest model distance:", tot["d_model"], "largest score distance:", tot["d_score"], "allowance:", tol)
