"""orbfe_cpp::Optimizer::PoseOptimization (include/orbfe_classes.hpp) compiled with g++ against liborbfe.so: the array form
and the MapPointTable form equal the C-ABI on one mixed problem (tests/cpp/test_pose_opt.cpp)."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_optimizer_equals_the_cabi(tmp_path):
    exe = tmp_path / "test_pose_opt"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_pose_opt.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    kv = dict(t.split("=") for t in out.split())
    assert int(kv["rounds"]) == 4 and int(kv["array_equal"]) == 1 and int(kv["table_equal"]) == 1, out
    assert int(kv["planted"]) == int(kv["planted_flagged"]) == 60 and 150 < int(kv["inliers"]) <= 240, out
