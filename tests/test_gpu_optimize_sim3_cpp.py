"""orbfe_cpp::Optimizer::OptimizeSim3 / OptimizeSim3Multi (include/orbfe_classes.hpp) compiled with g++ against liborbfe.so
(tests/cpp/test_optimize_sim3.cpp): the class equals the C-ABI on one mixed problem, vpMatches1 is erased at exactly
idx1[bad != 0], S12 is left alone on the early return, the multi form equals the single calls, mismatched lengths throw."""
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_optimize_sim3_equals_the_cabi(tmp_path):
    exe = tmp_path / "test_optimize_sim3"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_optimize_sim3.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    kv = dict(t.split("=") for t in out.split())
    assert int(kv["rounds"]) == 2 and int(kv["class_equal"]) == 1 and int(kv["erased_right"]) == 1 and int(kv["moved"]) == 1, out
    assert int(kv["planted"]) == int(kv["planted_erased"]) == 16 and 55 <= int(kv["n_in"]) <= 64, out
    assert int(kv["early_return"]) == 0 and int(kv["early_rounds"]) == 1 and int(kv["early_untouched"]) == 1, out
    assert int(kv["early_erased"]) == int(kv["early_n_bad"]) >= 4, out
    assert int(kv["multi_equal"]) == 1 and int(kv["threw"]) == 3, out
