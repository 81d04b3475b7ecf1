"""orbfe_cpp::Optimizer::LocalBundleAdjustment / BundleAdjustment (include/orbfe_classes.hpp) compiled with g++ against
liborbfe.so (tests/cpp/test_lba.cpp) on scenes this test writes: the class equals the C-ABI and the Python binding bit for bit,
a stop flag raised at entry leaves everything as it came, mismatched lengths and refused operands throw."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lba_ref as lr
from lba_check import read_result, write_scene
from test_gpu_lba import device_run

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lbacpp") / "test_lba"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_lba.cpp"), "-o", str(exe),
                    f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    return exe


@pytest.mark.parametrize("id_", ["l3f2p40-mixed", "local-is-fixed", "global-20-robust"])
def test_cpp_bundle_adjustment_equals_the_cabi_and_the_python_binding(exe, tmp_path, id_):
    sc, kind = next((s, k) for i, s, k in lr.gpu_scenes() if i == id_)
    write_scene(tmp_path / "scene.bin", sc, kind)
    out = subprocess.run([str(exe), str(tmp_path / "scene.bin"), str(tmp_path / "out.bin")], check=True, capture_output=True, text=True).stdout
    kv = dict(t.split("=") for t in out.split())
    assert int(kv["class_equal"]) == 1 and int(kv["stopped"]) == 1 and int(kv["threw"]) == 3, out
    got, want = read_result(tmp_path / "out.bin", sc), device_run(sc, kind)
    for k in ("Tcw", "xw", "erase", "edge_chi2"):
        assert np.array_equal(np.ascontiguousarray(got[k]).view(np.uint8), want[k].view(np.uint8)), (id_, k)
    if kind == "local":
        assert np.array_equal(got["level1"], want["level1"])
    for k in ("rounds", "iterations", "trials", "termination", "lam", "chi2"):
        assert got[k] == want[k], (id_, k)
