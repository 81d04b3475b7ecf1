"""orbfe_cpp::ORBmatcher::TriangulateMatchesMulti / TriangulateMatches (include/orbfe_classes.hpp) compiled with g++ against
liborbfe.so (tests/cpp/test_triangulate.cpp) on one mixed scene: the pass condition of tests/test_gpu_triangulate.py."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import triangulate_ref as tr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_layer_equals_the_reference(tmp_path):
    exe = tmp_path / "test_triangulate"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tests' / 'cpp'}",
                    str(ROOT / "tests/cpp/test_triangulate.cpp"), "-o", str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"],
                   check=True)
    sc = dict(tr.gpu_scenes(full=False))[tr.CPP_ID]
    tr.write_scene(tmp_path / "scene.txt", sc)
    out = subprocess.run([str(exe), str(tmp_path / "scene.txt"), str(tmp_path / "out.txt")], check=True, capture_output=True,
                         text=True).stdout
    kv = dict(t.split("=") for t in out.split())
    assert int(kv["single_equal"]) == 1 and int(kv["resident_equal"]) == 1, out
    K, n1 = sc["K"], sc["n1"]
    status, x3d, rest = tr.read_result(tmp_path / "out.txt", K, n1)
    tr.compare(tr.CPP_ID, tr.run(sc), status, x3d, np.array(rest[:K], np.int32), np.array(rest[K:], np.int32), tr.s_tri())
