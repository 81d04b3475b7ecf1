"""The key-frame-row methods of orbfe_cpp::ObservationGraph (include/orbfe_classes.hpp) compiled with g++ against
liborbfe.so (tests/cpp/test_kfpoints.cpp) on a world made by a formula both sides repeat: the class equals the Python
binding and the restatement (tests/kfpoints_ref.py); refused operands throw."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import kfpoints_ref as kr
import orb_slam2_annotate_amd as amd

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K, P, W = 20, 300, 64


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("kfpointscpp") / "test_kfpoints"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_kfpoints.cpp"), "-o", str(exe),
                    f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return dict(t.split("=") for t in text.split())


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


def world():
    g = amd.ObservationGraph(P, K, 8)
    g.set_keyframes(list(range(K)), [100 + 3 * k for k in range(K)], np.zeros((K, 3), np.float32))
    pts = list(range(P - 20))
    g.set_points(pts, [int(p % 13 == 5) for p in pts], [-1] * len(pts))
    w = kr.KeyFramePoints()
    w.bad = {p for p in pts if p % 13 == 5} | set(range(P - 20, P))
    for p in range(0, P - 20, 3):
        n = 4 if p % 6 == 0 else 3
        g.add_observations([p] * n, list(range(n)), [p] * n, [0] * n, [int(k == 3) for k in range(n)])
        w.n_obs[p] = n + int(n == 4)
    g.enable_keyframe_points(W)
    for k in range(K):
        n = 0 if k == 6 else (W if k == 7 else 40 + k)
        row = [-1 if (i * 5 + k) % 4 == 0 else (i * 7 + k * 31) % P for i in range(n)]
        g.set_keyframe_points(k, row)
        w.set_row(k, row)
    g.set_keyframe_points(15, [-1] * W)
    w.set_row(15, [-1] * W)
    for kf, idx, slot in ((15, 63, P - 21), (16, 0, P - 21), (2, 1, -1), (2, 2, 11)):
        g.assign_keyframe_points([kf], [idx], [slot])
        w.assign(kf, idx, slot)
    return g, w


def test_cpp_key_frame_rows_equal_the_binding_and_the_restatement(out):
    g, w = world()
    assert ints(out["row2"]) == g.get_keyframe_points(2).tolist() == [-1 if s is None else s for s in w.rows[2]]
    assert ints(out["row15_device"]) == g.get_keyframe_points(15, from_device=True).tolist() == [-1] * 63 + [P - 21]
    q = list(range(K))
    want = w.local_points(q)
    assert ints(out["local"]) == want == g.local_points(q).tolist() and want.count(P - 21) == 1 and len(want) > 7
    assert ints(out["local_small_capacity"]) == want
    for i, kfs in enumerate(([16, 15], [], [3, 3, 9])):
        assert ints(out[f"union{i}"]) == w.local_points(kfs), kfs
    for m in (0, 3, 4):
        want_n = [w.tracked_points(k, m) for k in q]
        assert ints(out[f"tracked{m}"]) == want_n == g.tracked_points(q, m).tolist(), m
    assert sum(ints(out["tracked0"])) > sum(ints(out["tracked3"])) > sum(ints(out["tracked4"])) > 0
    assert int(out["threw"]) == 4
    g.close()
