"""orbfe_cpp::MapPointTable::SearchBySim3 / SearchByProjection (include/orbfe_classes.hpp) compiled with g++ against liborbfe.so
(tests/cpp/test_sim3_search_mappoints.cpp) on a world made by a formula both sides repeat: the class methods equal the Python
binding; refused operands throw."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd.map_points import MapPoints, camera_pose, sim3_leg

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
P, NKP, K = 120, 600, 2
BOUNDS = (0.0, 640.0, 0.0, 480.0)
K4 = (500.0, 500.0, 320.0, 240.0)


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("sim3cpp") / "test_sim3_search_mappoints"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_sim3_search_mappoints.cpp"),
                    "-o", str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return dict(t.split("=") for t in text.split())


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


def _leg(twx, tx):
    leg = sim3_leg(np.eye(3), [twx, 0, 0], np.eye(3), [tx, 0, 0], K4, BOUNDS, 1.2, 8)
    leg.log_scale_factor = 0.25
    return leg


def test_cpp_methods_equal_the_binding(out):
    i = np.arange(P)
    slot = ((i * 7) % 128).astype(np.int32)
    Z = (4 + i % 13).astype(np.float32)
    pos = np.stack([((i * 37) % 41 - 20) * 0.25, ((i * 17) % 23 - 11) * 0.25, Z], axis=1).astype(np.float32)
    desc = ((i[:, None] * 7 + np.arange(32)[None, :] * 13) & 255).astype(np.uint8)
    mp = MapPoints(128)
    mp.update(slot, pos, np.tile(np.float32([0, 0, 1]), (P, 1)), (0.125 * Z).astype(np.float32), (2 * Z + i % 8).astype(np.float32), desc,
              (i % 19 == 7).astype(np.uint8))
    sf = np.float32(1.25) ** np.arange(8, dtype=np.float32)
    j = np.arange(NKP)
    views = []
    for k in range(K + 1):
        x, y = ((j * 53 + k * 11) % 640).astype(np.float32), ((j * 29 + k * 5) % 480).astype(np.float32)
        # the first P keypoints of every frame sit on the projection of point j, where it is inside: KF1 and candidate 0 share a
        # camera, candidate 1 stands half a unit along x
        with np.errstate(all="ignore"):
            u = np.float32(500) * ((pos[:, 0] + np.float32(0.5 if k == 2 else 0.0)) / pos[:, 2]) + np.float32(320)
            v = np.float32(500) * (pos[:, 1] / pos[:, 2]) + np.float32(240)
        ins = (u >= 0) & (u < 640) & (v >= 0) & (v < 480)
        x[:P], y[:P] = np.where(ins, u, x[:P]), np.where(ins, v, y[:P])
        d = desc[j % P] ^ (np.arange(32)[None, :] == (j % 32)[:, None]).astype(np.uint8)
        views.append(amd.FrameView(x, y, ((j + (k > 0)) % 8).astype(np.int32), d, BOUNDS))
    slot1 = np.where(j % 4 == 0, -1, slot[j % P]).astype(np.int32)
    slot2 = [np.where(j % 5 == 0, -1, slot[np.where(j < P, j, (j * 3 + k) % P)]).astype(np.int32) for k in range(K)]
    matched = np.stack([np.where(j % 17 == 2, slot[(j + k) % P], -1) for k in range(K)]).astype(np.int32)
    already2 = [(j % 13 == 1).astype(np.uint8)] * K
    legs12, legs21 = [_leg(0.0, 0.0), _leg(0.0, 0.5)], [_leg(0.0, 0.0), _leg(0.5, -0.5)]
    cnt, match = mp.SearchBySim3(views[0], slot1, views[1:], slot2, legs12, legs21, sf, sf, 40.0)
    assert ints(out["found"]) == cnt.tolist() and ints(out["match12"]) == match.reshape(-1).tolist()
    assert (cnt > 0).all()  # both candidates, the translated one included
    cnt2, match2 = mp.SearchBySim3(views[0], slot1, views[1:], slot2, legs12, legs21, sf, sf, 40.0, matched12=matched, already2=already2)
    assert ints(out["found_masked"]) == cnt2.tolist() and ints(out["match12_masked"]) == match2.reshape(-1).tolist()
    assert (match2 != match).any()

    pose = camera_pose(np.eye(3), [0.5, 0, 0], K4, 40.0, BOUNDS, 1.2, 8, Ow=[-0.5, 0, 0])
    pose.log_scale_factor = 0.25
    n, m, proj = mp.SearchByProjectionSim3(views[1], slot, pose, sf, 40.0, matched=(j % 7 == 3).astype(np.uint8),
                                           skip=(i % 23 == 3).astype(np.uint8), return_projected=True)
    assert int(out["projection_n"]) == n and ints(out["projection"]) == m.tolist() and ints(out["projection_projected"]) == proj.tolist()
    assert n > 5
    assert int(out["threw"]) == 5
