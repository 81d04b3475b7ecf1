"""orbfe_cpp::MapPointTable::Fuse (include/orbfe_classes.hpp) compiled with g++ against liborbfe.so
(tests/cpp/test_fuse_mappoints.cpp) on a world made by a formula both sides repeat: the class equals the Python binding and
the CPU oracle fed with tests/fuse_ref.py's projection; refused operands throw."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fuse_ref as fr
import oracle_lib as orc
import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd.map_points import MapPoints, camera_pose

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
P, NKP, K = 120, 600, 3
BOUNDS = (0.0, 640.0, 0.0, 480.0)
K4, MBF = (500.0, 500.0, 320.0, 240.0), 40.0


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fusecpp") / "test_fuse_mappoints"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_fuse_mappoints.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return dict(t.split("=") for t in text.split())


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


def world():
    i = np.arange(P)
    slot = ((i * 7) % 128).astype(np.int32)
    Z = (4 + i % 13).astype(np.float32)
    pos = np.stack([((i * 37) % 41 - 20) * 0.25, ((i * 17) % 23 - 11) * 0.25, Z], axis=1).astype(np.float32)
    normal = np.tile(np.float32([0, 0, 1]), (P, 1))
    sc = dict(pos=pos, normal=normal, max_dist=(2 * Z + i % 8).astype(np.float32), min_dist=(0.125 * Z).astype(np.float32),
              flags=(i % 19 == 7).astype(np.uint8), desc=((i[:, None] * 7 + np.arange(32)[None, :] * 13) & 255).astype(np.uint8))
    sf = np.float32(1.25) ** np.arange(8, dtype=np.float32)
    sc["poses"] = [dict(Rcw=np.eye(3, dtype=np.float32), tcw=np.float32([0.5 * k, 0, 0]), Ow=np.float32([-0.5 * k, 0, 0])) for k in range(K)]
    sc["skip"] = (np.arange(K * P) % 23 == 3).astype(np.uint8).reshape(K, P)
    sc["in_kf"] = np.zeros((K, P), bool)
    frames = []
    j = np.arange(NKP)
    for k in range(K):
        x, y = ((j * 53 + k * 11) % 640).astype(np.float32), ((j * 29 + k * 5) % 480).astype(np.float32)
        d = sc["desc"][j % P] ^ (np.arange(32)[None, :] == (j % 32)[:, None]).astype(np.uint8)
        ur = np.where(j % 3 != 0, x - 8, -1).astype(np.float32) if k == 1 else None
        frames.append(dict(x=x, y=y, octave=((j + k) % 8).astype(np.int32), desc=d, u_right=ur))
    return sc, slot, sf, frames


def test_cpp_fuse_equals_the_binding_and_the_oracle(out):
    sc, slot, sf, frames = world()
    isig = (np.float32(1) / (sf * sf)).astype(np.float32)
    mp = MapPoints(128)
    mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
    poses = []
    for p in sc["poses"]:
        c = camera_pose(p["Rcw"], p["tcw"], K4, MBF, BOUNDS, 1.2, 8, Ow=p["Ow"])
        c.log_scale_factor = 0.25
        poses.append(c)
    ang = np.zeros(NKP, np.float32)
    views = [amd.FrameView(f["x"], f["y"], f["octave"], f["desc"], BOUNDS, angle=ang, u_right=f["u_right"]) for f in frames]
    oracles = [orc.Frame(f["x"], f["y"], f["octave"], f["desc"], BOUNDS, angle=ang, u_right=f["u_right"]) for f in frames]
    pr = fr.spec32(sc, bounds=BOUNDS, scale=float(np.exp(np.float32(0.25))), K4=K4, mbf=MBF)
    got = mp.project_fuse(poses, slot, skip=sc["skip"])
    assert np.array_equal(got["valid"], pr["valid"])

    def oracle(pr, chi2):
        return np.stack([orc.fuse_search(Ko, sf, isig, pr["valid"][k], pr["u"][k], pr["v"][k], pr["ur"][k], pr["level"][k], sc["desc"],
                                         40.0, chi2) for k, Ko in enumerate(oracles)])

    gated, projected = mp.fuse(views, poses, slot, skip=sc["skip"], th=40.0, scale_factors=sf, inv_level_sigma2=isig, return_projected=True)
    assert ints(out["gated"]) == gated.reshape(-1).tolist() == oracle(got, True).reshape(-1).tolist()
    assert ints(out["projected"]) == projected.reshape(-1).tolist() == pr["valid"].reshape(-1).tolist()
    ungated = mp.fuse(views, poses, slot, skip=sc["skip"], th=40.0, chi2_gate=False, scale_factors=sf)
    assert ints(out["ungated"]) == ungated.reshape(-1).tolist() == oracle(got, False).reshape(-1).tolist()
    assert (ungated >= 0).sum() > 10 and (ungated != gated).any()
    # the graph: point i observes key frame i % 3 when i % 5 == 1
    i = np.arange(P)
    in_kf = np.stack([(i % 5 == 1) & (i % 3 == k) for k in range(K)])
    want = mp.fuse(views, poses, slot, skip=in_kf, th=40.0, chi2_gate=False, scale_factors=sf, return_projected=True)
    assert ints(out["graph"]) == want[0].reshape(-1).tolist()
    assert ints(out["graph_projected"]) == want[1].reshape(-1).tolist()
    assert (want[1] != mp.fuse(views, poses, slot, th=40.0, chi2_gate=False, scale_factors=sf, return_projected=True)[1]).any()
    assert int(out["threw"]) == 5
