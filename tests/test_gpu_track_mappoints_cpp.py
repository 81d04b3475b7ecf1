"""orbfe_cpp::MapPointTable's last-frame / key-frame searches (include/orbfe_classes.hpp) compiled with g++ against liborbfe.so
(tests/cpp/test_track_mappoints.cpp) on a world made by a formula both sides repeat: the class equals the Python binding, and
the projections equal tests/track_ref.py's spec32; refused operands throw."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import track_ref as tr
import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd.map_points import MapPoints, camera_pose

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
P, NKP, K = 150, 300, 3
BOUNDS = (0.0, 640.0, 0.0, 480.0)
K4, MBF = (500.0, 500.0, 320.0, 240.0), 40.0
f32 = np.float32


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("trackcpp") / "test_track_mappoints"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_track_mappoints.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return dict(t.split("=") for t in text.split())


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


def world():
    i = np.arange(P)
    slot = ((i * 7) % 256).astype(np.int32)
    Z = (4 + i % 13).astype(f32)
    pos = np.stack([((i * 37) % 41 - 20) * 0.25, ((i * 17) % 23 - 11) * 0.25, np.where(i % 29 == 5, -Z, Z)], axis=1).astype(f32)
    sc = dict(pos=pos, normal=np.tile(f32([0, 0, 1]), (P, 1)), max_dist=(2 * Z + i % 8).astype(f32), min_dist=(0.125 * Z).astype(f32),
              flags=((i % 19 == 7) * 1 | (i % 5 != 0) * 2).astype(np.uint8), skip=(i % 23 == 3).astype(np.uint8),
              last_octave=(i % 8).astype(np.int32), angle=((i * 11) % 360).astype(f32),
              desc=((i[:, None] * 7 + np.arange(32)[None, :] * 13) & 255).astype(np.uint8))
    sc["poses"] = [dict(Rcw=np.eye(3, dtype=f32), tcw=f32([0.015625 * k, 0, 0]), Ow=f32([-0.015625 * k, 0, 0])) for k in range(K)]
    j = np.arange(NKP)
    src = j % P
    x = np.minimum(np.maximum((f32(500) * pos[src, 0]) / Z[src] + f32(320) + (j % 3).astype(f32), f32(0)), f32(639)).astype(f32)
    y = np.minimum(np.maximum((f32(500) * pos[src, 1]) / Z[src] + f32(240) - (j % 2).astype(f32), f32(0)), f32(479)).astype(f32)
    d = sc["desc"][src] ^ (np.arange(32)[None, :] == (j % 32)[:, None]).astype(np.uint8)
    ur = np.where(j % 3 != 0, x - f32(40) / Z[src], f32(-1)).astype(f32)
    cur = dict(x=x, y=y, octave=((src + 3 * (j // P)) % 8).astype(np.int32), angle=((src * 11 + 20) % 360).astype(f32), desc=d, u_right=ur)
    return sc, slot, f32(1.25) ** np.arange(8, dtype=f32), cur


def test_cpp_track_searches_equal_the_binding(out):
    sc, slot, sf, cur = world()
    mp = MapPoints(256)
    mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
    poses = []
    for p in sc["poses"]:
        c = camera_pose(p["Rcw"], p["tcw"], K4, MBF, BOUNDS, 1.2, 8, Ow=p["Ow"])
        c.log_scale_factor = 0.25
        poses.append(c)
    Cur = amd.FrameView(cur["x"], cur["y"], cur["octave"], cur["desc"], BOUNDS, angle=cur["angle"], u_right=cur["u_right"])
    ref = dict(bounds=BOUNDS, scale=float(np.exp(f32(0.25))), K4=K4, mbf=MBF)
    one = dict(sc, poses=sc["poses"][:1], offsets=np.array([0, P], np.int32))
    want = tr.spec32(one, "last", **ref)["valid"]
    assert ints(out["last_valid"]) == want.tolist() == mp.project_last_frame(slot, sc["last_octave"], poses[0], sf, 7.0, skip=sc["skip"])["valid"].tolist()
    assert 20 < want.sum() < P
    counts, matches = [], []
    for mode in range(3):
        nm, match, valid = mp.SearchByProjectionLastFrame(Cur, slot, sc["last_octave"], sc["angle"], poses[0], sf, 7.0, mode=mode,
                                                          skip=sc["skip"], return_valid=True)
        assert int(out[f"last_n{mode}"]) == nm and ints(out[f"last_match{mode}"]) == match.tolist()
        counts.append(nm)
        matches.append(match)
    assert ints(out["last_searched"]) == valid.tolist() == want.tolist()
    assert min(counts) > 10 and len(matches) == 3, counts
    off = np.array([0, 60, 60, P])
    jobs = lambda a: [a[off[k]:off[k + 1]] for k in range(K)]  # noqa: E731
    three = dict(sc, offsets=off.astype(np.int32))
    kf = tr.spec32(three, "kf", **ref)
    pk = mp.project_keyframes(poses, jobs(slot), skips=jobs(sc["skip"]))
    assert ints(out["kf_valid"]) == kf["valid"].tolist() == np.concatenate([p["valid"] for p in pk]).tolist()
    assert ints(out["kf_level"]) == kf["level"].tolist() == np.concatenate([p["level"] for p in pk]).tolist()
    cnt, match = mp.SearchByProjectionKeyFrames(Cur, poses, jobs(slot), jobs(sc["angle"]), sf, [10.0, 3.0, 10.0], [100, 64, 100],
                                                skips=jobs(sc["skip"]))
    assert ints(out["kf_n"]) == cnt.tolist() and ints(out["kf_match"]) == match.reshape(-1).tolist()
    assert cnt[0] > 10 and cnt[1] == 0 and cnt[2] > 10, cnt
    assert int(out["threw"]) == 6
