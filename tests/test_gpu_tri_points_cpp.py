"""The triangulated-point methods of include/orbfe_classes.hpp (ORBmatcher::TriangulatedPointsSelect,
MapPointTable::CreateTriangulatedPoints) compiled with g++ against liborbfe.so (tests/cpp/test_tri_points.cpp) on the
70-keypoint mixed scene of tests/test_gpu_tri_points.py, written to a file, with descriptors made by a formula both sides
repeat: the classes equal the Python binding and the restatement (tests/tri_points_ref.py); refused operands throw."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import orb_slam2_annotate_amd as amd
import tri_points_ref as ref
import triangulate_ref as tr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
SPEC = dict(seed=7, n1=70, K=3, kind="mixed", n_pairs=110)
KF_SLOTS, KF_IDS = [1, 3, 0, 4], [10, 3, 30, 11]


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


def floats(s):
    return np.array(ints(s), np.uint32).view(f32)


def test_cpp_tri_points_equal_the_binding_and_the_restatement(tmp_path):
    sc = tr.scene(**SPEC)
    scene_file = tmp_path / "scene.txt"
    tr.write_scene(scene_file, sc)
    exe = tmp_path / "test_tri_points"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tests/cpp'}",
                    str(ROOT / "tests/cpp/test_tri_points.cpp"), "-o", str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    text = subprocess.run([str(exe), str(scene_file)], check=True, capture_output=True, text=True).stdout
    out = dict(t.split("=") for t in text.split())
    assert "error" not in out, out

    K, n1 = sc["K"], sc["n1"]
    fr = [sc["kf1"]] + sc["kf2"]
    desc = [((np.arange(f["n"])[:, None] * 131 + np.arange(32)[None, :] * 17 + j * 7) % 256).astype(np.uint8) for j, f in enumerate(fr)]
    frames = [amd.FrameView(f["x"], f["y"], f["octave"], d, (0.0, 640.0, 0.0, 480.0), angle=np.zeros(f["n"], f32), u_right=f["u_right"]).upload()
              for f, d in zip(fr, desc)]
    cam = lambda c, f: amd.KeyFrameCamera(c["Tcw"], c["Ow"], c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], depth=f["depth"],
                                          x_raw=f["x_raw"], y_raw=f["y_raw"], invfx=c["invfx"], invfy=c["invfy"])
    cam1, cams2 = cam(sc["cam1"], sc["kf1"]), [cam(c, f) for c, f in zip(sc["cams2"], sc["kf2"])]
    centres = np.stack([sc["cam1"]["Ow"]] + [c["Ow"] for c in sc["cams2"]]).astype(f32)
    x3d, status, _, _ = amd.triangulate_matches_multi(frames[0], cam1, frames[1:], cams2, sc["match12"], tr.SCALE_FACTORS, tr.LEVEL_SIGMA2,
                                                      tr.RATIO_FACTOR)
    want = ref.select(sc["match12"], status, x3d, KF_IDS[0], KF_IDS[1:1 + K], centres[0], centres[1:], sc["kf1"]["octave"], tr.SCALE_FACTORS)
    sel = amd.triangulated_points_select(sc["match12"], status, x3d, KF_IDS[0], KF_IDS[1:1 + K], centres[0], centres[1:], sc["kf1"]["octave"],
                                         tr.SCALE_FACTORS)
    m = want["n_created"]
    assert m > 20
    for key, name in (("sel_k", "created_k"), ("sel_i1", "created_i1"), ("sel_i2", "created_i2"), ("sel_from", "desc_from")):
        assert ints(out[key]) == sel[name].tolist() == want[name].tolist(), key
    for key, name in (("sel_pos", "pos"), ("sel_normal", "normal"), ("sel_min", "min_dist"), ("sel_max", "max_dist")):
        assert ref.same_bits(floats(out[key]), sel[name].reshape(-1)) and ref.same_bits(sel[name], want[name]), key

    cap = 2 * n1 + 8
    g, mp = amd.ObservationGraph(cap, 6, 8), amd.MapPoints(cap)
    g.set_keyframes(KF_SLOTS[:1 + K], KF_IDS[:1 + K], centres)
    g.enable_keyframe_points((max(f["n"] for f in fr) + 63) // 64 * 64)
    for s, f in zip(KF_SLOTS, fr):
        g.set_keyframe_points(s, np.full(f["n"], -1, np.int32))
    new_slot = (cap - 1 - 2 * np.arange(n1)).astype(np.int32)
    got = mp.create_triangulated_points(g, frames[0], KF_SLOTS[0], cam1, frames[1:], KF_SLOTS[1:1 + K], cams2, sc["match12"], tr.SCALE_FACTORS,
                                        tr.LEVEL_SIGMA2, tr.RATIO_FACTOR, new_slot)
    for key, name in (("k", "created_k"), ("i1", "created_i1"), ("i2", "created_i2"), ("slot", "created_slot"),
                      ("per_neighbour", "n_created_per_neighbour")):
        assert ints(out[key]) == got[name].tolist(), key
    assert got["created_k"].tolist() == want["created_k"].tolist() and got["created_i1"].tolist() == want["created_i1"].tolist()
    assert ints(out["status"]) == got["status"].reshape(-1).tolist() == status.reshape(-1).tolist()
    pos = mp.positions(got["created_slot"])
    assert ref.same_bits(floats(out["positions"]), pos.reshape(-1)) and ref.same_bits(pos, want["pos"])
    d = mp.descriptors(got["created_slot"])
    want_desc = np.stack([desc[1 + k][i2] if frm else desc[0][i1]
                          for k, i1, i2, frm in zip(want["created_k"], want["created_i1"], want["created_i2"], want["desc_from"])])
    assert ints(out["descriptors"]) == d.reshape(-1).tolist() == want_desc.reshape(-1).tolist()
    assert ints(out["kf1_row"]) == g.get_keyframe_points(KF_SLOTS[0]).tolist()
    assert int(out["threw"]) == 5
    for f in frames:
        f.close()
    g.close()
    mp.close()
