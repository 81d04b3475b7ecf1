"""The stereo-point methods of include/orbfe_classes.hpp (Tracking::SelectStereoPoints, Tracking::CountClosePoints,
MapPointTable::CreateStereoPoints) compiled with g++ against liborbfe.so (tests/cpp/test_stereo_points.cpp) on a frame made
by a formula both sides repeat: the classes equal the Python binding and the restatement (tests/stereo_points_ref.py);
refused operands throw."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import orb_slam2_annotate_amd as amd
import stereo_points_ref as ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
N, CAP, KF, TH = 150, 400, 2, 10.0
SF = (1.0 + 0.25 * np.arange(8)).astype(f32)


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("stereopointscpp") / "test_stereo_points"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_stereo_points.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return dict(t.split("=") for t in text.split())


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


def floats(s):
    return np.array(ints(s), np.uint32).view(f32)


def frame():
    i = np.arange(N)
    x = (f32(20.0) + f32(4.5) * ((i * 37) % 150).astype(f32)).astype(f32)
    y = (f32(15.0) + f32(2.75) * ((i * 53) % 150).astype(f32)).astype(f32)
    octave = (i % 8).astype(np.int32)
    desc = ((i[:, None] * 131 + np.arange(32)[None, :] * 17) % 256).astype(np.uint8)
    depth = np.where(i % 10 == 9, f32(0), np.where(i % 5 == 4, f32(12.0) + f32(0.5) * (i % 13).astype(f32),
                                                   f32(0.5) + f32(0.0625) * ((i * 29) % 144).astype(f32))).astype(f32)
    depth[i % 11 == 0] = 4.0
    occupied = (i % 4 == 1).astype(np.uint8)
    stale = ((i % 6 == 2) & (occupied == 0)).astype(np.uint8)
    with np.errstate(all="ignore"):
        u_right = np.where(depth > 0, np.where(i % 7 == 3, f32(-2.0), x - f32(40.0) / depth), f32(-1.0)).astype(f32)
    outlier = (i % 9 == 1).astype(np.uint8)
    return dict(x=x, y=y, octave=octave, desc=desc, depth=depth, occupied=occupied, stale=stale, u_right=u_right,
                has_point=occupied | stale, outlier=outlier)


def test_cpp_stereo_points_equal_the_binding_and_the_restatement(out):
    f = frame()
    R = f32([[0, -1, 0], [1, 0, 0], [0, 0, 1]])
    ow = f32([1.5, -0.25, 0.75])
    pose = amd.camera_pose(R, -(R @ ow), ref.K4, 40.0, (0.0, 752.0, 0.0, 480.0), 1.2, 8, Ow=ow)  # (every product is 0 or +-Ow: exact)
    pose.log_scale_factor = 0.25
    centre = f32([1.53125, -0.3125, 0.765625])
    assert (int(out["tracked_close"]), int(out["non_tracked_close"])) == amd.count_close_points(f["depth"], f["has_point"], f["outlier"], TH) \
        == ref.count_close(f["depth"], f["has_point"], f["outlier"], TH)
    want = ref.select(f["x"], f["y"], f["octave"], f["depth"], f["occupied"], f["stale"], pose, TH, ref.KEYFRAME, SF, centre)
    sel = amd.stereo_points_select(f["x"], f["y"], f["octave"], f["depth"], pose, TH, ref.KEYFRAME, SF, centre=centre,
                                   occupied=f["occupied"], stale=f["stale"])
    m = want["n_created"]
    assert m > 60 and want["n_walked"] < int((f["depth"] > 0).sum()) and want["cleared"].any()
    assert ints(out["sel_idx"]) == sel["created_idx"].tolist() == want["created_idx"].tolist()
    for key, name in (("sel_pos", "pos"), ("sel_normal", "normal"), ("sel_min", "min_dist"), ("sel_max", "max_dist")):
        assert ref.same_bits(floats(out[key]), sel[name].reshape(-1)) and ref.same_bits(sel[name], want[name])
    assert ints(out["sel_cleared"]) == sel["cleared"].tolist() == want["cleared"].tolist()
    assert int(out["sel_walked"]) == sel["n_walked"] == want["n_walked"]

    g = amd.ObservationGraph(CAP, 4, 8)
    mp = amd.MapPoints(CAP)
    g.set_keyframes([0, KF], [3, 9], np.array([[9, 9, 9], centre], f32))
    g.enable_keyframe_points(192)
    held = np.flatnonzero(f["has_point"]).astype(np.int32)
    row = np.full(N, -1, np.int32)
    row[held] = held
    g.set_points(held, np.zeros(len(held), np.uint8), np.zeros(len(held), np.int32))
    g.set_keyframe_points(KF, row)
    new_slot = (N + (np.arange(N) * 7) % N).astype(np.int32)
    view = amd.FrameView(f["x"], f["y"], f["octave"], f["desc"], (0.0, 752.0, 0.0, 480.0), angle=np.zeros(N, f32), u_right=f["u_right"])
    F = view.upload()
    got = mp.create_stereo_points(g, F, KF, pose, f["depth"], TH, ref.KEYFRAME, SF, new_slot, occupied=f["occupied"], stale=f["stale"])
    assert ints(out["idx"]) == got["created_idx"].tolist() == want["created_idx"].tolist()
    assert ints(out["slot"]) == got["created_slot"].tolist() == new_slot[:m].tolist()
    assert ints(out["cleared"]) == got["cleared"].tolist() == want["cleared"].tolist()
    assert int(out["walked"]) == got["n_walked"] == want["n_walked"]
    pos = mp.positions(got["created_slot"])
    assert ref.same_bits(floats(out["positions"]), pos.reshape(-1)) and ref.same_bits(pos, want["pos"])
    assert ints(out["descriptors"]) == f["desc"][want["created_idx"]].reshape(-1).tolist()
    pr = mp.ProjectInFrustum(got["created_slot"], pose, -2.0)
    assert ints(out["in_view"]) == pr["in_view"].tolist() and ints(out["level"]) == pr["level"].tolist() and pr["in_view"].sum() > 20
    assert ref.same_bits(floats(out["view_cos"]), pr["view_cos"])

    wt = ref.select(f["x"], f["y"], f["octave"], f["depth"], f["occupied"], None, pose, TH, ref.TEMPORAL, SF, ow)
    assert ints(out["temporal_idx"]) == wt["created_idx"].tolist()
    assert ref.same_bits(floats(out["temporal_positions"]), wt["pos"].reshape(-1))
    assert int(out["threw"]) == 6
    F.close()
    g.close()
