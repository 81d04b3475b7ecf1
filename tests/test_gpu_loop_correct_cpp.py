"""The loop-correction methods of include/orbfe_classes.hpp (LoopClosing::CorrectedSim3s, MapPointTable::CorrectLoop,
LoopClosing::PropagateGBA, MapPointTable::GlobalBundleAdjustmentUpdate) compiled with g++ against liborbfe.so
(tests/cpp/test_loop_correct.cpp) on a world made by a formula both sides repeat: the classes equal the Python binding and
the restatement (tests/loop_correct_ref.py); refused operands throw."""
import copy
import subprocess
from pathlib import Path

import numpy as np
import pytest

import loop_correct_ref as lr
import obsgraph_ref as orf
import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd import loop_closing as lc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
P, CAP, NKF, W = 200, 256, 7, 64
ORDER, CUR = [4, 1, 6, 0, 2], 2
SF = (1.0 + 0.25 * np.arange(8)).astype(f32)
ROT = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1], [0, -1, 0, 1, 0, 0, 0, 0, 1], [1, 0, 0, 0, 0, -1, 0, 1, 0],
                [-1, 0, 0, 0, 1, 0, 0, 0, -1], [0, 0, 1, 0, 1, 0, -1, 0, 0]], f32).reshape(5, 3, 3)


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("loopcorrectcpp") / "test_loop_correct"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_loop_correct.cpp"), "-o",
                    str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return dict(t.split("=") for t in text.split())


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


def floats(s):
    return np.array(ints(s), np.uint32).view(f32)


def doubles(s):
    return np.array(ints(s), np.int64).view(np.float64)


def pose_of(r, t):
    T = np.eye(4, dtype=f32)
    T[:3, :3], T[:3, 3] = ROT[r], f32(t)
    return T


def inverse_of(T):
    out = np.eye(4, dtype=f32)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T @ T[:3, 3])  # every product is 0 or +-t: exact
    return out


def world():
    w = orf.World()
    for k in range(NKF):
        w.add_keyframe(100 + 3 * k, f32([0.5 * k, -0.25 * k, 0.125 * k]))
    kid = {k: 100 + 3 * k for k in range(NKF)}
    for p in range(P):
        w.add_point(p, ref=kid[(p + 1) % 7 if p % 5 == 0 else p % 7], bad=p % 17 == 5)
        for d in (0, 3, 5):
            w.add_observation(p, kid[(p + d) % 7], p, (p + d) % 8, False)
    pos = np.array([[p % 10 - 4.5, p % 7 - 3.0, 4.0 + p % 5] for p in range(P)], f32)
    rows = {kid[k]: [-1 if (i * 5 + k) % 4 == 0 else (i * 7 + k * 31) % P for i in range(40 + k)] for k in range(NKF)}
    g = amd.ObservationGraph(CAP, 8, 8)
    orf.load(w, g, {kid[k]: k for k in range(NKF)}, {p: p for p in range(P)})
    g.enable_keyframe_points(W)
    for k in range(NKF):
        g.set_keyframe_points(k, rows[kid[k]])
    mp = amd.MapPoints(CAP)
    mp.update(np.arange(P), pos, np.tile(f32([0, 0, 1]), (P, 1)), np.full(P, 0.125, f32), np.full(P, 128.0, f32), np.zeros((P, 32), np.uint8),
              np.zeros(P, np.uint8))
    return w, kid, rows, pos, g, mp


def test_cpp_loop_correction_equals_the_binding_and_the_restatement(out):
    w, kid, rows, pos, g, mp = world()
    K = len(ORDER)
    Tiw = np.array([pose_of(k, (0.5 * k, 0.25, -0.125 * k)) for k in range(K)])
    ow_new = np.array([[0.5 * k + 0.25, 1.0, -k] for k in range(K)], f32)
    Scw = np.array([0, 0, 0, 1, 0.5, -0.25, 0.125, 1.25])
    cor, non, T = lc.correct_loop_sim3s(Tiw, inverse_of(Tiw[CUR]), CUR, Scw)
    wc, wn, wT = lr.correct_loop_sim3s(Tiw, inverse_of(Tiw[CUR]), CUR, Scw)
    assert np.array_equal(doubles(out["corrected"]), cor.reshape(-1)) and np.array_equal(cor, wc)
    assert np.array_equal(doubles(out["noncorrected"]), non.reshape(-1)) and np.array_equal(non, wn)
    assert np.array_equal(floats(out["tiw_corrected"]), T.reshape(-1)) and np.array_equal(T, wT)
    slots, ref, valid = mp.correct_loop(g, ORDER, cor, non, ow_new, SF, skip=(3, 10))
    wpos = {p: pos[p] for p in range(P)}
    ids, refs, wvalid, _ = lr.correct_loop(copy.deepcopy(w), [kid[k] for k in ORDER], rows, cor, non, ow_new, wpos, (3, 10), SF)
    assert ints(out["slots"]) == slots.tolist() == ids and ints(out["ref"]) == ref.tolist() == refs
    assert ints(out["valid"]) == valid.tolist() == wvalid and len(ids) > 100 and 0 in wvalid and 1 in wvalid
    got = mp.positions(np.arange(P))
    assert np.array_equal(floats(out["positions"]).view(np.uint32), got.reshape(-1).view(np.uint32))
    want = np.array([wpos[p] for p in range(P)])
    assert np.abs(got - want).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(want).max())
    pose = amd.camera_pose(np.eye(3), (0, 0, 14), (500, 500, 320, 240), 40.0, (0, 640, 0, 480), 1.2, 8, Ow=(0, 0, -14))
    pose.log_scale_factor = 0.25
    pr = mp.ProjectInFrustum(np.arange(P), pose, -2.0)
    assert ints(out["in_view"]) == pr["in_view"].tolist() and ints(out["level"]) == pr["level"].tolist() and pr["in_view"].sum() > 20
    assert np.array_equal(floats(out["view_cos"]).view(np.uint32), pr["view_cos"].view(np.uint32))

    # the global bundle adjustment
    children = [[1, 2, 4], [], [3], [], [5], [], []]
    in_gba = np.array([1, 1, 0, 0, 0, 1, 0], np.uint8)
    Tcw = np.array([pose_of(k % 5, (0.25 * k, -0.5, 0.125 * k)) for k in range(NKF)])
    Twc = np.array([inverse_of(t) for t in Tcw])
    Tg = np.array([pose_of((k + 2) % 5, (0.25 * k + 0.125, -0.25, 0.5 * k)) for k in range(NKF)])
    new, reached, visited = lc.gba_propagate_keyframes([0], children, Tcw, Twc, in_gba, Tg)
    wnew, wr, wv = lr.gba_propagate_keyframes([0], children, Tcw, Twc, in_gba, Tg)
    assert np.array_equal(floats(out["tcw_new"]), new.reshape(-1)) and np.array_equal(new, wnew)
    assert ints(out["reached"]) == reached.tolist() == wr.tolist() == [1, 1, 1, 1, 1, 1, 0]
    assert ints(out["visited"]) == visited.tolist() == wv.tolist() == [1, 1, 1, 1, 1, 1, 0]
    compact = [5, 0, 2, 6, 1, 4]
    Tb, Tn = Tcw[compact], np.array([inverse_of(new[k]) for k in compact])
    p_in = np.array([p % 3 == 0 for p in range(P)], np.uint8)
    pg = np.array([[0.5 * (p % 9), -0.25 * (p % 11), 3.0 + p % 4] for p in range(P)], f32)
    moved = mp.gba_update(g, np.arange(P), p_in, pg, compact, reached[compact], Tb, Tn)
    refk = [(p + 1) % 7 if p % 5 == 0 else p % 7 for p in range(P)]
    wref = np.array([compact.index(k) if k in compact else -1 for k in refk], np.int32)
    wout, wmoved = lr.gba_update_points(got, [p % 17 == 5 for p in range(P)], p_in, pg, wref, reached[compact], Tb, Tn)
    assert ints(out["moved"]) == moved.tolist() == wmoved.tolist() and set(wmoved.tolist()) == {0, 1, 2}
    after = mp.positions(np.arange(P))
    assert np.array_equal(floats(out["positions_gba"]).view(np.uint32), after.reshape(-1).view(np.uint32))
    assert np.array_equal(after.view(np.uint32), wout.view(np.uint32))
    assert int(out["threw"]) == 6
    g.close()
