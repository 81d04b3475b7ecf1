"""orbfe_stereo_points_select and orbfe_count_close_points (host code, no device) against the sequential restatement
tests/stereo_points_ref.py: every output exactly equal, the floats by their bits, on frames engineered so that one branch
of the walk decides each outcome; every argument error; the capacity rule."""
import numpy as np
import pytest

import orb_slam2_annotate_amd as amd
import stereo_points_ref as ref
from orb_slam2_annotate_amd import _lib

FRAMES = ref.frames()
EXPECTED_WALK = {  # (n_walked in KEYFRAME / TEMPORAL) where the frame's name promises one
    "exact100_far": 100, "stop101": 101, "stop101_tail": 101, "eq_th": 102, "close_then_far": 106, "occupied_stale": 106,
    "special_depths": 4, "ties": 12,
}


def centre_of(f, pose, mode):
    """TEMPORAL: the frame's own centre; else a key frame's, a little off it."""
    ow = np.array(list(pose.Ow), np.float32)
    return ow if mode == ref.TEMPORAL else ow + np.array([0.03125, -0.0625, 0.015625], np.float32)


def run_both(f, mode, capacity=None):
    pose = ref.frame_pose(f)
    c = centre_of(f, pose, mode)
    want = ref.select(f["x"], f["y"], f["octave"], f["depth"], f["occupied"], f["stale"], pose, f["th"], mode, ref.SCALE, c)
    got = amd.stereo_points_select(f["x"], f["y"], f["octave"], f["depth"], pose, f["th"], mode, ref.SCALE, centre=c,
                                   occupied=f["occupied"], stale=f["stale"], capacity=capacity)
    return want, got


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("f", FRAMES, ids=[f["name"] for f in FRAMES])
def test_select_equals_the_restatement(f, mode):
    want, got = run_both(f, mode)
    assert got["n_created"] == want["n_created"] and got["n_walked"] == want["n_walked"]
    assert np.array_equal(got["created_idx"], want["created_idx"])
    assert np.array_equal(got["cleared"], want["cleared"])
    for k in ("pos", "normal", "min_dist", "max_dist"):
        assert ref.same_bits(got[k], want[k], nan_by_place=False), k  # host and numpy on one CPU: every bit, NaN included


@pytest.mark.parametrize("f", [f for f in FRAMES if f["name"] in EXPECTED_WALK], ids=lambda f: f["name"])
def test_the_frames_take_the_branch_they_are_named_for(f):
    for mode in (ref.KEYFRAME, ref.TEMPORAL):
        want, _ = run_both(f, mode)
        assert want["n_walked"] == EXPECTED_WALK[f["name"]]
    want, _ = run_both(f, ref.ALL)
    assert want["n_walked"] == want["n_created"] == int((f["depth"] > 0).sum())  # ALL: every candidate, the mask unread


def test_frames_cover_what_they_claim():
    by = {f["name"]: f for f in FRAMES}
    w, _ = run_both(by["occupied_stale"], ref.KEYFRAME)
    f = by["occupied_stale"]
    walked = set(np.argsort(np.where(f["depth"] > 0, f["depth"], np.inf), kind="stable")[:106].tolist())
    occ, st = set(np.flatnonzero(f["occupied"]).tolist()), set(np.flatnonzero(f["stale"]).tolist())
    assert occ & walked and occ - walked and st & walked and st - walked  # inside and outside the walked prefix
    assert set(np.flatnonzero(w["cleared"]).tolist()) == st & walked
    assert not run_both(f, ref.TEMPORAL)[0]["cleared"].any() and not run_both(f, ref.ALL)[0]["cleared"].any()
    w, _ = run_both(by["inf_created"], ref.KEYFRAME)
    assert w["created_idx"][-1] == 3 and not np.isfinite(w["pos"][-1]).all()
    w, _ = run_both(by["all_occupied"], ref.KEYFRAME)
    assert w["n_created"] == 0 and w["n_walked"] == 40
    assert run_both(by["all_occupied"], ref.ALL)[0]["n_created"] == 40
    w, _ = run_both(by["ties"], ref.KEYFRAME)
    assert w["created_idx"].tolist() == [1, 3, 6, 9, 0, 2, 5, 8, 10, 4, 7, 11]
    # the far pose: a float accumulation of the same product differs from the double one somewhere
    f = by["far_pose"]
    pose = ref.frame_pose(f)
    w, _ = run_both(f, ref.ALL)
    R = np.array(list(pose.Rcw), np.float32).reshape(3, 3).T
    Ow = np.array(list(pose.Ow), np.float32)
    differs = False
    for j, i in enumerate(w["created_idx"]):
        z = f["depth"][i]
        xc = ((f["x"][i] - np.float32(pose.cx)) * z) * (np.float32(1) / np.float32(pose.fx))
        yc = ((f["y"][i] - np.float32(pose.cy)) * z) * (np.float32(1) / np.float32(pose.fy))
        P32 = np.array([((R[r, 0] * xc + R[r, 1] * yc) + R[r, 2] * z) + Ow[r] for r in range(3)], np.float32)
        differs |= not np.array_equal(P32.view(np.uint32), w["pos"][j].view(np.uint32))
    assert differs


@pytest.mark.parametrize("mode", ref.MODES)
def test_capacity_rule(mode):
    f = {x["name"]: x for x in FRAMES}["close_then_far"]
    want, got = run_both(f, mode, capacity=None)
    k = want["n_created"]
    assert k > 1
    _, got = run_both(f, mode, capacity=k)
    assert got["n_created"] == k
    with pytest.raises(amd.OrbfeError) as ei:
        run_both(f, mode, capacity=k - 1)
    assert ei.value.code == _lib.ERR_CAPACITY and ei.value.n_created == k and ei.value.n_walked == want["n_walked"]


def test_argument_errors():
    f = {x["name"]: x for x in FRAMES}["n65"]
    pose = ref.frame_pose(f)

    def call(**kw):
        a = dict(x=f["x"], y=f["y"], octave=f["octave"], depth=f["depth"], pose=pose, th_depth=f["th"], mode=ref.KEYFRAME,
                 scale_factors=ref.SCALE, occupied=f["occupied"], stale=f["stale"])
        a.update(kw)
        return amd.stereo_points_select(**a)

    call()

    def invalid(**kw):
        with pytest.raises(amd.OrbfeError) as ei:
            call(**kw)
        assert ei.value.code == _lib.ERR_INVALID

    invalid(mode=3)
    invalid(mode=-1)
    bad = f["octave"].copy()
    bad[5] = ref.N_LEVELS
    invalid(octave=bad)
    bad[5] = -1
    invalid(octave=bad)
    both = f["stale"].copy()
    both[np.flatnonzero(f["occupied"])[0]] = 1
    invalid(stale=both)
    amd.stereo_points_select(f["x"], f["y"], f["octave"], f["depth"], pose, f["th"], ref.ALL, ref.SCALE, occupied=f["occupied"],
                             stale=both)  # (ALL reads neither mask)
    for field, value in (("fx", 0.0), ("fy", 0.0), ("fx", float("nan")), ("cx", float("inf"))):
        p = ref.frame_pose(f)
        setattr(p, field, value)
        invalid(pose=p)
    p = ref.frame_pose(f)
    p.Rcw[4] = float("nan")
    invalid(pose=p)
    p = ref.frame_pose(f)
    p.Ow[1] = float("inf")
    invalid(pose=p, centre=np.zeros(3, np.float32))
    invalid(centre=np.array([0.0, np.nan, 0.0], np.float32))
    invalid(scale_factors=np.zeros(0, np.float32))
    invalid(scale_factors=np.ones(257, np.float32))
    n = 16385
    z = np.zeros(n, np.float32)
    with pytest.raises(amd.OrbfeError) as ei:
        amd.stereo_points_select(z, z, np.zeros(n, np.int32), z, pose, 1.0, ref.ALL, ref.SCALE)
    assert ei.value.code == _lib.ERR_INVALID
    assert amd.stereo_points_select(z[:16384], z[:16384], np.zeros(16384, np.int32), z[:16384], pose, 1.0, ref.ALL, ref.SCALE)["n_walked"] == 0


def test_count_close_points():
    rng = np.random.default_rng(5)
    th = np.float32(10.0)
    for n in (0, 1, 64, 130):
        z = rng.uniform(-2.0, 20.0, n).astype(np.float32)
        if n >= 64:
            z[:6] = [0.0, th, np.nan, np.inf, np.nextafter(th, np.float32(0)), np.nextafter(np.float32(0), np.float32(1))]
        hp = (rng.random(n) < 0.6).astype(np.uint8)
        ol = (rng.random(n) < 0.3).astype(np.uint8)
        assert amd.count_close_points(z, hp, ol, th) == ref.count_close(z, hp, ol, th)
    z = np.array([0.0, 10.0, 9.999, 1e-30], np.float32)  # strict on both sides
    assert amd.count_close_points(z, np.ones(4, np.uint8), np.zeros(4, np.uint8), 10.0) == (2, 0)
    assert amd.count_close_points(z, np.ones(4, np.uint8), np.array([0, 0, 1, 0], np.uint8), 10.0) == (1, 1)
    L = _lib.load()
    assert L.orbfe_count_close_points(-1, None, None, None, 1.0, None, None) == _lib.ERR_INVALID
    assert L.orbfe_count_close_points(3, None, None, None, 1.0, None, None) == _lib.ERR_INVALID
