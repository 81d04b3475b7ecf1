"""GPU: the device map-point table (orbfe_mappoints), orbfe_project_in_frustum against tests/frustum_ref.py and
orbfe_search_local_points against the existing SearchByProjection and the CPU oracle."""
import numpy as np
import pytest

import frustum_ref as fr

pytestmark = pytest.mark.gpu

CAP = 4096
SF = (1.2 ** np.arange(8)).astype(np.float32)


def _pose(sc):
    from orb_slam2_annotate_amd.map_points import camera_pose
    return camera_pose(sc["Rcw"], sc["tcw"], (fr.FX, fr.FY, fr.CX, fr.CY), fr.MBF, fr.BOUNDS, fr.SCALE, fr.LEVELS, Ow=sc["Ow"])


def _slots(n, seed):
    """a permutation with gaps: n distinct slots of the CAP-slot table, in no order"""
    return np.random.default_rng(77 + seed).permutation(CAP)[:n].astype(np.int32)


def _table(sc, slot):
    from orb_slam2_annotate_amd.map_points import MapPoints
    mp = MapPoints(CAP)
    mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
    return mp


@pytest.fixture(scope="module")
def projected():
    """(scene, slots, spec32, ref64, device outputs) for every size, computed once"""
    out = {}
    for n in (0, 1, 33, 2000):
        sc = fr.scene(0, n)
        slot = _slots(n, 0)
        mp = _table(sc, slot)
        got = mp.ProjectInFrustum(slot, _pose(sc), fr.LIMIT, skip=sc["skip"])
        mp.close()
        out[n] = (sc, slot, fr.spec32(sc, sc["skip"]), fr.ref64(sc, sc["skip"]), got)
    return out


@pytest.mark.parametrize("n", [0, 1, 33, 2000])
def test_project_equals_spec32_bit_for_bit(projected, n):
    sc, slot, s32, r64, got = projected[n]
    _assert_equals_spec32(got, s32, r64, n)


def _assert_equals_spec32(got, s32, r64, n):
    assert np.array_equal(got["in_view"], s32["in_view"]), np.flatnonzero(got["in_view"] != s32["in_view"])
    ok = s32["in_view"] != 0
    for name in ("proj_x", "proj_y", "proj_xr", "inv_z", "dist", "view_cos"):
        a, b = got[name][ok].view(np.uint32), s32[name][ok].view(np.uint32)
        assert np.array_equal(a, b), (name, int((a != b).sum()), got[name][ok][a != b][:4], s32[name][ok][a != b][:4])
        assert not got[name][~ok].any(), name
    excused = fr.near_integer(r64) & ok
    print(f"n={n}: {int(ok.sum())} in view, {int(excused.sum())} level(s) excused")
    assert excused.sum() <= 0.005 * max(int(ok.sum()), 1)
    strict = ok & ~excused
    assert np.array_equal(got["level"][strict], s32["level"][strict])
    assert ((got["level"] >= 0) & (got["level"] < fr.LEVELS)).all() and not got["level"][~ok].any()


@pytest.mark.parametrize("n", [1, 33, 2000])
def test_project_against_ref64(projected, n):
    sc, slot, s32, r64, got = projected[n]
    near = fr.near_threshold(r64)
    assert near.sum() <= 0.01 * n
    differs = got["in_view"] != r64["in_view"]
    assert not (differs & ~near).any(), np.flatnonzero(differs & ~near)
    ok = (got["in_view"] != 0) & (r64["in_view"] != 0)
    if ok.any():
        du, dv = np.abs(got["proj_x"][ok] - r64["u"][ok]).max(), np.abs(got["proj_y"][ok] - r64["v"][ok]).max()
        su, sv = np.abs(s32["u"][ok] - r64["u"][ok]).max(), np.abs(s32["v"][ok] - r64["v"][ok]).max()
        print(f"n={n}: max|u-u64| {du:.3g} (spec32 {su:.3g}), max|v-v64| {dv:.3g} (spec32 {sv:.3g})")
        assert du <= 2 * su and dv <= 2 * sv


def test_skip_bad_and_a_second_update_are_honoured():
    n = 2000
    sc = fr.scene(1, n)
    slot = _slots(n, 1)
    mp = _table(sc, slot)
    pose = _pose(sc)
    free = mp.ProjectInFrustum(slot, pose, fr.LIMIT)  # no mask
    assert np.array_equal(free["in_view"], fr.spec32(sc, None)["in_view"])
    skipped = mp.ProjectInFrustum(slot, pose, fr.LIMIT, skip=sc["skip"])
    assert not skipped["in_view"][sc["skip"] != 0].any() and not skipped["in_view"][(sc["flags"] & 1) != 0].any()
    assert free["in_view"][sc["skip"] != 0].any()  # (the mask did hide points that are otherwise visible)
    # a slot that was never updated is bad
    unused = np.setdiff1d(np.arange(CAP, dtype=np.int32), slot)[:40]
    assert not mp.ProjectInFrustum(unused, pose, fr.LIMIT)["in_view"].any()
    # move 100 points and flip their bad flag, keeping the descriptors
    rng = np.random.default_rng(5)
    moved = rng.choice(n, 100, replace=False)
    sc2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
    sc2["pos"][moved] += rng.normal(0, 0.7, (100, 3)).astype(np.float32)
    sc2["flags"][moved] ^= 1
    mp.update(slot[moved], sc2["pos"][moved], sc2["normal"][moved], sc2["min_dist"][moved], sc2["max_dist"][moved], None,
              sc2["flags"][moved])
    again = mp.ProjectInFrustum(slot, pose, fr.LIMIT, skip=sc["skip"])
    want = fr.spec32(sc2, sc["skip"])
    assert np.array_equal(again["in_view"], want["in_view"])
    ok = want["in_view"] != 0
    assert np.array_equal(again["proj_x"][ok].view(np.uint32), want["proj_x"][ok].view(np.uint32))
    assert (again["in_view"] != skipped["in_view"]).any()
    # the descriptors survived the update without descriptors: the search below still finds the points by them
    F, _ = _frame_for(sc2, want, True, seed=9)
    from orb_slam2_annotate_amd import ORBmatcher
    nm, match, iv = mp.SearchLocalPoints(F, slot, pose, SF, th=3.0, skip=sc["skip"])
    n2, m2 = ORBmatcher(0.8).SearchByProjection(F, SF, again["in_view"], again["level"], again["view_cos"], again["proj_x"],
                                                again["proj_y"], sc["desc"], th=3.0, proj_xr=again["proj_xr"],
                                                mp_obs_positive=(sc2["flags"] >> 1) & 1)
    assert nm == n2 and nm > 50 and np.array_equal(match, m2)
    mp.close()


@pytest.mark.parametrize("with_desc", [False, True], ids=["nodesc", "desc"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257])
def test_update_whose_arrays_end_around_a_256_byte_line(n, with_desc):
    """An update stages slots | records | flags | descriptors: 64 slots, 8 records of 32 bytes and 256 flags are exactly one
    256-byte line each, so the four arrays end just before, on and just after a line.  What the table then holds is read back
    through the projection (records, flags) and through SearchLocalPoints (descriptors).  Scene 20 has a point in view at
    every size and no level inside the excuse band of test_project_equals_spec32_bit_for_bit (tests/frustum_ref.py alone
    decides both)."""
    from orb_slam2_annotate_amd import ORBmatcher
    from orb_slam2_annotate_amd.map_points import MapPoints
    sc = fr.scene(20, n)
    slot = np.random.default_rng(n).permutation(300)[:n].astype(np.int32)
    mp = MapPoints(300)
    pose = _pose(sc)
    mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"] if with_desc else None, sc["flags"])
    first = mp.ProjectInFrustum(slot, pose, fr.LIMIT, skip=sc["skip"])
    s32 = fr.spec32(sc, sc["skip"])
    assert s32["in_view"].any()
    _assert_equals_spec32(first, s32, fr.ref64(sc, sc["skip"]), n)
    unused = np.setdiff1d(np.arange(300, dtype=np.int32), slot)
    assert not mp.ProjectInFrustum(unused, pose, fr.LIMIT)["in_view"].any()  # no other slot was written
    if with_desc:
        # move every point, keeping the descriptors
        sc2 = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in sc.items()}
        sc2["pos"] += np.random.default_rng(20).normal(0, 0.05, (n, 3)).astype(np.float32)
        mp.update(slot, sc2["pos"], sc2["normal"], sc2["min_dist"], sc2["max_dist"], None, sc2["flags"])
        again = mp.ProjectInFrustum(slot, pose, fr.LIMIT, skip=sc["skip"])
        want = fr.spec32(sc2, sc["skip"])
        _assert_equals_spec32(again, want, fr.ref64(sc2, sc["skip"]), n)
        assert want["in_view"].any() and not np.array_equal(again["proj_x"], first["proj_x"])
        # the search reads the table's descriptors, the two-step form the host's: equal matches, and some.  (Every visible
        # point has a key point within a few pixels that carries its descriptor with an eighth of the bits flipped, two in
        # three of them at an accepted octave; from 63 points on, 18 or more are visible)
        F, _ = _frame_for(sc2, want, True, seed=9)
        nm, match, iv = mp.SearchLocalPoints(F, slot, pose, SF, th=3.0, skip=sc["skip"])
        n2, m2 = ORBmatcher(0.8).SearchByProjection(F, SF, again["in_view"], again["level"], again["view_cos"], again["proj_x"],
                                                    again["proj_y"], sc["desc"], th=3.0, proj_xr=again["proj_xr"],
                                                    mp_obs_positive=(sc2["flags"] >> 1) & 1)
        assert nm == n2 and np.array_equal(match, m2) and np.array_equal(iv, again["in_view"])
        assert nm > 0 or n < 63
    mp.close()


def test_bad_arguments_raise_and_launch_nothing():
    from orb_slam2_annotate_amd import OrbfeError
    from orb_slam2_annotate_amd._lib import ERR_INVALID
    from orb_slam2_annotate_amd.map_points import MapPoints
    from orb_slam2_annotate_amd.matcher import debug_thread_stream_idle
    sc = fr.scene(2, 33)
    slot = _slots(33, 2)
    mp = _table(sc, slot)
    pose = _pose(sc)
    assert debug_thread_stream_idle()
    for bad in (CAP, -1, 1 << 30):
        s = slot.copy()
        s[7] = bad
        with pytest.raises(OrbfeError) as ei:
            mp.update(s, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
        assert ei.value.code == ERR_INVALID
        with pytest.raises(OrbfeError) as ei:
            mp.ProjectInFrustum(s, pose)
        assert ei.value.code == ERR_INVALID
    assert debug_thread_stream_idle()
    # the refused calls changed nothing
    got = mp.ProjectInFrustum(slot, pose, fr.LIMIT, skip=sc["skip"])
    assert np.array_equal(got["in_view"], fr.spec32(sc, sc["skip"])["in_view"])
    with pytest.raises(OrbfeError):
        MapPoints(0)
    mp.close()
    assert mp.closed
    for call in (lambda: mp.ProjectInFrustum(slot, pose), lambda: mp.SearchLocalPoints(None, slot, pose, SF),
                 lambda: mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])):
        with pytest.raises(ValueError):
            call()
    mp.close()  # (idempotent)


def _frame_for(sc, s32, stereo, seed):
    """A 1500-keypoint KITTI-sized frame (the `_scene` style of tests/test_projection_oracle.py) in which the map points in view
    have counterparts: keypoints moved next to their projections, with their octave near the predicted level and a noisy copy
    of their descriptor.  Returns (FrameView, oracle Frame)."""
    import oracle_lib as O
    from orb_slam2_annotate_amd import FrameView
    from test_projection_oracle import random_frame
    rng = np.random.default_rng(seed)
    nk = 1500
    x, y, octv, ang, desc, ur = random_frame(rng, nk, w=1241, h=376, stereo=stereo)
    x = np.clip(x, 0, 1240).astype(np.float32)
    y = np.clip(y, 0, 375).astype(np.float32)
    vis = np.flatnonzero(s32["in_view"])
    take = rng.choice(vis, min(len(vis), 1100), replace=False)
    kp = rng.choice(nk, len(take), replace=False)
    x[kp] = np.clip(s32["proj_x"][take] + rng.normal(0, 1.5, len(take)), 0, 1240).astype(np.float32)
    y[kp] = np.clip(s32["proj_y"][take] + rng.normal(0, 1.5, len(take)), 0, 375).astype(np.float32)
    octv[kp] = np.clip(s32["level"][take] - rng.integers(0, 3, len(take)) + 1, 0, 7).astype(np.int32)
    noise = rng.integers(0, 256, (len(take), 32), dtype=np.uint8) & rng.integers(0, 256, (len(take), 32), dtype=np.uint8) & \
        rng.integers(0, 256, (len(take), 32), dtype=np.uint8)
    desc[kp] = sc["desc"][take] ^ noise
    if stereo:  # most counterparts agree with the projected right coordinate, some do not, some have none
        ur[kp] = np.where(rng.random(len(take)) < 0.8, s32["proj_xr"][take] + rng.normal(0, 2.0, len(take)), ur[kp]).astype(np.float32)
    F = FrameView(x, y, octv, desc, fr.BOUNDS, angle=ang, u_right=ur)
    Fo = O.Frame(x, y, octv, desc, fr.BOUNDS, angle=ang, u_right=ur)
    return F, Fo


@pytest.fixture(scope="module")
def local_map():
    sc = fr.scene(2, 2000)
    slot = _slots(2000, 3)
    return sc, slot, _table(sc, slot), fr.spec32(sc, sc["skip"])


@pytest.mark.parametrize("stereo", [True, False])
@pytest.mark.parametrize("th", [1.0, 3.0, 5.0])
def test_search_local_points_equals_the_two_step_form_and_the_oracle(local_map, oracle_mod, stereo, th):
    from orb_slam2_annotate_amd import ORBmatcher
    sc, slot, mp, s32 = local_map
    pose = _pose(sc)
    F, Fo = _frame_for(sc, s32, stereo, seed=11 + int(stereo))
    rng = np.random.default_rng(3)
    blocked = (rng.random(F.N) < 0.05).astype(np.uint8)
    obs = ((sc["flags"] >> 1) & 1).astype(np.uint8)
    # today's path: the projection, then SearchByProjection with uploaded operands
    p = mp.ProjectInFrustum(slot, pose, fr.LIMIT, skip=sc["skip"])
    n_two, m_two = ORBmatcher(0.8).SearchByProjection(F, SF, p["in_view"], p["level"], p["view_cos"], p["proj_x"], p["proj_y"],
                                                      sc["desc"], th=th, proj_xr=p["proj_xr"] if stereo else None, blocked=blocked,
                                                      mp_obs_positive=obs)
    # the CPU oracle on the spec's outputs
    n_orc, m_orc = oracle_mod.search_by_projection_mappoints(Fo, SF, blocked, s32["in_view"], s32["level"], s32["view_cos"],
                                                             s32["proj_x"], s32["proj_y"], s32["proj_xr"], sc["desc"], obs, th, 0.8)
    R = F.upload()
    for frame in (R, F):  # resident, host arrays
        nm, match, iv = mp.SearchLocalPoints(frame, slot, pose, SF, th=th, nnratio=0.8, viewing_cos_limit=fr.LIMIT, skip=sc["skip"],
                                             blocked=blocked)
        assert np.array_equal(iv, p["in_view"]) and np.array_equal(iv, s32["in_view"])
        assert nm == n_two and np.array_equal(match, m_two)
        assert nm == n_orc and np.array_equal(match, m_orc)
    R.close()
    print(f"stereo={stereo} th={th}: {nm} matches of {int(s32['in_view'].sum())} points in view")
    assert nm > 100


def _crowd_on_a_point(sc, s32, n_crowd, seed):
    """_frame_for's monocular / stereo frame with n_crowd more key points inside 3 px of one visible map point's projection, at
    its predicted level: that point's window holds more than the 32 entries the search's lists start with.
    -> (FrameView, oracle Frame, index of the point)"""
    import oracle_lib as O
    from orb_slam2_annotate_amd import FrameView
    rng = np.random.default_rng(seed)
    F, _ = _frame_for(sc, s32, True, seed)
    inside = (s32["in_view"] != 0) & (s32["proj_x"] > 20) & (s32["proj_x"] < 1220) & (s32["proj_y"] > 20) & (s32["proj_y"] < 355) & \
        (s32["level"] >= 1)
    p = int(np.flatnonzero(inside)[0])
    x, y, octv, desc, ang, ur = F.x.copy(), F.y.copy(), F.octave.copy(), F.desc.copy(), F.angle.copy(), F.u_right.copy()
    kp = rng.choice(F.N, n_crowd, replace=False)
    x[kp] = (s32["proj_x"][p] + rng.uniform(-3, 3, n_crowd)).astype(np.float32)
    y[kp] = (s32["proj_y"][p] + rng.uniform(-3, 3, n_crowd)).astype(np.float32)
    octv[kp] = s32["level"][p] - rng.integers(0, 2, n_crowd)
    desc[kp] = sc["desc"][p] ^ (rng.integers(0, 256, (n_crowd, 32), dtype=np.uint8) & rng.integers(0, 256, (n_crowd, 32), dtype=np.uint8) &
                                rng.integers(0, 256, (n_crowd, 32), dtype=np.uint8))
    ur[kp] = -1.0  # (no stereo check on the crowd)
    return (FrameView(x, y, octv, desc, fr.BOUNDS, angle=ang, u_right=ur), O.Frame(x, y, octv, desc, fr.BOUNDS, angle=ang, u_right=ur), p)


@pytest.mark.parametrize("n_crowd", [40, 65])
def test_search_local_points_grows_its_lists(local_map, oracle_mod, n_crowd):
    """A map point whose window holds more key points than a list has entries: the one-call form (k_project_frustum writes
    the queries on the device) searches again with longer lists and still equals the two-step form and the oracle."""
    from orb_slam2_annotate_amd import ORBmatcher
    sc, slot, mp, s32 = local_map
    pose = _pose(sc)
    F, Fo, p = _crowd_on_a_point(sc, s32, n_crowd, seed=21)
    lv = int(s32["level"][p])
    # the oracle's own window of that point, at the smaller of the two radii (RadiusByViewingCos): more than 32 candidates
    assert Fo.features_in_area(s32["proj_x"][p], s32["proj_y"][p], 2.5 * 3.0 * SF[lv], lv - 1, lv).size >= n_crowd > 32
    obs = ((sc["flags"] >> 1) & 1).astype(np.uint8)
    n_orc, m_orc = oracle_mod.search_by_projection_mappoints(Fo, SF, None, s32["in_view"], s32["level"], s32["view_cos"], s32["proj_x"],
                                                             s32["proj_y"], s32["proj_xr"], sc["desc"], obs, 3.0, 0.8)
    q = mp.ProjectInFrustum(slot, pose, fr.LIMIT, skip=sc["skip"])
    n_two, m_two = ORBmatcher(0.8).SearchByProjection(F, SF, q["in_view"], q["level"], q["view_cos"], q["proj_x"], q["proj_y"], sc["desc"],
                                                      th=3.0, proj_xr=q["proj_xr"], mp_obs_positive=obs)
    R = F.upload()
    for frame in (R, F):  # resident, host arrays
        nm, match, iv = mp.SearchLocalPoints(frame, slot, pose, SF, th=3.0, nnratio=0.8, viewing_cos_limit=fr.LIMIT, skip=sc["skip"])
        assert np.array_equal(iv, s32["in_view"]) and np.array_equal(iv, q["in_view"])
        assert nm == n_two == n_orc and np.array_equal(match, m_two) and np.array_equal(match, m_orc)
    R.close()
    assert nm > 100
