"""GPU tests of the last-frame / key-frame SearchByProjection on the resident map points (include/orbfe.h:
orbfe_project_last_frame, orbfe_search_last_frame_mappoints, orbfe_project_keyframe, orbfe_search_keyframe_mappoints_multi): the
projections pinned to tests/track_ref.py bit for bit, the one call against the two-step form through the existing host-array
searches, table updates, re-entrancy, and track_with_motion_model against its three calls chained by hand."""
import threading

import numpy as np
import pytest

import track_ref as tr
from test_track_ref import CAP, CAP_ALL, GPU_SCENES, IDS, KF_SCENES, LAST_SCENES

pytestmark = pytest.mark.gpu

TABLE = 4096
K4 = (tr.FX, tr.FY, tr.CX, tr.CY)
K5 = np.float32([tr.FX, tr.FY, tr.CX, tr.CY, tr.MBF])
LAST_FIELDS = ("valid", "u", "v", "inv_z", "ur", "radius")
KF_FIELDS = ("valid", "u", "v", "inv_z", "level", "dist")
BIG = [s for s in GPU_SCENES if np.max(s[1]) >= 255]
BIG_IDS = [i for i, s in zip(IDS, GPU_SCENES) if np.max(s[1]) >= 255]


def _slots(N, seed):
    return np.random.default_rng(900 + seed).permutation(TABLE)[:N].astype(np.int32)


def _table(sc, slot):
    from orb_slam2_annotate_amd.map_points import MapPoints
    mp = MapPoints(TABLE)
    mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
    return mp


def _poses(sc):
    from orb_slam2_annotate_amd.map_points import camera_pose
    return [camera_pose(p["Rcw"], p["tcw"], K4, tr.MBF, tr.BOUNDS, tr.SCALE, tr.LEVELS, Ow=p["Ow"]) for p in sc["poses"]]


def _view(f, resident):
    from orb_slam2_annotate_amd import FrameView
    V = FrameView(f["x"], f["y"], f["octave"], f["desc"], tr.BOUNDS, angle=f["angle"], u_right=f["u_right"])
    return V.upload() if resident else V


def _jobs(sc, a):
    return [a[sc["offsets"][k]:sc["offsets"][k + 1]] for k in range(len(sc["poses"]))]


def _same_bits(got, want, fields):
    for name in fields:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]).astype(got[name].dtype)
        assert a.shape == b.shape, name
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8])


def _cat(dicts, fields):
    return {name: np.concatenate([d[name] for d in dicts] + [np.zeros(0, dicts[0][name].dtype if dicts else np.float32)]) for name in fields}


def _project_kf(mp, sc, slot, skip=True):
    return mp.project_keyframes(_poses(sc), _jobs(sc, slot), skips=_jobs(sc, sc["skip"]) if skip else None)


@pytest.mark.parametrize("seed,n,K", GPU_SCENES, ids=IDS)
def test_projections_equal_spec32_bit_for_bit(seed, n, K):
    sc = tr.scene(seed, n, K)
    slot = _slots(len(sc["pos"]), seed)
    mp = _table(sc, slot)
    none = np.zeros(len(slot), np.uint8)
    _same_bits(_cat(_project_kf(mp, sc, slot), KF_FIELDS), tr.spec32(sc, "kf"), KF_FIELDS)
    _same_bits(_cat(_project_kf(mp, sc, slot, skip=False), KF_FIELDS), tr.spec32(sc, "kf", skip=none), KF_FIELDS)
    for k, pose in enumerate(_poses(sc)):  # the last-frame form takes one job a call
        lo, hi = sc["offsets"][k], sc["offsets"][k + 1]
        one = dict(sc, poses=[sc["poses"][k]], offsets=np.array([0, hi - lo], np.int32),
                   **{f: sc[f][lo:hi] for f in ("pos", "normal", "min_dist", "max_dist", "flags", "skip", "last_octave", "angle", "desc")})
        for mode, th in ((sc["mode"], 7.0), ((sc["mode"] + 1) % 3, 15.0)):
            got = mp.project_last_frame(slot[lo:hi], one["last_octave"], pose, tr.SF, th, mode=mode, skip=one["skip"])
            _same_bits(got, tr.spec32(one, "last", th=th), LAST_FIELDS)
        got = mp.project_last_frame(slot[lo:hi], one["last_octave"], pose, tr.SF, 7.0)
        _same_bits(got, tr.spec32(one, "last", skip=none[lo:hi]), LAST_FIELDS)


@pytest.mark.parametrize("seed,n,K", BIG, ids=BIG_IDS)
def test_projections_agree_with_ref64_outside_the_guard_bands(seed, n, K):
    sc = tr.scene(seed, n, K)
    N = len(sc["pos"])
    slot = _slots(N, seed)
    mp = _table(sc, slot)
    got = {"kf": _cat(_project_kf(mp, sc, slot), KF_FIELDS)}
    if K == 1:
        got["last"] = mp.project_last_frame(slot, sc["last_octave"], _poses(sc)[0], tr.SF, 7.0, mode=sc["mode"], skip=sc["skip"])
    for form, g in got.items():
        r64 = tr.ref64(sc, form)
        out = tr.excluded(r64, form)
        print(f"{form}: {int(out.sum())} of {N} pairs inside the guard bands")
        assert (out & ~tr.on_threshold_by_design(sc)).sum() <= CAP * N and out.sum() <= CAP_ALL * N  # (tests/test_track_ref.py)
        keep = ~out
        assert np.array_equal(g["valid"][keep], r64["valid"][keep])
        ok = keep & (r64["valid"] != 0)
        assert ok.sum() > 20
        for name in ("u", "v") + (("ur",) if form == "last" else ()):
            # float32 projection of a KITTI-sized image: |u| < 1241 -> half an ulp is 6e-5, a handful of operations deep
            assert np.abs(g[name][ok] - r64[name][ok]).max() < 2e-3, name
        assert np.allclose(g["inv_z"][ok], r64["inv_z"][ok], rtol=1e-5)
        if form == "kf":
            assert np.array_equal(g["level"][keep], r64["level"][keep])
            assert np.allclose(g["dist"][ok], r64["dist"][ok], rtol=1e-6)
        else:
            assert np.allclose(g["radius"][ok], r64["radius"][ok], rtol=1e-6)


def _blocked(seed, n):
    return (np.random.default_rng(70 + seed).random(n) < 0.1).astype(np.uint8)


def _two_step_last(mp, sc, slot, Cur, pose, th, mode, blocked):
    import orb_slam2_annotate_amd as amd
    pr = mp.project_last_frame(slot, sc["last_octave"], pose, tr.SF, th, mode=mode, skip=sc["skip"])
    return amd.ORBmatcher(0.9, True).SearchByProjectionLastFrame(
        Cur, tr.SF, pr["valid"], pr["u"], pr["v"], sc["last_octave"], sc["angle"], mp.descriptors(slot), th, mode=mode, mbf=tr.MBF,
        invzc=pr["inv_z"], obs_positive=(sc["flags"] >> 1) & 1, blocked=blocked)


@pytest.mark.parametrize("resident", [False, True], ids=["host_view", "resident"])
@pytest.mark.parametrize("with_blocked", [False, True], ids=["free", "blocked"])
@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_last_frame_search_equals_the_two_step_form(mode, stereo, with_blocked, resident):
    seed, n, K = LAST_SCENES[-1]
    sc = tr.scene(seed, n, K)
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    pose = _poses(sc)[0]
    Cur = _view(sc["cur_stereo" if stereo else "cur"], resident)
    blocked = _blocked(seed, tr.CUR_POINTS) if with_blocked else None
    th = 7.0 if stereo else 15.0
    nm, match, valid = mp.SearchByProjectionLastFrame(Cur, slot, sc["last_octave"], sc["angle"], pose, tr.SF, th, mode=mode,
                                                      skip=sc["skip"], blocked=blocked, return_valid=True)
    nm2, match2 = _two_step_last(mp, sc, slot, Cur, pose, th, mode, blocked)
    assert nm == nm2 and np.array_equal(match, match2)
    assert np.array_equal(valid, tr.spec32(sc, "last")["valid"])
    assert nm == (match >= 0).sum() and nm > 20, nm
    if with_blocked:
        assert (match[blocked != 0] == -1).all()
    # without the rotation histogram more matches stay
    nm3, match3 = mp.SearchByProjectionLastFrame(Cur, slot, sc["last_octave"], None, pose, tr.SF, th, mode=mode, skip=sc["skip"],
                                                 blocked=blocked, check_orientation=False)
    assert nm3 > nm


def test_last_frame_search_grows_its_lists():
    """40 keypoints inside the window of one map point, more than the 32 entries the search's lists start with: the one call
    (k_project_track writes the queries on the device) searches a second time with longer lists, behind a producer whose
    staging starts anew, and still equals the two-step form.  The scene is the smallest of this file that holds a searched
    point (the size-1 scene's only point projects outside the image)."""
    import oracle_lib as O
    seed, n, K = LAST_SCENES[2]
    sc = tr.scene(seed, n, K)
    s32 = tr.spec32(sc, "last", th=7.0)
    p = int(np.flatnonzero((s32["valid"] != 0) & (s32["u"] > 40) & (s32["u"] < 1200) & (s32["v"] > 40) & (s32["v"] < 330) &
                           (sc["last_octave"] >= 1))[0])
    lv, n_crowd = int(sc["last_octave"][p]), 40
    rng = np.random.default_rng(41)
    f = {k: (v.copy() if v is not None else None) for k, v in sc["cur"].items()}
    kp = rng.choice(tr.CUR_POINTS, n_crowd, replace=False)
    f["x"][kp] = (s32["u"][p] + rng.uniform(-3, 3, n_crowd)).astype(np.float32)
    f["y"][kp] = (s32["v"][p] + rng.uniform(-3, 3, n_crowd)).astype(np.float32)
    f["octave"][kp] = lv - rng.integers(0, 2, n_crowd)
    f["desc"][kp] = sc["desc"][p] ^ (rng.integers(0, 256, (n_crowd, 32), dtype=np.uint8) & rng.integers(0, 256, (n_crowd, 32), dtype=np.uint8) &
                                    rng.integers(0, 256, (n_crowd, 32), dtype=np.uint8))
    # the oracle's own window of that point (mode 0: octaves [lv - 1, lv + 1], src/ORBmatcher.cc:1541-1550) holds the crowd
    Fo = O.Frame(f["x"], f["y"], f["octave"], f["desc"], tr.BOUNDS, angle=f["angle"])
    assert Fo.features_in_area(s32["u"][p], s32["v"][p], s32["radius"][p], lv - 1, lv + 1).size >= n_crowd > 32
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    pose = _poses(sc)[0]
    for resident in (True, False):
        Cur = _view(f, resident)
        nm, match, valid = mp.SearchByProjectionLastFrame(Cur, slot, sc["last_octave"], sc["angle"], pose, tr.SF, 7.0, mode=0,
                                                          skip=sc["skip"], return_valid=True)
        nm2, match2 = _two_step_last(mp, sc, slot, Cur, pose, 7.0, 0, None)
        assert nm == nm2 and np.array_equal(match, match2)
        assert np.array_equal(valid, s32["valid"])
        assert nm == (match >= 0).sum() and nm > 20


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_last_frame_search_at_the_workgroup_boundary(n):
    seed = [s for s, m, _ in LAST_SCENES if m == n][0]
    sc = tr.scene(seed, n, 1)
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    pose = _poses(sc)[0]
    Cur = _view(sc["cur_stereo"], True)
    nm, match = mp.SearchByProjectionLastFrame(Cur, slot, sc["last_octave"], sc["angle"], pose, tr.SF, 7.0, mode=sc["mode"], skip=sc["skip"])
    nm2, match2 = _two_step_last(mp, sc, slot, Cur, pose, 7.0, sc["mode"], None)
    assert nm == nm2 and np.array_equal(match, match2) and match.shape == (tr.CUR_POINTS,)
    assert nm > 20 or n < 255


@pytest.mark.parametrize("resident", [False, True], ids=["host_view", "resident"])
@pytest.mark.parametrize("with_blocked", [False, True], ids=["free", "blocked"])
@pytest.mark.parametrize("seed,n,K", KF_SCENES, ids=[f"K{K}" for _, _, K in KF_SCENES])
def test_keyframe_search_equals_single_calls(seed, n, K, with_blocked, resident):
    import orb_slam2_annotate_amd as amd
    sc = tr.scene(seed, n, K)
    slot = _slots(len(sc["pos"]), seed)
    mp = _table(sc, slot)
    Cur = _view(sc["cur_stereo"], resident)  # (the key-frame search reads no u_right)
    blocked = [_blocked(seed + k, tr.CUR_POINTS) if k != 1 else None for k in range(K)] if with_blocked else None
    cnt, match = mp.SearchByProjectionKeyFrames(Cur, _poses(sc), _jobs(sc, slot), _jobs(sc, sc["angle"]), tr.SF, sc["th"], sc["orb_dist"],
                                                skips=_jobs(sc, sc["skip"]), blocked=blocked)
    assert match.shape == (K, tr.CUR_POINTS)
    pr = _project_kf(mp, sc, slot)
    m = amd.ORBmatcher(0.9, True)
    for k in range(K):
        s = _jobs(sc, slot)[k]
        nm, one = m.SearchByProjectionKeyFrame(Cur, tr.SF, pr[k]["valid"], pr[k]["u"], pr[k]["v"], pr[k]["level"], _jobs(sc, sc["angle"])[k],
                                               mp.descriptors(s), float(sc["th"][k]), int(sc["orb_dist"][k]),
                                               blocked=None if blocked is None else blocked[k])
        assert cnt[k] == nm and np.array_equal(match[k], one), k
        assert len(s) < 255 or nm > 10, (k, nm)
    # the same thresholds for every candidate as scalars
    cnt2, match2 = mp.SearchByProjectionKeyFrames(Cur, _poses(sc), _jobs(sc, slot), _jobs(sc, sc["angle"]), tr.SF, 10.0, 100,
                                                  skips=_jobs(sc, sc["skip"]), blocked=blocked)
    assert np.array_equal(match2[0], match[0]) and cnt2[0] == cnt[0]


def test_table_update_between_two_calls_is_honoured():
    seed, n, K = LAST_SCENES[-1]
    sc = tr.scene(seed, n, K)
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    pose = _poses(sc)[0]
    Cur = _view(sc["cur"], True)

    def both():
        a = mp.SearchByProjectionLastFrame(Cur, slot, sc["last_octave"], sc["angle"], pose, tr.SF, 15.0, skip=sc["skip"], return_valid=True)
        b = _two_step_last(mp, sc, slot, Cur, pose, 15.0, 0, None)
        assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], tr.spec32(sc, "last")["valid"])
        kf = mp.SearchByProjectionKeyFrames(Cur, [pose], [slot], [sc["angle"]], tr.SF, 10.0, 100, skips=[sc["skip"]])
        return a[1], kf[1][0]

    before, kf_before = both()
    hit = np.unique(before[before >= tr.ENGINEERED])
    moved, redescribed = hit[:2]
    flipped = np.unique(kf_before[(kf_before >= tr.ENGINEERED) & ~np.isin(kf_before, [moved, redescribed])])[0]
    sc["pos"][moved] = sc["pos"][moved] + (sc["poses"][0]["Rcw"].T @ np.float32([0.0, 0.0, -60.0]))  # behind the camera
    sc["desc"][redescribed] ^= 0xFF
    sc["flags"][flipped] |= 1
    ch = np.array([moved, redescribed, flipped])
    mp.update(slot[ch], sc["pos"][ch], sc["normal"][ch], sc["min_dist"][ch], sc["max_dist"][ch], sc["desc"][ch], sc["flags"][ch])
    after, kf_after = both()
    assert not (after == moved).any() and not (after == redescribed).any()
    assert not (kf_after == flipped).any()  # a bad point leaves the key-frame form only


def test_two_threads_on_one_table():
    seed, n, K = KF_SCENES[1]
    sc = tr.scene(seed, n, K)
    slot = _slots(len(sc["pos"]), seed)
    mp = _table(sc, slot)
    poses = _poses(sc)
    Cur = _view(sc["cur"], True)
    j0 = slice(sc["offsets"][0], sc["offsets"][1])

    def last():
        return mp.SearchByProjectionLastFrame(Cur, slot[j0], sc["last_octave"][j0], sc["angle"][j0], poses[0], tr.SF, 15.0, skip=sc["skip"][j0])[1]

    def kf():
        return mp.SearchByProjectionKeyFrames(Cur, poses, _jobs(sc, slot), _jobs(sc, sc["angle"]), tr.SF, sc["th"], sc["orb_dist"],
                                              skips=_jobs(sc, sc["skip"]))[1]

    want = {"last": last(), "kf": kf()}
    got, errors = {}, []

    def work(name, call):
        try:
            got[name] = [call() for _ in range(8)]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=("last", last)), threading.Thread(target=work, args=("kf", kf))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(np.array_equal(r, want[name]) for name in want for r in got[name])


def _T(R, t):
    T = np.eye(4, dtype=np.float32)
    T[:3, :3], T[:3, 3] = R, t
    return T


@pytest.mark.parametrize("case", ["mono", "stereo_forward", "stereo_backward", "stereo_retry"])
def test_track_with_motion_model_equals_the_three_calls_chained_by_hand(case):
    from orb_slam2_annotate_amd import track_with_motion_model
    seed, n, K = LAST_SCENES[-1]
    sc = tr.scene(seed, n, K)
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    pose = _poses(sc)[0]
    mono = case == "mono"
    frame = sc["cur" if mono else "cur_stereo"]
    if case == "stereo_retry":  # every keypoint beyond the th = 7 window of its point and inside the th = 14 one
        frame = tr.current_frame(np.random.default_rng(3), sc, stereo=True, offset=(1.15, 1.8))
    Cur = _view(frame, True)
    Tcw = _T(sc["poses"][0]["Rcw"], sc["poses"][0]["tcw"])
    mb = 0.5
    dz = {"mono": 2.0, "stereo_forward": 2.0, "stereo_backward": -2.0, "stereo_retry": 0.1}[case]
    Tlw = _T(sc["poses"][0]["Rcw"], sc["poses"][0]["tcw"] + np.float32([0, 0, dz]))  # tlc = (0, 0, dz)
    mode = {"mono": 0, "stereo_forward": 1, "stereo_backward": 2, "stereo_retry": 0}[case]
    got = track_with_motion_model(mp, Cur, slot, sc["last_octave"], sc["angle"], Tcw, Tlw, mb, mono, K5, tr.BOUNDS, tr.SCALE, tr.SF,
                                  tr.INV_SIGMA2, skip=sc["skip"])
    th = 15.0 if mono else 7.0
    nm, match = mp.SearchByProjectionLastFrame(Cur, slot, sc["last_octave"], sc["angle"], pose, tr.SF, th, mode=mode, skip=sc["skip"])
    assert (nm < 20) == (case == "stereo_retry"), nm
    if nm < 20:
        th = 2 * th
        nm, match = mp.SearchByProjectionLastFrame(Cur, slot, sc["last_octave"], sc["angle"], pose, tr.SF, th, mode=mode, skip=sc["skip"])
    assert nm >= 20
    ni, Tout, flags, _, _ = mp.pose_optimization(Cur, slot, match, Tcw, K5, tr.INV_SIGMA2)
    assert got["mode"] == mode and got["th"] == th and got["nmatches"] == nm and np.array_equal(got["match"], match)
    assert got["n_inliers"] == ni and np.array_equal(got["Tcw"].view(np.uint8), Tout.view(np.uint8)) and np.array_equal(got["outlier"], flags)
    assert np.isfinite(Tout).all()
    # keypoints within a pixel of their projections are inliers; those of the retry scene were put 1.15 .. 1.8 window radii
    # (8 .. 90 px) aside, far beyond the chi-square bound of the optimisation, so no inlier count is asked of it
    assert ni >= 10 or case == "stereo_retry"
