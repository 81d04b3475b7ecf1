"""GPU tests of ORBmatcher::Fuse on the resident map points (include/orbfe.h: orbfe_project_fuse, orbfe_fuse_mappoints): the
projection pinned to tests/fuse_ref.py bit for bit, the one call against the two-step form and the CPU oracle, IsInKeyFrame
from the observation graph, table updates, the Sim3 form, the argument checks and re-entrancy."""
import threading

import numpy as np
import pytest

import fuse_ref as fr
import oracle_lib as orc
from test_fuse_ref import GPU_SCENES, PROJECTION_SHAPES

pytestmark = pytest.mark.gpu

CAP = 4096
K4 = (fr.FX, fr.FY, fr.CX, fr.CY)
FIELDS = ("valid", "u", "v", "ur", "level", "dist")


def _slots(n, seed):
    return np.random.default_rng(900 + seed).permutation(CAP)[:n].astype(np.int32)


def _table(sc, slot, capacity=CAP):
    from orb_slam2_annotate_amd.map_points import MapPoints
    mp = MapPoints(capacity)
    mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
    return mp


def _poses(poses):
    from orb_slam2_annotate_amd.map_points import camera_pose
    return [camera_pose(p["Rcw"], p["tcw"], K4, fr.MBF, fr.BOUNDS, fr.SCALE, fr.LEVELS, Ow=p["Ow"]) for p in poses]


def _frames(sc, resident, u_right=None):
    """(library views, oracle frames) of the scene's key frames; u_right: replaces the stereo coordinates of every frame"""
    from orb_slam2_annotate_amd import FrameView
    views, oracles = [], []
    for k, f in enumerate(sc["frames"]):
        ur = f["u_right"] if u_right is None else u_right[k]
        ang = np.zeros(len(f["x"]), np.float32)
        V = FrameView(f["x"], f["y"], f["octave"], f["desc"], fr.BOUNDS, angle=ang, u_right=ur)
        views.append(V.upload() if resident and k % 3 != 1 else V)  # (resident: one host-array frame stays in the group)
        oracles.append(orc.Frame(f["x"], f["y"], f["octave"], f["desc"], fr.BOUNDS, angle=ang, u_right=ur))
    return views, oracles


def _mask(sc):
    return (sc["skip"] != 0) | sc["in_kf"]


def _oracle(sc, pr, oracles, chi2, th=3.0):
    return np.stack([orc.fuse_search(Ko, fr.SF, fr.INV_SIGMA2, pr["valid"][k], pr["u"][k], pr["v"][k], pr["ur"][k], pr["level"][k],
                                     sc["desc"], th, chi2) for k, Ko in enumerate(oracles)])


def _same_bits(got, want):
    for name in FIELDS:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]).astype(got[name].dtype)
        assert a.shape == b.shape, name
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8])


@pytest.mark.parametrize("seed,n,K", GPU_SCENES[:len(PROJECTION_SHAPES)])
def test_projection_equals_spec32_bit_for_bit(seed, n, K):
    sc = fr.scene(seed, n, K)
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    got = mp.project_fuse(_poses(sc["poses"]), slot, skip=_mask(sc))
    _same_bits(got, fr.spec32(sc))
    # no mask at all
    none = mp.project_fuse(_poses(sc["poses"]), slot)
    _same_bits(none, fr.spec32(sc, skip=np.zeros((K, n), np.uint8), in_kf=np.zeros((K, n), bool)))


@pytest.mark.parametrize("seed,n,K", [s for s in GPU_SCENES[:len(PROJECTION_SHAPES)] if s[1] >= 255 and s[2] in (3, 20)])
def test_projection_agrees_with_ref64_outside_the_guard_bands(seed, n, K):
    sc = fr.scene(seed, n, K)
    slot = _slots(n, seed)
    got = _table(sc, slot).project_fuse(_poses(sc["poses"]), slot, skip=_mask(sc))
    r64 = fr.ref64(sc)
    out = fr.excluded(r64)
    share = out.mean()
    print(f"excluded share {share:.4f}")
    assert share <= 0.02
    keep = ~out
    assert np.array_equal(got["valid"][keep], r64["valid"][keep])
    assert np.array_equal(got["level"][keep], r64["level"][keep])
    ok = keep & (r64["valid"] != 0)
    for name in ("u", "v", "ur"):
        # float32 projection of a KITTI-sized image: |u| < 1241 -> half an ulp is 6e-5, a handful of operations deep
        assert np.abs(got[name][ok] - r64[name][ok]).max() < 2e-3, name
    assert np.allclose(got["dist"][ok], r64["dist"][ok], rtol=1e-6)


@pytest.mark.parametrize("resident", [False, True], ids=["host_arrays", "resident_frames"])
@pytest.mark.parametrize("chi2", [True, False], ids=["gated", "ungated"])
def test_one_call_equals_two_step_form_and_oracle(chi2, resident):
    import orb_slam2_annotate_amd as amd
    seed, n, K = GPU_SCENES[len(PROJECTION_SHAPES)]
    sc = fr.scene(seed, n, K)
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    poses = _poses(sc["poses"])
    views, oracles = _frames(sc, resident)
    best, projected = mp.fuse(views, poses, slot, skip=_mask(sc), th=3.0, chi2_gate=chi2, scale_factors=fr.SF,
                              inv_level_sigma2=fr.INV_SIGMA2 if chi2 else None, return_projected=True)
    pr = mp.project_fuse(poses, slot, skip=_mask(sc))
    two = amd.ORBmatcher(0.6).FuseSearchMulti(views, fr.SF, pr["valid"], pr["u"], pr["v"], pr["level"], mp.descriptors(slot), th=3.0,
                                              inv_level_sigma2=fr.INV_SIGMA2 if chi2 else None, ur=pr["ur"])
    assert np.array_equal(best, two)
    assert np.array_equal(projected, pr["valid"])
    ref = _oracle(sc, pr, oracles, chi2)
    assert np.array_equal(best, ref)
    assert ((ref >= 0).sum(axis=1) > 10).all(), (ref >= 0).sum(axis=1)
    if chi2:  # the gate really rejects something the ungated search accepts
        assert (_oracle(sc, pr, oracles, False) != ref).any()


def _graph_for(sc, slot, kf_slot, point_capacity, row_width=8):
    """An ObservationGraph in which point i observes key frame k where sc['in_kf'][k, i] (slots the graph has no room for
    observe nothing), plus observations of key frames that are no target."""
    from orb_slam2_annotate_amd.observation_graph import ObservationGraph
    K, n = sc["in_kf"].shape
    g = ObservationGraph(point_capacity, 64, row_width)
    others = np.array([k for k in range(40, 64) if k not in set(kf_slot.tolist())][:row_width], np.int32)
    allkf = np.concatenate([kf_slot, others]).astype(np.int32)
    # the targets get the LARGEST ids: a row is ordered by id, so a target is the last entry a scan reaches
    ids = np.concatenate([1000 + K - np.arange(K), np.arange(len(others))]).astype(np.int64)  # (target 0 the largest of all)
    g.set_keyframes(allkf, ids, np.zeros((len(allkf), 3), np.float32))
    inside = slot < point_capacity
    g.set_points(slot[inside], np.zeros(inside.sum(), np.uint8), np.full(inside.sum(), -1, np.int32))
    kk, ii = np.nonzero(sc["in_kf"] & inside[None, :])
    g.add_observations(slot[ii], kf_slot[kk], np.arange(len(ii)) % 300, np.zeros(len(ii), np.uint8), np.zeros(len(ii), np.uint8))
    rng = np.random.default_rng(5)
    extra = np.flatnonzero(inside & (rng.random(n) < 0.3))
    for j in range(3):  # unrelated observations in front of the targets
        g.add_observations(slot[extra], np.full(len(extra), others[j], np.int32), np.zeros(len(extra), np.uint16),
                           np.zeros(len(extra), np.uint8), np.ones(len(extra), np.uint8))
    return g, others


def _host_mask(g, sc, slot, kf_slot):
    """IsInKeyFrame from the rows of the graph's mirror"""
    K, n = sc["in_kf"].shape
    m = np.zeros((K, n), bool)
    for i in range(n):
        if slot[i] >= g.point_capacity:
            continue
        seen = set(g.get_row(int(slot[i]))["entries"]["kf_slot"].tolist())
        for k in range(K):
            m[k, i] = int(kf_slot[k]) in seen
    return m


def test_is_in_keyframe_from_the_graph():
    seed, n, K = GPU_SCENES[len(PROJECTION_SHAPES) + 1]
    sc = fr.scene(seed, n, K)
    slot = _slots(n, seed)
    full = 3  # (engineered: level 3 for pose 0, searched unless it observes key frame 0); its slot must lie inside the graph
    if slot[full] >= CAP // 2:
        j = 16 + int(np.flatnonzero(slot[16:] < CAP // 2)[0])
        slot[[full, j]] = slot[[j, full]]
    mp = _table(sc, slot)
    poses = _poses(sc["poses"])
    views, _ = _frames(sc, True)
    kf_slot = np.array([7, 3, 11], np.int32)[:K]
    g, others = _graph_for(sc, slot, kf_slot, CAP // 2)
    # a row filled to row_width whose LAST entry is target 0
    have = len(g.get_row(int(slot[full]))["entries"])
    fill = [int(k) for k in others if k not in g.get_row(int(slot[full]))["entries"]["kf_slot"].tolist()][:g.row_width - have - 1]
    g.add_observations(np.full(len(fill), slot[full], np.int32), fill, np.zeros(len(fill), np.uint16), np.zeros(len(fill), np.uint8),
                       np.zeros(len(fill), np.uint8))
    g.add_observations([slot[full]], [kf_slot[0]], [5], [0], [0])
    row = g.get_row(int(slot[full]))["entries"]
    assert len(row) == g.row_width and row["kf_slot"][-1] == kf_slot[0]

    def both():
        mask = _host_mask(g, sc, slot, kf_slot)
        a = mp.fuse(views, poses, slot, graph=g, kf_slot=kf_slot, skip=sc["skip"], scale_factors=fr.SF, inv_level_sigma2=fr.INV_SIGMA2,
                    return_projected=True)
        b = mp.fuse(views, poses, slot, skip=(sc["skip"] != 0) | mask, scale_factors=fr.SF, inv_level_sigma2=fr.INV_SIGMA2,
                    return_projected=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        pg = mp.project_fuse(poses, slot, graph=g, kf_slot=kf_slot, skip=sc["skip"])
        _same_bits(pg, fr.spec32(sc, in_kf=mask))
        return mask, a

    mask, (best, projected) = both()
    assert mask[0, full] and not projected[0, full]
    assert mask.sum() > 20 and (mask.any(axis=1)).all()
    assert not mask[:, slot >= CAP // 2].any() and (slot >= CAP // 2).any()
    assert (best >= 0).sum() > 20
    # MapPoint::EraseObservation: the point is searched again
    gone_k, gone_i = np.nonzero(mask)
    gone_k, gone_i = np.append(gone_k[:10], 0), np.append(gone_i[:10], full)
    g.erase_observations(slot[gone_i], kf_slot[gone_k])
    mask2, (best2, projected2) = both()
    assert not mask2[gone_k, gone_i].any()
    assert projected2[0, full] == fr.spec32(sc, in_kf=mask2)["valid"][0, full] == 1
    g.close()


def test_table_update_between_two_calls_is_honoured():
    seed, n, K = GPU_SCENES[len(PROJECTION_SHAPES) + 2]
    sc = fr.scene(seed, n, K)
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    poses = _poses(sc["poses"])
    views, oracles = _frames(sc, True)
    kw = dict(skip=_mask(sc), scale_factors=fr.SF, inv_level_sigma2=fr.INV_SIGMA2)
    before = mp.fuse(views, poses, slot, **kw)
    assert np.array_equal(before, _oracle(sc, fr.spec32(sc), oracles, True))
    hit = np.flatnonzero((before[0] >= 0) & (np.arange(n) >= fr.ENGINEERED + 3))
    moved, flipped, redescribed = hit[:3]
    sc["pos"][moved] = sc["pos"][moved] + np.float32([0.0, 0.0, -60.0])  # behind every camera
    sc["flags"][flipped] |= 1
    sc["desc"][redescribed] ^= 0xFF
    ch = np.array([moved, flipped, redescribed])
    mp.update(slot[ch], sc["pos"][ch], sc["normal"][ch], sc["min_dist"][ch], sc["max_dist"][ch], sc["desc"][ch], sc["flags"][ch])
    after, projected = mp.fuse(views, poses, slot, return_projected=True, **kw)
    pr = fr.spec32(sc)
    assert np.array_equal(projected, pr["valid"])
    assert np.array_equal(after, _oracle(sc, pr, oracles, True))
    assert (after[:, moved] == -1).all() and (after[:, flipped] == -1).all() and after[0, redescribed] != before[0, redescribed]


def test_sim3_form():
    seed, n, K = GPU_SCENES[len(PROJECTION_SHAPES) + 3]
    sc = fr.scene(seed, n, K)
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    sim = fr.sim3_poses(sc, 1.37)
    assert any(not np.array_equal(a["tcw"], b["tcw"]) or not np.array_equal(a["Rcw"], b["Rcw"]) for a, b in zip(sim, sc["poses"]))
    poses = _poses(sim)
    pr = fr.spec32(sc, poses=sim)
    _same_bits(mp.project_fuse(poses, slot, skip=_mask(sc)), pr)
    views, oracles = _frames(sc, False)
    best = mp.fuse(views, poses, slot, skip=_mask(sc), th=4.0, chi2_gate=False, scale_factors=fr.SF)
    assert np.array_equal(best, _oracle(sc, pr, oracles, False, th=4.0))
    assert (best >= 0).sum() > 20
    # a stereo key frame's u_right does not influence the ungated search (src/ORBmatcher.cc:1197-1214 reads no mvuRight)
    assert sc["frames"][0]["u_right"] is not None
    junk = [None if f["u_right"] is None else (f["x"] - 500.0).astype(np.float32) for f in sc["frames"]]
    views2, _ = _frames(sc, True, u_right=junk)
    assert np.array_equal(mp.fuse(views2, poses, slot, skip=_mask(sc), th=4.0, chi2_gate=False, scale_factors=fr.SF), best)


def test_bad_arguments_return_invalid_and_launch_nothing():
    import ctypes as C
    from orb_slam2_annotate_amd import OrbfeError, _lib
    from orb_slam2_annotate_amd._lib import ERR_INVALID, ptr
    from orb_slam2_annotate_amd.matcher import debug_thread_stream_idle
    from orb_slam2_annotate_amd.observation_graph import ObservationGraph
    sc = fr.scene(41, 64, 2)
    n, K = 64, 2
    slot = _slots(n, 1)
    mp = _table(sc, slot)
    poses = _poses(sc["poses"])
    views, _ = _frames(sc, False)
    g = ObservationGraph(CAP, 16, 8)
    kw = dict(scale_factors=fr.SF, inv_level_sigma2=fr.INV_SIGMA2)
    good = mp.fuse(views, poses, slot, **kw)
    assert debug_thread_stream_idle()

    def refused(call):
        with pytest.raises(OrbfeError) as ei:
            call()
        assert ei.value.code == ERR_INVALID
        assert debug_thread_stream_idle()

    for bad in (CAP, -1, 1 << 30):  # a slot outside the table
        s = slot.copy()
        s[7] = bad
        refused(lambda: mp.project_fuse(poses, s))
        refused(lambda: mp.fuse(views, poses, s, **kw))
    many = [poses[0]] * 65  # K = 65
    refused(lambda: mp.project_fuse(many, slot))
    refused(lambda: mp.fuse([views[0]] * 65, many, slot, **kw))
    for bad in (16, -1):  # a kf slot outside the graph
        refused(lambda: mp.project_fuse(poses, slot, graph=g, kf_slot=[0, bad]))
        refused(lambda: mp.fuse(views, poses, slot, graph=g, kf_slot=[0, bad], **kw))
    # a pose that predicts more levels than the tables hold; a key-frame octave outside the pyramid (gated only)
    refused(lambda: mp.fuse(views, poses, slot, scale_factors=fr.SF[:5], inv_level_sigma2=fr.INV_SIGMA2[:5]))
    short = _poses(sc["poses"])
    for p in short:
        p.n_levels = 5
    refused(lambda: mp.fuse(views, short, slot, scale_factors=fr.SF[:5], inv_level_sigma2=fr.INV_SIGMA2[:5]))
    assert mp.fuse(views, short, slot, chi2_gate=False, scale_factors=fr.SF[:5]).shape == (K, n)
    # NULL arrays, straight at the C ABI
    L = _lib.load()
    pa = (_lib.CameraPoseC * K)(*poses)
    best = np.zeros(K * n, np.int32)
    vw = (C.POINTER(_lib.FrameViewC) * K)(*[C.pointer(v.c) for v in views])
    assert L.orbfe_project_fuse(mp._h, None, n, None, K, None, pa, *([None] * 7)) == ERR_INVALID
    assert L.orbfe_project_fuse(mp._h, None, n, ptr(slot), K, None, None, *([None] * 7)) == ERR_INVALID
    assert L.orbfe_project_fuse(mp._h, g._h, n, ptr(slot), K, None, pa, *([None] * 7)) == ERR_INVALID
    assert L.orbfe_fuse_mappoints(mp._h, None, n, ptr(slot), K, vw, None, pa, None, None, ptr(fr.INV_SIGMA2), 8, 3.0, 1, ptr(best), None) == ERR_INVALID
    assert L.orbfe_fuse_mappoints(mp._h, None, n, ptr(slot), K, vw, None, pa, None, ptr(fr.SF), None, 8, 3.0, 1, ptr(best), None) == ERR_INVALID
    assert L.orbfe_fuse_mappoints(mp._h, None, n, ptr(slot), K, None, None, pa, None, ptr(fr.SF), ptr(fr.INV_SIGMA2), 8, 3.0, 1, ptr(best), None) == ERR_INVALID
    assert L.orbfe_fuse_mappoints(mp._h, None, n, ptr(slot), K, vw, None, pa, None, ptr(fr.SF), ptr(fr.INV_SIGMA2), 8, 3.0, 1, None, None) == ERR_INVALID
    assert debug_thread_stream_idle()
    # nothing to do is fine, and touches nothing
    assert mp.fuse([], [], slot, **kw).shape == (0, n)
    assert mp.fuse(views, poses, [], **kw).shape == (K, 0)
    assert mp.project_fuse([], slot)["valid"].shape == (0, n)
    assert debug_thread_stream_idle()
    # the refused calls changed nothing
    assert np.array_equal(mp.fuse(views, poses, slot, **kw), good)
    g.close()


def test_two_threads_on_one_table():
    seed, n, K = GPU_SCENES[len(PROJECTION_SHAPES) + 4]
    sc = fr.scene(seed, n, K)
    slot = _slots(n, seed)
    mp = _table(sc, slot)
    poses = _poses(sc["poses"])
    views, _ = _frames(sc, True)
    kw = dict(skip=_mask(sc), scale_factors=fr.SF, inv_level_sigma2=fr.INV_SIGMA2)
    want_all = mp.fuse(views, poses, slot, **kw)
    half = n // 2
    want_half = mp.fuse(views[:2], poses[:2], slot[:half], skip=_mask(sc)[:2, :half], scale_factors=fr.SF, inv_level_sigma2=fr.INV_SIGMA2)
    got, errors = {}, []

    def work(name, call):
        try:
            got[name] = [call() for _ in range(8)]
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=("all", lambda: mp.fuse(views, poses, slot, **kw))),
               threading.Thread(target=work, args=("half", lambda: mp.fuse(views[:2], poses[:2], slot[:half], skip=_mask(sc)[:2, :half],
                                                                           scale_factors=fr.SF, inv_level_sigma2=fr.INV_SIGMA2)))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert all(np.array_equal(r, want_all) for r in got["all"]) and all(np.array_equal(r, want_half) for r in got["half"])
