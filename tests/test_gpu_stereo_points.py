"""GPU: orbfe_create_stereo_points -- stereo / RGB-D map points born on the resident map-point table and observation
graph -- against the sequential restatement tests/stereo_points_ref.py, on the engineered frames of that file (at most 130
keypoints) plus one of 2100 and one of 16384 keypoints, which exist for the sort's multi-wave and full-LDS forms only.

The world of a case: kf slot 0 (mnId 3) observes the points that occupy keypoints of the frame; kf slot 2 (mnId 9) is the
new key frame, its centre a little off the frame's (so a wrong centre shows).  Keypoint i's earlier point, occupied or
stale, lives in slot i; the new points take a shuffled list of slots above n.  Normal and range cannot be read from the
table: they are observed through Frame::isInFrustum (ProjectInFrustum) on a second table that holds the restatement's
values -- view_cos from four camera centres pins the normal, the predicted level and the in / out decision of a camera
moved back by three units, which puts part of the points outside 1.2 * max_dist, pin the range."""
import threading

import numpy as np
import pytest

import orb_slam2_annotate_amd as amd
import stereo_points_ref as ref
from orb_slam2_annotate_amd import OrbfeError, _lib
from orb_slam2_annotate_amd.map_points import MP_OBSERVED

pytestmark = pytest.mark.gpu

f32 = np.float32
KF_OLD, KF_NEW = 0, 2
FRAMES = ref.frames()
BY_NAME = {f["name"]: f for f in FRAMES}
INV_SIGMA2 = (1.0 / (ref.SCALE * ref.SCALE)).astype(f32)


def big_frame(n, seed, all_candidates, keep_every):
    """n keypoints; every depth positive (all_candidates) or 60 % of them; all occupied but every keep_every-th"""
    rng = np.random.default_rng(seed)
    d = rng.uniform(0.5, 30.0, n).astype(f32)
    if not all_candidates:
        d[rng.random(n) < 0.4] = 0.0
    d[::7] = f32(7.25)  # ties across waves
    occ = np.ones(n, np.uint8)
    occ[::keep_every] = 0
    st = np.zeros(n, np.uint8)
    st[::2 * keep_every] = 1
    return ref._frame(f"big{n}", d, 25.0, occ, st & (1 - occ), seed=seed)


def centre_of(f, pose, mode):
    ow = np.array(list(pose.Ow), f32)
    return ow if mode == ref.TEMPORAL else ow + f32([0.03125, -0.0625, 0.015625])


class Case:
    """graph + table + resident frame of one engineered frame, as they stand before the call"""

    def __init__(self, f, mode, capacity=None):
        self.f, self.mode, n = f, mode, f["n"]
        self.pose = ref.frame_pose(f)
        self.centre = centre_of(f, self.pose, mode)
        self.want = ref.select(f["x"], f["y"], f["octave"], f["depth"], f["occupied"], f["stale"], self.pose, f["th"], mode,
                               ref.SCALE, self.centre)
        cap = max(n, 1) if capacity is None else capacity
        self.p_cap = n + max(n, 1) + 8
        self.new_slot = (n + np.random.default_rng(f["seed"]).permutation(max(n, 1) + 8)[:cap]).astype(np.int32)
        self.mp = amd.MapPoints(self.p_cap)
        self.view = amd.FrameView(f["x"], f["y"], f["octave"], f["desc"], (0.0, ref.WIDTH, 0.0, ref.HEIGHT),
                                  angle=np.zeros(n, f32), u_right=f["u_right"])
        self.frame = self.view.upload()
        self.g = None
        self.row = np.full(n, -1, np.int32)
        held = np.flatnonzero(f["occupied"] | f["stale"]).astype(np.int32)
        self.row[held] = held
        if len(held):  # the earlier points, somewhere else
            self.mp.update(held, np.tile(f32([50, 50, 50]), (len(held), 1)), np.tile(f32([0, 0, 1]), (len(held), 1)),
                           np.full(len(held), 0.1, f32), np.full(len(held), 100.0, f32), np.zeros((len(held), 32), np.uint8),
                           np.full(len(held), MP_OBSERVED, np.uint8))
        if mode != ref.TEMPORAL:
            g = self.g = amd.ObservationGraph(self.p_cap, 4, 8)
            g.set_keyframes([KF_OLD, KF_NEW], [3, 9], np.array([[9.0, 9.0, 9.0], self.centre], f32))
            g.enable_keyframe_points(max(64, (n + 63) // 64 * 64))
            occ = np.flatnonzero(f["occupied"]).astype(np.int32)
            g.set_points(held, np.zeros(len(held), np.uint8), np.full(len(held), KF_OLD, np.int32))
            g.add_observations(occ, np.full(len(occ), KF_OLD), occ, np.zeros(len(occ), np.uint8), np.ones(len(occ), np.uint8))
            g.set_keyframe_points(KF_NEW, self.row)

    def call(self):
        f = self.f
        return self.mp.create_stereo_points(self.g, self.frame, KF_NEW, self.pose, f["depth"], f["th"], self.mode, ref.SCALE,
                                            self.new_slot, occupied=f["occupied"], stale=f["stale"])

    def probes(self):
        """the frame's own pose, two moved sideways, one moved back by three units"""
        R = np.array(list(self.pose.Rcw), f32).reshape(3, 3)
        ow = np.array(list(self.pose.Ow), f32)
        out = []
        for d in ([0, 0, 0], [0.3, 0, 0], [0, 0.3, 0.1], list(-3.0 * R[2])):
            c = ow + f32(d)
            out.append(amd.camera_pose(R, -(R @ c), ref.K4, 40.0, (-1e4, 1e4, -1e4, 1e4), 1.2, ref.N_LEVELS, Ow=c))
        return out

    def observe(self, mp, slots):
        return [mp.ProjectInFrustum(slots, p, viewing_cos_limit=-2.0) for p in self.probes()]

    def close(self):
        self.frame.close()
        self.mp.close()
        if self.g is not None:
            self.g.close()


def same_observation(a, b):
    for pa, pb in zip(a, b):
        for k in pa:
            if pa[k].dtype == np.float32:
                assert ref.same_bits(pa[k], pb[k]), k
            else:
                assert np.array_equal(pa[k], pb[k]), k


def check_case(c, got, rows_of=None):
    f, want, mode = c.f, c.want, c.mode
    m = want["n_created"]
    assert got["n_created"] == m and got["n_walked"] == want["n_walked"]
    assert np.array_equal(got["created_idx"], want["created_idx"])
    assert np.array_equal(got["created_slot"], c.new_slot[:m])
    assert np.array_equal(got["cleared"], want["cleared"])
    slots = c.new_slot[:m]
    assert ref.same_bits(c.mp.positions(slots), want["pos"])
    assert np.array_equal(c.mp.descriptors(slots), f["desc"][want["created_idx"]])
    # normal and range, through isInFrustum on a table that holds the restatement's values
    twin = amd.MapPoints(c.p_cap)
    if m:
        twin.update(slots, want["pos"], want["normal"], want["min_dist"], want["max_dist"], f["desc"][want["created_idx"]],
                    np.zeros(m, np.uint8))
    seen = c.observe(c.mp, slots)
    same_observation(seen, c.observe(twin, slots))
    twin.close()
    if mode == ref.TEMPORAL:
        return seen
    stereo = (f["u_right"] >= 0).astype(np.uint8)
    for j in (range(m) if rows_of is None else rows_of):
        i = int(want["created_idx"][j])
        r = c.g.get_row(int(slots[j]), from_device=True)
        assert len(r["entries"]) == 1 and r["bad"] == 0 and r["ref_kf_slot"] == KF_NEW and r["n_obs"] == (2 if stereo[i] else 1)
        e = r["entries"][0]
        assert (e["kf_slot"], e["idx"], e["octave"], e["flags"]) == (KF_NEW, i, f["octave"][i], stereo[i])
    row = c.row.copy()
    row[want["created_idx"]] = slots
    assert np.array_equal(c.g.get_keyframe_points(KF_NEW, from_device=True), row)
    # a later UpdateNormalAndDepth on the new slots changes nothing
    if m:
        assert c.g.update_normal_depth(slots, ref.SCALE, mp=c.mp).all()
        same_observation(seen, c.observe(c.mp, slots))
    return seen


@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("f", FRAMES, ids=[f["name"] for f in FRAMES])
def test_equals_the_restatement(f, mode):
    c = Case(f, mode)
    try:
        check_case(c, c.call())
    finally:
        c.close()


def test_the_probes_separate_right_from_wrong():
    """on the 130-keypoint frame: every probe sees points, the one moved back sees some and rejects some (the range gate),
    and a normal or a range that is a little off changes what the probes return"""
    c = Case(BY_NAME["n130"], ref.KEYFRAME)
    try:
        seen = check_case(c, c.call())
        assert all(p["in_view"].any() for p in seen) and not seen[3]["in_view"].all()
        w, m = c.want, c.want["n_created"]
        slots = c.new_slot[:m]
        for field, bump in (("normal", f32(1) + f32(2.0 ** -20)), ("max_dist", f32(1.3)), ("min_dist", f32(1.3))):
            v = {k: w[k].copy() for k in ("pos", "normal", "min_dist", "max_dist")}
            v[field] = (v[field] * bump).astype(f32)
            twin = amd.MapPoints(c.p_cap)
            twin.update(slots, v["pos"], v["normal"], v["min_dist"], v["max_dist"], np.zeros((m, 32), np.uint8), np.zeros(m, np.uint8))
            other = c.observe(twin, slots)
            twin.close()
            assert any(not np.array_equal(a[k], b[k]) for a, b in zip(seen, other) for k in a), field
    finally:
        c.close()


@pytest.mark.parametrize("n,all_candidates,keep", [(2100, False, 4), (2100, True, 4), (16384, True, 32)],
                         ids=["2100_two_tiles", "2100_sort4096", "16384_full_lds"])
def test_large_frames(n, all_candidates, keep):
    f = big_frame(n, 40 + keep + all_candidates, all_candidates, keep)
    c = Case(f, ref.KEYFRAME)
    try:
        got = c.call()
        m = c.want["n_created"]
        assert m > 200 and c.want["n_walked"] < int((f["depth"] > 0).sum())
        check_case(c, got, rows_of=list(range(0, m, max(1, m // 48))))
    finally:
        c.close()


@pytest.mark.parametrize("mode", ref.MODES)
def test_capacity_leaves_both_tables_as_they_were(mode):
    f = BY_NAME["close_then_far"]
    pose = ref.frame_pose(f)
    K = ref.select(f["x"], f["y"], f["octave"], f["depth"], f["occupied"], f["stale"], pose, f["th"], mode, ref.SCALE,
                   centre_of(f, pose, mode))["n_created"] - 1
    c = Case(f, mode, capacity=K)
    try:
        every = np.arange(c.p_cap, dtype=np.int32)

        def state():
            s = [c.mp.positions(every), c.mp.descriptors(every)] + [p[k] for p in c.observe(c.mp, every) for k in sorted(p)]
            if c.g is not None:
                s.append(c.g.get_keyframe_points(KF_NEW, from_device=True))
                for slot in c.new_slot:
                    r = c.g.get_row(int(slot), from_device=True)
                    s += [r["entries"].view(np.uint8), np.array([r["n_obs"], r["bad"], r["ref_kf_slot"]])]
            return s

        before = state()
        with pytest.raises(OrbfeError) as ei:
            c.call()
        assert ei.value.code == _lib.ERR_CAPACITY and ei.value.n_created == K + 1
        for a, b in zip(before, state()):
            assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    finally:
        c.close()


def test_argument_errors():
    f = BY_NAME["n65"]
    c = Case(f, ref.KEYFRAME)
    try:
        def invalid(**kw):
            a = dict(graph=c.g, frame=c.frame, kf_slot=KF_NEW, pose=c.pose, depth=f["depth"], th_depth=f["th"], mode=ref.KEYFRAME,
                     scale_factors=ref.SCALE, new_slot=c.new_slot, occupied=f["occupied"], stale=f["stale"])
            a.update(kw)
            with pytest.raises(OrbfeError) as ei:
                c.mp.create_stereo_points(**a)
            assert ei.value.code == _lib.ERR_INVALID

        invalid(depth=f["depth"][:-1], occupied=None, stale=None)  # n != F->n
        # n > 16384: a resident frame holds at most 16384 keypoints, so such an n is also never the frame's
        invalid(depth=np.ones(16385, f32), occupied=None, stale=None)
        invalid(scale_factors=ref.SCALE[:int(f["octave"].max())])  # an octave at n_levels
        for bad in (-1, c.p_cap, int(c.new_slot[1])):
            s = c.new_slot.copy()
            s[0] = bad
            invalid(new_slot=s)
        s = c.new_slot.copy()
        s[0] = int(np.flatnonzero(f["occupied"])[0])  # a live row
        invalid(new_slot=s)
        invalid(kf_slot=1)  # never set
        invalid(kf_slot=4)
        invalid(graph=None)
        invalid(graph=None, mode=ref.ALL)
        both = f["stale"].copy()
        both[np.flatnonzero(f["occupied"])[0]] = 1
        invalid(stale=both)
        p = ref.frame_pose(f)
        p.fx = 0.0
        invalid(pose=p)
        p = ref.frame_pose(f)
        p.Rcw[0] = float("inf")
        invalid(pose=p)
        small = amd.ObservationGraph(f["n"] + 4, 4, 8)  # the new slots lie past its point capacity
        small.set_keyframes([KF_NEW], [9], np.zeros((1, 3), f32))
        invalid(graph=small)
        small.close()
        check_case(c, c.call())  # and the handles are as usable as before
        # no candidate at all: zero counts
        got = c.mp.create_stereo_points(None, c.frame, KF_NEW, c.pose, np.zeros(f["n"], f32), f["th"], ref.TEMPORAL, ref.SCALE, c.new_slot)
        assert got["n_created"] == 0 and got["n_walked"] == 0 and not got["cleared"].any()
    finally:
        c.close()


def second_frame(c, slots_pos, idx):
    """the created points seen from a camera a little further on: keypoints at their projections, the same descriptors"""
    f = c.f
    R = np.array(list(c.pose.Rcw), f32).reshape(3, 3)
    ow = np.array(list(c.pose.Ow), f32) + f32([0.05, -0.02, 0.04])
    t = -(R @ ow)
    pose2 = amd.camera_pose(R, t, ref.K4, 40.0, (0.0, ref.WIDTH, 0.0, ref.HEIGHT), 1.2, ref.N_LEVELS, Ow=ow)
    Xc = slots_pos @ R.T + t
    x = (ref.K4[0] * Xc[:, 0] / Xc[:, 2] + ref.K4[2]).astype(f32)
    y = (ref.K4[1] * Xc[:, 1] / Xc[:, 2] + ref.K4[3]).astype(f32)
    ur = (x - f32(40.0) / Xc[:, 2]).astype(f32)
    view = amd.FrameView(x, y, f["octave"][idx], f["desc"][idx], (0.0, ref.WIDTH, 0.0, ref.HEIGHT), angle=np.zeros(len(x), f32), u_right=ur)
    T = np.eye(4, dtype=f32)
    T[:3, :3], T[:3, 3] = R, t + f32([0.01, 0.0, -0.01])  # the optimisation starts a little off
    return view, pose2, T


def test_chain_equals_the_five_trip_host_path():
    """create_stereo_points(KEYFRAME) -> SearchLocalPoints on a second frame -> pose_optimization, against the same chain
    fed by orbfe_mappoints_update, set_points, add_observations, assign_keyframe_points and update_normal_depth_mappoints
    with the restatement's values"""
    f = BY_NAME["n130"]
    a, b = Case(f, ref.KEYFRAME), Case(f, ref.KEYFRAME)
    try:
        got = a.call()
        w, m = b.want, b.want["n_created"]
        slots, idx = b.new_slot[:m], b.want["created_idx"]
        b.mp.update(slots, w["pos"], np.zeros((m, 3), f32), np.zeros(m, f32), np.zeros(m, f32), f["desc"][idx], np.full(m, MP_OBSERVED, np.uint8))
        b.g.set_points(slots, np.zeros(m, np.uint8), np.full(m, KF_NEW, np.int32))
        b.g.add_observations(slots, np.full(m, KF_NEW), idx, f["octave"][idx], (f["u_right"][idx] >= 0))
        b.g.assign_keyframe_points(np.full(m, KF_NEW), idx, slots)
        assert b.g.update_normal_depth(slots, ref.SCALE, mp=b.mp).all()
        assert np.array_equal(got["created_slot"], slots)
        view, pose2, T0 = second_frame(a, w["pos"], idx)
        k5 = f32(list(ref.K4) + [40.0])
        results = []
        for c in (a, b):
            nm, match, in_view = c.mp.SearchLocalPoints(view, slots, pose2, ref.SCALE, th=3.0)
            ni, T, flags, _, chi2 = c.mp.pose_optimization(view, slots, match, T0, k5, INV_SIGMA2)
            results.append((nm, match, in_view, ni, T, flags, chi2))
        assert results[0][0] > 20 and results[0][3] > 10
        for x, y in zip(*results):
            assert np.array_equal(np.asarray(x), np.asarray(y))
        assert np.array_equal(a.g.get_keyframe_points(KF_NEW, True), b.g.get_keyframe_points(KF_NEW, True))
    finally:
        a.close()
        b.close()


def test_two_threads_on_two_tables():
    names = ("occupied_stale", "n130")
    single = []
    for name in names:
        c = Case(BY_NAME[name], ref.KEYFRAME)
        got = c.call()
        single.append((got, c.mp.positions(c.new_slot), c.mp.descriptors(c.new_slot)))
        c.close()
    cases = [Case(BY_NAME[name], ref.KEYFRAME) for name in names]
    out, errors = [None, None], []

    def work(k):
        try:
            got = cases[k].call()
            out[k] = (got, cases[k].mp.positions(cases[k].new_slot), cases[k].mp.descriptors(cases[k].new_slot))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert not errors, errors
        for (g1, p1, d1), (g2, p2, d2) in zip(single, out):
            assert all(np.array_equal(g1[k], g2[k]) for k in g1)
            assert ref.same_bits(p1, p2) and np.array_equal(d1, d2)
    finally:
        for c in cases:
            c.close()
