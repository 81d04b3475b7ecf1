"""GPU: orbfe_create_triangulated_points -- CreateNewMapPoints' triangulated points born on the resident map-point table
and observation graph -- against the seven-trip path it replaces, run on a twin table and a twin graph with the same
inputs: orbfe_triangulate_matches_multi, the host replay of `winner`, orbfe_mappoints_update, set_points, add_observations
twice, assign_keyframe_points, orbfe_obsgraph_distinctive_descriptors_mappoints and
orbfe_obsgraph_update_normal_depth_mappoints.  Both must leave byte-identical state.

The scenes are tests/triangulate_ref.py's (every tri_pair branch planted).  Key frame 1 lives in kf slot 1 with mnId 10; the
neighbours take kf slots 3, 0, 4 with mnIds 3, 30, 11, so the winning descriptor comes from either side.  Normal and range
cannot be read from the table: they are observed through Frame::isInFrustum (ProjectInFrustum) from four camera centres, one
moved back so that the range gate rejects part of the points, and a fifth moved forward, where min_dist decides."""
import threading

import numpy as np
import pytest

import orb_slam2_annotate_amd as amd
import tri_points_ref as ref
import triangulate_ref as tr
from orb_slam2_annotate_amd import OrbfeError, _lib
from orb_slam2_annotate_amd.map_points import MP_OBSERVED

pytestmark = pytest.mark.gpu

f32 = np.float32
KF1_SLOT, KF1_ID = 1, 10
KF2_SLOTS, KF2_IDS = [3, 0, 4], [3, 30, 11]
KF_CAP = 6
K4 = (tr.FX, tr.FY, tr.CX, tr.CY)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
INV_SIGMA2 = (1.0 / tr.LEVEL_SIGMA2).astype(f32)
SMALL = dict(seed=7, n1=70, K=3, kind="mixed", n_pairs=110)


def make_scene(seed, n1, K, kind, n_pairs, trim=None):
    """trim: the neighbours keep their first `trim` keypoints (the generator gives them a few more than key frame 1, and a
    frame holds 16384 at the most); matches to the others go"""
    sc = tr.scene(seed, n1, K, kind, n_pairs)
    if trim is not None:
        sc["match12"] = np.where(sc["match12"] >= trim, -1, sc["match12"]).astype(np.int32)
        for f in sc["kf2"]:
            for key in ("x", "y", "octave", "u_right", "depth", "x_raw", "y_raw"):
                if f[key] is not None:
                    f[key] = np.ascontiguousarray(f[key][:trim])
            f["n"] = trim
    rng = np.random.default_rng(seed + 1000)
    for f in [sc["kf1"]] + sc["kf2"]:
        f["desc"] = rng.integers(0, 256, (f["n"], 32), dtype=np.uint8)
    return sc


_SCENES = {}


def scene_of(**spec):
    key = tuple(sorted(spec.items()))
    if key not in _SCENES:
        _SCENES[key] = make_scene(**spec)
    return _SCENES[key]


def cam_of(c, f, ow=None):
    return amd.KeyFrameCamera(c["Tcw"], c["Ow"] if ow is None else ow, c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], depth=f["depth"],
                              x_raw=f["x_raw"], y_raw=f["y_raw"], invfx=c["invfx"], invfy=c["invfy"])


class World:
    """graph + table + resident frames of one scene, as they stand before the birth.  centre_shift moves the centres the
    graph holds away from the cameras' Ow; cam_shift moves the neighbours' cam.Ow instead."""

    def __init__(self, sc, rows=True, capacity=None, centre_shift=0.0, cam_shift=0.0, match12=None):
        self.sc, K, n1 = sc, sc["K"], sc["n1"]
        self.K, self.n1 = K, n1
        self.match12 = sc["match12"] if match12 is None else match12
        frames = [sc["kf1"]] + sc["kf2"]
        self.views = [amd.FrameView(f["x"], f["y"], f["octave"], f["desc"], BOUNDS, angle=np.zeros(f["n"], f32), u_right=f["u_right"])
                      for f in frames]
        self.frames = [v.upload() for v in self.views]
        self.cam1 = cam_of(sc["cam1"], sc["kf1"])
        self.cams2 = [cam_of(c, f, ow=(c["Ow"] + f32(cam_shift)).astype(f32)) for c, f in zip(sc["cams2"], sc["kf2"])]
        self.kf_slots = [KF1_SLOT] + KF2_SLOTS[:K]
        self.kf_ids = [KF1_ID] + KF2_IDS[:K]
        self.centres = np.stack([sc["cam1"]["Ow"]] + [c["Ow"] for c in sc["cams2"]]).astype(f32)
        self.centres = (self.centres + f32(centre_shift) * f32([1.0, -0.5, 0.25])).astype(f32)
        cap = n1 if capacity is None else capacity
        self.p_cap = 2 * n1 + 8
        self.new_slot = (np.random.default_rng(7).permutation(self.p_cap)[:cap]).astype(np.int32)
        self.mp = amd.MapPoints(self.p_cap)
        g = self.g = amd.ObservationGraph(self.p_cap, KF_CAP, 8)
        g.set_keyframes(self.kf_slots, self.kf_ids, self.centres)
        self.rows = rows
        if rows:
            g.enable_keyframe_points(max(64, (max(f["n"] for f in frames) + 63) // 64 * 64))
            for s, f in zip(self.kf_slots, frames):
                g.set_keyframe_points(s, np.full(f["n"], -1, np.int32))
        g.enable_keyframe_descriptors(max(64, (max(f["n"] for f in frames) + 63) // 64 * 64))
        for s, fr in zip(self.kf_slots, self.frames):
            g.set_keyframe_descriptors(s, fr)

    def call(self, **kw):
        a = dict(graph=self.g, kf1=self.frames[0], kf1_slot=KF1_SLOT, cam1=self.cam1, neighbours=self.frames[1:], kf2_slots=self.kf_slots[1:],
                 cams=self.cams2, match12=self.match12, scale_factors=tr.SCALE_FACTORS, level_sigma2=tr.LEVEL_SIGMA2,
                 ratio_factor=tr.RATIO_FACTOR, new_slot=self.new_slot)
        a.update(kw)
        return self.mp.create_triangulated_points(**a)

    def seven_trips(self):
        """the path the call replaces -> the same dict"""
        sc, K, n1 = self.sc, self.K, self.n1
        x3d, status, _, winner = amd.triangulate_matches_multi(self.frames[0], self.cam1, self.frames[1:], self.cams2, self.match12,
                                                               tr.SCALE_FACTORS, tr.LEVEL_SIGMA2, tr.RATIO_FACTOR)
        ck, ci1 = [], []
        for k in range(K):  # the replay of include/orbfe.h: neighbours in order, the pair with k == winner[i1]
            for i1 in range(n1):
                if status[k, i1] == tr.CREATED and winner[i1] == k:
                    ck.append(k)
                    ci1.append(i1)
        ck, ci1 = np.asarray(ck, np.int32), np.asarray(ci1, np.int32)
        m = len(ck)
        ci2 = self.match12[ck, ci1].astype(np.int32) if m else np.zeros(0, np.int32)
        per = np.bincount(ck, minlength=K).astype(np.int32)[:K]
        out = dict(created_k=ck, created_i1=ci1, created_i2=ci2, created_slot=self.new_slot[:m].copy(), status=status.copy(),
                   n_created_per_neighbour=per, n_created=m, x3d=x3d)
        if m > len(self.new_slot):
            raise AssertionError("the twin's slot list is too short")
        if m == 0:
            return out
        slots = self.new_slot[:m]
        f1, g = sc["kf1"], self.g
        self.mp.update(slots, x3d[ck, ci1], np.zeros((m, 3), f32), np.zeros(m, f32), np.zeros(m, f32), np.zeros((m, 32), np.uint8),
                       np.full(m, MP_OBSERVED, np.uint8))
        st = lambda f, i: np.zeros(len(i), np.uint8) if f["u_right"] is None else (f["u_right"][i] >= 0).astype(np.uint8)
        kf2 = np.asarray(self.kf_slots[1:], np.int32)[ck]
        oct2 = np.array([sc["kf2"][k]["octave"][i] for k, i in zip(ck, ci2)], np.uint8)
        st2 = np.array([st(sc["kf2"][k], np.array([i]))[0] for k, i in zip(ck, ci2)], np.uint8)
        g.set_points(slots, np.zeros(m, np.uint8), np.full(m, KF1_SLOT, np.int32))
        g.add_observations(slots, np.full(m, KF1_SLOT), ci1, f1["octave"][ci1].astype(np.uint8), st(f1, ci1))
        g.add_observations(slots, kf2, ci2, oct2, st2)
        if self.rows:
            g.assign_keyframe_points(np.full(m, KF1_SLOT), ci1, slots)
            g.assign_keyframe_points(kf2, ci2, slots)
        assert g.distinctive_descriptors(slots, mp=self.mp)[2].all()
        assert g.update_normal_depth(slots, tr.SCALE_FACTORS, mp=self.mp).all()
        return out

    def probes(self):
        """key frame 1's own pose, two moved sideways, one moved back by three units (the upper range gate rejects part of
        the points) and one moved forward by one and a half (the lower one does)"""
        c = self.sc["cam1"]
        R, ow = c["Tcw"][:, :3].astype(f32), c["Ow"].astype(f32)
        out = []
        for d in ([0, 0, 0], [0.3, 0, 0], [0, 0.3, 0.1], list(-3.0 * R[2]), list(1.5 * R[2])):
            o = (ow + f32(d)).astype(f32)
            out.append(amd.camera_pose(R, -(R @ o), K4, tr.MBF, (-1e4, 1e4, -1e4, 1e4), 1.2, tr.N_LEVELS, Ow=o))
        return out

    def observe(self, slots):
        return [self.mp.ProjectInFrustum(slots, p, viewing_cos_limit=-2.0) for p in self.probes()]

    def state(self, slots, row_slots=None):
        """everything the call may change, as bytes, read from the device"""
        slots = np.asarray(slots, np.int32)
        s = [self.mp.positions(slots), self.mp.descriptors(slots)] + [p[k] for p in self.observe(slots) for k in sorted(p)]
        for slot in (slots if row_slots is None else row_slots):
            r = self.g.get_row(int(slot), from_device=True)
            s += [r["entries"].view(np.uint8), np.array([r["n_obs"], r["bad"], r["ref_kf_slot"]])]
        if self.rows:
            s += [self.g.get_keyframe_points(k, from_device=True) for k in self.kf_slots]
        return [np.ascontiguousarray(a).view(np.uint8) for a in s]

    def close(self):
        for fr in self.frames:
            fr.close()
        self.mp.close()
        self.g.close()


def same_state(a, b):
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(x, y), j


def same_lists(got, want):
    assert got["n_created"] == want["n_created"]
    for k in ("created_k", "created_i1", "created_i2", "created_slot", "status", "n_created_per_neighbour"):
        assert np.array_equal(got[k], want[k]), k


def both(sc, row_slots=None, **kw):
    """the call on one world, the seven trips on its twin: lists, counts, statuses and state equal -> (world, got, want)"""
    a, b = World(sc, **kw), World(sc, **kw)
    try:
        got, want = a.call(), b.seven_trips()
        same_lists(got, want)
        m = got["n_created"]
        slots = a.new_slot[:m]
        assert ref.same_bits(a.mp.positions(slots), want["x3d"][want["created_k"], want["created_i1"]])
        rs = None if row_slots is None else slots[::max(1, m // row_slots)]
        every = np.arange(a.p_cap, dtype=np.int32) if row_slots is None else slots
        same_state(a.state(every, rs), b.state(every, rs))
    except BaseException:
        a.close()
        raise
    finally:
        b.close()
    return a, got, want


@pytest.mark.parametrize("rows", [True, False], ids=["kf_rows", "no_kf_rows"])
def test_small_mixed_scene_equals_the_seven_trips(rows):
    sc = scene_of(**SMALL)
    a, got, _ = both(sc, rows=rows)
    try:
        st = got["status"]
        assert set(tr.REACHABLE) <= set(np.unique(st).tolist())  # every tri_pair branch that can be reached
        made = (st == tr.CREATED).sum(axis=0)
        assert (made >= 2).any()  # a contested keypoint: the lower neighbour has it
        i1 = int(np.flatnonzero(made >= 2)[0])
        k_lo = int(np.flatnonzero(st[:, i1] == tr.CREATED)[0])
        at = int(np.flatnonzero(got["created_i1"] == i1)[0])
        assert got["created_k"][at] == k_lo and (got["created_i1"] == i1).sum() == 1
        assert got["n_created"] > 20 and len(set(got["created_k"].tolist())) == 3
        m = got["n_created"]
        stereo1 = np.zeros(sc["n1"], bool) if sc["kf1"]["u_right"] is None else sc["kf1"]["u_right"] >= 0
        r = a.g.get_row(int(got["created_slot"][at]), from_device=True)
        assert len(r["entries"]) == 2 and r["bad"] == 0 and r["ref_kf_slot"] == KF1_SLOT
        i2 = int(got["created_i2"][at])
        stereo2 = sc["kf2"][k_lo]["u_right"][i2] >= 0
        assert r["n_obs"] == (2 if stereo1[i1] else 1) + (2 if stereo2 else 1)
        # the descriptor: the key frame with the smaller mnId
        want_desc = np.stack([sc["kf2"][k]["desc"][j2] if KF2_IDS[k] < KF1_ID else sc["kf1"]["desc"][j1]
                              for k, j1, j2 in zip(got["created_k"], got["created_i1"], got["created_i2"])])
        assert np.array_equal(a.mp.descriptors(got["created_slot"]), want_desc)
        assert {KF2_IDS[k] < KF1_ID for k in got["created_k"]} == {True, False}
        assert m == got["n_created_per_neighbour"].sum()
    finally:
        a.close()


def test_probes_separate_right_from_wrong():
    """every probe sees points, the one moved back sees some and rejects some (the range gate), and a normal or a range
    that is a little off changes what the probes return"""
    sc = scene_of(**SMALL)
    a, got, want = both(sc)
    try:
        slots, m = got["created_slot"], got["n_created"]
        seen = a.observe(slots)
        assert all(p["in_view"].any() for p in seen) and not seen[3]["in_view"].all() and not seen[4]["in_view"].all()
        sel = ref.select(a.match12, got["status"], want["x3d"], KF1_ID, KF2_IDS[:a.K], a.centres[0], a.centres[1:], sc["kf1"]["octave"],
                         tr.SCALE_FACTORS)
        assert np.array_equal(sel["created_i1"], got["created_i1"])
        for field, bump in ((None, None), ("normal", f32(1) + f32(2.0 ** -20)), ("max_dist", f32(1.3)), ("min_dist", f32(1.3))):
            v = {k: sel[k].copy() for k in ("pos", "normal", "min_dist", "max_dist")}
            if field:
                v[field] = (v[field] * bump).astype(f32)
            a.mp.update(slots, v["pos"], v["normal"], v["min_dist"], v["max_dist"], None, np.full(m, MP_OBSERVED, np.uint8))
            other = a.observe(slots)
            differs = any(not np.array_equal(x[k], y[k]) for x, y in zip(seen, other) for k in x)
            assert differs == (field is not None), field  # (None: the restatement's own values give the same bytes)
    finally:
        a.close()


def test_pair_list_across_wave_workgroup_and_chunk():
    sc = scene_of(seed=3, n1=1100, K=2, kind="mixed", n_pairs=2150)
    a, got, _ = both(sc, row_slots=64)
    try:
        k, i1 = np.nonzero(a.match12 >= 0)  # the dense list, in (k, i1) order
        assert len(k) == 2150
        kept = np.zeros(len(k), bool)
        place = {(int(x), int(y)): p for p, (x, y) in enumerate(zip(k, i1))}
        for x, y in zip(got["created_k"], got["created_i1"]):
            kept[place[(int(x), int(y))]] = True
        for lo, hi in ((0, 64), (64, 128), (960, 1024), (1024, 1088), (1984, 2048), (2048, 2150)):
            assert kept[lo:hi].any(), (lo, hi)
        assert (got["n_created_per_neighbour"] > 0).all()  # (the second neighbour makes only what the first could not)
    finally:
        a.close()


def test_16384_keypoints():
    sc = scene_of(seed=5, n1=16384, K=1, kind="mono", n_pairs=16384, trim=16384)
    a, got, _ = both(sc, row_slots=48)
    try:
        assert got["n_created"] > 4000  # (the generator plants a failure in seven of every ten pairs)
    finally:
        a.close()


def test_following_updates_change_no_byte():
    sc = scene_of(**SMALL)
    a = World(sc)
    try:
        got = a.call()
        slots = got["created_slot"]
        before = a.state(slots)
        assert a.g.update_normal_depth(slots, tr.SCALE_FACTORS, mp=a.mp).all()
        kf, idx, valid = a.g.distinctive_descriptors(slots, mp=a.mp)
        assert valid.all()
        lower = np.array([KF2_IDS[k] < KF1_ID for k in got["created_k"]])
        assert np.array_equal(kf, np.where(lower, np.asarray(KF2_SLOTS)[got["created_k"]], KF1_SLOT))
        assert np.array_equal(idx, np.where(lower, got["created_i2"], got["created_i1"]))
        same_state(before, a.state(slots))
    finally:
        a.close()


def test_cam_ow_decides_the_pairs_and_the_graph_centres_normal_and_range():
    sc = scene_of(**SMALL)
    base, got0, _ = both(sc)
    moved, got1, _ = both(sc, centre_shift=0.0625)       # the graph's centres off cam.Ow: still the seven trips' state
    camow, got2, _ = both(sc, cam_shift=0.75)            # the neighbours' cam.Ow off the graph's centres: likewise
    try:
        slots = got0["created_slot"]
        # the graph's centres are not read by tri_pair: same pairs, same positions ...
        same_lists(got1, got0)
        assert ref.same_bits(moved.mp.positions(slots), base.mp.positions(slots))
        # ... but they are what normal and range come from
        s0, s1 = base.observe(slots), moved.observe(slots)
        assert any(not np.array_equal(x[k], y[k]) for x, y in zip(s0, s1) for k in x)
        sel = ref.select(moved.match12, got1["status"], np.zeros((moved.K, moved.n1, 3), f32), KF1_ID, KF2_IDS[:moved.K], moved.centres[0],
                         moved.centres[1:], sc["kf1"]["octave"], tr.SCALE_FACTORS)
        assert np.array_equal(sel["created_i1"], got1["created_i1"])
        # cam.Ow is what the scale test (and UnprojectStereo) of tri_pair reads: moving it changes statuses or positions
        same = got2["n_created"] == got0["n_created"] and np.array_equal(got2["status"], got0["status"]) and \
            ref.same_bits(camow.mp.positions(got2["created_slot"]), base.mp.positions(slots))
        assert not same
    finally:
        base.close()
        moved.close()
        camow.close()


def test_capacity_leaves_both_tables_as_they_were():
    sc = scene_of(**SMALL)
    a = World(sc)
    m = a.call()["n_created"]
    a.close()
    for cap, ok in ((m, True), (m + 1, True), (m - 1, False)):
        c = World(sc, capacity=cap)
        try:
            every = np.arange(c.p_cap, dtype=np.int32)
            before = c.state(every)
            if ok:
                assert c.call()["n_created"] == m
                continue
            with pytest.raises(OrbfeError) as ei:
                c.call()
            assert ei.value.code == _lib.ERR_CAPACITY and ei.value.n_created == m
            same_state(before, c.state(every))
        finally:
            c.close()


def test_argument_errors_leave_the_tables_unchanged():
    sc = scene_of(**SMALL)
    c = World(sc)
    try:
        every = np.arange(c.p_cap, dtype=np.int32)
        before = c.state(every)

        def invalid(**kw):
            with pytest.raises(OrbfeError) as ei:
                c.call(**kw)
            assert ei.value.code == _lib.ERR_INVALID, kw.keys()

        live = np.argwhere(c.match12 >= 0)
        k0, i0 = (int(v) for v in live[0])
        m = c.match12.copy(); m[k0, i0] = sc["kf2"][k0]["n"]
        invalid(match12=m)  # what triangulate_matches_multi rejects: a match outside n2 ...
        m = c.match12.copy(); m[k0, i0] = -2
        invalid(match12=m)
        invalid(scale_factors=tr.SCALE_FACTORS[:3], level_sigma2=tr.LEVEL_SIGMA2[:3])  # ... an octave outside the table ...
        c1 = c.cam1
        invalid(cam1=amd.KeyFrameCamera(c1.Tcw.reshape(3, 4), c1.Ow, c1.fx, c1.fy, c1.cx, c1.cy, c1.mb, c1.mbf))  # ... a stereo keypoint, no depth
        m = c.match12.copy()
        other = [int(i) for kk, i in live if kk == k0 and i != i0][0]
        m[k0, other] = m[k0, i0]
        invalid(match12=m)  # a keypoint i2 named twice within one neighbour
        for bad in (-1, KF_CAP, 2, KF2_SLOTS[0]):  # out of range, never set, a neighbour's
            invalid(kf1_slot=bad)
        for bad in (-1, KF_CAP, 5, KF1_SLOT, KF2_SLOTS[1]):
            invalid(kf2_slots=[bad] + c.kf_slots[2:])
        for bad in (-1, c.p_cap, int(c.new_slot[1])):
            s = c.new_slot.copy(); s[0] = bad
            invalid(new_slot=s)
        # a bad key frame
        c.g.set_keyframes([KF2_SLOTS[1]], [KF2_IDS[1]], c.centres[2:3], bad=[1])
        invalid()
        c.g.set_keyframes([KF2_SLOTS[1]], [KF2_IDS[1]], c.centres[2:3], bad=[0])
        # a live graph row
        s0 = int(c.new_slot[0])
        c.g.set_points([s0], [0], [KF1_SLOT])
        c.g.add_observations([s0], [KF1_SLOT], [0], [0], [0])
        invalid()
        assert c.g.erase_observations([s0], [KF1_SLOT])[0] == 1  # bad again, the row empty
        # a graph too small for the slots, a key-frame row shorter than its frame
        small = amd.ObservationGraph(int(c.new_slot.max()), KF_CAP, 8)
        small.set_keyframes(c.kf_slots, c.kf_ids, c.centres)
        invalid(graph=small)
        small.close()
        short = amd.ObservationGraph(c.p_cap, KF_CAP, 8)
        short.set_keyframes(c.kf_slots, c.kf_ids, c.centres)
        short.enable_keyframe_points(128)
        for s, f in zip(c.kf_slots, [sc["kf1"]] + sc["kf2"]):
            short.set_keyframe_points(s, np.full(f["n"] - (1 if s == KF2_SLOTS[0] else 0), -1, np.int32))
        invalid(graph=short)
        short.close()
        # NULL arrays, straight at the C-ABI
        import ctypes as C
        L, p = _lib.load(), _lib.ptr
        K, n1 = c.K, c.n1
        frames = (C.c_void_p * K)(*[f._h.value for f in c.frames[1:]])
        cc = (_lib.KeyFrameCameraC * K)()
        for k, cm in enumerate(c.cams2):
            cm.fill(cc[k])
        cc1 = c.cam1.c
        ks = np.asarray(c.kf_slots[1:], np.int32)
        m12 = np.ascontiguousarray(c.match12, np.int32)
        outs = [np.zeros(n1, np.int32) for _ in range(4)]
        per, n = np.zeros(K, np.int32), C.c_int32(0)
        good = [c.mp._h, c.g._h, c.frames[0]._h, KF1_SLOT, C.byref(cc1), K, frames, p(ks), cc, p(m12), p(tr.SCALE_FACTORS),
                p(tr.LEVEL_SIGMA2), tr.N_LEVELS, float(tr.RATIO_FACTOR), p(c.new_slot), len(c.new_slot)] + [p(o) for o in outs] + \
               [None, p(per), C.byref(n)]
        for j in (0, 1, 2, 4, 6, 7, 8, 9, 10, 11, 14, 16, 17, 18, 19, 21, 22):
            a = list(good); a[j] = None
            assert L.orbfe_create_triangulated_points(*a) == _lib.ERR_INVALID, j
        same_state(before, c.state(every))
        # and the handles are as usable as before: the call (status NULL at the C-ABI) equals a fresh world's
        assert L.orbfe_create_triangulated_points(*good) == 0
        d = World(sc)
        got = d.call()
        assert n.value == got["n_created"] and np.array_equal(outs[1][:n.value], got["created_i1"])
        same_state(c.state(every), d.state(every))
        d.close()
        # no neighbour, and no pair at all: zero counts
        e = World(sc)
        r = e.call(neighbours=[], kf2_slots=[], cams=[], match12=np.zeros((0, e.n1), np.int32))
        assert r["n_created"] == 0
        r = e.call(match12=np.full_like(e.match12, -1))
        assert r["n_created"] == 0 and not r["status"].any() and not r["n_created_per_neighbour"].any()
        same_state(before, e.state(every))
        e.close()
    finally:
        c.close()


def test_two_runs_give_identical_bytes():
    sc = scene_of(**SMALL)
    a, b = World(sc), World(sc)
    try:
        same_lists(a.call(), b.call())
        every = np.arange(a.p_cap, dtype=np.int32)
        same_state(a.state(every), b.state(every))
    finally:
        a.close()
        b.close()


def test_equals_single_neighbour_calls_in_order():
    """the reference's sequential meaning: one neighbour at a time, a keypoint of key frame 1 masked out of the later
    neighbours once it has its point"""
    sc = scene_of(**SMALL)
    a, b = World(sc), World(sc)
    try:
        got = a.call()
        has = np.zeros(b.n1, bool)
        used, ks, i1s = 0, [], []
        for k in range(b.K):
            m = b.match12[k].copy()
            m[has] = -1
            r = b.call(neighbours=[b.frames[1 + k]], kf2_slots=[b.kf_slots[1 + k]], cams=[b.cams2[k]], match12=m[None],
                       new_slot=b.new_slot[used:])
            assert np.array_equal(r["created_slot"], b.new_slot[used:used + r["n_created"]])
            used += r["n_created"]
            has[r["created_i1"]] = True
            ks += [k] * r["n_created"]
            i1s += r["created_i1"].tolist()
        assert ks == got["created_k"].tolist() and i1s == got["created_i1"].tolist()
        every = np.arange(a.p_cap, dtype=np.int32)
        same_state(a.state(every), b.state(every))
    finally:
        a.close()
        b.close()


def test_chain_into_fuse_equals_the_chain_after_the_seven_trips():
    sc = scene_of(**SMALL)
    a, b = World(sc), World(sc)
    try:
        got, want = a.call(), b.seven_trips()
        same_lists(got, want)
        slots = got["created_slot"]
        poses = []
        for c in sc["cams2"]:
            R, t = c["Tcw"][:, :3].astype(f32), c["Tcw"][:, 3].astype(f32)
            poses.append(amd.camera_pose(R, t, K4, tr.MBF, BOUNDS, 1.2, tr.N_LEVELS, Ow=c["Ow"]))
        res = [w.mp.fuse(w.frames[1:], poses, slots, graph=w.g, kf_slot=w.kf_slots[1:], th=3.0, scale_factors=tr.SCALE_FACTORS,
                         inv_level_sigma2=INV_SIGMA2, return_projected=True) for w in (a, b)]
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
        assert res[0][1].any()
    finally:
        a.close()
        b.close()


def test_two_threads_on_two_tables():
    specs = (SMALL, dict(seed=1, n1=70, K=3, kind="stereo", n_pairs=90))
    single = []
    for sp in specs:
        w = World(scene_of(**sp))
        got = w.call()
        single.append((got, w.state(got["created_slot"])))
        w.close()
    worlds = [World(scene_of(**sp)) for sp in specs]
    out, errors = [None, None], []

    def work(j):
        try:
            got = worlds[j].call()
            out[j] = (got, worlds[j].state(got["created_slot"]))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    try:
        assert not errors, errors
        for (g1, s1), (g2, s2) in zip(single, out):
            same_lists(g1, g2)
            same_state(s1, s2)
    finally:
        for w in worlds:
            w.close()
