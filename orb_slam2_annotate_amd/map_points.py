"""Device-resident map points (include/orbfe.h: orbfe_mappoints): what ``Frame::isInFrustum`` (src/Frame.cc:292-353) and
``SearchByProjection(Frame&, vector<MapPoint*>&, th)`` read of a MapPoint, kept in HBM and indexed by slot, and
``Tracking::SearchLocalPoints`` on top of it.  The caller keeps the MapPoint <-> slot map."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import CameraPoseC, PoseOptStatsC, Sim3LegC, check, ptr

MP_BAD, MP_OBSERVED = 1, 2  # flags: MapPoint::isBad(), MapPoint::Observations() > 0


def camera_pose(Rcw, tcw, K4, mbf, bounds, scale_factor: float, n_levels: int, Ow=None) -> CameraPoseC:
    """orbfe_camera_pose from mRcw (3 x 3), mtcw, (fx, fy, cx, cy), mbf, (mnMinX, mnMaxX, mnMinY, mnMaxY) and the pyramid.
    Ow defaults to -Rcw^T tcw in float32 as Frame::UpdatePoseMatrices computes it (src/Frame.cc:277-283); a caller that
    holds mOw passes it.  log_scale_factor = (float)log(scaleFactor) (mfLogScaleFactor, src/Frame.cc:72)."""
    R = np.asarray(Rcw, dtype=np.float32).reshape(3, 3)
    t = np.asarray(tcw, dtype=np.float32).reshape(3)
    if Ow is None:
        Ow = -(R.T @ t)
    Ow = np.asarray(Ow, dtype=np.float32).reshape(3)
    p = CameraPoseC()
    p.Rcw[:] = [float(v) for v in R.reshape(9)]
    p.tcw[:] = [float(v) for v in t]
    p.Ow[:] = [float(v) for v in Ow]
    p.fx, p.fy, p.cx, p.cy = [float(np.float32(v)) for v in K4]
    p.mbf = float(np.float32(mbf))
    p.min_x, p.max_x, p.min_y, p.max_y = [float(np.float32(v)) for v in bounds]
    p.log_scale_factor = float(np.float32(np.log(np.float32(scale_factor))))
    p.n_levels = int(n_levels)
    return p


def sim3_leg(Rw, tw, sR, t, K4, bounds, scale_factor: float, n_levels: int) -> Sim3LegC:
    """orbfe_sim3_leg: the SOURCE key frame's GetRotation (3 x 3) / GetTranslation, the 12 floats sR / t that take its camera
    frame to the target's (sR21, t21 or sR12, t12 -- composed by the caller, see loop_closing.sim3_legs), and the TARGET's
    (fx, fy, cx, cy), (mnMinX, mnMaxX, mnMinY, mnMaxY) and pyramid.  Every value is rounded to float32 once, here."""
    leg = Sim3LegC()
    leg.Rw[:] = [float(v) for v in np.asarray(Rw, dtype=np.float32).reshape(9)]
    leg.tw[:] = [float(v) for v in np.asarray(tw, dtype=np.float32).reshape(3)]
    leg.sR[:] = [float(v) for v in np.asarray(sR, dtype=np.float32).reshape(9)]
    leg.t[:] = [float(v) for v in np.asarray(t, dtype=np.float32).reshape(3)]
    leg.fx, leg.fy, leg.cx, leg.cy = [float(np.float32(v)) for v in K4]
    leg.min_x, leg.max_x, leg.min_y, leg.max_y = [float(np.float32(v)) for v in bounds]
    leg.log_scale_factor = float(np.float32(np.log(np.float32(scale_factor))))
    leg.n_levels = int(n_levels)
    return leg


class MapPoints:
    """A table of `capacity` map-point slots on the device.  After close() every method raises, as ResidentFrame does."""

    def __init__(self, capacity: int, device: int = 0):
        self._L = _lib.load()
        self._handle = C.c_void_p()
        check(self._L.orbfe_mappoints_create(int(device), int(capacity), C.byref(self._handle)))
        self.capacity, self.device = int(capacity), int(device)

    @property
    def _h(self):
        if self._handle is None:
            raise ValueError("MapPoints is closed")
        return self._handle

    @property
    def closed(self):
        return self._handle is None

    def close(self):
        if getattr(self, "_handle", None):
            self._L.orbfe_mappoints_destroy(self._handle)
        self._handle = None

    __del__ = close

    def update(self, slot, pos, normal, min_dist, max_dist, desc, flags):
        """orbfe_mappoints_update: GetWorldPos / GetNormal ([n, 3]), the raw mfMinDistance / mfMaxDistance, GetDescriptor
        ([n, 32] uint8, or None to keep what the slots hold) and flags (MP_BAD | MP_OBSERVED) into slot[n]."""
        h = self._h
        s = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        n = len(s)
        p = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        nv = np.ascontiguousarray(normal, dtype=np.float32).reshape(-1, 3)
        lo = np.ascontiguousarray(min_dist, dtype=np.float32).reshape(-1)
        hi = np.ascontiguousarray(max_dist, dtype=np.float32).reshape(-1)
        fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
        d = None if desc is None else np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        if not (len(p) == len(nv) == len(lo) == len(hi) == len(fl) == n and (d is None or len(d) == n)):
            raise ValueError("MapPoints.update: the arrays must hold one entry per slot")
        check(self._L.orbfe_mappoints_update(h, n, ptr(s), ptr(p), ptr(nv), ptr(lo), ptr(hi), ptr(d), ptr(fl)))

    @staticmethod
    def _slots(slot, skip):
        s = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        k = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8).reshape(-1)
        if k is not None and len(k) != len(s):
            raise ValueError("skip must hold one entry per slot")
        return s, k

    def ProjectInFrustum(self, slot, pose: CameraPoseC, viewing_cos_limit: float = 0.5, skip=None):
        """Frame::isInFrustum(pMP, viewingCosLimit) for the points in slot[] -> dict of in_view (uint8), level (int32),
        view_cos, proj_x, proj_y, proj_xr, inv_z, dist (float32); the fields are 0 where in_view is."""
        h = self._h
        s, k = self._slots(slot, skip)
        n = len(s)
        out = {"in_view": np.zeros(n, np.uint8), "level": np.zeros(n, np.int32)}
        for name in ("view_cos", "proj_x", "proj_y", "proj_xr", "inv_z", "dist"):
            out[name] = np.zeros(n, np.float32)
        check(self._L.orbfe_project_in_frustum(h, n, ptr(s), ptr(k), C.byref(pose), float(viewing_cos_limit),
                                               *[ptr(out[f]) for f in ("in_view", "level", "view_cos", "proj_x", "proj_y",
                                                                       "proj_xr", "inv_z", "dist")]))
        return out

    def SearchLocalPoints(self, F, slot, pose: CameraPoseC, scale_factors, th: float = 1.0, nnratio: float = 0.8,
                          viewing_cos_limit: float = 0.5, skip=None, blocked=None):
        """Tracking::SearchLocalPoints: isInFrustum for slot[] and SearchByProjection(F, points, th) in one call ->
        (nmatches, match[F.N], in_view[n]); match[idx] = position in slot[] of the point given to feature idx, or -1."""
        h = self._h
        s, k = self._slots(slot, skip)
        n = len(s)
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
        blk = None if blocked is None else np.ascontiguousarray(blocked, dtype=np.uint8)
        match = np.full(max(F.N, 1), -1, dtype=np.int32)
        in_view = np.zeros(max(n, 1), np.uint8)
        nm = C.c_int32(0)
        check(self._L.orbfe_search_local_points(h, n, ptr(s), ptr(k), C.byref(pose), float(viewing_cos_limit), C.byref(F.c),
                                                ptr(sf), len(sf), ptr(blk), float(th), float(nnratio), ptr(match),
                                                C.byref(nm), ptr(in_view)))
        return nm.value, match[:F.N], in_view[:n]

    def _fuse_operands(self, poses, slot, graph, kf_slot, skip):
        """(K, n, slots, pose array, graph handle, kf slots, mask) of project_fuse / fuse."""
        s = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        poses = list(poses)
        K, n = len(poses), len(s)
        pa = (CameraPoseC * max(K, 1))(*poses)
        kf = None
        if graph is not None:
            if kf_slot is None:
                raise ValueError("a graph needs the kf slots of the key frames")
            kf = np.ascontiguousarray(kf_slot, dtype=np.int32).reshape(-1)
            if len(kf) != K:
                raise ValueError("kf_slot must hold one entry per pose")
        k = None
        if skip is not None:
            k = np.ascontiguousarray(skip, dtype=np.uint8).reshape(-1)
            if len(k) != K * n:
                raise ValueError("skip must hold K * n entries")
        return K, n, s, pa, (graph._h if graph is not None else None), kf, k

    def project_fuse(self, poses, slot, graph=None, kf_slot=None, skip=None):
        """The prologue of ORBmatcher::Fuse (src/ORBmatcher.cc:960-1006) for slot[] against the K key-frame poses
        (orbfe_project_fuse) -> dict of valid (uint8), u, v, ur, dist (float32), level (int32), each [K, n]; the fields are
        0 where valid is.  With `graph` a point that observes kf_slot[k] is rejected for pose k (IsInKeyFrame)."""
        h = self._h
        K, n, s, pa, gh, kf, k = self._fuse_operands(poses, slot, graph, kf_slot, skip)
        q = max(K * n, 1)
        flat = {"valid": np.zeros(q, np.uint8), "level": np.zeros(q, np.int32)}
        for name in ("u", "v", "ur", "dist"):
            flat[name] = np.zeros(q, np.float32)
        check(self._L.orbfe_project_fuse(h, gh, n, ptr(s), K, ptr(kf), pa, ptr(k),
                                         *[ptr(flat[f]) for f in ("valid", "u", "v", "ur", "level", "dist")]))
        return {name: a[:K * n].reshape(K, n) for name, a in flat.items()}

    def fuse(self, frames, poses, slot, graph=None, kf_slot=None, skip=None, th: float = 3.0, chi2_gate: bool = True,
             scale_factors=None, inv_level_sigma2=None, return_projected: bool = False):
        """ORBmatcher::Fuse for slot[] against K key frames (views or resident frames) in one call (orbfe_fuse_mappoints):
        the projection, the windows and the search all on the device -> best_idx [K, n] (keypoint of key frame k for point
        i, or -1); scale_factors = mvScaleFactors; with return_projected also the [K, n] mask of the points that passed the prologue.  chi2_gate=True is
        Fuse(pKF, vpMapPoints, th) and needs inv_level_sigma2 = mvInvLevelSigma2; False is the Sim3 overload with the
        caller's decomposition of Scw in the poses.  Replace / AddObservation / AddMapPoint stay with the caller, and the
        results are those of the state at entry (include/orbfe.h)."""
        h = self._h
        frames = list(frames)
        K, n, s, pa, gh, kf, k = self._fuse_operands(poses, slot, graph, kf_slot, skip)
        if len(frames) != K:
            raise ValueError("MapPoints.fuse: one pose per key frame")
        if scale_factors is None:
            raise ValueError("MapPoints.fuse: scale_factors (mvScaleFactors) is needed")
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
        isg = None
        if chi2_gate:
            if inv_level_sigma2 is None:
                raise ValueError("MapPoints.fuse: the chi-square gate needs inv_level_sigma2")
            isg = np.ascontiguousarray(inv_level_sigma2, dtype=np.float32).reshape(-1)
            if len(isg) != len(sf):
                raise ValueError("MapPoints.fuse: inv_level_sigma2 must hold one entry per level")
        views = (C.POINTER(_lib.FrameViewC) * max(K, 1))(*[C.pointer(f.c) for f in frames])
        best = np.full(max(K * n, 1), -1, dtype=np.int32)
        proj = np.zeros(max(K * n, 1), np.uint8) if return_projected else None
        check(self._L.orbfe_fuse_mappoints(h, gh, n, ptr(s), K, views, ptr(kf), pa, ptr(k), ptr(sf), ptr(isg), len(sf), float(th),
                                           int(bool(chi2_gate)), ptr(best), ptr(proj)))
        best = best[:K * n].reshape(K, n)
        return (best, proj[:K * n].reshape(K, n)) if return_projected else best

    @staticmethod
    def _last_frame_operands(slot, last_octave, skip):
        s = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        o = np.ascontiguousarray(last_octave, dtype=np.int32).reshape(-1)
        k = None if skip is None else np.ascontiguousarray(skip, dtype=np.uint8).reshape(-1)
        if len(o) != len(s) or (k is not None and len(k) != len(s)):
            raise ValueError("last_octave (and skip) must hold one entry per slot")
        return s, o, k

    def project_last_frame(self, slot, last_octave, pose: CameraPoseC, scale_factors, th: float, mode: int = 0, skip=None):
        """The prologue of SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1516-1550) for the compact
        list slot[] / last_octave[] (orbfe_project_last_frame) -> dict of valid (uint8), u, v, inv_z, ur, radius (float32);
        the fields are 0 where valid is."""
        h = self._h
        s, o, k = self._last_frame_operands(slot, last_octave, skip)
        n = len(s)
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
        out = {"valid": np.zeros(max(n, 1), np.uint8)}
        for name in ("u", "v", "inv_z", "ur", "radius"):
            out[name] = np.zeros(max(n, 1), np.float32)
        check(self._L.orbfe_project_last_frame(h, n, ptr(s), ptr(k), ptr(o), C.byref(pose), ptr(sf), len(sf), float(th), int(mode),
                                               *[ptr(out[f]) for f in ("valid", "u", "v", "inv_z", "ur", "radius")]))
        return {name: a[:n] for name, a in out.items()}

    def SearchByProjectionLastFrame(self, Cur, slot, last_octave, last_angle, pose: CameraPoseC, scale_factors, th: float,
                                    mode: int = 0, skip=None, blocked=None, check_orientation: bool = True,
                                    return_valid: bool = False):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono) in one call (orbfe_search_last_frame_mappoints): slot[] names
        the last frame's features that hold a non-outlier map point, in ascending feature order; last_octave / last_angle are
        their mvKeysUn -> (nmatches, match_cur[Cur.N]) with match_cur[i2] = position in slot[] or -1 (what pose_optimization
        takes), and with return_valid the points that were searched."""
        h = self._h
        s, o, k = self._last_frame_operands(slot, last_octave, skip)
        n = len(s)
        la = None
        if check_orientation:
            la = np.ascontiguousarray(last_angle, dtype=np.float32).reshape(-1)
            if len(la) != n:
                raise ValueError("last_angle must hold one entry per slot")
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
        blk = None if blocked is None else np.ascontiguousarray(blocked, dtype=np.uint8).reshape(-1)
        if blk is not None and len(blk) != Cur.N:
            raise ValueError("blocked must hold one entry per feature of the frame")
        match = np.full(max(Cur.N, 1), -1, dtype=np.int32)
        valid = np.zeros(max(n, 1), np.uint8) if return_valid else None
        nm = C.c_int32(0)
        check(self._L.orbfe_search_last_frame_mappoints(h, n, ptr(s), ptr(k), ptr(o), ptr(la), C.byref(pose), C.byref(Cur.c), ptr(sf),
                                                        len(sf), ptr(blk), int(mode), float(th), int(bool(check_orientation)),
                                                        ptr(match), C.byref(nm), ptr(valid)))
        return (nm.value, match[:Cur.N], valid[:n]) if return_valid else (nm.value, match[:Cur.N])

    @staticmethod
    def _keyframe_operands(poses, slots, skips):
        """(K, offsets [K + 1], concatenated slots, pose array, concatenated mask) of project_keyframes / SearchByProjectionKeyFrames"""
        poses = list(poses)
        lists = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in slots]
        K = len(poses)
        if len(lists) != K:
            raise ValueError("one slot list per pose")
        off = np.zeros(K + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in lists])
        s = np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32)
        k = None
        if skips is not None:
            masks = [np.ascontiguousarray(m, dtype=np.uint8).reshape(-1) for m in skips]
            if [len(m) for m in masks] != [len(x) for x in lists]:
                raise ValueError("one skip entry per slot")
            k = np.concatenate(masks + [np.zeros(0, np.uint8)]).astype(np.uint8)
        return K, off, s, (CameraPoseC * max(K, 1))(*poses), k

    def project_keyframes(self, poses, slots, skips=None):
        """The prologue of SearchByProjection(CurrentFrame, pKF_k, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1665-1699) for K
        candidates in one launch (orbfe_project_keyframe): slots[k] names pKF_k's non-null map points in feature order,
        skips[k] = sAlreadyFound -> list of K dicts of valid (uint8), u, v, inv_z, dist (float32), level (int32)."""
        h = self._h
        K, off, s, pa, k = self._keyframe_operands(poses, slots, skips)
        q = max(len(s), 1)
        flat = {"valid": np.zeros(q, np.uint8), "level": np.zeros(q, np.int32)}
        for name in ("u", "v", "inv_z", "dist"):
            flat[name] = np.zeros(q, np.float32)
        check(self._L.orbfe_project_keyframe(h, K, ptr(off), ptr(s), ptr(k), pa,
                                             *[ptr(flat[f]) for f in ("valid", "u", "v", "inv_z", "level", "dist")]))
        return [{name: a[off[j]:off[j + 1]] for name, a in flat.items()} for j in range(K)]

    def SearchByProjectionKeyFrames(self, Cur, poses, slots, kf_angles, scale_factors, th, ORBdist, skips=None, blocked=None,
                                    check_orientation: bool = True):
        """Tracking::Relocalization's SearchByProjection for K candidates in one call (orbfe_search_keyframe_mappoints_multi):
        th[k] / ORBdist[k] per candidate (scalars apply to all), kf_angles[k] = pKF_k->mvKeysUn[.].angle of slots[k], blocked[k]
        (or None) = Cur.mvpMapPoints[i2] != NULL -> (n_matches[K], match_cur[K, Cur.N]) with match_cur[k, i2] = position in
        slots[k] or -1."""
        h = self._h
        K, off, s, pa, k = self._keyframe_operands(poses, slots, skips)
        ka = None
        if check_orientation:
            ka = np.concatenate([np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in kf_angles] +
                                [np.zeros(0, np.float32)]).astype(np.float32)
            if len(ka) != len(s):
                raise ValueError("kf_angles must hold one entry per slot")
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
        tha = np.ascontiguousarray(np.broadcast_to(np.asarray(th, np.float32), (K,)) if K else np.zeros(1, np.float32))
        od = np.ascontiguousarray(np.broadcast_to(np.asarray(ORBdist, np.int32), (K,)) if K else np.zeros(1, np.int32))
        keep, bp = [], None
        if blocked is not None:
            addr = []
            for b in blocked:
                if b is None:
                    addr.append(None)
                    continue
                b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1)
                if len(b) != Cur.N:
                    raise ValueError("blocked[k] must hold one entry per feature of the frame")
                keep.append(b)
                addr.append(b.ctypes.data)
            if len(addr) != K:
                raise ValueError("one blocked entry (or None) per candidate")
            bp = (C.c_void_p * max(K, 1))(*addr)
        match = np.full((max(K, 1), max(Cur.N, 1)), -1, dtype=np.int32)
        cnt = np.zeros(max(K, 1), dtype=np.int32)
        check(self._L.orbfe_search_keyframe_mappoints_multi(h, C.byref(Cur.c), ptr(sf), len(sf), K, ptr(off), ptr(s), ptr(k), ptr(ka), pa,
                                                            bp, ptr(tha), ptr(od), int(bool(check_orientation)), ptr(match), ptr(cnt)))
        return cnt[:K], match[:K, :Cur.N]

    def project_sim3(self, legs, slots, skips=None):
        """The prologue of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1298-1340, :1379-1420) for many legs in one launch
        (orbfe_project_sim3): slots[l] = the source key frame's GetMapPointMatches() in slot space (-1 = none), skips[l] =
        vbAlreadyMatched -> list of dicts of valid (uint8), u, v, dist (float32), level (int32), one per leg."""
        h = self._h
        legs = list(legs)
        lists = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in slots]
        n = len(legs)
        if len(lists) != n:
            raise ValueError("one slot list per leg")
        off = np.zeros(n + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in lists])
        s = np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32)
        k = None
        if skips is not None:
            masks = [np.zeros(len(x), np.uint8) if m is None else np.ascontiguousarray(m, dtype=np.uint8).reshape(-1)
                     for m, x in zip(skips, lists)]
            if [len(m) for m in masks] != [len(x) for x in lists]:
                raise ValueError("one skip entry per slot")
            k = np.concatenate(masks + [np.zeros(0, np.uint8)]).astype(np.uint8)
        la = (Sim3LegC * max(n, 1))(*legs)
        q = max(len(s), 1)
        flat = {"valid": np.zeros(q, np.uint8), "level": np.zeros(q, np.int32)}
        for name in ("u", "v", "dist"):
            flat[name] = np.zeros(q, np.float32)
        check(self._L.orbfe_project_sim3(h, n, ptr(off), ptr(s), ptr(k), la,
                                         *[ptr(flat[f]) for f in ("valid", "u", "v", "level", "dist")]))
        return [{name: a[off[j]:off[j + 1]] for name, a in flat.items()} for j in range(n)]

    def SearchBySim3(self, KF1, slot1, KF2s, slot2s, legs12, legs21, scale_factors1, scale_factors2, th: float,
                     matched12=None, graph=None, kf2_slot=None, already2=None):
        """ORBmatcher::SearchBySim3 for K candidates of KF1 in one call (orbfe_search_by_sim3_mappoints_multi).  slot1 /
        slot2s[k] = GetMapPointMatches() of KF1 / KF2_k in slot space (-1 = none); legs12[k] / legs21[k] from
        loop_closing.sim3_legs; matched12 [K, N1] = the slots of vpMatches12_k at entry (-1 = NULL).  vbAlreadyMatched2 comes
        from already2[k] (masks over KF2_k's keypoints) and / or, with graph and kf2_slot, from the observation rows on the
        device -> (n_found[K], match12[K, N1]) with match12[k, i1] = i2 or -1."""
        h = self._h
        KF2s, legs12, legs21 = list(KF2s), list(legs12), list(legs21)
        K = len(KF2s)
        s1 = np.ascontiguousarray(slot1, dtype=np.int32).reshape(-1)
        lists = [np.ascontiguousarray(s, dtype=np.int32).reshape(-1) for s in slot2s]
        if not (len(lists) == len(legs12) == len(legs21) == K):
            raise ValueError("MapPoints.SearchBySim3: one slot list and two legs per candidate")
        if len(s1) != KF1.N:
            raise ValueError("MapPoints.SearchBySim3: slot1 must hold one entry per keypoint of KF1")
        N1 = len(s1)
        off = np.zeros(K + 1, np.int32)
        off[1:] = np.cumsum([len(s) for s in lists])
        s2 = np.concatenate(lists + [np.zeros(0, np.int32)]).astype(np.int32)
        m_in = None
        if matched12 is not None:
            m_in = np.ascontiguousarray(matched12, dtype=np.int32).reshape(-1)
            if len(m_in) != K * N1:
                raise ValueError("MapPoints.SearchBySim3: matched12 must be [K, N1]")
        a2 = None
        if already2 is not None:
            masks = [np.zeros(len(x), np.uint8) if m is None else np.ascontiguousarray(m, dtype=np.uint8).reshape(-1)
                     for m, x in zip(already2, lists)]
            if [len(m) for m in masks] != [len(x) for x in lists]:
                raise ValueError("MapPoints.SearchBySim3: already2[k] must hold one entry per keypoint of KF2_k")
            a2 = np.concatenate(masks + [np.zeros(0, np.uint8)]).astype(np.uint8)
        kf = None
        if graph is not None:
            if kf2_slot is None:
                raise ValueError("a graph needs the kf slots of the candidates")
            kf = np.ascontiguousarray(kf2_slot, dtype=np.int32).reshape(-1)
            if len(kf) != K:
                raise ValueError("kf2_slot must hold one entry per candidate")
        sf1 = np.ascontiguousarray(scale_factors1, dtype=np.float32).reshape(-1)
        sf2 = np.ascontiguousarray(scale_factors2, dtype=np.float32).reshape(-1)
        if len(sf1) != len(sf2):
            raise ValueError("MapPoints.SearchBySim3: the two level tables must hold the same number of levels")
        views = (C.POINTER(_lib.FrameViewC) * max(K, 1))(*[C.pointer(f.c) for f in KF2s])
        l12 = (Sim3LegC * max(K, 1))(*legs12)
        l21 = (Sim3LegC * max(K, 1))(*legs21)
        match = np.full(max(K * N1, 1), -1, dtype=np.int32)
        cnt = np.zeros(max(K, 1), dtype=np.int32)
        check(self._L.orbfe_search_by_sim3_mappoints_multi(h, graph._h if graph is not None else None, C.byref(KF1.c), ptr(s1), K,
                                                           views, ptr(off), ptr(s2), l12, l21, ptr(m_in), ptr(kf), ptr(a2),
                                                           ptr(sf1), ptr(sf2), len(sf1), float(th), ptr(match), ptr(cnt)))
        return cnt[:K], match[:K * N1].reshape(K, N1)

    def SearchByProjectionSim3(self, KF, slot, pose: CameraPoseC, scale_factors, th: float, matched=None, skip=None,
                               return_projected: bool = False):
        """SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:335-451) in one call
        (orbfe_search_by_projection_sim3_mappoints): slot[] = vpPoints in slot space, pose = the decomposition of Scw (as for
        fuse), matched[idx] = vpMatched[idx] != NULL, skip[i] = the point is in spAlreadyFound -> (nmatches, match[KF.N]) with
        match[idx] = position in slot[] or -1, and with return_projected the points that passed the prologue."""
        h = self._h
        s, k = self._slots(slot, skip)
        n = len(s)
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
        blk = None if matched is None else np.ascontiguousarray(matched, dtype=np.uint8).reshape(-1)
        if blk is not None and len(blk) != KF.N:
            raise ValueError("matched must hold one entry per keypoint of the key frame")
        match = np.full(max(KF.N, 1), -1, dtype=np.int32)
        proj = np.zeros(max(n, 1), np.uint8) if return_projected else None
        nm = C.c_int32(0)
        check(self._L.orbfe_search_by_projection_sim3_mappoints(h, n, ptr(s), ptr(k), C.byref(pose), C.byref(KF.c), ptr(sf), len(sf),
                                                                ptr(blk), float(th), ptr(match), C.byref(nm), ptr(proj)))
        return (nm.value, match[:KF.N], proj[:n]) if return_projected else (nm.value, match[:KF.N])

    def pose_optimization(self, frame, slot, match, pose, K5, inv_level_sigma2, outlier=None):
        """Optimizer::PoseOptimization on the table (orbfe_pose_optimization_mappoints): `match` is what SearchLocalPoints
        returned for `frame` and `slot`, `pose` the 4 x 4 mTcw, inv_level_sigma2 = mvInvLevelSigma2 -> (n_inliers, Tcw_out
        [4, 4], outlier [frame.N], stats dict, edge_chi2 [frame.N]).  Features without an edge (no match, or a bad slot)
        keep the flag `outlier` gave them and a chi2 of 0."""
        from .optimizer import _flags, stats_dict
        h = self._h
        s = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        m = np.ascontiguousarray(match, dtype=np.int32).reshape(-1)
        if len(m) != frame.N:
            raise ValueError("MapPoints.pose_optimization: match must hold one entry per feature of the frame")
        lv = np.ascontiguousarray(inv_level_sigma2, dtype=np.float32).reshape(-1)
        k = np.ascontiguousarray(K5, dtype=np.float32).reshape(5)
        T = np.ascontiguousarray(pose, dtype=np.float32).reshape(16)
        out = np.zeros(16, np.float32)
        flags = _flags(outlier, frame.N, "MapPoints.pose_optimization")
        chi2 = np.zeros(max(frame.N, 1), np.float64)
        ni, st = C.c_int32(0), PoseOptStatsC()
        check(self._L.orbfe_pose_optimization_mappoints(h, len(s), ptr(s), C.byref(frame.c), ptr(m), ptr(lv), len(lv), ptr(k), ptr(T),
                                                        ptr(out), ptr(flags), C.byref(ni), C.byref(st), ptr(chi2)))
        return ni.value, out.reshape(4, 4), flags[:frame.N], stats_dict(st), chi2[:frame.N]

    def local_bundle_adjustment(self, slot, n_local, Tcw, cam, edge_pose, edge_point, u, v, u_right, inv_sigma2,
                                local_is_fixed=None, stop_flag=None):
        """Optimizer::LocalBundleAdjustment with the local points in the table (orbfe_local_bundle_adjustment_mappoints):
        point p of the edges is slot[p]; positions are read from and written back to the table on the device -> what
        optimizer.local_bundle_adjustment returns, bit for bit.  Normal and distance range remain the caller's
        UpdateNormalAndDepth, written through update()."""
        from .optimizer import LbaOperands, _stop_ptr
        s = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        o = LbaOperands(n_local, Tcw, cam, None, edge_pose, edge_point, u, v, u_right, inv_sigma2, local_is_fixed, n_points=len(s))
        check(self._L.orbfe_local_bundle_adjustment_mappoints(self._h, len(s), ptr(s), o.n_local, o.n_fixed, ptr(o.T), o.fixed_ptr(),
                                                              ptr(o.cam), *o.edges(), _stop_ptr(stop_flag), ptr(o.Tout), ptr(o.xout),
                                                              ptr(o.erase), ptr(o.level1), C.cast(C.byref(o.st), C.c_void_p),
                                                              ptr(o.chi2)))
        return o.result()

    def essential_graph_correct(self, slot, sim3, sim3_out, ref_vertex):
        """The tail of Optimizer::OptimizeEssentialGraph on the table (orbfe_essential_graph_correct_mappoints): the position
        of slot[p] becomes Sout[r]^-1 .map(S[r] .map(P)), r = ref_vertex[p] (-1: left as it is), in place and bit-equal to
        optimizer.essential_graph_correct_points.  Normal and distance range remain the caller's UpdateNormalAndDepth."""
        from .optimizer import _correction
        s, so, r = _correction(sim3, sim3_out, ref_vertex)
        sl = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        if len(r) != len(sl):
            raise ValueError("MapPoints.essential_graph_correct: ref_vertex must hold one entry per slot")
        check(self._L.orbfe_essential_graph_correct_mappoints(self._h, len(s), ptr(s), ptr(so), len(sl), ptr(sl), ptr(r)))

    def correct_loop(self, graph, kf_slots, corrected, noncorrected, Ow_corrected, scale_factors, skip=(), capacity=None):
        """The point loop at the head of LoopClosing::CorrectLoop (src/LoopClosing.cc:558-600) with UpdateNormalAndDepth, on
        the table (orbfe_correct_loop_mappoints): `graph` holds the key-frame rows, the observation rows and Ow; kf_slots the
        key frames in visiting order (ascending mnId recommended), corrected / noncorrected [K, 8] from
        loop_closing.correct_loop_sim3s, Ow_corrected [K, 3] the centres after SetPose, skip the slots with
        mnCorrectedByKF == current -> (slots, ref, valid): the claimed slots in claim order, the claimant's list position
        and whether normal and range were rewritten.  The graph's Ow of the K key frames are Ow_corrected afterwards."""
        kf = np.ascontiguousarray(kf_slots, dtype=np.int32).reshape(-1)
        K = len(kf)
        cor = np.ascontiguousarray(corrected, dtype=np.float64).reshape(-1, 8)
        non = np.ascontiguousarray(noncorrected, dtype=np.float64).reshape(-1, 8)
        ow = np.ascontiguousarray(Ow_corrected, dtype=np.float32).reshape(-1, 3)
        if not (len(cor) == len(non) == len(ow) == K):
            raise ValueError("MapPoints.correct_loop: corrected, noncorrected and Ow_corrected must hold one entry per key frame")
        sk = np.ascontiguousarray(skip, dtype=np.int32).reshape(-1)
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
        cap = graph.point_capacity if capacity is None else int(capacity)
        slots, ref, valid = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.uint8)
        n = C.c_int32(0)
        check(self._L.orbfe_correct_loop_mappoints(graph._h, self._h, K, ptr(kf), ptr(cor), ptr(non), ptr(ow), len(sk), ptr(sk), ptr(sf),
                                                   len(sf), cap, ptr(slots), ptr(ref), ptr(valid), C.byref(n)))
        return slots[:n.value].copy(), ref[:n.value].copy(), valid[:n.value].copy()

    def gba_update(self, graph, slot, in_gba, pos_gba, kf_slots, reached, Tcw_bef, Twc_new):
        """The map-point loop at the tail of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:818-852) on the table
        (orbfe_gba_update_mappoints): slot = GetAllMapPoints (distinct), in_gba / pos_gba aligned with it; kf_slots a compact
        list with reached, Tcw_bef = mTcwBefGBA and Twc_new = GetPoseInverse() after SetPose.  The bad flag and the reference
        key frame come from `graph` -> moved [n]: 0 skipped, 1 took pos_gba, 2 moved through its reference key frame."""
        sl = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        g = np.ascontiguousarray(in_gba, dtype=np.uint8).reshape(-1)
        pg = np.ascontiguousarray(pos_gba, dtype=np.float32).reshape(-1, 3)
        if not (len(g) == len(pg) == len(sl)):
            raise ValueError("MapPoints.gba_update: in_gba and pos_gba must hold one entry per slot")
        kf = np.ascontiguousarray(kf_slots, dtype=np.int32).reshape(-1)
        rc = np.ascontiguousarray(reached, dtype=np.uint8).reshape(-1)
        tb = np.ascontiguousarray(Tcw_bef, dtype=np.float32).reshape(-1, 16)
        tn = np.ascontiguousarray(Twc_new, dtype=np.float32).reshape(-1, 16)
        if not (len(rc) == len(tb) == len(tn) == len(kf)):
            raise ValueError("MapPoints.gba_update: reached, Tcw_bef and Twc_new must hold one entry per kf slot")
        moved = np.zeros(max(len(sl), 1), np.uint8)
        check(self._L.orbfe_gba_update_mappoints(graph._h, self._h, len(sl), ptr(sl), ptr(g), ptr(pg), len(kf), ptr(kf), ptr(rc), ptr(tb),
                                                 ptr(tn), ptr(moved)))
        return moved[:len(sl)]

    def positions(self, slot):
        """orbfe_mappoints_positions: the world positions the table holds for slot[] -> [n, 3] float32."""
        sl = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        out = np.zeros((max(len(sl), 1), 3), np.float32)
        check(self._L.orbfe_mappoints_positions(self._h, len(sl), ptr(sl), ptr(out)))
        return out[:len(sl)]

    def descriptors(self, slot):
        """orbfe_mappoints_descriptors: GetDescriptor as the table holds it for slot[] -> [n, 32] uint8."""
        sl = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        out = np.zeros((max(len(sl), 1), 32), np.uint8)
        check(self._L.orbfe_mappoints_descriptors(self._h, len(sl), ptr(sl), ptr(out)))
        return out[:len(sl)]

    def create_stereo_points(self, graph, frame, kf_slot, pose: CameraPoseC, depth, th_depth: float, mode: int, scale_factors,
                             new_slot, occupied=None, stale=None):
        """orbfe_create_stereo_points: the stereo / RGB-D points of Tracking::StereoInitialization (mode tracking.STEREO_ALL),
        CreateNewKeyFrame (STEREO_KEYFRAME) or UpdateLastFrame (STEREO_TEMPORAL; graph may be None) born on the device.
        `frame` is the ResidentFrame (keypoints, octaves, descriptors, stereo bit), depth its mvDepth, new_slot the free
        slots the created points take in creation order (its length is the capacity), occupied / stale the masks of
        tracking.stereo_points_select -> dict of created_idx, created_slot [m], cleared [n], n_created, n_walked.  In modes
        ALL and KEYFRAME the graph's mirror receives the points, their observation by kf_slot and -- with key-frame rows
        enabled -- kf_slot's mvpMapPoints entries.  More created points than len(new_slot) raises OrbfeError(ERR_CAPACITY)
        with neither table touched."""
        z = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1)
        n = len(z)
        occ = None if occupied is None else np.ascontiguousarray(occupied, dtype=np.uint8).reshape(-1)
        st = None if stale is None else np.ascontiguousarray(stale, dtype=np.uint8).reshape(-1)
        if (occ is not None and len(occ) != n) or (st is not None and len(st) != n):
            raise ValueError("create_stereo_points: the masks must hold one entry per keypoint")
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
        ns = np.ascontiguousarray(new_slot, dtype=np.int32).reshape(-1)
        cap = len(ns)
        idx, slot = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.int32)
        cleared = np.zeros(max(n, 1), np.uint8)
        nc, nw = C.c_int32(0), C.c_int32(0)
        rc = self._L.orbfe_create_stereo_points(self._h, graph._h if graph is not None else None, frame._h, int(kf_slot), C.byref(pose), n,
                                                ptr(z), ptr(occ), ptr(st), float(th_depth), int(mode), ptr(sf), len(sf), ptr(ns), cap,
                                                ptr(idx), ptr(slot), ptr(cleared), C.byref(nc), C.byref(nw))
        if rc == _lib.ERR_CAPACITY:  # the needed count travels with the error
            err = _lib.OrbfeError(rc, self._L.orbfe_last_error().decode("utf-8", "replace"))
            err.n_created = nc.value
            raise err
        check(rc)
        k = nc.value
        return dict(created_idx=idx[:k].copy(), created_slot=slot[:k].copy(), cleared=cleared[:n].copy(), n_created=k, n_walked=nw.value)

    def create_triangulated_points(self, graph, kf1, kf1_slot, cam1, neighbours, kf2_slots, cams, match12, scale_factors, level_sigma2,
                                   ratio_factor: float, new_slot):
        """orbfe_create_triangulated_points: LocalMapping::CreateNewMapPoints' pair loop and the birth at its tail
        (src/LocalMapping.cc:331-501) on the resident state, in one call.  kf1 / neighbours are ResidentFrames, kf1_slot /
        kf2_slots their kf slots in `graph`, cam1 / cams local_mapping.KeyFrameCamera, match12 [K, n1] as
        SearchForTriangulationMulti returns it, new_slot the free slots the created points take in creation order (its
        length is the capacity) -> dict of created_k, created_i1, created_i2, created_slot [m], status [K, n1],
        n_created_per_neighbour [K], n_created.  The graph's mirror receives the points, their two observations and -- with
        key-frame rows enabled -- both key frames' mvpMapPoints entries.  More created points than len(new_slot) raises
        OrbfeError(ERR_CAPACITY) with n_created set and neither table touched."""
        from ._lib import KeyFrameCameraC
        K, n1 = len(neighbours), kf1.N
        if len(cams) != K or len(kf2_slots) != K:
            raise ValueError("create_triangulated_points: one camera and one kf slot per neighbour")
        m = np.ascontiguousarray(np.asarray(match12, dtype=np.int32).reshape(K, n1) if K else np.zeros((0, n1), np.int32))
        for cm, n in [(cam1, n1)] + [(cm, nb.N) for cm, nb in zip(cams, neighbours)]:
            for name in ("depth", "x_raw", "y_raw"):
                a = getattr(cm, name)
                if a is not None and len(a) != n:
                    raise ValueError(f"create_triangulated_points: {name} must hold {n} entries, not {len(a)}")
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
        sg = np.ascontiguousarray(level_sigma2, dtype=np.float32).reshape(-1)
        if len(sf) != len(sg):
            raise ValueError("create_triangulated_points: scale_factors and level_sigma2 must hold one entry per level")
        ns = np.ascontiguousarray(new_slot, dtype=np.int32).reshape(-1)
        ks = np.ascontiguousarray(kf2_slots, dtype=np.int32).reshape(-1)
        cap = len(ns)
        frames = (C.c_void_p * max(K, 1))(*[nb._h.value for nb in neighbours])
        cc = (KeyFrameCameraC * max(K, 1))()
        for k, cm in enumerate(cams):
            cm.fill(cc[k])
        c1 = cam1.c
        room = max(cap, 1)
        ck, ci1, ci2, slot = (np.zeros(room, np.int32) for _ in range(4))
        status = np.zeros((max(K, 1), max(n1, 1)), np.uint8)
        per = np.zeros(max(K, 1), np.int32)
        nc = C.c_int32(0)
        rc = self._L.orbfe_create_triangulated_points(self._h, graph._h, kf1._h, int(kf1_slot), C.byref(c1), K, frames, ptr(ks), cc, ptr(m),
                                                      ptr(sf), ptr(sg), len(sf), float(ratio_factor), ptr(ns), cap, ptr(ck), ptr(ci1),
                                                      ptr(ci2), ptr(slot), ptr(status), ptr(per), C.byref(nc))
        if rc == _lib.ERR_CAPACITY:  # the needed count travels with the error
            err = _lib.OrbfeError(rc, self._L.orbfe_last_error().decode("utf-8", "replace"))
            err.n_created = nc.value
            raise err
        check(rc)
        k = nc.value
        return dict(created_k=ck[:k].copy(), created_i1=ci1[:k].copy(), created_i2=ci2[:k].copy(), created_slot=slot[:k].copy(),
                    status=status[:K, :n1].copy(), n_created_per_neighbour=per[:K].copy(), n_created=k)

    def compute_distinctive_descriptors(self, graph, slot):
        """MapPoint::ComputeDistinctiveDescriptors for slot[] on the device (orbfe_obsgraph_distinctive_descriptors_mappoints):
        `graph` is the ObservationGraph that holds the rows and the key frames' descriptors; the winners' bytes land in this
        table's descriptors -> (best_kf_slot, best_idx, valid); slots with valid = 0 keep what they hold."""
        return graph.distinctive_descriptors(slot, mp=self)


def motion_model_mode(Tcw_cur, Tlw, mb: float, mono: bool) -> int:
    """The `mode` of SearchByProjectionLastFrame from the two poses (src/ORBmatcher.cc:1494-1506): tlc = Rlw * twc + tlw with
    twc = -Rcw^T tcw, in float32; 1 (bForward) when tlc.z > mb, 2 (bBackward) when -tlc.z > mb, never for a monocular frame."""
    Tc = np.asarray(Tcw_cur, dtype=np.float32).reshape(4, 4)
    Tl = np.asarray(Tlw, dtype=np.float32).reshape(4, 4)
    twc = -(Tc[:3, :3].T @ Tc[:3, 3])
    tlc = Tl[:3, :3] @ twc + Tl[:3, 3]
    if mono:
        return 0
    return 1 if tlc[2] > np.float32(mb) else (2 if -tlc[2] > np.float32(mb) else 0)


def track_with_motion_model(mp: MapPoints, cur, slot, last_octave, last_angle, Tcw_cur, Tlw, mb: float, mono: bool, K5, bounds,
                            scale_factor: float, scale_factors, inv_level_sigma2, skip=None, blocked=None,
                            check_orientation: bool = True, outlier=None):
    """The device part of Tracking::TrackWithMotionModel (src/Tracking.cc:958-1010) on the resident map points, with no
    per-point host work: `mode` from tlc, SearchByProjection(mCurrentFrame, mLastFrame, th, mono) with th = 15 for a monocular
    sensor and 7 otherwise, once more with 2 * th when fewer than 20 matches came back (:969-973), then
    Optimizer::PoseOptimization on the same slot[].  Tcw_cur = mVelocity * mLastFrame.mTcw, Tlw = mLastFrame.mTcw, K5 = fx fy
    cx cy mbf, bounds = mnMinX mnMaxX mnMinY mnMaxY -> dict of nmatches, match [cur.N] (positions in slot[], -1 none), th (the
    one that was used), mode, n_inliers, Tcw [4, 4], outlier [cur.N].  With fewer than 20 matches after the retry the
    reference returns false before the optimisation: n_inliers is then 0, Tcw is Tcw_cur and no flag is set.  Everything
    behind (discarding the outliers' map points, mnLastFrameSeen, nmatchesMap and the decision, :988-1010) stays with the caller."""
    Tc = np.ascontiguousarray(Tcw_cur, dtype=np.float32).reshape(4, 4)
    k5 = np.ascontiguousarray(K5, dtype=np.float32).reshape(5)
    sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
    pose = camera_pose(Tc[:3, :3], Tc[:3, 3], k5[:4], k5[4], bounds, scale_factor, len(sf))
    mode = motion_model_mode(Tc, Tlw, mb, mono)
    th = 15.0 if mono else 7.0
    args = (cur, slot, last_octave, last_angle, pose, sf)
    kw = dict(mode=mode, skip=skip, blocked=blocked, check_orientation=check_orientation)
    nmatches, match = mp.SearchByProjectionLastFrame(*args, th, **kw)
    if nmatches < 20:
        th = 2.0 * th
        nmatches, match = mp.SearchByProjectionLastFrame(*args, th, **kw)
    out = dict(nmatches=nmatches, match=match, th=th, mode=mode, n_inliers=0, Tcw=Tc.copy(),
               outlier=np.zeros(cur.N, np.uint8) if outlier is None else np.asarray(outlier, np.uint8).copy())
    if nmatches < 20:
        return out
    ni, Tout, flags, _, _ = mp.pose_optimization(cur, slot, match, Tc, k5, inv_level_sigma2, outlier=outlier)
    out.update(n_inliers=ni, Tcw=Tout, outlier=flags)
    return out
