"""LocalMapping::CreateNewMapPoints' per-pair loop (src/LocalMapping.cc:331-501) on the device (include/orbfe.h:
orbfe_triangulate_matches*): the triangulation of the pairs SearchForTriangulation matched, one kernel launch per call.
ComputeF12 and the baseline test stay with the caller.  Where the created pairs become map points -- who, in what order, with
what descriptor, normal and range -- is orbfe_triangulated_points_select (triangulated_points_select below; on the resident
state: MapPoints.create_triangulated_points)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import FrameViewC, KeyFrameCameraC, check, ptr

TRI_NO_MATCH, TRI_CREATED, TRI_LOW_PARALLAX, TRI_W_ZERO, TRI_BEHIND_1, TRI_BEHIND_2, TRI_REPROJ_1, TRI_REPROJ_2, \
    TRI_DIST_ZERO, TRI_SCALE = range(10)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class KeyFrameCamera:
    """orbfe_keyframe_camera: Tcw = [Rcw | tcw] (3 x 4, or the 4 x 4 pose), Ow = GetCameraCenter(), the intrinsics, mb, mbf,
    and the arrays mvDepth (None: monocular) and mvKeys positions (None: the view's own x / y)."""

    def __init__(self, Tcw, Ow, fx, fy, cx, cy, mb=0.0, mbf=0.0, depth=None, x_raw=None, y_raw=None, invfx=None, invfy=None):
        T = _f32(Tcw).reshape(-1, 4)[:3]
        self.Tcw = _f32(T).reshape(12)
        self.Ow = _f32(Ow).reshape(3)
        f = np.float32
        self.fx, self.fy, self.cx, self.cy, self.mb, self.mbf = f(fx), f(fy), f(cx), f(cy), f(mb), f(mbf)
        self.invfx = f(1.0) / self.fx if invfx is None else f(invfx)  # invfx = 1.0f / fx (src/Frame.cc:93)
        self.invfy = f(1.0) / self.fy if invfy is None else f(invfy)
        self.depth = None if depth is None else _f32(depth).reshape(-1)
        self.x_raw = None if x_raw is None else _f32(x_raw).reshape(-1)
        self.y_raw = None if y_raw is None else _f32(y_raw).reshape(-1)

    def fill(self, c: KeyFrameCameraC):
        c.Tcw[:] = self.Tcw.tolist()
        c.Ow[:] = self.Ow.tolist()
        c.fx, c.fy, c.cx, c.cy, c.invfx, c.invfy, c.mb, c.mbf = (float(v) for v in (
            self.fx, self.fy, self.cx, self.cy, self.invfx, self.invfy, self.mb, self.mbf))
        c.depth, c.x_raw, c.y_raw = ptr(self.depth), ptr(self.x_raw), ptr(self.y_raw)
        return c

    @property
    def c(self):
        return self.fill(KeyFrameCameraC())


def _check_camera(cam: KeyFrameCamera, n: int, what: str):
    for name in ("depth", "x_raw", "y_raw"):
        a = getattr(cam, name)
        if a is not None and len(a) != n:
            raise ValueError(f"{what}: {name} must hold {n} entries, not {len(a)}")


def triangulate_matches_multi(kf1, cam1: KeyFrameCamera, neighbours, cams, match12, scale_factors, level_sigma2,
                              ratio_factor: float, device: int = 0):
    """kf1 / neighbours: FrameView or ResidentFrame; match12 [K, n1] as SearchForTriangulationMulti returns it ->
    (x3d [K, n1, 3] float32, status [K, n1] uint8, n_created [K], winner [n1]).  Keep, for keypoint i1, only the pair of
    neighbour winner[i1] (the first neighbour in order whose pair was created)."""
    K, n1 = len(neighbours), kf1.N
    if len(cams) != K:
        raise ValueError("triangulate_matches_multi: one camera per neighbour")
    m = np.ascontiguousarray(np.asarray(match12, dtype=np.int32).reshape(K, n1) if K else np.zeros((0, n1), np.int32))
    _check_camera(cam1, n1, "triangulate_matches_multi")
    for nb, cm in zip(neighbours, cams):
        _check_camera(cm, nb.N, "triangulate_matches_multi")
    sf, sg = _f32(scale_factors).reshape(-1), _f32(level_sigma2).reshape(-1)
    if len(sf) != len(sg):
        raise ValueError("triangulate_matches_multi: scale_factors and level_sigma2 must hold one entry per level")
    views = (C.POINTER(FrameViewC) * max(K, 1))(*[C.pointer(nb.c) for nb in neighbours])
    cc = (KeyFrameCameraC * max(K, 1))()
    for k, cm in enumerate(cams):
        cm.fill(cc[k])
    x3d = np.zeros((max(K, 1), max(n1, 1), 3), np.float32)
    status = np.zeros((max(K, 1), max(n1, 1)), np.uint8)
    created = np.zeros(max(K, 1), np.int32)
    winner = np.full(max(n1, 1), -1, np.int32)
    c1 = cam1.c
    check(_lib.load().orbfe_triangulate_matches_multi(int(device), C.byref(kf1.c), C.byref(c1), K, views, cc, ptr(m), ptr(sf),
                                                      ptr(sg), len(sf), float(ratio_factor), ptr(x3d), ptr(status), ptr(created),
                                                      ptr(winner)))
    if n1 == 0 or K == 0:
        return np.zeros((K, n1, 3), np.float32), np.zeros((K, n1), np.uint8), created[:K], winner[:n1]
    return x3d, status, created[:K], winner[:n1]


def triangulate_matches(kf1, cam1: KeyFrameCamera, kf2, cam2: KeyFrameCamera, match12, scale_factors, level_sigma2,
                        ratio_factor: float, device: int = 0):
    """One neighbour: match12 [n1] -> (x3d [n1, 3], status [n1], n_created)."""
    n1 = kf1.N
    m = np.ascontiguousarray(np.asarray(match12, dtype=np.int32).reshape(n1))
    _check_camera(cam1, n1, "triangulate_matches")
    _check_camera(cam2, kf2.N, "triangulate_matches")
    sf, sg = _f32(scale_factors).reshape(-1), _f32(level_sigma2).reshape(-1)
    if len(sf) != len(sg):
        raise ValueError("triangulate_matches: scale_factors and level_sigma2 must hold one entry per level")
    x3d = np.zeros((max(n1, 1), 3), np.float32)
    status = np.zeros(max(n1, 1), np.uint8)
    created = C.c_int32(0)
    c1, c2 = cam1.c, cam2.c
    check(_lib.load().orbfe_triangulate_matches(int(device), C.byref(kf1.c), C.byref(c1), C.byref(kf2.c), C.byref(c2), ptr(m),
                                                ptr(sf), ptr(sg), len(sf), float(ratio_factor), ptr(x3d), ptr(status),
                                                C.byref(created)))
    return x3d[:n1], status[:n1], created.value


def triangulated_points_select(match12, status, x3d, kf1_id: int, kf2_ids, centre1, centre2, octave1, scale_factors, capacity=None):
    """orbfe_triangulated_points_select: the birth at the tail of CreateNewMapPoints' pair loop (src/LocalMapping.cc:484-500) on
    the outputs of triangulate_matches_multi.  match12 / status [K, n1], x3d [K, n1, 3]; kf1_id / kf2_ids [K] the mnIds,
    centre1 [3] / centre2 [K, 3] the camera centres, octave1 [n1] key frame 1's octaves -> dict of created_k, created_i1,
    created_i2, pos [m, 3], normal [m, 3], min_dist, max_dist, desc_from (0: key frame 1's descriptor row i1, 1: the
    neighbour's row i2) in creation order, n_created.  capacity None: room for every keypoint of key frame 1.  More created
    points than capacity raises OrbfeError(ERR_CAPACITY) whose n_created is the needed count."""
    ids = np.ascontiguousarray(kf2_ids, dtype=np.int64).reshape(-1)
    K = len(ids)
    oc = np.ascontiguousarray(octave1, dtype=np.int32).reshape(-1)
    n1 = len(oc)
    m = np.ascontiguousarray(np.asarray(match12, dtype=np.int32).reshape(K, n1))
    st = np.ascontiguousarray(np.asarray(status, dtype=np.uint8).reshape(K, n1))
    x = np.ascontiguousarray(np.asarray(x3d, dtype=np.float32).reshape(K, n1, 3))
    c1 = _f32(centre1).reshape(3)
    c2 = np.ascontiguousarray(np.asarray(centre2, dtype=np.float32).reshape(K, 3))
    sf = _f32(scale_factors).reshape(-1)
    cap = n1 if capacity is None else int(capacity)
    room = max(cap, 1)
    ck, ci1, ci2 = np.zeros(room, np.int32), np.zeros(room, np.int32), np.zeros(room, np.int32)
    pos, nrm = np.zeros((room, 3), np.float32), np.zeros((room, 3), np.float32)
    lo, hi, frm = np.zeros(room, np.float32), np.zeros(room, np.float32), np.zeros(room, np.uint8)
    nc = C.c_int32(0)
    L = _lib.load()
    rc = L.orbfe_triangulated_points_select(n1, K, ptr(m), ptr(st), ptr(x), int(kf1_id), ptr(ids), ptr(c1), ptr(c2), ptr(oc), ptr(sf), len(sf),
                                            cap, ptr(ck), ptr(ci1), ptr(ci2), ptr(pos), ptr(nrm), ptr(lo), ptr(hi), ptr(frm), C.byref(nc))
    if rc == _lib.ERR_CAPACITY:  # the needed count travels with the error
        err = _lib.OrbfeError(rc, L.orbfe_last_error().decode("utf-8", "replace"))
        err.n_created = nc.value
        raise err
    check(rc)
    k = nc.value
    return dict(created_k=ck[:k].copy(), created_i1=ci1[:k].copy(), created_i2=ci2[:k].copy(), pos=pos[:k].copy(), normal=nrm[:k].copy(),
                min_dist=lo[:k].copy(), max_dist=hi[:k].copy(), desc_from=frm[:k].copy(), n_created=k)
