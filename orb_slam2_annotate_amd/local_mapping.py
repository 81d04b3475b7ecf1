"""LocalMapping::CreateNewMapPoints' per-pair loop (src/LocalMapping.cc:331-501) on the device (include/orbfe.h:
orbfe_triangulate_matches*): the triangulation of the pairs SearchForTriangulation matched, one kernel launch per call.
ComputeF12, the baseline test and the MapPoint bookkeeping stay with the caller."""
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
