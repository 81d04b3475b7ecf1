"""Where stereo and RGB-D map points are born (include/orbfe.h: orbfe_stereo_points_select, orbfe_count_close_points):
the host definitions of ``Tracking::StereoInitialization`` (src/Tracking.cc:563-578), the depth-sorted loop of
``Tracking::CreateNewKeyFrame`` (:1182-1234) and ``Tracking::UpdateLastFrame`` (:899-949), and the close-point counts of
``Tracking::NeedNewKeyFrame`` (:1100-1114).  The resident form is ``MapPoints.create_stereo_points``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import CameraPoseC, check, ptr

STEREO_ALL, STEREO_KEYFRAME, STEREO_TEMPORAL = 0, 1, 2  # ORBFE_STEREO_*


def _mask(a, n, name):
    if a is None:
        return None
    m = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)
    if len(m) != n:
        raise ValueError(f"{name} must hold one entry per keypoint")
    return m


def stereo_points_select(x, y, octave, depth, pose: CameraPoseC, th_depth: float, mode: int, scale_factors, centre=None,
                         occupied=None, stale=None, capacity=None):
    """orbfe_stereo_points_select on arrays: mvKeysUn x / y / octave, mvDepth, the masks occupied (mvpMapPoints[i] &&
    Observations() >= 1) and stale (a point with Observations() < 1), the pose (Rcw, Ow, fx fy cx cy are read), mThDepth,
    the mode and mvScaleFactors.  centre: the camera centre the normal and the range are taken from (the key frame's;
    default pose.Ow) -> dict of created_idx [m] (creation order), pos / normal [m, 3], min_dist / max_dist [m], cleared [n],
    n_created, n_walked.  capacity (default n) below the created count raises OrbfeError(ERR_CAPACITY)."""
    L = _lib.load()
    xs = np.ascontiguousarray(x, dtype=np.float32).reshape(-1)
    n = len(xs)
    ys = np.ascontiguousarray(y, dtype=np.float32).reshape(-1)
    oc = np.ascontiguousarray(octave, dtype=np.int32).reshape(-1)
    z = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1)
    if not (len(ys) == len(oc) == len(z) == n):
        raise ValueError("stereo_points_select: the arrays must hold one entry per keypoint")
    occ, st = _mask(occupied, n, "occupied"), _mask(stale, n, "stale")
    sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
    c = np.ascontiguousarray(pose.Ow if centre is None else centre, dtype=np.float32).reshape(3)
    cap = n if capacity is None else int(capacity)
    m = max(cap, 1)
    idx = np.zeros(m, np.int32)
    pos, nrm = np.zeros((m, 3), np.float32), np.zeros((m, 3), np.float32)
    lo, hi = np.zeros(m, np.float32), np.zeros(m, np.float32)
    cleared = np.zeros(max(n, 1), np.uint8)
    nc, nw = C.c_int32(0), C.c_int32(0)
    rc = L.orbfe_stereo_points_select(n, ptr(xs), ptr(ys), ptr(oc), ptr(z), ptr(occ), ptr(st), C.byref(pose), float(th_depth), int(mode),
                                      ptr(sf), len(sf), ptr(c), cap, ptr(idx), ptr(pos), ptr(nrm), ptr(lo), ptr(hi), ptr(cleared),
                                      C.byref(nc), C.byref(nw))
    if rc == _lib.ERR_CAPACITY:  # the needed count travels with the error
        err = _lib.OrbfeError(rc, L.orbfe_last_error().decode("utf-8", "replace"))
        err.n_created, err.n_walked = nc.value, nw.value
        raise err
    check(rc)
    k = nc.value
    return dict(created_idx=idx[:k].copy(), pos=pos[:k].copy(), normal=nrm[:k].copy(), min_dist=lo[:k].copy(), max_dist=hi[:k].copy(),
                cleared=cleared[:n].copy(), n_created=k, n_walked=nw.value)


def count_close_points(depth, has_point, outlier, th_depth: float):
    """orbfe_count_close_points: (nTrackedClose, nNonTrackedClose) of Tracking::NeedNewKeyFrame over mvDepth, mvpMapPoints[i] !=
    NULL and mvbOutlier: 0 < z < mThDepth, strict on both sides."""
    z = np.ascontiguousarray(depth, dtype=np.float32).reshape(-1)
    n = len(z)
    hp, ol = _mask(has_point, n, "has_point"), _mask(outlier, n, "outlier")
    if hp is None or ol is None:
        raise ValueError("count_close_points: has_point and outlier are required")
    a, b = C.c_int32(0), C.c_int32(0)
    check(_lib.load().orbfe_count_close_points(n, ptr(z), ptr(hp), ptr(ol), float(th_depth), C.byref(a), C.byref(b)))
    return a.value, b.value
