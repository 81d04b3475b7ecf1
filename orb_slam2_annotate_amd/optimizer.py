"""Optimizer::PoseOptimization (src/Optimizer.cc:256-473) on the device (include/orbfe.h: orbfe_pose_optimization*): the
pose-only optimisation Tracking runs between its searches, one kernel launch per call.  The other Optimizer functions are
not covered.  The map-point table form is ``MapPoints.pose_optimization``."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import PoseOptStatsC, check, ptr


def stats_dict(st: PoseOptStatsC) -> dict:
    r = st.rounds
    return dict(rounds=r, iterations=list(st.iterations)[:r], trials=list(st.trials)[:r], lam=list(st.lam)[:r],
                chi2=list(st.chi2)[:r])


def _flags(outlier, n, what):
    """The flag array a call starts from: a copy of `outlier` (one entry per edge / keypoint), or zeros."""
    if outlier is None:
        return np.zeros(max(n, 1), np.uint8)
    f = np.array(outlier, dtype=np.uint8).reshape(-1)
    if len(f) != n:
        raise ValueError(f"{what}: outlier must hold {n} entries, not {len(f)}")
    return f if n else np.zeros(1, np.uint8)


def _edges(xw, u, v, u_right, inv_sigma2):
    xw = np.ascontiguousarray(xw, dtype=np.float32).reshape(-1, 3)
    arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (u, v, u_right, inv_sigma2)]
    if any(len(a) != len(xw) for a in arrs):
        raise ValueError("pose_optimization: the arrays must hold one entry per edge")
    return [xw] + arrs


def pose_optimization(xw, u, v, u_right, inv_sigma2, K5, Tcw, outlier=None, device: int = 0):
    """One problem: xw [n, 3], u / v / u_right (< 0: monocular) / inv_sigma2 [n], K5 = (fx, fy, cx, cy, mbf), Tcw 4 x 4 ->
    (n_inliers, Tcw_out [4, 4] float32, outlier [n] uint8, stats dict, edge_chi2 [n] float64).  `outlier`: the flags the call
    starts from; with fewer than 3 edges they and the pose come back untouched."""
    xw, u, v, ur, w = _edges(xw, u, v, u_right, inv_sigma2)
    n = len(xw)
    k = np.ascontiguousarray(K5, dtype=np.float32).reshape(5)
    T = np.ascontiguousarray(Tcw, dtype=np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    flags = _flags(outlier, n, "pose_optimization")
    chi2 = np.zeros(max(n, 1), np.float64)
    ni, st = C.c_int32(0), PoseOptStatsC()
    check(_lib.load().orbfe_pose_optimization(int(device), n, ptr(xw), ptr(u), ptr(v), ptr(ur), ptr(w), ptr(k), ptr(T), ptr(out),
                                              ptr(flags), C.byref(ni), C.byref(st), ptr(chi2)))
    return ni.value, out.reshape(4, 4), flags[:n], stats_dict(st), chi2[:n]


def pose_optimization_batch(offsets, xw, u, v, u_right, inv_sigma2, K5, Tcw, outlier=None, device: int = 0):
    """Q problems in one launch (Relocalization's candidates): problem p owns edges [offsets[p], offsets[p + 1]); K5 [Q, 5],
    Tcw [Q, 4, 4] -> (n_inliers [Q], Tcw_out [Q, 4, 4], outlier [N], list of stats dicts, edge_chi2 [N])."""
    off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
    Q = len(off) - 1
    xw, u, v, ur, w = _edges(xw, u, v, u_right, inv_sigma2)
    n = len(xw)
    if Q < 0 or off[-1] != n:
        raise ValueError("pose_optimization_batch: offsets must end at the edge count")
    k = np.ascontiguousarray(K5, dtype=np.float32).reshape(-1)
    T = np.ascontiguousarray(Tcw, dtype=np.float32).reshape(-1)
    if len(k) != 5 * Q or len(T) != 16 * Q:
        raise ValueError("pose_optimization_batch: K5 / Tcw must hold one entry per problem")
    out = np.zeros(max(16 * Q, 1), np.float32)
    flags = _flags(outlier, n, "pose_optimization_batch")
    chi2 = np.zeros(max(n, 1), np.float64)
    ni = np.zeros(max(Q, 1), np.int32)
    st = (PoseOptStatsC * max(Q, 1))()
    check(_lib.load().orbfe_pose_optimization_batch(int(device), Q, ptr(off), ptr(xw), ptr(u), ptr(v), ptr(ur), ptr(w), ptr(k),
                                                    ptr(T), ptr(out), ptr(flags), ptr(ni), C.cast(st, C.c_void_p), ptr(chi2)))
    return ni[:Q], out[:16 * Q].reshape(Q, 4, 4), flags[:n], [stats_dict(st[p]) for p in range(Q)], chi2[:n]
