"""Optimizer::PoseOptimization (src/Optimizer.cc:256-473) on the device (include/orbfe.h: orbfe_pose_optimization*): the
pose-only optimisation Tracking runs between its searches, one kernel launch per call.  The map-point table form is
``MapPoints.pose_optimization``.

Optimizer::OptimizeSim3 (src/Optimizer.cc:1116-1323; orbfe_optimize_sim3*): the Sim3 refinement LoopClosing::ComputeSim3
runs on a loop candidate after Sim3Solver and SearchBySim3, one kernel launch for all candidates of a call.
Optimizer::LocalBundleAdjustment (:483-814; orbfe_local_bundle_adjustment*) and Optimizer::BundleAdjustment (:54-253;
orbfe_bundle_adjustment): g2o's Levenberg loop on the host over kernels for the linearisation, the Schur complement of the
points, the dense solve of the reduced camera system and the back-substitution.
Optimizer::OptimizeEssentialGraph (:833-1104; orbfe_optimize_essential_graph, orbfe_essential_graph_correct_*): the same
loop over kernels for the linearisation of the EdgeSim3 pose graph, a block-sparse Cholesky factorisation of its normal
equations and the correction of the map points; ``block_sparse_solve7`` is that solver on its own."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import EssGraphStatsC, LbaStatsC, OptSim3StatsC, PoseOptStatsC, check, ptr


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


def optsim3_stats_dict(st: OptSim3StatsC) -> dict:
    r = st.rounds
    return dict(rounds=r, n_bad=st.n_bad, iterations=list(st.iterations)[:r], trials=list(st.trials)[:r], lam=list(st.lam)[:r],
                chi2=list(st.chi2)[:r])


def sim3_to_Rts(sim3_out):
    """sim3_out = (qx, qy, qz, qw, tx, ty, tz, s), g2o::Sim3's own members -> (R [3, 3], t [3], s) in float64: the
    rotation().toRotationMatrix(), translation() and scale() that LoopClosing reads of g2oS12 (src/LoopClosing.cc:393-396)
    and that SearchByProjection / Sim3Solver users hold.  The quaternion is used as it is, as Eigen does (not normalised)."""
    x, y, z, w, tx, ty, tz, s = [float(c) for c in np.asarray(sim3_out, np.float64).reshape(8)]
    t2x, t2y, t2z = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = t2x * w, t2y * w, t2z * w
    txx, txy, txz = t2x * x, t2y * x, t2z * x
    tyy, tyz, tzz = t2y * y, t2z * y, t2z * z
    R = np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                  [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])
    return R, np.array([tx, ty, tz]), s


def _pairs(x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2):
    x1 = np.ascontiguousarray(x3dc1, dtype=np.float32).reshape(-1, 3)
    n = len(x1)
    out = [x1]
    for a, k in ((x3dc2, 3), (obs1, 2), (obs2, 2), (inv_sigma2_1, 1), (inv_sigma2_2, 1)):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        if len(a) != k * n:
            raise ValueError("optimize_sim3: the arrays must hold one entry per pair")
        out.append(a)
    return out


def optimize_sim3(x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2, sim3_in, th2=10.0, fix_scale=False,
                  device: int = 0):
    """One loop candidate: x3dc1 / x3dc2 [n, 3] (the matched map points in camera 1 / camera 2), obs1 / obs2 [n, 2], the two
    inv_sigma2 [n], cam1 / cam2 = (fx, fy, cx, cy), sim3_in [13] = R row-major, t, s (what Sim3Solver hands over) ->
    (n_in, sim3_out [8] float64 = qx qy qz qw tx ty tz s, bad [n] uint8 (0 kept, 1 / 2 erased after round one / two), stats
    dict, chi2_12 [n], chi2_21 [n] float64).  n_in = 0 with rounds < 2 is the reference's early return: sim3_out is the
    incoming S12 and the erasures of round one stay."""
    x1, x2, o1, o2, w1, w2 = _pairs(x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2)
    n = len(x1)
    k1 = np.ascontiguousarray(cam1, dtype=np.float32).reshape(4)
    k2 = np.ascontiguousarray(cam2, dtype=np.float32).reshape(4)
    s_in = np.ascontiguousarray(sim3_in, dtype=np.float32).reshape(13)
    out = np.zeros(8, np.float64)
    bad = np.zeros(max(n, 1), np.uint8)
    c12, c21 = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.float64)
    ni, st = C.c_int32(0), OptSim3StatsC()
    check(_lib.load().orbfe_optimize_sim3(int(device), n, ptr(x1), ptr(x2), ptr(o1), ptr(o2), ptr(w1), ptr(w2), ptr(k1), ptr(k2),
                                          ptr(s_in), float(th2), int(bool(fix_scale)), ptr(out), ptr(bad), C.byref(ni),
                                          C.byref(st), ptr(c12), ptr(c21)))
    return ni.value, out, bad[:n], optsim3_stats_dict(st), c12[:n], c21[:n]


def optimize_sim3_multi(pair_off, x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2, sim3_in, th2, fix_scale,
                        device: int = 0):
    """K candidates in one launch: candidate p owns pairs [pair_off[p], pair_off[p + 1]); cam1 / cam2 [K, 4], sim3_in [K, 13],
    th2 [K], fix_scale [K] -> (n_in [K], sim3_out [K, 8], bad [N], list of stats dicts, chi2_12 [N], chi2_21 [N]).  Equal to K
    single calls, bit for bit."""
    off = np.ascontiguousarray(pair_off, dtype=np.int32).reshape(-1)
    K = len(off) - 1
    x1, x2, o1, o2, w1, w2 = _pairs(x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2)
    n = len(x1)
    if K < 0 or off[-1] != n:
        raise ValueError("optimize_sim3_multi: pair_off must end at the pair count")
    k1 = np.ascontiguousarray(cam1, dtype=np.float32).reshape(-1)
    k2 = np.ascontiguousarray(cam2, dtype=np.float32).reshape(-1)
    s_in = np.ascontiguousarray(sim3_in, dtype=np.float32).reshape(-1)
    t2 = np.ascontiguousarray(th2, dtype=np.float32).reshape(-1)
    fix = np.ascontiguousarray(np.asarray(fix_scale).astype(bool), dtype=np.uint8).reshape(-1)
    if len(k1) != 4 * K or len(k2) != 4 * K or len(s_in) != 13 * K or len(t2) != K or len(fix) != K:
        raise ValueError("optimize_sim3_multi: cam1 / cam2 / sim3_in / th2 / fix_scale must hold one entry per problem")
    out = np.zeros(max(8 * K, 1), np.float64)
    bad = np.zeros(max(n, 1), np.uint8)
    c12, c21 = np.zeros(max(n, 1), np.float64), np.zeros(max(n, 1), np.float64)
    ni = np.zeros(max(K, 1), np.int32)
    st = (OptSim3StatsC * max(K, 1))()
    check(_lib.load().orbfe_optimize_sim3_multi(int(device), K, ptr(off), ptr(x1), ptr(x2), ptr(o1), ptr(o2), ptr(w1), ptr(w2),
                                                ptr(k1), ptr(k2), ptr(s_in), ptr(t2), ptr(fix), ptr(out), ptr(bad), ptr(ni),
                                                C.cast(st, C.c_void_p), ptr(c12), ptr(c21)))
    return ni[:K], out[:8 * K].reshape(K, 8), bad[:n], [optsim3_stats_dict(st[p]) for p in range(K)], c12[:n], c21[:n]


LBA_TERMINATION = ("none", "iterations", "trials", "rho_zero", "no_progress", "stop")


def lba_stats_dict(st: LbaStatsC) -> dict:
    return dict(rounds=st.rounds, stopped=st.stopped, host_syncs=st.host_syncs, n_level1=st.n_level1,
                iterations=list(st.iterations), trials=list(st.trials), termination=list(st.termination), lam=list(st.lam),
                chi2=list(st.chi2))


class LbaOperands:
    """The operands of the bundle-adjustment calls as contiguous arrays of the C types: Tcw [n_local + n_fixed, 4, 4] (local
    key frames first), cam [.., 5] = fx fy cx cy bf, xw [n_points, 3] (None in the table form), the edges grouped by point."""

    def __init__(self, n_local, Tcw, cam, xw, edge_pose, edge_point, u, v, u_right, inv_sigma2, local_is_fixed, n_points=None):
        self.T = np.ascontiguousarray(Tcw, dtype=np.float32).reshape(-1, 16)
        self.n_local, self.n_fixed = int(n_local), len(self.T) - int(n_local)
        self.cam = np.ascontiguousarray(cam, dtype=np.float32).reshape(-1)
        if self.n_fixed < 0 or len(self.cam) != 5 * len(self.T):
            raise ValueError("bundle adjustment: Tcw and cam must hold one entry per key frame, n_local of them local")
        self.xw = None if xw is None else np.ascontiguousarray(xw, dtype=np.float32).reshape(-1, 3)
        self.n_points = len(self.xw) if n_points is None else int(n_points)
        self.ep = np.ascontiguousarray(edge_pose, dtype=np.int32).reshape(-1)
        self.n_edges = len(self.ep)
        self.ept = np.ascontiguousarray(edge_point, dtype=np.int32).reshape(-1)
        self.obs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1) for a in (u, v, u_right, inv_sigma2)]
        if any(len(a) != self.n_edges for a in [self.ept] + self.obs):
            raise ValueError("bundle adjustment: the edge arrays must hold one entry per edge")
        self.fixed = None
        if local_is_fixed is not None:
            self.fixed = np.ascontiguousarray(np.asarray(local_is_fixed).astype(bool), dtype=np.uint8).reshape(-1)
            if len(self.fixed) != self.n_local:
                raise ValueError("bundle adjustment: local_is_fixed must hold one entry per local key frame")
        self.Tout = np.zeros((max(self.n_local, 1), 4, 4), np.float64)
        self.xout = np.zeros((max(self.n_points, 1), 3), np.float64)
        self.erase = np.zeros(max(self.n_edges, 1), np.uint8)
        self.level1 = np.zeros(max(self.n_edges, 1), np.uint8)
        self.chi2 = np.zeros(max(self.n_edges, 1), np.float64)
        self.st = LbaStatsC()

    def edges(self):
        return [self.n_edges, ptr(self.ep), ptr(self.ept)] + [ptr(a) for a in self.obs]

    def fixed_ptr(self):
        return None if self.fixed is None else ptr(self.fixed)

    def result(self, with_flags=True):
        out = [self.Tout[:self.n_local], self.xout[:self.n_points]]
        if with_flags:
            out += [self.erase[:self.n_edges], self.level1[:self.n_edges]]
        return tuple(out + [lba_stats_dict(self.st), self.chi2[:self.n_edges]])


def _stop_ptr(stop_flag):
    """stop_flag: None, or a ctypes c_int the caller may raise from another thread (pbStopFlag)."""
    return None if stop_flag is None else C.cast(C.byref(stop_flag), C.c_void_p)


def local_bundle_adjustment(n_local, Tcw, cam, xw, edge_pose, edge_point, u, v, u_right, inv_sigma2, local_is_fixed=None,
                            stop_flag=None, device: int = 0):
    """Optimizer::LocalBundleAdjustment from the graph on (src/Optimizer.cc:538-777) -> (Tcw_out [n_local, 4, 4] float64,
    xw_out [n_points, 3] float64, erase [n_edges] uint8 (nonzero: the pair goes into vToErase; 1 level 1 after round one, 2 by
    the final test only), level1 [n_edges] uint8, stats dict, edge_chi2 [n_edges] float64: what the final test read)."""
    o = LbaOperands(n_local, Tcw, cam, xw, edge_pose, edge_point, u, v, u_right, inv_sigma2, local_is_fixed)
    check(_lib.load().orbfe_local_bundle_adjustment(int(device), o.n_local, o.n_fixed, ptr(o.T), o.fixed_ptr(), ptr(o.cam), o.n_points,
                                                    ptr(o.xw), *o.edges(), _stop_ptr(stop_flag), ptr(o.Tout), ptr(o.xout),
                                                    ptr(o.erase), ptr(o.level1), C.cast(C.byref(o.st), C.c_void_p), ptr(o.chi2)))
    return o.result()


def bundle_adjustment(n_local, Tcw, cam, xw, edge_pose, edge_point, u, v, u_right, inv_sigma2, n_iterations=5, robust=True,
                      local_is_fixed=None, stop_flag=None, device: int = 0):
    """Optimizer::BundleAdjustment (src/Optimizer.cc:54-253): one optimize(n_iterations) -> (Tcw_out, xw_out, stats dict,
    edge_chi2)."""
    o = LbaOperands(n_local, Tcw, cam, xw, edge_pose, edge_point, u, v, u_right, inv_sigma2, local_is_fixed)
    check(_lib.load().orbfe_bundle_adjustment(int(device), o.n_local, o.n_fixed, ptr(o.T), o.fixed_ptr(), ptr(o.cam), o.n_points,
                                              ptr(o.xw), *o.edges(), int(n_iterations), int(bool(robust)), _stop_ptr(stop_flag),
                                              ptr(o.Tout), ptr(o.xout), C.cast(C.byref(o.st), C.c_void_p), ptr(o.chi2)))
    return o.result(with_flags=False)


def essgraph_stats_dict(st: EssGraphStatsC) -> dict:
    return dict(iterations=st.iterations, trials=st.trials, termination=st.termination, stopped=st.stopped, host_syncs=st.host_syncs,
                n_free=st.n_free, blocks_A=st.blocks_A, blocks_L=st.blocks_L, solve_failures=st.solve_failures, lam=st.lam,
                chi2_initial=st.chi2_initial, chi2=st.chi2)


def _sim3_records(a, n, what):
    a = np.ascontiguousarray(a, dtype=np.float64).reshape(-1, 8)
    if n is not None and len(a) != n:
        raise ValueError(f"{what} must hold one (qx qy qz qw tx ty tz s) record per vertex")
    return a


def optimize_essential_graph(sim3, edge_i, edge_j, sim3_meas=None, is_fixed=None, edge_kind=None, fix_scale=False,
                             n_iterations=20, device: int = 0):
    """Optimizer::OptimizeEssentialGraph from the graph on (src/Optimizer.cc:862-1067): sim3 [n, 8] = vScw as
    (qx qy qz qw tx ty tz s), sim3_meas [n, 8] = Snc (None: sim3), is_fixed [n] (the loop key frame), the edges (i, j) with
    edge_kind 0 (measurement from sim3_meas: spanning tree, old loops, covisibility) or 1 (from sim3: the new loop
    connections) -> (sim3_out [n, 8] float64, Tiw_out [n, 4, 4] float32 = [R | t / s], stats dict, edge_chi2 [n_edges])."""
    s = _sim3_records(sim3, None, "sim3")
    n = len(s)
    m = None if sim3_meas is None else _sim3_records(sim3_meas, n, "sim3_meas")
    ei = np.ascontiguousarray(edge_i, dtype=np.int32).reshape(-1)
    ej = np.ascontiguousarray(edge_j, dtype=np.int32).reshape(-1)
    ne = len(ei)
    if len(ej) != ne:
        raise ValueError("optimize_essential_graph: edge_i and edge_j must hold one entry per edge")
    kind = None if edge_kind is None else np.ascontiguousarray(edge_kind, dtype=np.uint8).reshape(-1)
    fixed = None if is_fixed is None else np.ascontiguousarray(np.asarray(is_fixed).astype(bool), dtype=np.uint8).reshape(-1)
    if (kind is not None and len(kind) != ne) or (fixed is not None and len(fixed) != n):
        raise ValueError("optimize_essential_graph: edge_kind / is_fixed must hold one entry per edge / vertex")
    out = np.zeros((max(n, 1), 8), np.float64)
    Tiw = np.zeros((max(n, 1), 4, 4), np.float32)
    chi2 = np.zeros(max(ne, 1), np.float64)
    st = EssGraphStatsC()
    check(_lib.load().orbfe_optimize_essential_graph(int(device), n, ptr(s), ptr(m), ptr(fixed), ne, ptr(ei), ptr(ej), ptr(kind),
                                                     int(bool(fix_scale)), int(n_iterations), ptr(out), ptr(Tiw), ptr(chi2),
                                                     C.cast(C.byref(st), C.c_void_p)))
    return out[:n], Tiw[:n], essgraph_stats_dict(st), chi2[:ne]


def _correction(sim3, sim3_out, ref_vertex):
    s = _sim3_records(sim3, None, "sim3")
    so = _sim3_records(sim3_out, len(s), "sim3_out")
    return s, so, np.ascontiguousarray(ref_vertex, dtype=np.int32).reshape(-1)


def essential_graph_correct_points(sim3, sim3_out, xw, ref_vertex, device: int = 0):
    """The tail of OptimizeEssentialGraph (:1070-1103): xw [n, 3] float32, ref_vertex [n] (the reference key frame's vertex,
    -1: copied through) -> xw_out [n, 3] float32 = Sout[r]^-1 .map(S[r] .map(P))."""
    s, so, r = _correction(sim3, sim3_out, ref_vertex)
    x = np.ascontiguousarray(xw, dtype=np.float32).reshape(-1, 3)
    if len(r) != len(x):
        raise ValueError("essential_graph_correct_points: ref_vertex must hold one entry per point")
    out = np.zeros((max(len(x), 1), 3), np.float32)
    check(_lib.load().orbfe_essential_graph_correct_points(int(device), len(s), ptr(s), ptr(so), len(x), ptr(x), ptr(r), ptr(out)))
    return out[:len(x)]


def block_sparse_solve7(colptr, rowidx, blocks, rhs, device: int = 0):
    """orbfe_block_sparse_solve7: the block lower triangle of a symmetric positive definite matrix in block-CSC (7 x 7 blocks
    [k, 7, 7], every column beginning with its diagonal block, rows ascending) and rhs [7 n] -> (x [7 n], ok, blocks_L)."""
    cp = np.ascontiguousarray(colptr, dtype=np.int32).reshape(-1)
    ri = np.ascontiguousarray(rowidx, dtype=np.int32).reshape(-1)
    n = len(cp) - 1
    bl = np.ascontiguousarray(blocks, dtype=np.float64).reshape(-1, 49)
    b = np.ascontiguousarray(rhs, dtype=np.float64).reshape(-1)
    if n < 1 or cp[-1] != len(ri) or len(bl) != len(ri) or len(b) != 7 * n:
        raise ValueError("block_sparse_solve7: colptr must end at the block count; one block per row index; 7 entries of rhs per column")
    x = np.zeros(7 * n, np.float64)
    ok, nl = C.c_int32(0), C.c_int32(0)
    check(_lib.load().orbfe_block_sparse_solve7(int(device), n, ptr(cp), ptr(ri), ptr(bl), ptr(b), ptr(x), C.byref(ok), C.byref(nl)))
    return x, ok.value, nl.value
