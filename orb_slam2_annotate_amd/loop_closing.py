"""Sim3Solver (src/Sim3Solver.cc), the RANSAC of LoopClosing::ComputeSim3 (src/LoopClosing.cc:286-404), on the device
(include/orbfe.h: orbfe_sim3_ransac*): every hypothesis of every candidate's solver is evaluated in ONE kernel launch
(Sim3Solver.evaluate_all); iterate() then replays the reference's stateful loop (:150-220) over the results on the host.  The
map-graph side of the constructor (:64-79), the random stream of the triples and OptimizeSim3 stay with the caller."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, ptr

SIM3_OK, SIM3_NONFINITE = 0, 1


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def sim3_legs(R1w, t1w, R2w, t2w, s12, R12, t12, K4_1, bounds1, scale_factor1, n_levels1, K4_2=None, bounds2=None,
              scale_factor2=None, n_levels2=None):
    """The two legs of ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th) (src/ORBmatcher.cc:1260-1270) for
    MapPoints.SearchBySim3 -> (leg12, leg21): leg12 projects KF1's points into KF2 (R1w, t1w, then sR21, t21, KF2's camera),
    leg21 KF2's points into KF1 (R2w, t2w, then sR12, t12, KF1's camera).  The camera of KF2 defaults to KF1's.

    The rounding of the 24 composed floats is fixed HERE, not in the kernel, because the reference leaves it to OpenCV's
    matrix expressions, whose arithmetic depends on the OpenCV version and build:
      sR12 = float32(s12) * R12 entry by entry, one binary32 product each;
      sR21 = (1.0 / s12) * R12^T: the reciprocal in binary64, each entry the binary64 product rounded to binary32 once;
      t21  = -(sR21 t12): per row ((a0*b0 + a1*b1) + a2*b2) in binary32, products and sums rounded one by one, then negated;
      t12 unchanged.
    A caller that must match one particular OpenCV build bit for bit composes the 24 floats itself and calls
    map_points.sim3_leg."""
    from .map_points import sim3_leg

    s = np.float32(s12)
    R = np.asarray(R12, dtype=np.float32).reshape(3, 3)
    t = np.asarray(t12, dtype=np.float32).reshape(3)
    sR12 = (s * R).astype(np.float32)
    sR21 = ((1.0 / np.float64(s)) * R.T.astype(np.float64)).astype(np.float32)
    p = (sR21 * t[None, :]).astype(np.float32)
    t21 = -((p[:, 0] + p[:, 1]).astype(np.float32) + p[:, 2]).astype(np.float32)
    if K4_2 is None:
        K4_2, bounds2, scale_factor2, n_levels2 = K4_1, bounds1, scale_factor1, n_levels1
    leg12 = sim3_leg(R1w, t1w, sR21, t21, K4_2, bounds2, scale_factor2, n_levels2)
    leg21 = sim3_leg(R2w, t2w, sR12, t, K4_1, bounds1, scale_factor1, n_levels1)
    return leg12, leg21


def sim3_max_iterations(n: int, prob: float = 0.99, min_inliers: int = 6, max_its: int = 300) -> int:
    """What SetRansacParameters (:118-142) leaves in mRansacMaxIts (orbfe_sim3_max_iterations)."""
    return int(_lib.load().orbfe_sim3_max_iterations(int(n), float(prob), int(min_inliers), int(max_its)))


def sim3_triples_from_draws(n: int, draws) -> np.ndarray:
    """draws [H, 3], draws[h, i] in [0, n - 1 - i] = the three RandomInt values of :178 -> triples [H, 3], the pairs the
    reference's selection without replacement (:173-187) takes."""
    d = _i32(draws).reshape(-1, 3)
    t = np.zeros((max(len(d), 1), 3), np.int32)
    check(_lib.load().orbfe_sim3_triples_from_draws(int(n), len(d), ptr(d), ptr(t)))
    return t[:len(d)]


_GOLDEN, _M1, _M2 = np.uint64(0x9E3779B97F4A7C15), np.uint64(0xBF58476D1CE4E5B9), np.uint64(0x94D049BB133111EB)


def seeded_draws(seed: int, first: int, n: int, H: int) -> np.ndarray:
    """The documented generator of evaluate_all(solvers, seed): draw number c (counted from `first` over solvers, hypotheses
    and picks in order) is splitmix64's output for the state seed + (c + 1) * 0x9E3779B97F4A7C15 (mod 2^64), reduced modulo the
    size n - i of the list it indexes.  The C++ class computes the same.  This is NOT the reference's rand() stream."""
    with np.errstate(over="ignore"):
        c = np.arange(first + 1, first + 1 + 3 * H, dtype=np.uint64)
        z = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + c * _GOLDEN
        z = (z ^ (z >> np.uint64(30))) * _M1
        z = (z ^ (z >> np.uint64(27))) * _M2
        z = z ^ (z >> np.uint64(31))
    size = np.tile(np.array([n, n - 1, n - 2], np.uint64), H)
    return (z % size).astype(np.int32).reshape(H, 3)


def sim3_ransac_multi(pair_off, x3dc1, x3dc2, max_err1, max_err2, cam1, cam2, fix_scale, hyp_off, triples, device: int = 0):
    """orbfe_sim3_ransac_multi -> (n_inliers [H], status [H], sim3 [H, 13], mask_words, word_off [K + 1])."""
    po, ho = _i32(pair_off).reshape(-1), _i32(hyp_off).reshape(-1)
    K = len(po) - 1
    if K < 0 or len(ho) != K + 1:
        raise ValueError("sim3_ransac_multi: pair_off and hyp_off must hold K + 1 entries")
    x1, x2 = _f32(x3dc1).reshape(-1, 3), _f32(x3dc2).reshape(-1, 3)
    e1, e2 = _f32(max_err1).reshape(-1), _f32(max_err2).reshape(-1)
    c1, c2 = _f32(cam1).reshape(-1, 4), _f32(cam2).reshape(-1, 4)
    tr = _i32(triples).reshape(-1, 3)
    N, H = len(x1), len(tr)
    if not (len(x2) == len(e1) == len(e2) == N) or len(c1) != K or len(c2) != K:
        raise ValueError("sim3_ransac_multi: one entry per pair in x3dc2 / max_err1 / max_err2, one camera per candidate")
    n_k, h_k = np.diff(po).astype(np.int64), np.diff(ho).astype(np.int64)
    total = int((np.maximum(h_k, 0) * ((np.maximum(n_k, 0) + 31) // 32)).sum())
    n_inl = np.zeros(max(H, 1), np.int32)
    status = np.zeros(max(H, 1), np.uint8)
    sim3 = np.zeros((max(H, 1), 13), np.float32)
    words = np.zeros(max(total, 1), np.uint32)
    word_off = np.zeros(K + 1, np.int32)
    check(_lib.load().orbfe_sim3_ransac_multi(int(device), K, N, H, ptr(po), ptr(x1), ptr(x2), ptr(e1), ptr(e2), ptr(c1), ptr(c2),
                                              int(bool(fix_scale)), ptr(ho), ptr(tr), ptr(n_inl), ptr(status), ptr(sim3),
                                              ptr(words), ptr(word_off)))
    return n_inl[:H], status[:H], sim3[:H], words[:total], word_off


def sim3_ransac(x3dc1, x3dc2, max_err1, max_err2, cam1, cam2, fix_scale, triples, device: int = 0):
    """One candidate (orbfe_sim3_ransac) -> (n_inliers [H], status [H], sim3 [H, 13], mask_words [H, ceil(n / 32)])."""
    x1, x2 = _f32(x3dc1).reshape(-1, 3), _f32(x3dc2).reshape(-1, 3)
    e1, e2 = _f32(max_err1).reshape(-1), _f32(max_err2).reshape(-1)
    c1, c2 = _f32(cam1).reshape(4), _f32(cam2).reshape(4)
    tr = _i32(triples).reshape(-1, 3)
    n, H = len(x1), len(tr)
    if not (len(x2) == len(e1) == len(e2) == n):
        raise ValueError("sim3_ransac: one entry per pair in x3dc2 / max_err1 / max_err2")
    w = (n + 31) // 32
    n_inl = np.zeros(max(H, 1), np.int32)
    status = np.zeros(max(H, 1), np.uint8)
    sim3 = np.zeros((max(H, 1), 13), np.float32)
    words = np.zeros(max(H * w, 1), np.uint32)
    check(_lib.load().orbfe_sim3_ransac(int(device), n, ptr(x1), ptr(x2), ptr(e1), ptr(e2), ptr(c1), ptr(c2), int(bool(fix_scale)),
                                        H, ptr(tr), ptr(n_inl), ptr(status), ptr(sim3), ptr(words)))
    return n_inl[:H], status[:H], sim3[:H], words[:H * w].reshape(H, w)


def unpack_mask(words, n: int) -> np.ndarray:
    """mask words of one hypothesis -> bool [n] (pair i at bit i & 31 of word i >> 5)"""
    i = np.arange(n)
    return ((np.asarray(words, np.uint32)[i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


class Sim3Solver:
    """The reference's Sim3Solver without the map graph.  The caller walks vpMatched12 as the reference's constructor does
    (:62-103) and hands in, for the n pairs it keeps: indices1 (mvnIndices1, :92), x3dc1 / x3dc2 [n, 3] (mvX3Dc1 / mvX3Dc2,
    :95-98), sigma2_1 / sigma2_2 [n] (mvLevelSigma2 of the two keypoints' octaves, :84-85), cam1 / cam2 = (fx, fy, cx, cy) of
    mK1 / mK2, N1 = vpMatched12.size() and fix_scale.  The class computes maxErr = (float)(9.210 * sigma2) (:87-88) and calls
    SetRansacParameters() with the reference's defaults (:111).

    Sim3Solver.evaluate_all(solvers, triples_or_seed) evaluates every solver's mRansacMaxIts hypotheses in one device call;
    iterate(n) then behaves as the reference's (:150-220), hypothesis mnIterations of the evaluated list standing where the
    reference draws and solves one."""

    def __init__(self, indices1, x3dc1, x3dc2, sigma2_1, sigma2_2, cam1, cam2, N1: int, fix_scale: bool):
        self.indices1 = np.ascontiguousarray(indices1, dtype=np.int64).reshape(-1)
        self.x3dc1, self.x3dc2 = _f32(x3dc1).reshape(-1, 3), _f32(x3dc2).reshape(-1, 3)
        self.N = len(self.indices1)
        s1, s2 = _f32(sigma2_1).reshape(-1), _f32(sigma2_2).reshape(-1)
        if not (len(self.x3dc1) == len(self.x3dc2) == len(s1) == len(s2) == self.N):
            raise ValueError("Sim3Solver: one entry per pair in every array")
        self.mN1 = int(N1)
        if self.N and (self.indices1.min() < 0 or self.indices1.max() >= self.mN1):
            raise ValueError("Sim3Solver: indices1 outside [0, N1)")
        self.max_err1 = (9.210 * s1.astype(np.float64)).astype(np.float32)  # :87
        self.max_err2 = (9.210 * s2.astype(np.float64)).astype(np.float32)  # :88
        self.cam1, self.cam2 = _f32(cam1).reshape(4), _f32(cam2).reshape(4)
        self.mbFixScale = bool(fix_scale)
        self.mnIterations = 0
        self.mnBestInliers = 0
        self._best = None
        self._results = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability: float = 0.99, minInliers: int = 6, maxIterations: int = 300):
        """:118-142; what an earlier evaluate_all left is dropped (the number of hypotheses may have changed)"""
        self.mRansacProb, self.mRansacMinInliers = float(probability), int(minInliers)
        self.mRansacMaxIts = sim3_max_iterations(self.N, probability, minInliers, maxIterations)
        self.mnIterations = 0
        self._results = None

    @property
    def n_hypotheses(self) -> int:
        """what evaluate_all evaluates for this solver: none when iterate() would return at :156"""
        return 0 if self.N < self.mRansacMinInliers else self.mRansacMaxIts

    @staticmethod
    def evaluate_all(solvers, triples_or_seed=0, device: int = 0):
        """One orbfe_sim3_ransac_multi call for every solver's hypotheses.  triples_or_seed: a list with one [H_k, 3] array of
        pair indices per solver (H_k = solver.n_hypotheses; e.g. sim3_triples_from_draws of the reference's random stream), or
        an int seed for the documented generator seeded_draws.  All solvers share fix_scale.  Returns the triples used."""
        solvers = list(solvers)
        if len({s.mbFixScale for s in solvers}) > 1:
            raise ValueError("Sim3Solver.evaluate_all: the solvers of one call share fix_scale")
        if isinstance(triples_or_seed, (int, np.integer)):
            triples, first = [], 0
            for s in solvers:
                H = s.n_hypotheses
                triples.append(sim3_triples_from_draws(s.N, seeded_draws(int(triples_or_seed), first, s.N, H)) if H
                               else np.zeros((0, 3), np.int32))
                first += 3 * H
        else:
            triples = [_i32(t).reshape(-1, 3) for t in triples_or_seed]
            if len(triples) != len(solvers) or any(len(t) != s.n_hypotheses for t, s in zip(triples, solvers)):
                raise ValueError("Sim3Solver.evaluate_all: one [n_hypotheses, 3] array of triples per solver")
        cat = lambda arrs, shape, dt: np.concatenate(arrs) if arrs else np.zeros(shape, dt)
        pair_off = np.concatenate([[0], np.cumsum([s.N for s in solvers])]).astype(np.int32)
        hyp_off = np.concatenate([[0], np.cumsum([len(t) for t in triples])]).astype(np.int32)
        n_inl, status, sim3, words, word_off = sim3_ransac_multi(
            pair_off, cat([s.x3dc1 for s in solvers], (0, 3), np.float32), cat([s.x3dc2 for s in solvers], (0, 3), np.float32),
            cat([s.max_err1 for s in solvers], 0, np.float32), cat([s.max_err2 for s in solvers], 0, np.float32),
            cat([s.cam1[None] for s in solvers], (0, 4), np.float32), cat([s.cam2[None] for s in solvers], (0, 4), np.float32),
            bool(solvers and solvers[0].mbFixScale), hyp_off, cat(triples, (0, 3), np.int32), device)
        for k, s in enumerate(solvers):
            h0, h1, w = int(hyp_off[k]), int(hyp_off[k + 1]), (s.N + 31) // 32
            s._results = dict(n_inliers=n_inl[h0:h1].copy(), status=status[h0:h1].copy(), sim3=sim3[h0:h1].copy(),
                              words=words[int(word_off[k]):int(word_off[k + 1])].reshape(h1 - h0, w).copy())
        return triples

    def _T12(self, h):
        v = self._results["sim3"][h]
        T = np.eye(4, dtype=np.float32)
        T[:3, :3] = v[12] * v[:9].reshape(3, 3)  # :356
        T[:3, 3] = v[9:12]
        return T

    def iterate(self, nIterations: int):
        """-> (T12 [4, 4] float32 or None, bNoMore, vbInliers [N1] bool, nInliers), :150-220"""
        if self._results is None:
            raise RuntimeError("Sim3Solver.iterate: call Sim3Solver.evaluate_all first")
        vbInliers = np.zeros(self.mN1, bool)  # :153
        if self.N < self.mRansacMinInliers:   # :156
            return None, True, vbInliers, 0
        r = self._results
        cur = 0
        while self.mnIterations < self.mRansacMaxIts and cur < nIterations:  # :168
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            n = int(r["n_inliers"][h])
            if n >= self.mnBestInliers:  # :195
                self._best, self.mnBestInliers = r["sim3"][h].copy(), n  # :197-202
                if n > self.mRansacMinInliers:  # :204
                    vbInliers[self.indices1[unpack_mask(r["words"][h], self.N)]] = True  # :207-209
                    return self._T12(h), False, vbInliers, n
        return None, self.mnIterations >= self.mRansacMaxIts, vbInliers, 0  # :216-219

    def find(self):
        """-> (T12 or None, vbInliers12, nInliers), :222-226"""
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n

    def _best_sim3(self):
        if self._best is None:
            raise RuntimeError("Sim3Solver: no hypothesis has been taken yet")
        return self._best

    def GetEstimatedRotation(self):
        return self._best_sim3()[:9].reshape(3, 3).copy()

    def GetEstimatedTranslation(self):
        return self._best_sim3()[9:12].copy()

    def GetEstimatedScale(self):
        return float(self._best_sim3()[12])


# ---- Loop correction: the head of CorrectLoop (src/LoopClosing.cc:514-604) and the map update at the tail of
# RunGlobalBundleAdjustment (src/LoopClosing.cc:787-852).  The resident forms are MapPoints.correct_loop / gba_update. ----
def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = _i32(np.concatenate([np.asarray(x, np.int32).reshape(-1) for x in lists])) if off[-1] else np.zeros(1, np.int32)
    return off, flat


def correct_loop_sim3s(Tiw, Twc_cur, cur: int, Scw):
    """CorrectedSim3, NonCorrectedSim3 (:519-551) and the corrected poses (:590-596) of mvpCurrentConnectedKFs
    (orbfe_correct_loop_sim3s): Tiw [K, 4, 4] = GetPose(), Twc_cur = the current key frame's GetPoseInverse(), cur its index,
    Scw = mg2oScw as qx qy qz qw tx ty tz s -> (corrected [K, 8], noncorrected [K, 8], Tiw_corrected [K, 4, 4])."""
    T = _f32(Tiw).reshape(-1, 16)
    K = len(T)
    tw = _f32(Twc_cur).reshape(16)
    s = np.ascontiguousarray(Scw, dtype=np.float64).reshape(8)
    cor, non, out = np.zeros((max(K, 1), 8)), np.zeros((max(K, 1), 8)), np.zeros((max(K, 1), 16), np.float32)
    check(_lib.load().orbfe_correct_loop_sim3s(K, ptr(T), ptr(tw), int(cur), ptr(s), ptr(cor), ptr(non), ptr(out)))
    return cor[:K], non[:K], out[:K].reshape(-1, 4, 4)


def correct_loop_points(corrected, noncorrected, kf_points, xw, skip=None):
    """The point loop of :558-587 on arrays (orbfe_correct_loop_points): kf_points[k] = the point indices key frame k lists
    (-1 = NULL), skip[p] = isBad() or mnCorrectedByKF == current -> (xw_out [n, 3], corrected_ref [n]: the claiming list
    position, -1 = untouched)."""
    cor = np.ascontiguousarray(corrected, dtype=np.float64).reshape(-1, 8)
    non = np.ascontiguousarray(noncorrected, dtype=np.float64).reshape(-1, 8)
    if len(cor) != len(non) or len(cor) != len(kf_points):
        raise ValueError("correct_loop_points: corrected, noncorrected and kf_points must hold one entry per key frame")
    off, flat = _csr(kf_points)
    x = _f32(xw).reshape(-1, 3)
    n = len(x)
    sk = None if skip is None else _u8(skip).reshape(-1)
    if sk is not None and len(sk) != n:
        raise ValueError("correct_loop_points: skip must hold one entry per point")
    out, ref = np.zeros((max(n, 1), 3), np.float32), np.zeros(max(n, 1), np.int32)
    check(_lib.load().orbfe_correct_loop_points(len(cor), ptr(cor), ptr(non), ptr(off), ptr(flat), n, ptr(x), ptr(sk), ptr(out), ptr(ref)))
    return out[:n], ref[:n]


def gba_propagate_keyframes(origins, children, Tcw, Twc, in_gba, Tcw_gba):
    """The spanning-tree walk of :788-815 (orbfe_gba_propagate_keyframes): origins = mvpKeyFrameOrigins as indices,
    children[k] = the indices of key frame k's children, Tcw / Twc [n, 4, 4] at entry, in_gba[k] = mnBAGlobalForKF == nLoopKF,
    Tcw_gba [n, 4, 4] = mTcwGBA (read where in_gba) -> (Tcw_new [n, 4, 4], reached [n], visited [n])."""
    T, Tw, Tg = _f32(Tcw).reshape(-1, 16), _f32(Twc).reshape(-1, 16), _f32(Tcw_gba).reshape(-1, 16)
    n = len(T)
    g = _u8(in_gba).reshape(-1)
    if not (len(Tw) == len(Tg) == len(g) == len(children) == n):
        raise ValueError("gba_propagate_keyframes: every per-key-frame array must hold n entries")
    o = _i32(origins).reshape(-1)
    off, flat = _csr(children)
    out, reached, visited = np.zeros((max(n, 1), 16), np.float32), np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
    check(_lib.load().orbfe_gba_propagate_keyframes(n, len(o), ptr(o), ptr(off), ptr(flat), ptr(T), ptr(Tw), ptr(g), ptr(Tg), ptr(out),
                                                    ptr(reached), ptr(visited)))
    return out[:n].reshape(-1, 4, 4), reached[:n], visited[:n]


def gba_update_points(xw, bad, in_gba, pos_gba, ref_kf, reached, Tcw_bef, Twc_new):
    """The point loop of :818-852 on arrays (orbfe_gba_update_points) -> (xw_out [p, 3], moved [p]: 0 skipped, 1 took
    pos_gba, 2 moved through its reference key frame ref_kf[p], an index into reached / Tcw_bef / Twc_new; -1 = none)."""
    x, pg = _f32(xw).reshape(-1, 3), _f32(pos_gba).reshape(-1, 3)
    p = len(x)
    b, g, r = _u8(bad).reshape(-1), _u8(in_gba).reshape(-1), _i32(ref_kf).reshape(-1)
    if not (len(pg) == len(b) == len(g) == len(r) == p):
        raise ValueError("gba_update_points: every per-point array must hold p entries")
    rc, tb, tn = _u8(reached).reshape(-1), _f32(Tcw_bef).reshape(-1, 16), _f32(Twc_new).reshape(-1, 16)
    if not (len(tb) == len(tn) == len(rc)):
        raise ValueError("gba_update_points: every per-key-frame array must hold one entry per key frame")
    out, moved = np.zeros((max(p, 1), 3), np.float32), np.zeros(max(p, 1), np.uint8)
    check(_lib.load().orbfe_gba_update_points(p, ptr(x), ptr(b), ptr(g), ptr(pg), ptr(r), len(rc), ptr(rc), ptr(tb), ptr(tn), ptr(out),
                                              ptr(moved)))
    return out[:p], moved[:p]
