"""PnPsolver (src/PnPsolver.cc), the RANSAC of Tracking::Relocalization (src/Tracking.cc:1487-1560): every EPnP hypothesis
of every candidate in one kernel launch, every Refine() problem in a second one (orbfe_pnp_*), and iterate() / find() as a
host replay over the two result sets.  Two deviations from the reference are documented in include/orbfe.h: Jacobi
decompositions in the place of OpenCV's, and a canonical null-space basis for the 4-point problem."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import check, ptr

PNP_OK, PNP_NONFINITE = 0, 1


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]).astype(np.int32)


def _points(point_off, p3d, p2d, max_err2, cam):
    off = np.ascontiguousarray(point_off, dtype=np.int32).reshape(-1)
    K = len(off) - 1
    a = np.ascontiguousarray(p3d, dtype=np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(p2d, dtype=np.float32).reshape(-1, 2)
    e = np.ascontiguousarray(max_err2, dtype=np.float32).reshape(-1)
    k = np.ascontiguousarray(cam, dtype=np.float32).reshape(-1)
    if K < 0 or not (len(a) == len(b) == len(e)) or len(k) != 4 * K:
        raise ValueError("pnp: p3d / p2d / max_err2 must hold one entry per correspondence, cam one per candidate")
    return K, off, a, b, e, k


def _words_total(off, item_off):
    n = np.diff(off).astype(np.int64)
    return int(np.sum(np.diff(item_off).astype(np.int64) * ((n + 31) // 32)))


def pnp_sets_from_draws(n: int, draws):
    """PnPsolver::iterate's selection without replacement (:201-214): draws [H, 4] -> sets [H, 4]."""
    d = np.ascontiguousarray(draws, dtype=np.int32).reshape(-1, 4)
    s = np.zeros_like(d)
    check(_lib.load().orbfe_pnp_sets_from_draws(int(n), len(d), ptr(d), ptr(s)))
    return s


def pnp_ransac_multi(point_off, p3d, p2d, max_err2, cam, hyp_off, sets, device: int = 0):
    """All hypotheses of K candidates in one launch -> (n_inliers [H], status [H], pose [H, 12] = R row-major, t,
    word_off [K + 1], mask_words)."""
    K, off, a, b, e, k = _points(point_off, p3d, p2d, max_err2, cam)
    ho = np.ascontiguousarray(hyp_off, dtype=np.int32).reshape(-1)
    s = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 4)
    H = len(s)
    if len(ho) != K + 1:
        raise ValueError("pnp_ransac_multi: hyp_off must hold K + 1 entries")
    ni, st, pose = np.zeros(max(H, 1), np.int32), np.zeros(max(H, 1), np.uint8), np.zeros(max(H, 1) * 12, np.float32)
    wo = np.zeros(K + 1, np.int32)
    nw = _words_total(off, ho)
    words = np.zeros(max(nw, 1), np.uint32)
    check(_lib.load().orbfe_pnp_ransac_multi(int(device), K, len(a), H, ptr(off), ptr(a), ptr(b), ptr(e), ptr(k), ptr(ho), ptr(s),
                                            ptr(ni), ptr(st), ptr(pose), ptr(wo), ptr(words)))
    return ni[:H], st[:H], pose[:12 * H].reshape(H, 12), wo, words[:nw]


def pnp_ransac(p3d, p2d, max_err2, cam, sets, device: int = 0):
    """One candidate -> (n_inliers [H], status [H], pose [H, 12], mask_words [H, ceil(n / 32)])."""
    a = np.ascontiguousarray(p3d, dtype=np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(p2d, dtype=np.float32).reshape(-1, 2)
    e = np.ascontiguousarray(max_err2, dtype=np.float32).reshape(-1)
    k = np.ascontiguousarray(cam, dtype=np.float32).reshape(4)
    s = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 4)
    if not (len(a) == len(b) == len(e)):
        raise ValueError("pnp_ransac: p3d / p2d / max_err2 must hold one entry per correspondence")
    H, w = len(s), (len(a) + 31) // 32
    ni, st, pose = np.zeros(max(H, 1), np.int32), np.zeros(max(H, 1), np.uint8), np.zeros(max(H, 1) * 12, np.float32)
    words = np.zeros(max(H * w, 1), np.uint32)
    check(_lib.load().orbfe_pnp_ransac(int(device), len(a), ptr(a), ptr(b), ptr(e), ptr(k), H, ptr(s), ptr(ni), ptr(st), ptr(pose),
                                      ptr(words)))
    return ni[:H], st[:H], pose[:12 * H].reshape(H, 12), words[:H * w].reshape(H, w)


def pnp_refine_multi(point_off, p3d, p2d, max_err2, cam, rec_off, rec_masks, device: int = 0):
    """The Refine() problems of K candidates in one launch; rec_masks: ceil(n_k / 32) words per record -> as
    pnp_ransac_multi, per record."""
    K, off, a, b, e, k = _points(point_off, p3d, p2d, max_err2, cam)
    ro = np.ascontiguousarray(rec_off, dtype=np.int32).reshape(-1)
    m = np.ascontiguousarray(rec_masks, dtype=np.uint32).reshape(-1)
    if len(ro) != K + 1:
        raise ValueError("pnp_refine_multi: rec_off must hold K + 1 entries")
    R = int(ro[-1]) if len(ro) else 0
    nw = _words_total(off, ro)
    if len(m) != nw:
        raise ValueError("pnp_refine_multi: rec_masks must hold ceil(n_k / 32) words per record")
    m = m if nw else np.zeros(1, np.uint32)
    ni, st, pose = np.zeros(max(R, 1), np.int32), np.zeros(max(R, 1), np.uint8), np.zeros(max(R, 1) * 12, np.float32)
    wo, words = np.zeros(K + 1, np.int32), np.zeros(max(nw, 1), np.uint32)
    check(_lib.load().orbfe_pnp_refine_multi(int(device), K, len(a), R, ptr(off), ptr(a), ptr(b), ptr(e), ptr(k), ptr(ro), ptr(m),
                                            ptr(ni), ptr(st), ptr(pose), ptr(wo), ptr(words)))
    return ni[:R], st[:R], pose[:12 * R].reshape(R, 12), wo, words[:nw]


def pnp_solve_multi(point_off, p3d, p2d, max_err2, cam, hyp_off, sets, min_inliers, device: int = 0):
    """Both launches and the record scan in one call -> dict: n_inliers, status, pose, word_off, mask_words (per hypothesis),
    rec_off [K + 1], rec_hyp, rec_n_inliers, rec_status, rec_pose, rec_word_off, rec_mask_words (per Refine record)."""
    K, off, a, b, e, k = _points(point_off, p3d, p2d, max_err2, cam)
    ho = np.ascontiguousarray(hyp_off, dtype=np.int32).reshape(-1)
    s = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 4)
    mi = np.ascontiguousarray(min_inliers, dtype=np.int32).reshape(-1)
    H = len(s)
    if len(ho) != K + 1 or len(mi) != K:
        raise ValueError("pnp_solve_multi: hyp_off must hold K + 1 entries, min_inliers K")
    nw = _words_total(off, ho)
    Hn, Wn = max(H, 1), max(nw, 1)
    ni, st, pose, wo, words = np.zeros(Hn, np.int32), np.zeros(Hn, np.uint8), np.zeros(Hn * 12, np.float32), \
        np.zeros(K + 1, np.int32), np.zeros(Wn, np.uint32)
    ro, rh = np.zeros(K + 1, np.int32), np.zeros(Hn, np.int32)
    rni, rst, rpose, rwo, rwords = np.zeros(Hn, np.int32), np.zeros(Hn, np.uint8), np.zeros(Hn * 12, np.float32), \
        np.zeros(K + 1, np.int32), np.zeros(Wn, np.uint32)
    mi_ = mi if K else np.zeros(1, np.int32)
    check(_lib.load().orbfe_pnp_solve_multi(int(device), K, len(a), H, ptr(off), ptr(a), ptr(b), ptr(e), ptr(k), ptr(ho), ptr(s),
                                           ptr(mi_), ptr(ni), ptr(st), ptr(pose), ptr(wo), ptr(words), ptr(ro), ptr(rh), ptr(rni),
                                           ptr(rst), ptr(rpose), ptr(rwo), ptr(rwords)))
    R = int(ro[K])
    return dict(n_inliers=ni[:H], status=st[:H], pose=pose[:12 * H].reshape(H, 12), word_off=wo, mask_words=words[:nw],
                rec_off=ro, rec_hyp=rh[:R], rec_n_inliers=rni[:R], rec_status=rst[:R], rec_pose=rpose[:12 * R].reshape(R, 12),
                rec_word_off=rwo, rec_mask_words=rwords[:int(rwo[K])])


def words_to_mask(words, n: int):
    w = np.asarray(words, np.uint32)
    i = np.arange(n)
    return ((w[i >> 5] >> (i & 31).astype(np.uint32)) & 1).astype(bool)


def ransac_parameters(N: int, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
    """PnPsolver::SetRansacParameters (:127-164) with its float and int conversions -> (mRansacMinInliers, mRansacMaxIts)."""
    eps = np.float32(epsilon)
    n_min = int(np.float32(N) * eps)  # :141
    n_min = max(n_min, int(minInliers), int(minSet))  # :142-145
    ratio = np.float32(n_min) / np.float32(N) if N > 0 else np.float32(np.inf)  # :148 (N = 0: the reference's x / 0)
    if eps < ratio:
        eps = ratio
    if n_min == N:  # :154
        its = 1
    else:
        d = math.log(1 - float(eps) ** 3) if 0 < float(eps) < 1 else float("nan")
        q = math.log(1 - probability) / d if d == d and d != 0 else float("nan")
        its = int(math.ceil(q)) if math.isfinite(q) else 1
    return n_min, max(1, min(its, int(maxIterations)))


class PnPsolver:
    """The reference's PnPsolver from arrays.  p3d [n, 3] (the matched MapPoints' world positions), p2d [n, 2] (mvKeysUn of
    the matched key points), sigma2 [n] (mvLevelSigma2 of their octaves), cam = (fx, fy, cx, cy); kp_indices [n] =
    mvKeyPointIndices and n_keypoints = the size of vbInliers (default: the correspondences themselves).  `sets` [H, 4]
    are the 4-sets of the hypotheses in order (pnp_sets_from_draws of the reference's RandomInt stream gives the
    reference's).  solve_all() runs a list of solvers in one call; a solver that has not been solved does so alone on its
    first iterate().  vbInliers is a bool array usable directly as the edge mask of pose_optimization_batch."""

    def __init__(self, p3d, p2d, sigma2, cam, sets, kp_indices=None, n_keypoints=None, device: int = 0):
        self.p3d = np.ascontiguousarray(p3d, dtype=np.float32).reshape(-1, 3)
        self.p2d = np.ascontiguousarray(p2d, dtype=np.float32).reshape(-1, 2)
        self.sigma2 = np.ascontiguousarray(sigma2, dtype=np.float32).reshape(-1)
        self.cam = np.ascontiguousarray(cam, dtype=np.float32).reshape(4)
        self.sets = np.ascontiguousarray(sets, dtype=np.int32).reshape(-1, 4)
        self.N = len(self.p3d)
        if not (len(self.p2d) == len(self.sigma2) == self.N):
            raise ValueError("PnPsolver: p3d / p2d / sigma2 must hold one entry per correspondence")
        self.kp_indices = np.arange(self.N) if kp_indices is None else np.asarray(kp_indices, np.int64).reshape(-1)
        self.n_keypoints = self.N if n_keypoints is None else int(n_keypoints)
        self.device = device
        self.mnIterations, self.mnBestInliers, self._best_h, self._rec = 0, 0, -1, -1
        self._res = None
        self.SetRansacParameters()

    def SetRansacParameters(self, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
        if minSet != 4:
            raise ValueError("PnPsolver: the minimal set is 4")
        self.mRansacMinInliers, self.mRansacMaxIts = ransac_parameters(self.N, probability, minInliers, maxIterations, minSet,
                                                                      epsilon, th2)
        self.max_err2 = (self.sigma2 * np.float32(th2)).astype(np.float32)  # :163
        self._res = None

    @staticmethod
    def solve_all(solvers):
        """Every hypothesis and every Refine problem of all solvers: two launches in all."""
        if not solvers:
            return
        live = [s for s in solvers if s.N >= 4 and s.N >= s.mRansacMinInliers]
        for s in solvers:
            s._res = dict(empty=True)
        if not live:
            return
        off, ho = _offsets([s.N for s in live]), _offsets([len(s.sets) for s in live])
        r = pnp_solve_multi(off, np.concatenate([s.p3d for s in live]), np.concatenate([s.p2d for s in live]),
                            np.concatenate([s.max_err2 for s in live]), np.stack([s.cam for s in live]), ho,
                            np.concatenate([s.sets for s in live]), [s.mRansacMinInliers for s in live], live[0].device)
        for k, s in enumerate(live):
            w = (s.N + 31) // 32
            h0, h1, r0, r1 = ho[k], ho[k + 1], r["rec_off"][k], r["rec_off"][k + 1]
            s._res = dict(empty=False, counts=r["n_inliers"][h0:h1], pose=r["pose"][h0:h1],
                          words=r["mask_words"][r["word_off"][k]:r["word_off"][k + 1]].reshape(h1 - h0, w),
                          rec_hyp=[int(h) - int(h0) for h in r["rec_hyp"][r0:r1]], rec_counts=r["rec_n_inliers"][r0:r1],
                          rec_pose=r["rec_pose"][r0:r1],
                          rec_words=r["rec_mask_words"][r["rec_word_off"][k]:r["rec_word_off"][k + 1]].reshape(r1 - r0, w))

    def _vb(self, words):
        vb = np.zeros(self.n_keypoints, bool)
        vb[self.kp_indices[words_to_mask(words, self.N)]] = True  # :242-247
        return vb

    @staticmethod
    def _T(pose):
        T = np.eye(4, dtype=np.float32)
        T[:3, :3], T[:3, 3] = pose[:9].reshape(3, 3), pose[9:]
        return T

    def iterate(self, nIterations: int):
        """-> (Tcw [4, 4] float32 or None, bNoMore, vbInliers, nInliers), as the reference's iterate (:178-271)."""
        none = np.zeros(0, bool)
        if self.N < self.mRansacMinInliers:  # :186
            return None, True, none, 0
        if self._res is None:
            PnPsolver.solve_all([self])
        r = self._res
        cur = 0
        while self.mnIterations < self.mRansacMaxIts or cur < nIterations:  # :195: || as the reference writes it
            if self.mnIterations >= len(self.sets):
                raise IndexError("PnPsolver.iterate: out of supplied hypotheses")
            cur += 1
            h = self.mnIterations
            self.mnIterations += 1
            n = int(r["counts"][h])
            if n >= self.mRansacMinInliers:  # :222
                if n > self.mnBestInliers:  # :225
                    self.mnBestInliers, self._best_h = n, h
                    self._rec = r["rec_hyp"].index(h)
                if int(r["rec_counts"][self._rec]) > self.mRansacMinInliers:  # Refine() (:307)
                    k = self._rec
                    return self._T(r["rec_pose"][k]), False, self._vb(r["rec_words"][k]), int(r["rec_counts"][k])
        if self.mnIterations >= self.mRansacMaxIts:  # :254
            if self.mnBestInliers >= self.mRansacMinInliers:
                h = self._best_h
                return self._T(r["pose"][h]), True, self._vb(r["words"][h]), self.mnBestInliers
            return None, True, none, 0
        return None, False, none, 0

    def find(self):
        """-> (Tcw, vbInliers, nInliers) (:166-170)."""
        T, _, vb, n = self.iterate(self.mRansacMaxIts)
        return T, vb, n
