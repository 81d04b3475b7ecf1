"""Initializer::FindHomography / FindFundamental (src/Initializer.cc:141-255), the RANSAC of monocular map initialisation, on
the device (include/orbfe.h: orbfe_initializer_ransac*): every hypothesis of both models is evaluated in ONE kernel launch;
the scans over the scores (`currentScore > score`, :192, :248) and the choice RH > 0.40 (:124-131) are replayed on the host.
ReconstructH / ReconstructF, which run once on the winner, and the random stream of the 8-sets stay with the caller."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, ptr

INIT_OK, INIT_NONFINITE = 0, 1
MODEL_H, MODEL_F = 0, 1


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def initializer_normalize(keys_xy) -> np.ndarray:
    """Normalize (:852-904) over ALL keys [n, 2] of a frame -> T = (sX, sY, meanX, meanY) float64."""
    k = _f32(keys_xy).reshape(-1, 2)
    T = np.zeros(4, np.float64)
    check(_lib.load().orbfe_initializer_normalize(len(k), ptr(k), ptr(T)))
    return T


def initializer_sets_from_draws(n: int, draws) -> np.ndarray:
    """draws [H, 8], draws[h, j] in [0, n - j) = the RandomInt values of :100 -> sets [H, 8], the pairs the reference's
    selection without replacement (:93-108) takes."""
    d = _i32(draws).reshape(-1, 8)
    s = np.zeros((max(len(d), 1), 8), np.int32)
    check(_lib.load().orbfe_initializer_sets_from_draws(int(n), len(d), ptr(d), ptr(s)))
    return s[:len(d)]


def initializer_ransac_multi(pair_off, pairs, T1, T2, sigma, hyp_off, sets, device: int = 0):
    """orbfe_initializer_ransac_multi -> (score [H, 2], status [H, 2], n_inliers [H, 2], model [H, 2, 3, 3], h12 [H, 3, 3],
    mask_words, word_off [K + 1]); axis 1 is the model, MODEL_H / MODEL_F."""
    po, ho = _i32(pair_off).reshape(-1), _i32(hyp_off).reshape(-1)
    K = len(po) - 1
    if K < 0 or len(ho) != K + 1:
        raise ValueError("initializer_ransac_multi: pair_off and hyp_off must hold K + 1 entries")
    p = _f32(pairs).reshape(-1, 4)
    t1, t2, sg = _f64(T1).reshape(-1, 4), _f64(T2).reshape(-1, 4), _f32(sigma).reshape(-1)
    st = _i32(sets).reshape(-1, 8)
    N, H = len(p), len(st)
    if len(t1) != K or len(t2) != K or len(sg) != K:
        raise ValueError("initializer_ransac_multi: one T1 / T2 / sigma per problem")
    n_k, h_k = np.diff(po).astype(np.int64), np.diff(ho).astype(np.int64)
    total = int((2 * np.maximum(h_k, 0) * ((np.maximum(n_k, 0) + 31) // 32)).sum())
    score = np.zeros((max(H, 1), 2), np.float64)
    status = np.zeros((max(H, 1), 2), np.uint8)
    n_inl = np.zeros((max(H, 1), 2), np.int32)
    model = np.zeros((max(H, 1), 2, 3, 3), np.float64)
    h12 = np.zeros((max(H, 1), 3, 3), np.float64)
    words = np.zeros(max(total, 1), np.uint32)
    word_off = np.zeros(K + 1, np.int32)
    check(_lib.load().orbfe_initializer_ransac_multi(int(device), K, N, H, ptr(po), ptr(p), ptr(t1), ptr(t2), ptr(sg), ptr(ho),
                                                     ptr(st), ptr(score), ptr(status), ptr(n_inl), ptr(model), ptr(h12),
                                                     ptr(words), ptr(word_off)))
    return score[:H], status[:H], n_inl[:H], model[:H], h12[:H], words[:total], word_off


def initializer_ransac(pairs, T1, T2, sigma, sets, device: int = 0):
    """One problem (orbfe_initializer_ransac) -> (score [H, 2], status [H, 2], n_inliers [H, 2], model [H, 2, 3, 3],
    h12 [H, 3, 3], mask_words [H, 2, ceil(n / 32)])."""
    p = _f32(pairs).reshape(-1, 4)
    t1, t2 = _f64(T1).reshape(4), _f64(T2).reshape(4)
    st = _i32(sets).reshape(-1, 8)
    n, H = len(p), len(st)
    w = (n + 31) // 32
    score = np.zeros((max(H, 1), 2), np.float64)
    status = np.zeros((max(H, 1), 2), np.uint8)
    n_inl = np.zeros((max(H, 1), 2), np.int32)
    model = np.zeros((max(H, 1), 2, 3, 3), np.float64)
    h12 = np.zeros((max(H, 1), 3, 3), np.float64)
    words = np.zeros(max(H * 2 * w, 1), np.uint32)
    check(_lib.load().orbfe_initializer_ransac(int(device), n, ptr(p), ptr(t1), ptr(t2), float(sigma), H, ptr(st), ptr(score),
                                               ptr(status), ptr(n_inl), ptr(model), ptr(h12), ptr(words)))
    return score[:H], status[:H], n_inl[:H], model[:H], h12[:H], words[:H * 2 * w].reshape(H, 2, w)


def unpack_mask(words, n: int) -> np.ndarray:
    """mask words of one (set, model) -> bool [n] (pair i at bit i & 31 of word i >> 5)"""
    i = np.arange(n)
    return ((np.asarray(words, np.uint32)[i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def replay_scan(score, model: int):
    """:174-198 / :229-254 over score [H, 2]: (the first hypothesis whose score is strictly greater than the best so far,
    starting at 0.0, or -1; that score).  NaN > x is false: a NaN score is never taken."""
    best, s = -1, 0.0
    for h, cur in enumerate(np.asarray(score, np.float64)[:, model]):
        if cur > s:  # :192, :248
            best, s = h, float(cur)
    return best, s


class Initializer:
    """The reference's Initializer up to the choice of the model.  keys1 [n1, 2] = the reference frame's mvKeysUn points
    (:36), sigma, iterations (mMaxIterations) as the reference's constructor takes them.

    FindModels(keys2, vMatches12, draws) does what Initialize does from :57 to :127: compacts vMatches12 into mvMatches12,
    builds mvSets from the caller's RandomInt values (draws [iterations, 8], draws[h, j] in [0, N - j)), evaluates every
    hypothesis of both models in one device call and replays the two scans.  It returns a dict: H21, F21 (float64 [3, 3], or
    None where no hypothesis scored above 0), SH, SF, RH, choose_H (RH > 0.40), vbMatchesInliersH / F (bool [N], indexed like
    mvMatches12), mvMatches12 [N, 2] and mvSets.  The caller then runs its own unchanged ReconstructH / ReconstructF."""

    def __init__(self, keys1, sigma: float = 1.0, iterations: int = 200, device: int = 0):
        self.mvKeys1 = _f32(keys1).reshape(-1, 2)
        self.mSigma, self.mMaxIterations, self.device = float(sigma), int(iterations), int(device)
        self._T1 = initializer_normalize(self.mvKeys1) if len(self.mvKeys1) else None

    def FindModels(self, keys2, vMatches12, draws):
        keys2 = _f32(keys2).reshape(-1, 2)
        m = _i32(vMatches12).reshape(-1)
        if len(m) != len(self.mvKeys1):
            raise ValueError("Initializer.FindModels: one entry of vMatches12 per reference key")
        first = np.nonzero(m >= 0)[0]  # :64-73
        mvMatches12 = np.stack([first, m[first]], axis=1).astype(np.int32)
        if len(first) and int(m[first].max()) >= len(keys2):
            raise ValueError("Initializer.FindModels: a match outside keys2")
        N = len(mvMatches12)
        sets = initializer_sets_from_draws(N, _i32(draws).reshape(-1, 8))  # :93-108
        if len(sets) != self.mMaxIterations:
            raise ValueError("Initializer.FindModels: draws must hold [iterations, 8] values")
        pairs = np.concatenate([self.mvKeys1[mvMatches12[:, 0]], keys2[mvMatches12[:, 1]]], axis=1)
        T2 = initializer_normalize(keys2)  # :149-150: over all keys
        score, status, n_inl, model, h12, words = initializer_ransac(pairs, self._T1, T2, self.mSigma, sets, self.device)
        out = dict(mvMatches12=mvMatches12, mvSets=sets, score=score, status=status, n_inliers=n_inl)
        for mi, name in ((MODEL_H, "H"), (MODEL_F, "F")):
            best, s = replay_scan(score, mi)
            out["best" + name] = best
            out["S" + name] = s
            out[name + "21"] = model[best, mi].copy() if best >= 0 else None
            out["vbMatchesInliers" + name] = unpack_mask(words[best, mi], N) if best >= 0 else np.zeros(N, bool)
        with np.errstate(all="ignore"):
            out["RH"] = float(np.float64(out["SH"]) / (np.float64(out["SH"]) + np.float64(out["SF"])))  # :124
        out["choose_H"] = bool(out["RH"] > 0.40)  # :127
        return out
