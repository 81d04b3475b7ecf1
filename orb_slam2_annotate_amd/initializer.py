"""Initializer::FindHomography / FindFundamental (src/Initializer.cc:141-255), the RANSAC of monocular map initialisation, on
the device (include/orbfe.h: orbfe_initializer_ransac*): every hypothesis of both models is evaluated in ONE kernel launch;
the scans over the scores (`currentScore > score`, :192, :248) and the choice RH > 0.40 (:124-131) are replayed on the host.
ReconstructH / ReconstructF (:536-824) follow on the device as well (orbfe_initializer_reconstruct*): the 8 or 4 motion
hypotheses of the chosen model and CheckRT of each over the inlier pairs in ONE launch; their tails (the clear-winner tests and
the parallax, :568-641, :778-823) are replayed on the host.  Initializer.Initialize returns what the reference's Initialize
returns.  Only the random stream of the 8-sets stays with the caller."""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import check, ptr

INIT_OK, INIT_NONFINITE = 0, 1
MODEL_H, MODEL_F = 0, 1
RECON_OK, RECON_NONFINITE = 0, 1
RECON_PROBLEM_OK, RECON_DEGENERATE = 0, 1
RECON_COUNTED, RECON_GOOD = 1, 2  # bits of pair_flags


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


def pack_mask(mask) -> np.ndarray:
    """bool [n] -> its ceil(n / 32) mask words"""
    m = np.asarray(mask, bool).reshape(-1)
    w = np.zeros((len(m) + 31) // 32, np.uint32)
    i = np.nonzero(m)[0]
    np.bitwise_or.at(w, i >> 5, (np.uint32(1) << (i & 31).astype(np.uint32)))
    return w


def initializer_reconstruct_multi(pair_off, pairs, model_kind, model, K4, sigma, inlier_words, in_word_off, device: int = 0):
    """orbfe_initializer_reconstruct_multi -> dict(hyp_off [K + 1], slot_off [K + 1], R [G, 3, 3], t [G, 3], n_good [G],
    cos_sel [G], hyp_status [G], x3d [S, 3], pair_flags [S], problem_status [K], n_inliers [K]); hypothesis g of problem k and
    its pair i are at slot slot_off[k] + (g - hyp_off[k]) * n_k + i."""
    po, wo = _i32(pair_off).reshape(-1), _i32(in_word_off).reshape(-1)
    K = len(po) - 1
    if K < 0 or len(wo) != K + 1:
        raise ValueError("initializer_reconstruct_multi: pair_off and in_word_off must hold K + 1 entries")
    p = _f32(pairs).reshape(-1, 4)
    kind, md = _i32(model_kind).reshape(-1), _f64(model).reshape(-1, 9)
    k4, sg = _f32(K4).reshape(-1, 4), _f32(sigma).reshape(-1)
    words = np.ascontiguousarray(inlier_words, dtype=np.uint32).reshape(-1)
    if not (len(kind) == len(md) == len(k4) == len(sg) == K):
        raise ValueError("initializer_reconstruct_multi: one model_kind / model / K4 / sigma per problem")
    nh = np.where(kind == MODEL_H, 8, 4).astype(np.int64)
    G, S = int(nh.sum()), int((nh * np.maximum(np.diff(po).astype(np.int64), 0)).sum())
    out = dict(hyp_off=np.zeros(K + 1, np.int32), slot_off=np.zeros(K + 1, np.int32), R=np.zeros((max(G, 1), 3, 3)),
               t=np.zeros((max(G, 1), 3)), n_good=np.zeros(max(G, 1), np.int32), cos_sel=np.zeros(max(G, 1)),
               hyp_status=np.zeros(max(G, 1), np.uint8), x3d=np.zeros((max(S, 1), 3)), pair_flags=np.zeros(max(S, 1), np.uint8),
               problem_status=np.zeros(max(K, 1), np.uint8), n_inliers=np.zeros(max(K, 1), np.int32))
    check(_lib.load().orbfe_initializer_reconstruct_multi(
        int(device), K, len(p), len(words), ptr(po), ptr(p), ptr(kind), ptr(md), ptr(k4), ptr(sg), ptr(words), ptr(wo),
        *[ptr(out[k]) for k in ("hyp_off", "slot_off", "R", "t", "n_good", "cos_sel", "hyp_status", "x3d", "pair_flags",
                                "problem_status", "n_inliers")]))
    for k in ("R", "t", "n_good", "cos_sel", "hyp_status"):
        out[k] = out[k][:G]
    out["x3d"], out["pair_flags"] = out["x3d"][:S], out["pair_flags"][:S]
    out["problem_status"], out["n_inliers"] = out["problem_status"][:K], out["n_inliers"][:K]
    return out


def initializer_reconstruct(pairs, model_kind: int, model, K4, sigma: float, inlier_words, device: int = 0):
    """One problem (orbfe_initializer_reconstruct) -> dict(R [g, 3, 3], t [g, 3], n_good [g], cos_sel [g], hyp_status [g],
    x3d [g, n, 3], pair_flags [g, n], problem_status, n_inliers), g = 8 (MODEL_H) or 4 (MODEL_F)."""
    p = _f32(pairs).reshape(-1, 4)
    md, k4 = _f64(model).reshape(9), _f32(K4).reshape(4)
    words = np.ascontiguousarray(inlier_words, dtype=np.uint32).reshape(-1)
    n = len(p)
    if len(words) != (n + 31) // 32:
        raise ValueError("initializer_reconstruct: inlier_words must hold ceil(n / 32) words")
    g = 8 if int(model_kind) == MODEL_H else 4
    out = dict(R=np.zeros((g, 3, 3)), t=np.zeros((g, 3)), n_good=np.zeros(g, np.int32), cos_sel=np.zeros(g),
               hyp_status=np.zeros(g, np.uint8), x3d=np.zeros((g, max(n, 1), 3)), pair_flags=np.zeros((g, max(n, 1)), np.uint8),
               problem_status=np.zeros(1, np.uint8), n_inliers=np.zeros(1, np.int32))
    if n == 0:
        words = np.zeros(1, np.uint32)  # (never read)
    check(_lib.load().orbfe_initializer_reconstruct(
        int(device), n, ptr(p) if n else None, int(model_kind), ptr(md), ptr(k4), float(sigma), ptr(words),
        *[ptr(out[k]) for k in ("R", "t", "n_good", "cos_sel", "hyp_status", "x3d", "pair_flags", "problem_status", "n_inliers")]))
    if n == 0:
        out["x3d"], out["pair_flags"] = np.zeros((g, 0, 3)), np.zeros((g, 0), np.uint8)
    out["problem_status"], out["n_inliers"] = int(out["problem_status"][0]), int(out["n_inliers"][0])
    return out


def parallax_degrees(n_good, cos_sel) -> float:
    """:1018-1026: acos(cos) * 180 / pi of the selected cosine, 0 when nGood == 0"""
    return float(np.degrees(np.arccos(np.float64(cos_sel)))) if int(n_good) > 0 else 0.0


def replay_reconstruct_f(N: int, n_good, parallax, minParallax: float = 1.0, minTriangulated: int = 50):
    """The tail of ReconstructF (:568-641) -> (success, the hypothesis taken or -1)"""
    g = [int(v) for v in n_good]
    maxGood = max(g)  # :568
    nMinGood = max(int(0.9 * N), minTriangulated)  # :575
    nsimilar = sum(1 for v in g if v > 0.7 * maxGood)  # :577-585
    if maxGood < nMinGood or nsimilar > 1:  # :589
        return False, -1
    for i in range(4):  # :595-639: the first hypothesis that equals maxGood, and only that one
        if maxGood == g[i]:
            return (True, i) if parallax[i] > minParallax else (False, -1)
    return False, -1


def replay_reconstruct_h(N: int, n_good, parallax, minParallax: float = 1.0, minTriangulated: int = 50):
    """The tail of ReconstructH (:778-823) -> (success, the hypothesis taken or -1)"""
    bestGood, secondBestGood, bestSolutionIdx, bestParallax = 0, 0, -1, -1.0
    for i in range(8):  # :788-810
        nGood = int(n_good[i])
        if nGood > bestGood:
            secondBestGood, bestGood, bestSolutionIdx, bestParallax = bestGood, nGood, i, parallax[i]
        elif nGood > secondBestGood:
            secondBestGood = nGood
    if secondBestGood < 0.75 * bestGood and bestParallax >= minParallax and bestGood > minTriangulated and bestGood > 0.9 * N:  # :813
        return True, bestSolutionIdx
    return False, -1


class Initializer:
    """The reference's Initializer.  keys1 [n1, 2] = the reference frame's mvKeysUn points
    (:36), sigma, iterations (mMaxIterations) as the reference's constructor takes them.

    FindModels(keys2, vMatches12, draws) does what Initialize does from :57 to :127: compacts vMatches12 into mvMatches12,
    builds mvSets from the caller's RandomInt values (draws [iterations, 8], draws[h, j] in [0, N - j)), evaluates every
    hypothesis of both models in one device call and replays the two scans.  It returns a dict: H21, F21 (float64 [3, 3], or
    None where no hypothesis scored above 0), SH, SF, RH, choose_H (RH > 0.40), vbMatchesInliersH / F (bool [N], indexed like
    mvMatches12), mvMatches12 [N, 2] and mvSets.

    Reconstruct(found, K) runs ReconstructH or ReconstructF (:129-131, minParallax 1.0, minTriangulated 50) on the model
    FindModels chose: one device call for the 8 or 4 hypotheses, then the replay of the tail.  K = the 3 x 3 camera matrix or
    (fx, fy, cx, cy).  It returns a dict: success, R21 [3, 3] and t21 [3] (None when not successful), vP3D (float32
    [n1, 3]) and vbTriangulated (bool [n1]), both indexed by the reference key (vMatches12[i].first), parallax, and the
    device's per-hypothesis results under "hypotheses".  Initialize(keys2, vMatches12, draws, K) is FindModels + Reconstruct and
    returns (success, R21, t21, vP3D, vbTriangulated) as the reference's Initialize does."""

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
        out["pairs"] = pairs
        return out

    def Reconstruct(self, found, K, minParallax: float = 1.0, minTriangulated: int = 50):
        K = np.asarray(K, np.float64)
        K4 = np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]], np.float32) if K.shape == (3, 3) else _f32(K).reshape(4)
        kind, name = (MODEL_H, "H") if found["choose_H"] else (MODEL_F, "F")
        n1 = len(self.mvKeys1)
        out = dict(success=False, R21=None, t21=None, vP3D=np.zeros((n1, 3), np.float32), vbTriangulated=np.zeros(n1, bool),
                   parallax=0.0, model_kind=kind, best=-1, hypotheses=None)
        if found[name + "21"] is None:  # an empty cv::Mat: the reference's SVD of it fails; nothing to reconstruct
            return out
        mask = np.asarray(found["vbMatchesInliers" + name], bool)
        r = initializer_reconstruct(found["pairs"], kind, found[name + "21"], K4, self.mSigma, pack_mask(mask), self.device)
        out["hypotheses"] = r
        if r["problem_status"] == RECON_DEGENERATE:  # :684-687
            return out
        par = [parallax_degrees(g, c) for g, c in zip(r["n_good"], r["cos_sel"])]
        ok, best = (replay_reconstruct_h if kind == MODEL_H else replay_reconstruct_f)(r["n_inliers"], r["n_good"], par,
                                                                                      minParallax, minTriangulated)
        if not ok:
            return out
        first = found["mvMatches12"][:, 0]
        counted = (r["pair_flags"][best] & RECON_COUNTED) != 0
        out["vP3D"][first[counted]] = r["x3d"][best][counted].astype(np.float32)             # :1011
        out["vbTriangulated"][first] = (r["pair_flags"][best] & RECON_GOOD) != 0              # :1014-1015
        out.update(success=True, R21=r["R"][best].copy(), t21=r["t"][best].copy(), parallax=par[best], best=best)
        return out

    def Initialize(self, keys2, vMatches12, draws, K):
        r = self.Reconstruct(self.FindModels(keys2, vMatches12, draws), K)
        return r["success"], r["R21"], r["t21"], r["vP3D"], r["vbTriangulated"]
