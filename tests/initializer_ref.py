"""Reference restatement of one RANSAC hypothesis of Initializer::FindHomography / FindFundamental (src/Initializer.cc:
ComputeH21 :260-305, ComputeF21 :307-345, CheckHomography :350-436, CheckFundamental :444-526, Normalize :852-904) in numpy
float64 on inputs widened from float32, of the selection without replacement (:93-108) and of the two scans and the choice of
the model (:174-198, :229-254, :124-131); the scene builders of the Initializer tests, the guard band, the ill-conditioning rule
and the pass condition.

The null vectors come from numpy.linalg.svd (LAPACK), which shares nothing with the one-sided Jacobi routine of
csrc/initializer_math.h.  Where the null vector is not defined by the data the hypothesis is ILL-CONDITIONED and only status
and finiteness are compared:
    H: (s8 - s9) / s1 < ILL of the 16 x 9 matrix (s1 >= ... >= s9 its singular values);
    F: s8 / s1 < ILL of the 8 x 9 matrix, or (w2 - w3) / w1 < ILL of Fpre (the rank-2 step drops an undefined direction).
"""
from pathlib import Path

import numpy as np

OK, NONFINITE = 0, 1
MH, MF = 0, 1
ILL = 1e-6         # relative singular-value gap below which a hypothesis is ill-conditioned
GUARD = 1e-6       # relative distance of a chi-square from its threshold inside which a decision is not compared
ILL_CAP = 0.05     # of a scene's hypotheses
GUARD_CAP = 0.001  # of a scene's pair decisions
TH_H, TH_F, TH_SCORE_F = 5.991, 3.841, 5.991  # :378, :462-463

KCAM = np.array([[520.0, 0, 320.0], [0, 520.0, 240.0], [0, 0, 1.0]])
PAIR_COUNTS = (8, 31, 32, 33, 63, 64, 65, 129)
SET_COUNTS = (1, 3, 4, 5, 9)
KINDS = ("planar", "rotation", "general")


# ---------------------------------------------------------------------------------------------------------------------
def sets_from_draws(n, draws):
    """:93-108, literally: the list of available indices, the pick, swap-with-back, pop_back"""
    out = []
    for d in np.asarray(draws).reshape(-1, 8):
        avail = list(range(n))  # :95
        s = []
        for j in range(8):
            randi = int(d[j])
            assert 0 <= randi <= len(avail) - 1  # RandomInt(0, size - 1), :100
            s.append(avail[randi])     # :101-103
            avail[randi] = avail[-1]   # :105
            avail.pop()                # :106
        out.append(s)
    return np.array(out, np.int32).reshape(-1, 8)


def normalize(xy):
    """Normalize (:852-904) -> (sX, sY, meanX, meanY), float64, sequential sums"""
    xy = np.asarray(xy, np.float32).astype(np.float64).reshape(-1, 2)
    mean = np.cumsum(xy, axis=0)[-1] / len(xy)          # :861-868
    dev = np.cumsum(np.abs(xy - mean), axis=0)[-1] / len(xy)  # :876-886
    with np.errstate(all="ignore"):
        return np.array([1.0 / dev[0], 1.0 / dev[1], mean[0], mean[1]])  # :889-890


def T_matrix(t):
    return np.array([[t[0], 0, -t[2] * t[0]], [0, t[1], -t[3] * t[1]], [0, 0, 1.0]])  # :899-903


def cv_inv3(M):
    """cv::Mat::inv() of [..., 3, 3]: the adjugate over the determinant, the zero matrix where the determinant is exactly 0"""
    m = lambda i, j: M[..., i, j]
    c0, c1, c2 = m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1), m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2), m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0)
    det = m(0, 0) * c0 + m(0, 1) * c1 + m(0, 2) * c2
    adj = np.stack([c0, m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2), m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1),
                    c1, m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0), m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2),
                    c2, m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1), m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)], axis=-1).reshape(M.shape)
    with np.errstate(all="ignore"):
        inv = adj / det[..., None, None]
    inv[det == 0.0] = 0.0
    return inv


def _gap(num, den):
    with np.errstate(all="ignore"):
        g = num / den
    return np.where(np.isfinite(g), g, 0.0)


def solve(P, T1, T2, reverse=False, negate=False):
    """ComputeH21 / ComputeF21 and the un-normalisation for S sets at once.  P [S, 8, 4] float64 = u1 v1 u2 v2 of the 8 pairs.
    reverse: the 8 pairs in reversed order; negate: the null vectors negated (both leave the result unchanged but for
    rounding and the sign of the model)."""
    S = len(P)
    if reverse:
        P = P[:, ::-1]
    u1, v1 = (P[..., 0] - T1[2]) * T1[0], (P[..., 1] - T1[3]) * T1[1]  # :878-896
    u2, v2 = (P[..., 2] - T2[2]) * T2[0], (P[..., 3] - T2[3]) * T2[1]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    AH = np.empty((S, 16, 9))
    AH[:, 0::2] = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], axis=-1)   # :275-283
    AH[:, 1::2] = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], axis=-1)   # :285-293
    AF = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], axis=-1)  # :320-328
    sgn = -1.0 if negate else 1.0
    if S == 0:
        e = np.zeros((0, 3, 3))
        return dict(H21=e, H12=e, F21=e, illH=np.zeros(0, bool), illF=np.zeros(0, bool))
    _, sH, vtH = np.linalg.svd(AH, full_matrices=False)  # :301
    Hn = sgn * vtH[:, 8].reshape(S, 3, 3)                # :304
    illH = _gap(sH[:, 7] - sH[:, 8], sH[:, 0]) < ILL
    _, sF, vtF = np.linalg.svd(AF, full_matrices=True)   # :334
    Fpre = sgn * vtF[:, 8].reshape(S, 3, 3)              # :336
    U, w, Vt = np.linalg.svd(Fpre)                       # :339
    illF = (_gap(sF[:, 7], sF[:, 0]) < ILL) | (_gap(w[:, 1] - w[:, 2], w[:, 0]) < ILL)
    w = w.copy()
    w[:, 2] = 0.0                                        # :341
    Fn = (U * w[:, None, :]) @ Vt                        # :344
    T1m, T2m = T_matrix(T1), T_matrix(T2)
    H21 = np.linalg.inv(T2m) @ Hn @ T1m  # :151, :187
    H12 = cv_inv3(H21)                   # :188
    F21 = T2m.T @ Fn @ T1m               # :215, :244
    return dict(H21=H21, H12=H12, F21=F21, illH=illH, illF=illF)


def chi_h(H21, H12, pairs, sigma):
    """CheckHomography's two chi-squares [S, n] (:398-422)"""
    u1, v1, u2, v2 = (pairs[:, i][None] for i in range(4))
    inv_s2 = 1.0 / (float(sigma) * float(sigma))
    h, hi = (lambda i, j: H21[:, i, j][:, None]), (lambda i, j: H12[:, i, j][:, None])
    with np.errstate(all="ignore"):
        w = 1.0 / (hi(2, 0) * u2 + hi(2, 1) * v2 + hi(2, 2))
        a, b = (hi(0, 0) * u2 + hi(0, 1) * v2 + hi(0, 2)) * w, (hi(1, 0) * u2 + hi(1, 1) * v2 + hi(1, 2)) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_s2
        w = 1.0 / (h(2, 0) * u1 + h(2, 1) * v1 + h(2, 2))
        a, b = (h(0, 0) * u1 + h(0, 1) * v1 + h(0, 2)) * w, (h(1, 0) * u1 + h(1, 1) * v1 + h(1, 2)) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_s2
    return chi1, chi2


def chi_f(F21, pairs, sigma):
    """CheckFundamental's two chi-squares [S, n] (:484-512)"""
    u1, v1, u2, v2 = (pairs[:, i][None] for i in range(4))
    inv_s2 = 1.0 / (float(sigma) * float(sigma))
    f = lambda i, j: F21[:, i, j][:, None]
    with np.errstate(all="ignore"):
        a2, b2, c2 = f(0, 0) * u1 + f(0, 1) * v1 + f(0, 2), f(1, 0) * u1 + f(1, 1) * v1 + f(1, 2), f(2, 0) * u1 + f(2, 1) * v1 + f(2, 2)
        num2 = a2 * u2 + b2 * v2 + c2
        chi1 = num2 * num2 / (a2 * a2 + b2 * b2) * inv_s2
        a1, b1, c1 = f(0, 0) * u2 + f(1, 0) * v2 + f(2, 0), f(0, 1) * u2 + f(1, 1) * v2 + f(2, 1), f(0, 2) * u2 + f(1, 2) * v2 + f(2, 2)
        num1 = a1 * u1 + b1 * v1 + c1
        chi2 = num1 * num1 / (a1 * a1 + b1 * b1) * inv_s2
    return chi1, chi2


def score_of(chi1, chi2, th, th_score):
    """the `if (chi > th) bIn = false; else score += thScore - chi` form: a NaN chi takes the else branch"""
    with np.errstate(all="ignore"):
        inl = ~(chi1 > th) & ~(chi2 > th)
        score = (np.where(chi1 > th, 0.0, th_score - chi1) + np.where(chi2 > th, 0.0, th_score - chi2)).sum(axis=1)
        guard = (np.abs(chi1 - th) <= GUARD * th) | (np.abs(chi2 - th) <= GUARD * th)
    return inl, score, guard


def score_float32(model, h12, pairs, sigma, is_h):
    """A literal float32 transcription of the scoring loop (:376-435, :460-525) for ONE hypothesis: every operation in
    float, the pairs in order."""
    f32 = np.float32
    m, mi = model.astype(f32).reshape(9), (h12.astype(f32).reshape(9) if is_h else None)
    score = f32(0)
    inv = f32(1.0 / (float(f32(sigma)) * float(f32(sigma))))
    th, ths = (f32(5.991), f32(5.991)) if is_h else (f32(3.841), f32(5.991))
    with np.errstate(all="ignore"):
        for u1, v1, u2, v2 in pairs.astype(f32):
            if is_h:
                w = f32(1.0) / (mi[6] * u2 + mi[7] * v2 + mi[8])
                a, b = (mi[0] * u2 + mi[1] * v2 + mi[2]) * w, (mi[3] * u2 + mi[4] * v2 + mi[5]) * w
                c1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv
                w = f32(1.0) / (m[6] * u1 + m[7] * v1 + m[8])
                a, b = (m[0] * u1 + m[1] * v1 + m[2]) * w, (m[3] * u1 + m[4] * v1 + m[5]) * w
                c2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv
            else:
                a2, b2, cc2 = m[0] * u1 + m[1] * v1 + m[2], m[3] * u1 + m[4] * v1 + m[5], m[6] * u1 + m[7] * v1 + m[8]
                n2 = a2 * u2 + b2 * v2 + cc2
                c1 = n2 * n2 / (a2 * a2 + b2 * b2) * inv
                a1, b1, cc1 = m[0] * u2 + m[3] * v2 + m[6], m[1] * u2 + m[4] * v2 + m[7], m[2] * u2 + m[5] * v2 + m[8]
                n1 = a1 * u1 + b1 * v1 + cc1
                c2 = n1 * n1 / (a1 * a1 + b1 * b1) * inv
            if not c1 > th:
                score = f32(score + (ths - c1))
            if not c2 > th:
                score = f32(score + (ths - c2))
    return float(score)


def run(sc, reverse=False, negate=False):
    """Every (set, model) of the scene -> dict(score [H, 2], status [H, 2], n_inliers [H, 2], model [H, 2, 3, 3], h12 [H, 3, 3],
    masks / guard (per set a pair [H-model, F-model] of bool [n_k]), ill [H, 2], prob [H])."""
    score, status, n_inl, model, h12, masks, guards, ill, prob = [], [], [], [], [], [], [], [], []
    for k, p in enumerate(sc["probs"]):
        S = len(p["sets"])
        if S == 0:
            continue
        pairs = p["pairs"].astype(np.float64)
        s = solve(pairs[p["sets"]], p["T1"], p["T2"], reverse, negate)
        cH, cF = chi_h(s["H21"], s["H12"], pairs, p["sigma"]), chi_f(s["F21"], pairs, p["sigma"])
        iH, sH, gH = score_of(*cH, TH_H, TH_H)
        iF, sF, gF = score_of(*cF, TH_F, TH_SCORE_F)
        badH = ~(np.isfinite(sH) & np.isfinite(s["H21"]).all((1, 2)) & np.isfinite(s["H12"]).all((1, 2)))
        badF = ~(np.isfinite(sF) & np.isfinite(s["F21"]).all((1, 2)))
        iH, gH, iF, gF = iH & ~badH[:, None], gH & ~badH[:, None], iF & ~badF[:, None], gF & ~badF[:, None]
        score.append(np.stack([sH, sF], axis=1)); status.append(np.stack([badH, badF], axis=1).astype(np.uint8))
        n_inl.append(np.stack([iH.sum(1), iF.sum(1)], axis=1)); model.append(np.stack([s["H21"], s["F21"]], axis=1)); h12.append(s["H12"])
        masks += [(iH[h], iF[h]) for h in range(S)]; guards += [(gH[h], gF[h]) for h in range(S)]
        ill.append(np.stack([s["illH"], s["illF"]], axis=1)); prob += [k] * S
    cat = lambda a, shape, dt: np.concatenate(a).astype(dt) if a else np.zeros(shape, dt)
    return dict(score=cat(score, (0, 2), np.float64), status=cat(status, (0, 2), np.uint8), n_inliers=cat(n_inl, (0, 2), np.int32),
                model=cat(model, (0, 2, 3, 3), np.float64), h12=cat(h12, (0, 3, 3), np.float64), masks=masks, guard=guards,
                ill=cat(ill, (0, 2), bool), prob=np.array(prob, np.int32))


def replay(score, model):
    """:174-198 / :229-254: the first hypothesis whose score is strictly greater than the best so far, from 0.0"""
    best, s = -1, 0.0
    for h in range(len(score)):
        if score[h, model] > s:
            best, s = h, float(score[h, model])
    return best, s


def choose(SH, SF):
    """:124-127 -> (RH, RH > 0.40)"""
    with np.errstate(all="ignore"):
        RH = float(np.float64(SH) / (np.float64(SH) + np.float64(SF)))
    return RH, RH > 0.40


# ---------------------------------------------------------------------------------------------------------------------
def _rot(axis, deg):
    a = np.deg2rad(deg)
    k = np.asarray(axis, float) / np.linalg.norm(axis)
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


R21 = _rot([0.2, 0.9, -0.3], 6.0)
T21 = np.array([0.35, -0.05, 0.25])  # (a z component: the two epipolar distances of a pair differ)
PLANE_N, PLANE_D = np.array([0.1, -0.15, 1.0]), 4.0  # n . X = d


def plant(kind):
    """(R, t) from camera 1 to camera 2 and, where the scene has one, the homography x2 ~ H x1 in pixels"""
    Ki = np.linalg.inv(KCAM)
    if kind == "rotation":
        return R21, np.zeros(3), KCAM @ R21 @ Ki
    if kind == "planar":
        return R21, T21, KCAM @ (R21 + np.outer(T21, PLANE_N) / PLANE_D) @ Ki
    return R21, T21, None


def fundamental():
    tx = np.array([[0, -T21[2], T21[1]], [T21[2], 0, -T21[0]], [-T21[1], T21[0], 0]])
    Ki = np.linalg.inv(KCAM)
    return Ki.T @ tx @ R21 @ Ki


def points(rng, kind, n):
    """n pairs (u1 v1 u2 v2, float64) of a scene kind, exact"""
    uv = np.stack([rng.uniform(40.0, 600.0, n), rng.uniform(30.0, 450.0, n), np.ones(n)], axis=1)
    ray = uv @ np.linalg.inv(KCAM).T
    depth = PLANE_D / (ray @ PLANE_N) if kind == "planar" else rng.uniform(2.0, 8.0, n)
    X1 = ray * depth[:, None]
    R, t, _ = plant(kind)
    x2 = (X1 @ R.T + t) @ KCAM.T
    return np.concatenate([uv[:, :2], x2[:, :2] / x2[:, 2:]], axis=1)


def problem(rng, kind, n, S, sigma=1.0, outliers=0.0, engineered=False):
    """One Initialize's inputs: n pairs of a scene kind -- inliers exact up to the float32 rounding of the coordinates,
    outliers with their second point displaced by 20-60 px -- T1 / T2 of Normalize over the matched keys and 40 unmatched ones,
    S sets drawn the reference's way.  engineered (general, n >= 60, S >= 8): pairs 0-31 and sets 0-4 are the cases of
    ENGINEERED, and T1 / T2 have their means at the coincident point."""
    P = points(rng, kind, n)
    inlier = rng.uniform(0, 1, n) >= outliers
    tags = {}
    if engineered:
        assert kind == "general" and n >= 60 and S >= 8
        inlier[:33] = [0] * 8 + [1] * 8 + [1] * 8 + [0] * 8 + [1]  # (32: not an outlier of the scene; see below)
        P[0:8] = [100.0, 200.0, 130.0, 180.0]              # 0-7: eight indices, one pair of coordinates
        line = np.stack([np.linspace(60, 560, 8), np.linspace(50, 400, 8), np.ones(8)], axis=1)
        X = (line @ np.linalg.inv(KCAM).T) * 4.0            # 8-15: collinear in space, hence in both images
        x2 = (X @ R21.T + T21) @ KCAM.T
        P[8:16] = np.concatenate([line[:, :2], x2[:, :2] / x2[:, 2:]], axis=1)
        # 16-23: inliers; 24-31: outliers (displaced below)
    out = np.nonzero(~inlier)[0]
    out = out[out >= 8] if engineered else out
    ang = rng.uniform(0, 2 * np.pi, len(out))
    P[out, 2:] += (rng.uniform(20.0, 60.0, len(out)) * np.array([np.cos(ang), np.sin(ang)])).T
    between = None
    if engineered:
        # pair 32: x2 displaced across its epipolar line so that ONE of the two chi-squares lies in (3.841, 5.991) and the
        # other below 3.841 (module function between_pair)
        P[32], between = between_pair(points(rng, kind, 400), sigma)
    pairs = P.astype(np.float32)
    extra = np.stack([rng.uniform(0, 640, 40), rng.uniform(0, 480, 40)], axis=1)
    T1 = normalize(np.concatenate([pairs[:, :2], extra]))
    T2 = normalize(np.concatenate([pairs[:, 2:], extra[::-1]]))
    if engineered:
        T1[2:], T2[2:] = pairs[0, :2], pairs[0, 2:]  # the means ARE the coincident point: its normalised coordinates are 0
    draws = np.stack([rng.integers(0, n - j, S) for j in range(8)], axis=1) if S else np.zeros((0, 8), np.int64)
    sets = sets_from_draws(n, draws) if S else np.zeros((0, 8), np.int32)
    if engineered:
        for h, (name, st) in enumerate(ENGINEERED.items()):
            sets[h] = st
            tags[h] = name
    return dict(kind=kind, n=n, pairs=pairs, T1=T1, T2=T2, sigma=float(sigma), sets=sets, inlier=inlier, tags=tags, between=between)


def between_pair(p, sigma):
    """p = candidate exact pairs of the general scene -> (one of them with x2 moved d pixels along the normal of its epipolar line
    l2 = F x1, (chi-square in image 2, chi-square in image 1)): d^2 / sigma^2 = 4.4 in the image whose distance is the larger,
    which leaves the smaller one near 3.4 for the best candidate's ratio of 0.77.
    The two distances share the numerator x2^T F x1 and differ by |l2|^2 / |l1|^2, which T21's z component keeps away from 1."""
    F = fundamental()

    def moved(c, d):
        l2 = F @ np.array([c[0], c[1], 1.0])
        q = c.copy()
        q[2:] += d * l2[:2] / np.linalg.norm(l2[:2])
        c1, c2 = chi_f(F[None], q[None], sigma)
        return q, float(c1[0, 0]), float(c2[0, 0])
    ratio = []
    for c in p:  # the candidate whose two distances differ most
        _, c1, c2 = moved(c, sigma)
        ratio.append(min(c1, c2) / max(c1, c2))
    c = p[int(np.argmin(ratio))]
    for d in np.linspace(0.5, 4.0, 351) * sigma:
        q, c1, c2 = moved(c, d)
        if max(c1, c2) >= 4.4:
            return q, (c1, c2)
    raise AssertionError("between_pair: no displacement found")


# set -> its eight pairs, in an engineered problem
ENGINEERED = {"coincident": tuple(range(0, 8)), "collinear": tuple(range(8, 16)), "inliers": tuple(range(16, 24)),
              "outliers": tuple(range(24, 32)), "inliers-permuted": (23, 16, 22, 17, 21, 18, 20, 19)}
DEGENERATE = ("coincident", "collinear")  # the null vector is not defined by the data: status and finiteness alone


def _outliers(kind, n):
    return 0.3 if kind == "general" and n >= 31 else 0.0


def specs():
    for kind in KINDS:
        for n in PAIR_COUNTS:
            S = SET_COUNTS[PAIR_COUNTS.index(n) % len(SET_COUNTS)]
            for sigma in (1.0, 2.0):
                yield f"{kind}-n{n}-S{S}-s{sigma:g}", dict(probs=[dict(kind=kind, n=n, S=S, sigma=sigma, outliers=_outliers(kind, n))])
    for S in SET_COUNTS:  # every set count at one pair count as well
        yield f"general-n65-S{S}-sets", dict(probs=[dict(kind="general", n=65, S=S, sigma=1.0, outliers=0.3)])
    yield "general-n300-S200", dict(probs=[dict(kind="general", n=300, S=200, sigma=1.0, outliers=0.3)])  # mMaxIterations
    empty = dict(kind="general", n=0, S=0)
    a, b = dict(kind="general", n=65, S=9, sigma=1.0, outliers=0.3), dict(kind="planar", n=33, S=5, sigma=2.0, outliers=0.0)
    yield "K3-empty-first", dict(probs=[empty, a, b])
    yield "K3-empty-middle", dict(probs=[a, empty, b])
    yield "K3-empty-last", dict(probs=[a, b, empty])
    for sigma in (1.0, 2.0):
        yield f"engineered-s{sigma:g}", dict(probs=[dict(kind="general", n=129, S=12, sigma=sigma, outliers=0.3, engineered=True)])


SEED = 0  # keeps every scene within the caps (tests/test_initializer_ref.py asserts it)


def build(id_, spec):
    rng = np.random.default_rng(SEED)
    probs = []
    for c in spec["probs"]:
        if c["n"] == 0:
            probs.append(dict(kind=c["kind"], n=0, pairs=np.zeros((0, 4), np.float32), T1=np.array([1.0, 1.0, 0.0, 0.0]),
                              T2=np.array([1.0, 1.0, 0.0, 0.0]), sigma=1.0, sets=np.zeros((0, 8), np.int32), inlier=np.zeros(0, bool),
                              tags={}, between=None))
        else:
            probs.append(problem(rng, **c))
    return dict(probs=probs)


def gpu_scenes():
    """(id, scene) of every scene the GPU test runs."""
    return [(id_, build(id_, spec)) for id_, spec in specs()]


def exempt(id_):
    """the engineered scene is exempt from the ill-conditioning cap, by name"""
    return id_.startswith("engineered")


def defined(sc, r):
    """[H, 2] bool: the (set, model)s whose model the scene kind defines.  A planar or pure-rotation problem has no fundamental
    matrix: every F of it is ill-conditioned by construction and is compared by status and finiteness, so it does not count
    towards the cap."""
    kinds = np.array([p["kind"] for p in sc["probs"]])[r["prob"]] if len(r["prob"]) else np.zeros(0, str)
    d = np.ones(r["ill"].shape, bool)
    d[:, MF] = kinds == "general"
    return d


def caps(sc, r):
    """(ill-conditioned (set, model)s among the defined ones, defined (set, model)s, guard-band decisions, decisions)"""
    d = defined(sc, r)
    return (int((r["ill"] & d).sum()), int(d.sum()), int(sum(g[0].sum() + g[1].sum() for g in r["guard"])),
            int(sum(g[0].size + g[1].size for g in r["guard"])))


# ---------------------------------------------------------------------------------------------------------------------
def operands(sc):
    """the flat arrays of orbfe_initializer_ransac_multi"""
    ps = sc["probs"]
    return dict(pair_off=np.concatenate([[0], np.cumsum([p["n"] for p in ps])]).astype(np.int32),
                hyp_off=np.concatenate([[0], np.cumsum([len(p["sets"]) for p in ps])]).astype(np.int32),
                pairs=np.concatenate([p["pairs"] for p in ps]).astype(np.float32), T1=np.stack([p["T1"] for p in ps]),
                T2=np.stack([p["T2"] for p in ps]), sigma=np.array([p["sigma"] for p in ps], np.float32),
                sets=np.concatenate([p["sets"] for p in ps]).astype(np.int32))


def word_offsets(sc):
    return np.concatenate([[0], np.cumsum([2 * len(p["sets"]) * ((p["n"] + 31) // 32) for p in sc["probs"]])]).astype(np.int32)


def unpack(words, n):
    i = np.arange(n)
    return ((np.asarray(words, np.uint32)[i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


TOLERANCE_FILE = Path(__file__).resolve().parent.parent / "profiles" / "initializer_tolerance.txt"


def recorded():
    """The restatement's own noise (s_model, s_score) as tests/test_initializer_ref.py measured and recorded it."""
    d = dict(t.split("=") for t in TOLERANCE_FILE.read_text().split() if "=" in t)
    return float(d["s_model"]), float(d["s_score"])


F32_2ULP = 2.0 * 2.0 ** -23  # 2 float32 ulps, relative


def allowance(s):
    """max(2 float32 ulps relative, 16 s)"""
    return max(F32_2ULP, 16.0 * s)


def model_distance(a, b):
    """relative distance of models [..., 3, 3] in Frobenius norm after scaling each to unit norm and fixing the sign"""
    a, b = np.asarray(a, np.float64).reshape(-1, 9), np.asarray(b, np.float64).reshape(-1, 9)
    with np.errstate(all="ignore"):
        a, b = a / np.linalg.norm(a, axis=1)[:, None], b / np.linalg.norm(b, axis=1)[:, None]
        sg = np.where((a * b).sum(1) < 0, -1.0, 1.0)
        return np.linalg.norm(a * sg[:, None] - b, axis=1)


def score_distance(a, b):
    """relative difference of scores; 0 where they are equal (a score of 0 included)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    with np.errstate(all="ignore"):
        return np.where(a == b, 0.0, np.abs(a - b) / np.abs(b))


def compare(id_, sc, r, score, status, n_inliers, model, h12, words, word_off, tol):
    """The pass condition of the Initializer tests; r = run(sc), tol = (allowance(s_model), allowance(s_score)).  Returns
    dict(ill, guard, differ, d_model, d_score): hypotheses not compared, guard-band decisions, decisions that differ inside the
    guard band, the largest model and score distances observed."""
    assert np.array_equal(word_off, word_offsets(sc)), id_
    H = len(r["status"])
    score, status, n_inliers = np.asarray(score).reshape(H, 2), np.asarray(status).reshape(H, 2), np.asarray(n_inliers).reshape(H, 2)
    model, h12 = np.asarray(model).reshape(H, 2, 3, 3), np.asarray(h12).reshape(H, 3, 3)
    assert len(words) == word_off[-1], id_
    fin = np.isfinite(score) & np.isfinite(model).all((2, 3))
    fin[:, MH] &= np.isfinite(h12).all((1, 2))
    assert np.array_equal(fin, status == OK), id_  # finite exactly where the status says so
    skip = r["ill"].copy()
    n_guard = n_diff = 0
    extra = np.zeros((H, 2))  # what guard-band decisions may move a score by
    h = 0
    for k, p in enumerate(sc["probs"]):
        w, w0 = (p["n"] + 31) // 32, int(word_off[k])
        for j in range(len(p["sets"])):
            for m in (MH, MF):
                wd = words[w0 + (2 * j + m) * w: w0 + (2 * j + m + 1) * w]
                mask = unpack(wd, p["n"])
                bits = sum(bin(int(x)).count("1") for x in wd)
                assert bits == mask.sum() == n_inliers[h, m], (id_, h, m)  # the count is the mask's; no bit beyond pair n - 1
                if status[h, m] == NONFINITE:
                    assert n_inliers[h, m] == 0 and not wd.any(), (id_, h, m)
                if p["tags"].get(j) in DEGENERATE:
                    skip[h, m] = True
                if skip[h, m]:
                    continue
                assert status[h, m] == r["status"][h, m], (id_, h, m)
                if status[h, m] == OK:
                    g = r["guard"][h][m]
                    diff = mask != r["masks"][h][m]
                    assert not (diff & ~g).any(), (id_, h, m, np.nonzero(diff & ~g)[0][:5])
                    assert abs(int(n_inliers[h, m]) - int(r["n_inliers"][h, m])) <= int(g.sum()), (id_, h, m)
                    n_guard += int(g.sum()); n_diff += int(diff.sum())
                    extra[h, m] = g.sum() * (TH_SCORE_F - TH_F if m == MF else 0.0)
            h += 1
    cmp = ~skip & (r["status"] == OK)
    d_model = model_distance(model[cmp], r["model"][cmp])
    assert (d_model <= tol[0]).all(), (id_, "model", float(d_model.max()), tol[0])
    cmp_h = cmp[:, MH]
    d_h12 = model_distance(h12[cmp_h], r["h12"][cmp_h])
    assert (d_h12 <= tol[0] * 1e3).all(), (id_, "h12", float(d_h12.max()))  # an inverse: the model's distance times cond(H)
    with np.errstate(all="ignore"):
        d_score = np.maximum(np.abs(score[cmp] - r["score"][cmp]) - extra[cmp], 0.0) / np.abs(r["score"][cmp])
    d_score = np.where(r["score"][cmp] == 0.0, np.abs(score[cmp]), d_score)
    assert (d_score <= tol[1]).all(), (id_, "score", float(d_score.max()), tol[1])
    return dict(ill=int(skip.sum()), guard=n_guard, differ=n_diff, d_model=float(d_model.max()) if d_model.size else 0.0,
                d_score=float(d_score.max()) if d_score.size else 0.0)


def write_scene(path, sc):
    """The scene as the text file tests/cpp/initializer_scene.h reads: whitespace-separated numbers, floats as their float32
    and doubles as their float64 bit patterns in hex."""
    def fl(a):
        return " ".join(f"{int(b):08x}" for b in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))

    def db(a):
        return " ".join(f"{int(b):016x}" for b in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))
    lines = [f"{len(sc['probs'])}"]
    for p in sc["probs"]:
        lines += [f"{p['n']} {len(p['sets'])}", fl([p["sigma"]]), db(p["T1"]), db(p["T2"]), fl(p["pairs"]),
                  " ".join(str(int(i)) for i in p["sets"].reshape(-1))]
    Path(path).write_text("\n".join(lines) + "\n")


def read_result(path, H):
    """What the programs write: score [H * 2] and model [H * 18] and h12 [H * 9] as float64 bit patterns, status [H * 2],
    n_inliers [H * 2], the number of mask words and the words in hex, then whatever else as integers."""
    tok = Path(path).read_text().split()
    at = 0

    def take(n, conv):
        nonlocal at
        out = [conv(t) for t in tok[at:at + n]]
        at += n
        return out
    hx = lambda t: int(t, 16)
    score = np.array(take(2 * H, hx), np.uint64).view(np.float64).reshape(H, 2)
    model = np.array(take(18 * H, hx), np.uint64).view(np.float64).reshape(H, 2, 3, 3)
    h12 = np.array(take(9 * H, hx), np.uint64).view(np.float64).reshape(H, 3, 3)
    status = np.array(take(2 * H, int), np.uint8).reshape(H, 2)
    n_inl = np.array(take(2 * H, int), np.int32).reshape(H, 2)
    W = take(1, int)[0]
    words = np.array(take(W, hx), np.uint32).reshape(W)
    rest = [int(t) for t in tok[at:]]
    return score, status, n_inl, model, h12, words, rest
