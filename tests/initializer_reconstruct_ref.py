"""Reference restatement of what Initializer::Initialize does after the choice of the model (src/Initializer.cc): ReconstructF
(:536-642) with DecomposeE (:1034-1057), ReconstructH (:653-824), Triangulate (:829-842) and CheckRT (:913-1029), in numpy
float64 on inputs widened from float32, with numpy.linalg.svd (LAPACK) wherever the reference calls cv::SVD -- it shares nothing
with the Jacobi routines of csrc/initializer_reconstruct_math.h and csrc/triangulate_math.h.  Also: the scenes of the
reconstruct tests (built on the scene generator of tests/initializer_ref.py, with a camera K), the guard bands, the matching of
hypotheses and the pass condition.

The SVD's sign ambiguity permutes the hypotheses (H: flipping (u_0, v_0) swaps 0 <-> 2 and 1 <-> 3 within each group of four;
F: flipping u_2 swaps t <-> -t and R1 <-> R2), so a comparison first matches hypotheses by the bijection that minimises
|R - R'|_F + |t - t'| (within its group of four for H), requires every matched distance within the allowance and then compares
per-hypothesis results through that bijection.

Guard bands.  A pair is inside one if a compared quantity it reaches lies within GUARD relative of its threshold (the cosine
against 0.99998, z against 0 relative to |X|, a squared error against th2) or if its 4 x 4 null vector is ill-conditioned
((s3 - s4) / s1 < ILL).  A problem is inside one if d1/d2 or d2/d3 lies within GUARD of 1.00001 or a replay comparison is an
equality.  SEEDS[id] is the first seed from 0 for which the restatement has no pair and no problem inside a guard band; with
such seeds n_good, pair_flags and every replay decision must be EQUAL.
"""
import itertools
from pathlib import Path

import numpy as np

import initializer_ref as ir

MH, MF = 0, 1
OK, NONFINITE = 0, 1
P_OK, DEGENERATE = 0, 1
COUNTED, GOOD = 1, 2
COS_TH, SV_TH = 0.99998, 1.00001  # :977, :684
ILL = 1e-6
GUARD = 1e-6
K4 = np.array([ir.KCAM[0, 0], ir.KCAM[1, 1], ir.KCAM[0, 2], ir.KCAM[1, 2]], np.float32)
K4_DYADIC = np.array([512.0, 512.0, 256.0, 256.0], np.float32)  # every entry of K, K^-1 and of F below is a dyadic rational
SIZES = (1, 32, 33, 51, 52, 64, 65, 256, 257, 300)


def kmat(k4):
    fx, fy, cx, cy = (float(v) for v in np.asarray(k4, np.float32))
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])


def kinv(k4):
    fx, fy, cx, cy = (float(v) for v in np.asarray(k4, np.float32))
    return np.array([[1.0 / fx, 0, -cx / fx], [0, 1.0 / fy, -cy / fy], [0, 0, 1.0]])


# ---------------------------------------------------------------------------------------------------------------------
def svd3(A, negate=False):
    U, w, Vt = np.linalg.svd(A)
    return (-U, w, -Vt) if negate else (U, w, Vt)


def motions_h(H21, k4, negate=False):
    """:667-775 -> (list of 8 (R, t), or None when :684 holds; the problem's guard flag)"""
    A = kinv(k4) @ np.asarray(H21, np.float64) @ kmat(k4)  # :667-668
    U, w, Vt = svd3(A, negate)                              # :673
    V = Vt.T
    s = np.linalg.det(U) * np.linalg.det(V)                 # :677
    d1, d2, d3 = w
    with np.errstate(all="ignore"):
        r12, r23 = d1 / d2, d2 / d3
        guard = bool(abs(r12 - SV_TH) <= GUARD * SV_TH or abs(r23 - SV_TH) <= GUARD * SV_TH)
        if r12 < SV_TH or r23 < SV_TH:                      # :684
            return None, guard
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))  # :697-700
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        aux_stheta = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)  # :703
        ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        stheta = [aux_stheta, -aux_stheta, -aux_stheta, aux_stheta]
        out = []
        for i in range(4):  # :708-737
            Rp = np.eye(3)
            Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ctheta, -stheta[i], stheta[i], ctheta
            t = U @ (np.array([x1[i], 0.0, -x3[i]]) * (d1 - d3))
            out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
        aux_sphi = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)  # :740
        cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sphi = [aux_sphi, -aux_sphi, -aux_sphi, aux_sphi]
        for i in range(4):  # :745-775
            Rp = np.eye(3)
            Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sphi[i], -1.0, sphi[i], -cphi
            t = U @ (np.array([x1[i], 0.0, x3[i]]) * (d1 + d3))
            out.append((s * U @ Rp @ Vt, t / np.linalg.norm(t)))
    return out, guard


def motions_f(F21, k4, negate=False):
    """:546-566 with DecomposeE (:1034-1057) -> the 4 (R, t)"""
    E = kmat(k4).T @ np.asarray(F21, np.float64) @ kmat(k4)  # :546
    U, _, Vt = svd3(E, negate)                               # :1037
    t = U[:, 2] / np.linalg.norm(U[:, 2])                     # :1040-1041
    W = np.array([[0, -1.0, 0], [1.0, 0, 0], [0, 0, 1.0]])    # :1043-1046
    R1 = U @ W @ Vt
    if np.linalg.det(R1) < 0:
        R1 = -R1
    R2 = U @ W.T @ Vt
    if np.linalg.det(R2) < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]             # :563-566


def check_rt(R, t, k4, pairs, mask, sigma, reverse=False, f32=False):
    """CheckRT (:913-1029) of one hypothesis over the pairs whose mask bit is set -> dict(n_good, cos_sel, nonfinite, flags [n],
    X [n, 3], cos [n], guard [n] (the pair is inside a guard band)).  reverse: the rows of the 4 x 4 A in reversed order (the
    result is the same but for rounding).  f32: the decisions after the triangulation in float32 arithmetic."""
    ft = np.float32 if f32 else np.float64
    n = len(pairs)
    Kd = kmat(k4)
    fx, fy, cx, cy = Kd[0, 0], Kd[1, 1], Kd[0, 2], Kd[1, 2]
    P1 = np.c_[Kd, np.zeros(3)]
    P2 = Kd @ np.c_[R, t]          # :936-939
    O2 = -R.T @ t                  # :941
    th2 = 4.0 * float(np.float32(sigma)) * float(np.float32(sigma))
    p = np.asarray(pairs, np.float32).astype(np.float64).reshape(n, 4)
    A = np.stack([p[:, 0, None] * P1[2] - P1[0], p[:, 1, None] * P1[2] - P1[1],
                  p[:, 2, None] * P2[2] - P2[0], p[:, 3, None] * P2[2] - P2[1]], axis=1)  # :834-837
    out = dict(n_good=0, cos_sel=0.0, nonfinite=False, flags=np.zeros(n, np.uint8), X=np.zeros((n, 3)), cos=np.zeros(n),
               guard=np.zeros(n, bool))
    if n == 0 or not np.isfinite(A).all():
        return out
    if reverse:
        A = A[:, ::-1]
    _, sv, vt = np.linalg.svd(A)   # :840
    h = vt[:, 3]
    with np.errstate(all="ignore"):
        X = h[:, :3] / h[:, 3:]    # :842
        fin = np.isfinite(X).all(1)  # :958
        Xc, Rc, tc, O2c = X.astype(ft), R.astype(ft), t.astype(ft), O2.astype(ft)
        fxc, fyc, cxc, cyc, pc, th2c, cth = ft(fx), ft(fy), ft(cx), ft(cy), p.astype(ft), ft(th2), ft(COS_TH)
        n2 = Xc - O2c
        dist1, dist2 = np.sqrt((Xc * Xc).sum(1)), np.sqrt((n2 * n2).sum(1))
        cos = (Xc * n2).sum(1) / (dist1 * dist2)  # :972
        z1 = Xc[:, 2]
        pass1 = ~((z1 <= 0) & (cos < cth))        # :977
        X2 = Xc @ Rc.T + tc                       # :981
        z2 = X2[:, 2]
        pass2 = ~((z2 <= 0) & (cos < cth))        # :983
        e1 = (fxc * Xc[:, 0] / z1 + cxc - pc[:, 0]) ** 2 + (fyc * Xc[:, 1] / z1 + cyc - pc[:, 1]) ** 2  # :988-992
        e2 = (fxc * X2[:, 0] / z2 + cxc - pc[:, 2]) ** 2 + (fyc * X2[:, 1] / z2 + cyc - pc[:, 3]) ** 2  # :1000-1004
        pass3, pass4 = ~(e1 > th2c), ~(e2 > th2c)  # :995, :1006
        m = np.asarray(mask, bool)
        r0 = m & fin
        r1, r2 = r0 & pass1, r0 & pass1 & pass2
        r3 = r2 & pass3
        counted = r3 & pass4
        good = counted & (cos < cth)              # :1014
        near = lambda a, b, scale: np.abs(a - b) <= GUARD * scale
        g = r0 & (near(cos, COS_TH, COS_TH) | near(z1, 0.0, dist1))
        g |= r1 & near(z2, 0.0, np.sqrt((X2 * X2).sum(1)))
        g |= r2 & near(e1, th2, th2)
        g |= r3 & near(e2, th2, th2)
        g |= m & ~(((sv[:, 2] - sv[:, 3]) / sv[:, 0]) >= ILL)
    out["flags"] = (counted * COUNTED + good * GOOD).astype(np.uint8)
    out["X"] = np.where(m[:, None], X, 0.0)
    out["cos"] = np.where(m, cos, 0.0).astype(np.float64)
    out["guard"] = g
    out["n_good"] = int(counted.sum())
    sel = np.sort(out["cos"][counted & np.isfinite(cos)])  # :1020
    out["nonfinite"] = bool(len(sel) != out["n_good"])
    if len(sel):
        out["cos_sel"] = float(sel[min(50, len(sel) - 1)])  # :1022
    return out


def parallax(n_good, cos_sel):
    """:1018-1026"""
    with np.errstate(all="ignore"):
        return float(np.degrees(np.arccos(cos_sel))) if n_good > 0 else 0.0


def replay_f(N, n_good, par, minParallax=1.0, minTriangulated=50):
    """:568-641 -> (success, hypothesis or -1, a comparison was an equality)"""
    maxGood = max(n_good)
    nMinGood = max(int(0.9 * N), minTriangulated)
    eq = any(g == 0.7 * maxGood for g in n_good) and maxGood > 0
    nsimilar = sum(1 for g in n_good if g > 0.7 * maxGood)
    if maxGood < nMinGood or nsimilar > 1:
        return False, -1, eq
    for i in range(4):
        if maxGood == n_good[i]:
            eq |= abs(par[i] - minParallax) <= GUARD * minParallax
            return (True, i, eq) if par[i] > minParallax else (False, -1, eq)
    return False, -1, eq


def replay_h(N, n_good, par, minParallax=1.0, minTriangulated=50):
    """:778-823"""
    best, second, idx, bpar = 0, 0, -1, -1.0
    for i in range(8):
        if n_good[i] > best:
            second, best, idx, bpar = best, n_good[i], i, par[i]
        elif n_good[i] > second:
            second = n_good[i]
    # (with best == 0 every count is 0 and `0 > 0` is the same in any arithmetic: no equality that rounding could decide)
    eq = best > 0 and (second == 0.75 * best or abs(bpar - minParallax) <= GUARD * minParallax or best == 0.9 * N)
    if second < 0.75 * best and bpar >= minParallax and best > minTriangulated and best > 0.9 * N:
        return True, idx, bool(eq)
    return False, -1, bool(eq)


def run_problem(p, reverse=False, negate=False, f32=False):
    """One problem p = dict(kind MH / MF, model, K4, sigma, pairs, mask) -> dict(status, guard (the problem is inside a guard
    band), hyps (list of check_rt results with R, t added), n_inliers, success, best, parallax, R21, t21, flags, X)"""
    mask = np.asarray(p["mask"], bool)
    N = int(mask.sum())
    nh = 8 if p["kind"] == MH else 4
    out = dict(status=P_OK, guard=False, hyps=[], n_inliers=N, success=False, best=-1, parallax=0.0, R21=None, t21=None)
    if p["kind"] == MH:
        mot, out["guard"] = motions_h(p["model"], p["K4"], negate)
        if mot is None:
            out["status"] = DEGENERATE
            n = len(p["pairs"])
            out["hyps"] = [dict(R=np.zeros((3, 3)), t=np.zeros(3), n_good=0, cos_sel=0.0, nonfinite=False, flags=np.zeros(n, np.uint8),
                                X=np.zeros((n, 3)), cos=np.zeros(n), guard=np.zeros(n, bool)) for _ in range(nh)]
            return out
    else:
        mot = motions_f(p["model"], p["K4"], negate)
    for R, t in mot:
        h = check_rt(R, t, p["K4"], p["pairs"], mask, p["sigma"], reverse, f32)
        h["R"], h["t"] = R, t
        out["hyps"].append(h)
    n_good = [h["n_good"] for h in out["hyps"]]
    par = [parallax(h["n_good"], h["cos_sel"]) for h in out["hyps"]]
    ok, best, eq = (replay_h if p["kind"] == MH else replay_f)(N, n_good, par)
    out["guard"] = bool(out["guard"] or eq)
    out.update(success=ok, best=best, par=par)
    if ok:
        out.update(parallax=par[best], R21=out["hyps"][best]["R"], t21=out["hyps"][best]["t"])
    return out


def run(sc, **kw):
    return [run_problem(p, **kw) for p in sc["probs"]]


def guard_count(r):
    """pairs and problems of a run inside a guard band"""
    return sum(int(h["guard"].sum()) for pr in r for h in pr["hyps"]), sum(int(pr["guard"]) for pr in r)


# ---------------------------------------------------------------------------------------------------------------------
def points_rt(rng, n, R, t, k4, depth=(2.0, 8.0)):
    """n exact pairs of a general scene seen by camera 1 = K [I | 0] and camera 2 = K [R | t]"""
    Kd = kmat(k4)
    uv = np.stack([rng.uniform(40.0, 600.0, n), rng.uniform(30.0, 450.0, n), np.ones(n)], axis=1)
    X1 = (uv @ np.linalg.inv(Kd).T) * rng.uniform(depth[0], depth[1], n)[:, None]
    x2 = (X1 @ R.T + t) @ Kd.T
    return np.concatenate([uv[:, :2], x2[:, :2] / x2[:, 2:]], axis=1)


def fundamental_rt(R, t, k4):
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = kinv(k4)
    return Ki.T @ tx @ R @ Ki


def problem(kind, model, pairs, mask, sigma=1.0, k4=K4, truth=None):
    return dict(kind=kind, model=np.asarray(model, np.float64), K4=np.asarray(k4, np.float32), sigma=float(sigma),
                pairs=np.asarray(pairs, np.float32).reshape(-1, 4), mask=np.asarray(mask, bool), truth=truth)


def _displace(rng, P, idx):
    ang = rng.uniform(0, 2 * np.pi, len(idx))
    P[idx, 2:] += (rng.uniform(20.0, 60.0, len(idx)) * np.array([np.cos(ang), np.sin(ang)])).T


def build(id_, seed):
    """The scene of an id: a list of problems.  Every sized scene holds a planar problem with the true H and a general one with
    the true F; the 7 and 3 wrong hypotheses of each are exercised with them."""
    rng = np.random.default_rng(seed)
    Hgen, Fgen = ir.plant("planar")[2], ir.fundamental()
    truth = (ir.R21, ir.T21 / np.linalg.norm(ir.T21))
    if id_[1:].isdigit():
        n = int(id_[1:])
        return dict(probs=[problem(MH, Hgen, ir.points(rng, "planar", n), np.ones(n, bool), truth=truth),
                           problem(MF, Fgen, ir.points(rng, "general", n), np.ones(n, bool), truth=truth)])
    if id_ == "zero-mask":
        return dict(probs=[problem(MH, Hgen, ir.points(rng, "planar", 40), np.zeros(40, bool)),
                           problem(MF, Fgen, ir.points(rng, "general", 40), np.zeros(40, bool))])
    if id_ == "interleaved":  # every third pair an outlier, displaced by 20-60 px: inliers straddle the word edges
        probs = []
        for kind, model, name in ((MH, Hgen, "planar"), (MF, Fgen, "general")):
            P = ir.points(rng, name, 100)
            mask = np.arange(100) % 3 != 0
            _displace(rng, P, np.nonzero(~mask)[0])
            probs.append(problem(kind, model, P, mask, truth=truth))
        return dict(probs=probs)
    if id_ == "rotation":  # no translation: H is K R K^-1 (:684 holds); under F every ray pair is parallel
        P = ir.points(rng, "rotation", 80)
        return dict(probs=[problem(MH, ir.plant("rotation")[2], P, np.ones(80, bool)), problem(MF, Fgen, P, np.ones(80, bool))])
    if id_ == "identity":
        P = ir.points(rng, "planar", 40)
        P[:, 2:] = P[:, :2]
        return dict(probs=[problem(MH, np.eye(3), P, np.ones(40, bool))])
    if id_ == "few":  # 40 accepted pairs: bestGood / maxGood do not reach minTriangulated = 50
        return dict(probs=[problem(MH, Hgen, ir.points(rng, "planar", 40), np.ones(40, bool), truth=truth),
                           problem(MF, Fgen, ir.points(rng, "general", 40), np.ones(40, bool), truth=truth)])
    if id_ == "nonfinite":
        # camera 2 = camera 1 moved along x, K dyadic: E = K^T F K is [t]x exactly and its SVD a signed permutation, so every
        # hypothesis has R = I or diag(1, -1, -1) and t = +-(1, 0, 0) exactly.  Pair 7 projects to the principal point in both
        # images (coincident projections): column 2 of its 4 x 4 A is exactly zero, the null vector is (0, 0, 1, 0) and
        # x3D[3] == 0: the point is (NaN, NaN, inf) under all four hypotheses.
        R, t = np.eye(3), np.array([1.0, 0.0, 0.0])
        P = points_rt(rng, 120, R, 0.3 * t, K4_DYADIC)
        P[7] = [256.0, 256.0, 256.0, 256.0]
        return dict(probs=[problem(MF, fundamental_rt(R, t, K4_DYADIC), P, np.ones(120, bool), k4=K4_DYADIC, truth=(R, t))])
    if id_ == "low-parallax":  # a short baseline: everything holds but parallax > minParallax
        # (a baseline along y at depths 3-4: every parallax lies between 0.36 degrees, where cos < 0.99998 begins, and 1 degree)
        R, t = ir.R21, np.array([0.0, 0.05, 0.0])
        P = points_rt(rng, 300, R, t, K4, depth=(3.0, 4.0))
        return dict(probs=[problem(MF, fundamental_rt(R, t, K4), P, np.ones(300, bool), truth=(R, t / np.linalg.norm(t)))])
    if id_ == "planar-unique":
        # The plane of tests/initializer_ref.py leaves Faugeras' two-fold ambiguity standing: both members of the pair accept
        # every point, secondBestGood == bestGood and ReconstructH returns false.  This plane and motion put a quarter and more
        # of the points behind a camera under the wrong member, so the reference's test has a winner.
        nrm, d, t = np.array([0.8, 0.3, 1.0]), 3.0, np.array([1.0, 0.2, -0.3])
        Ki = np.linalg.inv(ir.KCAM)
        uv = np.stack([rng.uniform(40.0, 600.0, 120), rng.uniform(30.0, 450.0, 120), np.ones(120)], axis=1)
        ray = uv @ Ki.T
        x2 = ((ray * (d / (ray @ nrm))[:, None]) @ ir.R21.T + t) @ ir.KCAM.T
        P = np.concatenate([uv[:, :2], x2[:, :2] / x2[:, 2:]], axis=1)
        return dict(probs=[problem(MH, ir.KCAM @ (ir.R21 + np.outer(t, nrm) / d) @ Ki, P, np.ones(120, bool),
                                   truth=(ir.R21, t / np.linalg.norm(t)))])
    raise KeyError(id_)


ENGINEERED = ("zero-mask", "interleaved", "rotation", "identity", "few", "nonfinite", "low-parallax", "planar-unique")
IDS = tuple(f"n{n}" for n in SIZES) + ENGINEERED
# the first seed from 0 without a pair or a problem inside a guard band (find_seed; tests/test_initializer_reconstruct_ref.py
# asserts it), recorded so that the scenes never move
SEEDS = {id_: 0 for id_ in IDS}
SEEDS.update({"n52": 1, "n257": 1, "interleaved": 2, "few": 1})


def find_seed(id_, limit=200):
    for seed in range(limit):
        if guard_count(run(build(id_, seed))) == (0, 0):
            return seed
    raise RuntimeError("no seed without a guard-band case")


_cache = {}


def scenes():
    """(id, scene, restatement's run) of every scene of the reconstruct tests, computed once"""
    if not _cache:
        for id_ in IDS:
            sc = build(id_, SEEDS[id_])
            _cache[id_] = (sc, run(sc))
    return [(id_,) + _cache[id_] for id_ in IDS]


# ---------------------------------------------------------------------------------------------------------------------
def operands(sc):
    """the flat arrays of orbfe_initializer_reconstruct_multi"""
    ps = sc["probs"]
    n = [len(p["pairs"]) for p in ps]
    words = [ir_pack(p["mask"]) for p in ps]
    return dict(pair_off=np.concatenate([[0], np.cumsum(n)]).astype(np.int32),
                pairs=np.concatenate([p["pairs"] for p in ps]).astype(np.float32).reshape(-1, 4),
                model_kind=np.array([p["kind"] for p in ps], np.int32), model=np.stack([p["model"] for p in ps]).reshape(-1, 9),
                K4=np.stack([p["K4"] for p in ps]).astype(np.float32), sigma=np.array([p["sigma"] for p in ps], np.float32),
                inlier_words=np.concatenate(words).astype(np.uint32),
                in_word_off=np.concatenate([[0], np.cumsum([len(w) for w in words])]).astype(np.int32))


def ir_pack(mask):
    m = np.asarray(mask, bool)
    w = np.zeros((len(m) + 31) // 32, np.uint32)
    for i in np.nonzero(m)[0]:
        w[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return w


def split(sc, out):
    """the dict of initializer_reconstruct_multi -> per problem dict(R [g, 3, 3], t, n_good, cos_sel, hyp_status, x3d [g, n, 3],
    pair_flags [g, n], problem_status, n_inliers)"""
    res = []
    ho, so = out["hyp_off"], out["slot_off"]
    for k, p in enumerate(sc["probs"]):
        n, g = len(p["pairs"]), (8 if p["kind"] == MH else 4)
        assert ho[k + 1] - ho[k] == g and so[k + 1] - so[k] == g * n
        hs = slice(int(ho[k]), int(ho[k + 1]))
        res.append(dict(R=out["R"][hs], t=out["t"][hs], n_good=out["n_good"][hs], cos_sel=out["cos_sel"][hs],
                        hyp_status=out["hyp_status"][hs], x3d=out["x3d"][int(so[k]):int(so[k + 1])].reshape(g, n, 3),
                        pair_flags=out["pair_flags"][int(so[k]):int(so[k + 1])].reshape(g, n),
                        problem_status=int(out["problem_status"][k]), n_inliers=int(out["n_inliers"][k])))
    return res


def motion_distance(Ra, ta, Rb, tb):
    return float(np.linalg.norm(Ra - Rb) + np.linalg.norm(ta - tb))


def match(dev_R, dev_t, hyps, group):
    """the bijection device hypothesis -> restatement hypothesis minimising the summed motion distance, within groups"""
    perm = [0] * len(hyps)
    for g0 in range(0, len(hyps), group):
        idx = list(range(g0, g0 + group))
        best = None
        for pm in itertools.permutations(idx):
            d = sum(motion_distance(dev_R[i], dev_t[i], hyps[j]["R"], hyps[j]["t"]) for i, j in zip(idx, pm))
            if best is None or d < best[0]:
                best = (d, pm)
        for i, j in zip(idx, best[1]):
            perm[i] = j
    return perm


TOLERANCE_FILE = Path(__file__).resolve().parent.parent / "profiles" / "initializer_reconstruct_tolerance.txt"


def recorded():
    """the restatement's own noise (s_motion, s_point, s_cos) as tests/test_initializer_reconstruct_ref.py measured it"""
    d = dict(t.split("=") for t in TOLERANCE_FILE.read_text().split() if "=" in t)
    return float(d["s_motion"]), float(d["s_point"]), float(d["s_cos"])


def point_tolerance(X, s_point):
    """the rule of triangulate_ref.tolerance: max(2 float32 ulps of the largest |component|, 16 s |X|)"""
    X = np.asarray(X, np.float64)
    big = np.abs(X).max(axis=-1)
    ulp = np.spacing(big.astype(np.float32)).astype(np.float64)
    return np.maximum(2 * ulp, 16 * s_point * np.linalg.norm(X, axis=-1))


def replay_device(p, d):
    """the replay on a device problem's numbers -> (success, best, parallax list)"""
    par = [parallax(int(g), float(c)) for g, c in zip(d["n_good"], d["cos_sel"])]
    if d["problem_status"] == DEGENERATE:
        return False, -1, par
    ok, best, _ = (replay_h if p["kind"] == MH else replay_f)(d["n_inliers"], [int(g) for g in d["n_good"]], par)
    return ok, best, par


def compare(id_, sc, r, dev, tol=None):
    """The pass condition; dev = split(sc, device result), r = run(sc).  Returns the largest (motion, point (relative to its
    tolerance's |X|), cos) distances observed."""
    s_motion, s_point, s_cos = tol or recorded()
    a_motion, a_cos = ir.allowance(s_motion), ir.allowance(s_cos)
    worst = [0.0, 0.0, 0.0]
    for k, (p, pr, d) in enumerate(zip(sc["probs"], r, dev)):
        assert d["problem_status"] == pr["status"] and d["n_inliers"] == pr["n_inliers"], (id_, k)
        ok, best, par = replay_device(p, d)
        assert ok == pr["success"], (id_, k)
        if pr["status"] == DEGENERATE:
            assert not d["R"].any() and not d["t"].any() and not d["n_good"].any() and not d["pair_flags"].any() and not d["x3d"].any()
            assert not d["cos_sel"].any() and not d["hyp_status"].any(), (id_, k)
            continue
        perm = match(d["R"], d["t"], pr["hyps"], 4)
        for i, j in enumerate(perm):
            h = pr["hyps"][j]
            dm = motion_distance(d["R"][i], d["t"][i], h["R"], h["t"])
            worst[0] = max(worst[0], dm)
            assert dm <= a_motion, (id_, k, i, dm, a_motion)
            assert int(d["n_good"][i]) == h["n_good"], (id_, k, i, int(d["n_good"][i]), h["n_good"])
            assert np.array_equal(d["pair_flags"][i], h["flags"]), (id_, k, i, np.nonzero(d["pair_flags"][i] != h["flags"])[0][:5])
            assert int(d["hyp_status"][i]) == (NONFINITE if h["nonfinite"] else OK), (id_, k, i)
            assert np.isfinite(d["cos_sel"][i]), (id_, k, i)
            if h["n_good"] > 0:
                dc = abs(float(d["cos_sel"][i]) - h["cos_sel"])
                worst[2] = max(worst[2], dc)
                assert dc <= a_cos * max(abs(h["cos_sel"]), 1e-300), (id_, k, i, dc)
            c = (h["flags"] & COUNTED) != 0
            if c.any():
                err = np.abs(d["x3d"][i][c] - h["X"][c]).max(axis=1)
                tolX = point_tolerance(h["X"][c], s_point)
                worst[1] = max(worst[1], float((err / np.linalg.norm(h["X"][c], axis=1)).max()))
                assert (err <= tolX).all(), (id_, k, i, float((err / tolX).max()))
            assert not d["x3d"][i][~p["mask"]].any() and not d["pair_flags"][i][~p["mask"]].any(), (id_, k, i)
        if pr["success"]:
            assert perm[best] == pr["best"], (id_, k)  # a successful reconstruction has a unique winner
            assert motion_distance(d["R"][best], d["t"][best], pr["R21"], pr["t21"]) <= a_motion, (id_, k)
            sin = max(np.sqrt(max(1.0 - pr["hyps"][pr["best"]]["cos_sel"] ** 2, 0.0)), 1e-12)
            assert abs(par[best] - pr["parallax"]) <= np.degrees(a_cos / sin) + 1e-12, (id_, k)
    return tuple(worst)


# ---------------------------------------------------------------------------------------------------------------------
def write_scene(path, sc):
    """The scene as the text file tests/cpp/initializer_reconstruct_scene.h reads: whitespace-separated numbers, floats as
    their float32 and doubles as their float64 bit patterns in hex."""
    fl = lambda a: " ".join(f"{int(b):08x}" for b in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))
    db = lambda a: " ".join(f"{int(b):016x}" for b in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))
    lines = [f"{len(sc['probs'])}"]
    for p in sc["probs"]:
        lines += [f"{len(p['pairs'])} {p['kind']}", fl([p["sigma"]]), fl(p["K4"]), db(p["model"]), fl(p["pairs"]),
                  " ".join(f"{int(w):08x}" for w in ir_pack(p["mask"]))]
    Path(path).write_text("\n".join(lines) + "\n")


def read_result(path, sc):
    """What the programs write, in the order of orbfe_initializer_reconstruct_multi's outputs: hyp_off, slot_off (integers),
    R, t (bit patterns), n_good, cos_sel (bit patterns), hyp_status, x3d (bit patterns), pair_flags, problem_status,
    n_inliers; then whatever else as tokens -> (dict, rest)"""
    tok = Path(path).read_text().split()
    at = 0

    def take(n, conv, dt):
        nonlocal at
        out = np.array([conv(t) for t in tok[at:at + n]], dt)
        at += n
        return out
    hx = lambda t: int(t, 16)
    K = len(sc["probs"])
    out = dict(hyp_off=take(K + 1, int, np.int32), slot_off=take(K + 1, int, np.int32))
    G, S = int(out["hyp_off"][-1]), int(out["slot_off"][-1])
    out["R"] = take(9 * G, hx, np.uint64).view(np.float64).reshape(G, 3, 3)
    out["t"] = take(3 * G, hx, np.uint64).view(np.float64).reshape(G, 3)
    out["n_good"] = take(G, int, np.int32)
    out["cos_sel"] = take(G, hx, np.uint64).view(np.float64)
    out["hyp_status"] = take(G, int, np.uint8)
    out["x3d"] = take(3 * S, hx, np.uint64).view(np.float64).reshape(S, 3)
    out["pair_flags"] = take(S, int, np.uint8)
    out["problem_status"] = take(K, int, np.uint8)
    out["n_inliers"] = take(K, int, np.int32)
    return out, tok[at:]
