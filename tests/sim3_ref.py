"""Reference restatement of one RANSAC hypothesis of Sim3Solver (src/Sim3Solver.cc: ComputeSim3 :254-370, CheckInliers /
Project / FromCameraToImage :374-463) in numpy float64 on inputs widened from float32, of the selection without replacement
(:173-187), of SetRansacParameters (:118-142) and of iterate's state (:150-220); the scene generator of the Sim3 tests, the
guard band, the ill-conditioning rule and the pass condition.

The eigenvector of N comes from numpy.linalg.eigh (LAPACK), which shares nothing with the cyclic Jacobi routine of
csrc/sim3_math.h.  Where the top eigenvalue is (nearly) repeated -- relative gap (l1 - l2) / |l1| below ILL_GAP, near-collinear
triples -- the eigenvector is not defined by the data, and only status and finiteness are compared.  One case of an exactly
repeated eigenvalue is decided by the reference's own algorithm and restated: N = 0 (three coincident points).  cv::eigen's
Jacobi iteration starts from the identity and rotates nothing there, so evec.row(0) = (1, 0, 0, 0), |vec| = 0 and :310 divides
by it.
"""
from pathlib import Path

import numpy as np

OK, NONFINITE = 0, 1
ILL_GAP = 1e-6     # relative eigen-gap below which a hypothesis is ill-conditioned
GUARD = 1e-6       # relative distance of err from maxErr inside which a decision is not compared
ILL_CAP = 0.05     # of a scene's random hypotheses
GUARD_CAP = 0.001  # of a scene's decisions

N_LEVELS = 8
LEVEL_SIGMA2 = ((np.float32(1.2) ** np.arange(N_LEVELS, dtype=np.float32)) ** 2).astype(np.float32)  # mvLevelSigma2
CAM1 = np.array([517.3, 516.5, 318.6, 255.3], np.float32)  # fx fy cx cy
CAM2 = np.array([520.9, 521.0, 325.1, 249.7], np.float32)

PAIR_COUNTS = (3, 20, 21, 31, 32, 33, 63, 64, 65, 257)
HYP_COUNTS = (1, 3, 4, 5, 300)
PLANT_S, PLANT_DEG, PLANT_T = 1.3, 25.0, np.array([0.3, -0.2, 0.4])


def planted(fix_scale):
    """the planted Sim3 from camera 2 to camera 1: X1 = s R X2 + t"""
    a = np.deg2rad(PLANT_DEG)
    k = np.array([0.2, 0.9, -0.3]) / np.linalg.norm([0.2, 0.9, -0.3])
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx
    return (1.0 if fix_scale else PLANT_S), R, PLANT_T


def max_err(sigma2):
    """mvnMaxError (:87-88): the double product 9.210 * sigma2 stored in a vector<float>"""
    return (9.210 * np.asarray(sigma2, np.float32).astype(np.float64)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
def triples_from_draws(n, draws):
    """:173-187, literally: the list of available indices, the pick, swap-with-back, pop"""
    out = []
    for d in np.asarray(draws).reshape(-1, 3):
        avail = list(range(n))  # :173
        t = []
        for i in range(3):
            randi = int(d[i])
            assert 0 <= randi <= len(avail) - 1  # RandomInt(0, size - 1), :178
            t.append(avail[randi])   # :180
            avail[randi] = avail[-1]  # :185
            avail.pop()               # :186
        out.append(t)
    return np.array(out, np.int32).reshape(-1, 3)


def max_iterations(n, prob=0.99, min_inliers=6, max_its=300):
    """SetRansacParameters (:118-142).  n < min_inliers: 1 without the formula (NaN in the reference, never read)."""
    if n < min_inliers or n <= 0:
        return 1
    if min_inliers == n:  # :134
        return 1
    eps = np.float32(min_inliers) / np.float32(n)  # :129, float
    with np.errstate(all="ignore"):
        its = np.ceil(np.log(1 - prob) / np.log(1 - np.float64(eps) ** 3))  # :137
    if not its < max_its:
        return max(1, max_its)
    return int(its) if its > 1 else 1  # :139 (a quotient of -inf, for a tiny epsilon, included)


class RefSolver:
    """iterate's state (:150-220) over per-hypothesis counts and masks, written apart from the classes under test"""

    def __init__(self, counts, masks, indices1, N1, min_inliers, max_its):
        self.counts, self.masks, self.indices1, self.N1 = counts, masks, np.asarray(indices1), N1
        self.N, self.min_inliers, self.max_its = len(self.indices1), min_inliers, max_its
        self.iterations = 0
        self.best_inliers = 0
        self.best = None

    def iterate(self, n_iterations):
        """-> (hypothesis returned or None, bNoMore, vbInliers, nInliers)"""
        vb = np.zeros(self.N1, bool)  # :153
        if self.N < self.min_inliers:  # :156
            return None, True, vb, 0
        done = 0
        while self.iterations < self.max_its and done < n_iterations:  # :168
            done += 1
            h = self.iterations
            self.iterations += 1
            if self.counts[h] >= self.best_inliers:  # :195
                self.best_inliers = self.counts[h]
                self.best = h
                if self.counts[h] > self.min_inliers:  # :204
                    for i in range(self.N):  # :207-209
                        if self.masks[h][i]:
                            vb[self.indices1[i]] = True
                    return h, False, vb, int(self.counts[h])
        return None, self.iterations >= self.max_its, vb, 0  # :216-219


# ---------------------------------------------------------------------------------------------------------------------
def solve(P1, P2, fix_scale, reverse=False, negate=False):
    """ComputeSim3 (:254-370) for H hypotheses at once.  P1, P2 [H, 3 pairs, 3 coords] float64.  reverse: the three pairs in
    reversed order; negate: the eigenvector negated (both leave the result unchanged but for rounding)."""
    H = len(P1)
    if reverse:
        P1, P2 = P1[:, ::-1], P2[:, ::-1]
    with np.errstate(all="ignore"):
        O1, O2 = P1.sum(1) / 3.0, P2.sum(1) / 3.0  # :234-235
        Pr1 = (P1 - O1[:, None]).transpose(0, 2, 1)  # [H, coord, pair], the reference's columns (:239)
        Pr2 = (P2 - O2[:, None]).transpose(0, 2, 1)
        M = Pr2 @ Pr1.transpose(0, 2, 1)  # :271
        m = lambda i, j: M[:, i, j]
        N11 = m(0, 0) + m(1, 1) + m(2, 2); N12 = m(1, 2) - m(2, 1); N13 = m(2, 0) - m(0, 2); N14 = m(0, 1) - m(1, 0)  # :279-282
        N22 = m(0, 0) - m(1, 1) - m(2, 2); N23 = m(0, 1) + m(1, 0); N24 = m(2, 0) + m(0, 2)  # :283-285
        N33 = -m(0, 0) + m(1, 1) - m(2, 2); N34 = m(1, 2) + m(2, 1); N44 = -m(0, 0) - m(1, 1) + m(2, 2)  # :286-288
        N = np.stack([N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44], axis=1).reshape(H, 4, 4)
        w, V = np.linalg.eigh(N) if H else (np.zeros((0, 4)), np.zeros((0, 4, 4)))  # :300; ascending
        q = V[:, :, 3].copy()
        q[~N.reshape(H, 16).any(axis=1)] = (1.0, 0.0, 0.0, 0.0)  # N = 0: cv::eigen leaves the identity (module docstring)
        gap = (w[:, 3] - w[:, 2]) / np.abs(w[:, 3])
        gap = np.where(np.isfinite(gap), gap, 0.0)
        if negate:
            q = -q
        vec = q[:, 1:]
        nv = np.linalg.norm(vec, axis=1)
        ang = np.arctan2(nv, q[:, 0])  # :308
        vec = vec * (2 * ang / nv)[:, None]  # :310
        theta = np.linalg.norm(vec, axis=1)  # cv::Rodrigues
        r = vec / theta[:, None]
        c, s = np.cos(theta)[:, None, None], np.sin(theta)[:, None, None]
        rx = np.zeros((H, 3, 3))
        rx[:, 0, 1], rx[:, 0, 2], rx[:, 1, 0], rx[:, 1, 2], rx[:, 2, 0], rx[:, 2, 1] = -r[:, 2], r[:, 1], r[:, 2], -r[:, 0], -r[:, 1], r[:, 0]
        R = c * np.eye(3) + (1 - c) * (r[:, :, None] * r[:, None, :]) + s * rx
        P3 = R @ Pr2  # :319
        if fix_scale:
            sc = np.ones(H)  # :343
        else:
            sc = (Pr1 * P3).sum((1, 2)) / (P3 * P3).sum((1, 2))  # :325-340
        sR = sc[:, None, None] * R
        t = O1 - (sR @ O2[:, :, None])[:, :, 0]  # :348
        T12 = np.concatenate([sR, t[:, :, None]], axis=2)  # :354-359
        sRinv = (1.0 / sc)[:, None, None] * R.transpose(0, 2, 1)  # :365
        T21 = np.concatenate([sRinv, -(sRinv @ t[:, :, None])], axis=2)  # :368
    return dict(R=R, t=t, s=sc, T12=T12, T21=T21, gap=gap)


def _image(T, K, X):
    """Project (:421-442) of X [n, 3] with T [H, 3, 4]; FromCameraToImage (:445-463) when T is None.  No depth test."""
    K = K.astype(np.float64)
    with np.errstate(all="ignore"):
        P = X if T is None else np.einsum("hij,nj->hni", T[:, :, :3], X) + T[:, None, :, 3]
        invz = 1.0 / P[..., 2]
        return K[0] * (P[..., 0] * invz) + K[2], K[1] * (P[..., 1] * invz) + K[3]


def run(sc, reverse=False, negate=False):
    """Every hypothesis of the scene -> dict(n_inliers [H], status [H], sim3 [H, 13] float64, masks (per hypothesis bool
    [n_k]), gap [H], guard (per hypothesis bool [n_k]), cand [H], and the per-candidate offsets)."""
    n_inl, status, sim3, masks, gaps, guards, cand = [], [], [], [], [], [], []
    for k, c in enumerate(sc["cands"]):
        T = c["triples"]
        if len(T) == 0:
            continue
        x1, x2 = c["x1"].astype(np.float64), c["x2"].astype(np.float64)
        s = solve(x1[T], x2[T], sc["fix_scale"], reverse, negate)
        flat = np.concatenate([s["R"].reshape(-1, 9), s["t"], s["s"][:, None]], axis=1)
        bad = ~np.isfinite(flat).all(axis=1)
        u11, v11 = _image(None, c["cam1"], x1)  # mvP1im1
        u22, v22 = _image(None, c["cam2"], x2)  # mvP2im2
        u21, v21 = _image(s["T12"], c["cam1"], x2)  # vP2im1 (:377)
        u12, v12 = _image(s["T21"], c["cam2"], x1)  # vP1im2 (:378)
        m1, m2 = c["max1"].astype(np.float64), c["max2"].astype(np.float64)
        with np.errstate(all="ignore"):
            e1 = (u11 - u21) ** 2 + (v11 - v21) ** 2  # :384, :387
            e2 = (u12 - u22) ** 2 + (v12 - v22) ** 2
            inl = (e1 < m1) & (e2 < m2) & ~bad[:, None]  # :390
            g = ((np.abs(e1 - m1) <= GUARD * m1) | (np.abs(e2 - m2) <= GUARD * m2)) & ~bad[:, None]
        n_inl += inl.sum(1).tolist(); status += np.where(bad, NONFINITE, OK).tolist(); sim3.append(flat)
        masks += list(inl); guards += list(g); gaps += s["gap"].tolist(); cand += [k] * len(T)
    H = len(n_inl)
    return dict(n_inliers=np.array(n_inl, np.int32).reshape(H), status=np.array(status, np.uint8).reshape(H),
                sim3=np.concatenate(sim3) if sim3 else np.zeros((0, 13)), masks=masks, gap=np.array(gaps).reshape(H), guard=guards,
                cand=np.array(cand, np.int32).reshape(H))


# ---------------------------------------------------------------------------------------------------------------------
def candidate(rng, n, H, fix_scale, outliers=0.3, engineered=False):
    """One Sim3Solver's inputs: n pairs around the planted transform -- inliers exact up to the float32 rounding of the
    points, outliers displaced by 1-2 m (hundreds of pixels at these depths, against a maxErr of at most 9.21 * 1.2^14 px^2)
    -- with mixed octaves, and H random triples drawn the reference's way.  engineered (n >= 40, H >= 8): pairs 0-15 and
    hypotheses 0-6 are the engineered cases of ENGINEERED."""
    s, R, t = planted(fix_scale)
    z = rng.uniform(2.0, 6.0, n)
    u, v = rng.uniform(60.0, 580.0, n), rng.uniform(40.0, 440.0, n)
    f = CAM2.astype(np.float64)
    X2 = np.stack([(u - f[2]) / f[0] * z, (v - f[3]) / f[1] * z, z], axis=1)
    inlier = rng.uniform(0, 1, n) >= outliers
    if engineered:
        assert n >= 40 and H >= 8
        inlier[:16] = [0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]
        X2[0:3] = [[0.5, 0.2, 3.0], [-0.4, 0.3, 2.5], [0.1, -0.6, 4.0]]    # 0-2: the same three points in both cameras
        X2[3:6] = X2[3] + np.outer([0.0, 1.0, 2.0], [0.3, 0.1, 0.5])          # 3-5: collinear, consistent with the plant
        X2[6:9] = X2[6]                                                       # 6-8: one point three times
        # 9-11: outliers (displaced below); 12-14: inliers; 15: behind both cameras and consistent with the plant
    X1 = s * X2 @ R.T + t
    if engineered:
        X1[0:3] = X2[0:3]
        X1[6:9] = X1[6] + np.array([1.5, -1.0, 0.5])  # (still one point three times)
        inlier[9:12] = False
        X1[15] = [0.3, 0.2, -3.0]
        X2[15] = (X1[15] - t) @ R / s  # R^T (X1 - t) / s
    out = np.nonzero(~inlier)[0]
    if engineered:
        out = out[out >= 9]  # (pairs 0-8 are what they are)
    d = rng.uniform(1.0, 2.0, (len(out), 3)) * rng.choice([-1.0, 1.0], (len(out), 3))
    X1[out] += d
    octave1, octave2 = rng.integers(0, N_LEVELS, n), rng.integers(0, N_LEVELS, n)
    draws = np.stack([rng.integers(0, n - i, H) for i in range(3)], axis=1) if H else np.zeros((0, 3), np.int64)
    triples = triples_from_draws(n, draws) if H else np.zeros((0, 3), np.int32)
    tags = {}
    if engineered:
        for h, (name, tr) in enumerate(ENGINEERED.items()):
            triples[h] = tr
            tags[h] = name
    N1 = n + 7
    return dict(n=n, x1=X1.astype(np.float32), x2=X2.astype(np.float32), sigma2_1=LEVEL_SIGMA2[octave1], sigma2_2=LEVEL_SIGMA2[octave2],
                max1=max_err(LEVEL_SIGMA2[octave1]), max2=max_err(LEVEL_SIGMA2[octave2]), cam1=CAM1, cam2=CAM2, triples=triples,
                inlier=inlier, tags=tags, indices1=np.sort(rng.permutation(N1)[:n]), N1=N1)


# hypothesis -> its three pairs, in an engineered candidate
ENGINEERED = {"identity": (0, 1, 2), "collinear": (3, 4, 5), "coincident": (6, 7, 8), "outliers": (9, 10, 11),
              "inliers": (12, 13, 14), "identity-permuted": (2, 0, 1), "with-negative-z": (15, 12, 13)}
DEGENERATE = ("collinear", "coincident")  # nothing but status (and finiteness) is compared


def scene(seed, spec):
    """spec: dict(fix_scale, cands=[dict(n, H, outliers, engineered)])"""
    rng = np.random.default_rng(seed)
    return dict(fix_scale=bool(spec["fix_scale"]), cands=[candidate(rng, fix_scale=spec["fix_scale"], **c) for c in spec["cands"]])


def _outliers(n):
    return 0.0 if n < 20 or n == 64 else 0.3  # small candidates and one full ballot: every pair an inlier


def specs():
    for fix in (0, 1):
        for n in PAIR_COUNTS:
            for H in HYP_COUNTS:
                yield f"n{n}-H{H}-fix{fix}", dict(fix_scale=fix, cands=[dict(n=n, H=H, outliers=_outliers(n))])
        yield f"K3-fix{fix}", dict(fix_scale=fix, cands=[dict(n=65, H=37, outliers=0.3), dict(n=40, H=0, outliers=0.3),
                                                          dict(n=33, H=5, outliers=0.0)])
        yield f"engineered-fix{fix}", dict(fix_scale=fix, cands=[dict(n=129, H=20, outliers=0.3, engineered=True)])
        yield f"class-fix{fix}", dict(fix_scale=fix, cands=[dict(n=60, H=0, outliers=0.95), dict(n=80, H=0, outliers=0.4),
                                                             dict(n=10, H=0, outliers=0.0)])


CLASS_MIN_INLIERS = 20  # the class scenes: SetRansacParameters(0.99, 20, 300) as LoopClosing.cc:328 does


def build(id_, spec):
    sc = scene(0, spec)  # seed 0 keeps every scene within the caps (tests/test_sim3_ref.py asserts it)
    if id_.startswith("class"):  # the hypotheses are what the solvers' SetRansacParameters asks for
        rng = np.random.default_rng(99)
        for c in sc["cands"]:
            H = 0 if c["n"] < CLASS_MIN_INLIERS else max_iterations(c["n"], 0.99, CLASS_MIN_INLIERS, 300)
            c["triples"] = triples_from_draws(c["n"], np.stack([rng.integers(0, c["n"] - i, H) for i in range(3)], axis=1)) \
                if H else np.zeros((0, 3), np.int32)
    return sc


def gpu_scenes():
    """(id, scene) of every scene the GPU test runs."""
    return [(id_, build(id_, spec)) for id_, spec in specs()]


def caps(sc, r):
    """(ill-conditioned random hypotheses, random hypotheses, guard-band decisions, decisions) of a scene"""
    tagged = np.zeros(len(r["gap"]), bool)
    h0 = 0
    for c in sc["cands"]:
        for h in c["tags"]:
            tagged[h0 + h] = True
        h0 += len(c["triples"])
    ill = (r["gap"] < ILL_GAP) & ~tagged
    return int(ill.sum()), int((~tagged).sum()), int(sum(g.sum() for g in r["guard"])), int(sum(g.size for g in r["guard"]))


# ---------------------------------------------------------------------------------------------------------------------
def operands(sc):
    """the flat arrays of orbfe_sim3_ransac_multi"""
    cs = sc["cands"]
    cat = lambda key, shape, dt: np.concatenate([c[key] for c in cs]).astype(dt) if cs else np.zeros(shape, dt)
    return dict(pair_off=np.concatenate([[0], np.cumsum([c["n"] for c in cs])]).astype(np.int32),
                hyp_off=np.concatenate([[0], np.cumsum([len(c["triples"]) for c in cs])]).astype(np.int32),
                x1=cat("x1", (0, 3), np.float32), x2=cat("x2", (0, 3), np.float32), max1=cat("max1", 0, np.float32),
                max2=cat("max2", 0, np.float32), cam1=np.stack([c["cam1"] for c in cs]), cam2=np.stack([c["cam2"] for c in cs]),
                triples=cat("triples", (0, 3), np.int32), fix_scale=sc["fix_scale"])


def word_offsets(sc):
    return np.concatenate([[0], np.cumsum([len(c["triples"]) * ((c["n"] + 31) // 32) for c in sc["cands"]])]).astype(np.int32)


def unpack(words, n):
    i = np.arange(n)
    return ((np.asarray(words, np.uint32)[i >> 5] >> (i & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)


def s_sim3():
    """The restatement's own noise as tests/test_sim3_ref.py measured and recorded it."""
    text = (Path(__file__).resolve().parent.parent / "profiles" / "sim3_tolerance.txt").read_text()
    return float(dict(line.split("=") for line in text.split() if "=" in line)["s_sim3"])


def rel_tolerance(magnitude, s):
    """max(2 float32 ulps of the quantity's magnitude, 16 s_sim3 of it)"""
    magnitude = np.asarray(magnitude, np.float64)
    return np.maximum(2 * np.spacing(magnitude.astype(np.float32)).astype(np.float64), 16 * s * magnitude)


def sim3_errors(a, b):
    """(|dR|_F, |R|_F), (|dt|, |t|), (|ds|, |s|) of sim3 rows a against b"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return ((np.linalg.norm(a[:, :9] - b[:, :9], axis=1), np.linalg.norm(b[:, :9], axis=1)),
            (np.linalg.norm(a[:, 9:12] - b[:, 9:12], axis=1), np.linalg.norm(b[:, 9:12], axis=1)),
            (np.abs(a[:, 12] - b[:, 12]), np.abs(b[:, 12])))


def compare(id_, sc, r, n_inliers, status, sim3, words, word_off, s):
    """The pass condition of the Sim3 tests; r = run(sc), s = s_sim3().  Returns (ill-conditioned hypotheses, guard-band
    decisions, decisions that differ inside the guard band)."""
    assert np.array_equal(word_off, word_offsets(sc)), id_
    H = len(r["status"])
    assert len(n_inliers) == len(status) == len(sim3) == H and len(words) == word_off[-1], id_
    assert np.array_equal(status, r["status"]), (id_, np.nonzero(np.asarray(status) != r["status"])[0][:5])
    sim3 = np.asarray(sim3)
    fin = np.isfinite(sim3).all(axis=1)
    assert np.array_equal(fin, r["status"] == OK), id_  # finite exactly where the status says so
    skip = r["gap"] < ILL_GAP
    h = 0
    n_guard = n_diff = 0
    for k, c in enumerate(sc["cands"]):
        w, w0 = (c["n"] + 31) // 32, int(word_off[k])
        for j in range(len(c["triples"])):
            wd = words[w0 + j * w: w0 + (j + 1) * w]
            mask = unpack(wd, c["n"])
            bits = sum(bin(int(x)).count("1") for x in wd)
            assert bits == mask.sum() == n_inliers[h], (id_, h)  # the count is the mask's; no bit beyond pair n - 1
            if r["status"][h] == NONFINITE:
                assert n_inliers[h] == 0 and not wd.any(), (id_, h)
            elif not skip[h] and c["tags"].get(j) not in DEGENERATE:
                g = r["guard"][h]
                diff = mask != r["masks"][h]
                assert not (diff & ~g).any(), (id_, h, np.nonzero(diff & ~g)[0][:5])
                assert abs(int(n_inliers[h]) - int(r["n_inliers"][h])) <= int(g.sum()), (id_, h)
                n_guard += int(g.sum()); n_diff += int(diff.sum())
            else:
                skip[h] = True
            h += 1
    cmp = ~skip & (r["status"] == OK)
    for (err, mag), what in zip(sim3_errors(sim3[cmp], r["sim3"][cmp]), ("R", "t", "s")):
        tol = rel_tolerance(mag, s)
        assert (err <= tol).all(), (id_, what, float((err / tol).max()))
    return int(skip.sum()), n_guard, n_diff


def write_scene(path, sc):
    """The scene as the text file tests/cpp/sim3_scene.h reads: whitespace-separated numbers, floats as their float32 bit
    patterns in hex."""
    def fl(a):
        return " ".join(f"{int(b):08x}" for b in np.ascontiguousarray(a, np.float32).reshape(-1).view(np.uint32))
    lines = [f"{len(sc['cands'])} {int(sc['fix_scale'])}"]
    for c in sc["cands"]:
        lines += [f"{c['n']} {len(c['triples'])} {c['N1']}", fl(c["cam1"]), fl(c["cam2"]), fl(c["x1"]), fl(c["x2"]),
                  fl(c["sigma2_1"]), fl(c["sigma2_2"]), " ".join(str(int(i)) for i in c["indices1"]),
                  " ".join(str(int(i)) for i in c["triples"].reshape(-1))]
    Path(path).write_text("\n".join(lines) + "\n")


def read_result(path, H):
    """What the programs write: n_inliers [H], status [H], sim3 [H * 13] as float32 bit patterns, the number of mask words and
    the words in hex, then whatever else as integers."""
    tok = Path(path).read_text().split()
    n_inl = np.array([int(t) for t in tok[:H]], np.int32).reshape(H)
    status = np.array([int(t) for t in tok[H:2 * H]], np.uint8).reshape(H)
    sim3 = np.array([int(t, 16) for t in tok[2 * H:15 * H]], np.uint32).view(np.float32).reshape(H, 13)
    W = int(tok[15 * H])
    words = np.array([int(t, 16) for t in tok[15 * H + 1:15 * H + 1 + W]], np.uint32).reshape(W)
    rest = [int(t) for t in tok[15 * H + 1 + W:]]
    return n_inl, status, sim3, words, rest
