"""Reference of Optimizer::OptimizeSim3 (src/Optimizer.cc:1116-1323) for orbfe_optimize_sim3*: a float64 restatement of the
one graph it builds -- one free VertexSim3Expmap S12 and, per correspondence, two fixed points with an EdgeSim3ProjectXYZ
(e12) and an EdgeInverseSim3ProjectXYZ (e21), Huber kernel, Levenberg on a dense 7 x 7 system -- written from

* Thirdparty/g2o/g2o/types/sim3.h (Sim3(Vector7d) :70-142, map :144-146, inverse :233-236, operator* :266-272),
* Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h (oplusImpl :60-69, cam_map1/2 :74-88, computeError :138-145, :160-167),
* Thirdparty/g2o/g2o/core/base_binary_edge.hpp (constructQuadraticForm :54-120, the numeric linearizeOplus :131-200),
* Thirdparty/g2o/g2o/core/robust_kernel_impl.cpp:78-91 (Huber), optimization_algorithm_levenberg.cpp:61-189,
* src/Converter.cc (toMatrix3d, toVector3d: float -> double) and Eigen's Quaternion <-> rotation-matrix conversions.

The quaternion helpers, the sequential sum and the Levenberg rules are those of tests/pose_opt_ref.py.  Per-edge arithmetic is
elementwise numpy float64 (IEEE, no contraction); the sums over edges of H (28 upper-triangle entries), b (7) and the robust
chi2 are strictly sequential in pair order, e12 then e21 of a pair, or in reversed order with reverse=True.  The 7 x 7 solve
is an unpivoted LDL^T; a non-positive pivot is a failed factorisation.

jacobian="numeric" is g2o's literal scheme: central differences with delta = 1e-9 through oplus on the vertex, _fix_scale
zeroing update[6] so that column 6 is exactly zero.  jacobian="analytic" is the Jacobian of the same left update
S' = Sim3(update) * S, column 6 zeroed with fix_scale: what csrc/optsim3_math.h computes.

chi2() in the two classifications (:1274, :1309) reads the _error of the last computeActiveErrors, which in Levenberg is the
last evaluated TRIAL, accepted or rejected: `stored` below."""
import math

import numpy as np

from frustum_ref import rodrigues
from pose_opt_ref import DBL_MAX, _matmul3, _seq_sum, f32, quat_from_R, quat_mul, quat_rotate, quat_to_R

SCALE, LEVELS = 1.2, 8
INV_LEVEL_SIGMA2 = np.array([1.0 / (f32(SCALE) ** (2 * l)) for l in range(LEVELS)], dtype=f32)  # mvInvLevelSigma2
TH2 = f32(10.0)  # LoopClosing::ComputeSim3 calls OptimizeSim3(..., 10, mbFixScale) (src/LoopClosing.cc:388)
CAM_A = np.array([718.856, 718.856, 607.1928, 185.2157], f32)  # fx fy cx cy
CAM_B = np.array([707.0912, 707.0912, 601.8873, 183.1104], f32)
W_IMG, H_IMG = 1241, 376
GUARD_CHI2, GUARD_Z = 1e-3, 0.1
MIN_PAIRS = 10  # nCorrespondences - nBad < 10 returns 0 (:1293)
TRI = [(r, c) for r in range(7) for c in range(r, 7)]  # the 28 upper-triangle entries, row-major
DIAG = [k for k, (r, c) in enumerate(TRI) if r == c]


# ---------------------------------------------------------------------------------------------------------------------
# g2o::Sim3: (q = (x, y, z, w), t, s) in Python floats (binary64)
def sim3_from_record(rec):
    """sim3[13] = R row-major, t, s (float32) -> Sim3(Matrix3d, Vector3d, double) (sim3.h:64-67): r = Quaterniond(R)."""
    rec = np.asarray(rec, f32).reshape(13)
    R = [[float(rec[3 * r + c]) for c in range(3)] for r in range(3)]
    return quat_from_R(R), [float(rec[9 + r]) for r in range(3)], float(rec[12])


def sim3_exp(u):
    """Sim3(const Vector7d&) (sim3.h:70-142), branch by branch; u = (omega, upsilon, sigma)."""
    wx, wy, wz = u[0], u[1], u[2]
    ups, sigma = u[3:6], u[6]
    theta = math.sqrt(wx * wx + wy * wy + wz * wz)
    Om = [[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]]
    Om2 = _matmul3(Om, Om)
    I = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    s = math.exp(sigma)
    eps = 0.00001
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B, small = 1.0 / 2.0, 1.0 / 6.0, True
        else:
            theta2 = theta * theta
            A = (1.0 - math.cos(theta)) / theta2
            B = (theta - math.sin(theta)) / (theta2 * theta)
            small = False
    else:
        C = (s - 1.0) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma)
            small = True
        else:
            a = s * math.sin(theta)
            b = s * math.cos(theta)
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2
            small = False
    if small:
        R = [[(I[r][c] + Om[r][c]) + Om2[r][c] for c in range(3)] for r in range(3)]
    else:
        ra, rb = math.sin(theta) / theta, (1.0 - math.cos(theta)) / (theta * theta)
        R = [[(I[r][c] + ra * Om[r][c]) + rb * Om2[r][c] for c in range(3)] for r in range(3)]
    W = [[(A * Om[r][c] + B * Om2[r][c]) + C * I[r][c] for c in range(3)] for r in range(3)]
    t = [(W[r][0] * ups[0] + W[r][1] * ups[1]) + W[r][2] * ups[2] for r in range(3)]
    return quat_from_R(R), t, s  # r = Quaterniond(R): not normalised


def sim3_mul(a, b):
    """Sim3::operator* (sim3.h:266-272)."""
    qa, ta, sa = a
    qb, tb, sb = b
    rx, ry, rz = quat_rotate(qa, tb[0], tb[1], tb[2])
    return quat_mul(qa, qb), [sa * rx + ta[0], sa * ry + ta[1], sa * rz + ta[2]], sa * sb


def sim3_map(S, X, Y, Z):
    """Sim3::map (sim3.h:144-146): s (r * xyz) + t.  X, Y, Z: floats or arrays."""
    q, t, s = S
    rx, ry, rz = quat_rotate(q, X, Y, Z)
    return s * rx + t[0], s * ry + t[1], s * rz + t[2]


def sim3_inverse(S):
    """Sim3::inverse (sim3.h:233-236)."""
    q, t, s = S
    qc = [-q[0], -q[1], -q[2], q[3]]
    k = -1.0 / s
    rx, ry, rz = quat_rotate(qc, k * t[0], k * t[1], k * t[2])
    return qc, [rx, ry, rz], 1.0 / s


def sim3_to_Rts(sim3_out):
    """(qx, qy, qz, qw, tx, ty, tz, s) -> R [3, 3], t [3], s in float64: what Converter::toCvMat(g2oS12.rotation()...) reads."""
    v = [float(c) for c in sim3_out]
    return np.array(quat_to_R(v[:4])), np.array(v[4:7]), v[7]


def solve_ldlt7(Hs, lam, b):
    """(H + lam I) x = b by unpivoted LDL^T; Hs: the 28 upper-triangle entries.  (ok, x): ok False and x = 0 on a pivot <= 0."""
    A = [[0.0] * 7 for _ in range(7)]
    for k, (r, c) in enumerate(TRI):
        A[r][c] = A[c][r] = Hs[k]
    for j in range(7):
        A[j][j] = A[j][j] + lam
    L = [[0.0] * 7 for _ in range(7)]
    D = [0.0] * 7
    for j in range(7):
        d = A[j][j]
        for k in range(j):
            d = d - (L[j][k] * L[j][k]) * D[k]
        if not d > 0.0:
            return False, [0.0] * 7
        D[j] = d
        for i in range(j + 1, 7):
            s = A[j][i]
            for k in range(j):
                s = s - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = s / d
    y = [0.0] * 7
    for i in range(7):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    x = [0.0] * 7
    for i in range(6, -1, -1):
        s = y[i] / D[i]
        for k in range(i + 1, 7):
            s = s - L[k][i] * x[k]
        x[i] = s
    return True, x


class _Pairs:
    def __init__(self, x3dc1, x3dc2, obs1, obs2, w1, w2, cam1, cam2, th2, fix_scale):
        wide = lambda a, k: np.asarray(a, f32).reshape(-1, k).astype(np.float64)
        self.X1, self.X2, self.o1, self.o2 = wide(x3dc1, 3), wide(x3dc2, 3), wide(obs1, 2), wide(obs2, 2)
        self.w1, self.w2 = wide(w1, 1)[:, 0], wide(w2, 1)[:, 0]
        self.n = len(self.X1)
        self.K1 = [float(f32(k)) for k in cam1]
        self.K2 = [float(f32(k)) for k in cam2]
        self.th2 = float(f32(th2))
        self.delta = float(np.sqrt(f32(th2), dtype=f32))  # const float deltaHuber = sqrt(th2) (:1168)
        self.dsqr = self.delta * self.delta
        self.fix_scale = bool(fix_scale)

    def errors(self, S):
        """(e12 [2], chi2_12, P12 [3]), (e21, chi2_21, P21) at S."""
        with np.errstate(all="ignore"):
            P = sim3_map(S, self.X2[:, 0], self.X2[:, 1], self.X2[:, 2])
            fx, fy, cx, cy = self.K1
            ea = (self.o1[:, 0] - ((P[0] / P[2]) * fx + cx), self.o1[:, 1] - ((P[1] / P[2]) * fy + cy))
            ca = ea[0] * (self.w1 * ea[0]) + ea[1] * (self.w1 * ea[1])
            Q = sim3_map(sim3_inverse(S), self.X1[:, 0], self.X1[:, 1], self.X1[:, 2])
            fx, fy, cx, cy = self.K2
            eb = (self.o2[:, 0] - ((Q[0] / Q[2]) * fx + cx), self.o2[:, 1] - ((Q[1] / Q[2]) * fy + cy))
            cb = eb[0] * (self.w2 * eb[0]) + eb[1] * (self.w2 * eb[1])
        return (ea, ca, P), (eb, cb, Q)

    def huber(self, chi2):
        with np.errstate(all="ignore"):
            over = chi2 > self.dsqr
            sq = np.sqrt(chi2)
            return np.where(over, 2 * sq * self.delta - self.dsqr, chi2), np.where(over, self.delta / sq, 1.0)

    def jac_analytic(self, S, P, Q):
        """J0 [7], J1 [7] of e12 and of e21: d e / d update of S' = Sim3(update) * S at update = 0."""
        zero = np.zeros(self.n)
        with np.errstate(all="ignore"):
            fx, fy, _, _ = self.K1
            x, y = P[0], P[1]
            invz = 1.0 / P[2]
            invz_2 = invz * invz
            A0 = [x * y * invz_2 * fx, -(1.0 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx, zero]
            A1 = [(1.0 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy, zero]
            fx, fy, _, _ = self.K2
            Si = sim3_inverse(S)
            R = quat_to_R(Si[0])
            M = [[Si[2] * R[r][c] for c in range(3)] for r in range(3)]
            x, y = Q[0], Q[1]
            invz = 1.0 / Q[2]
            invz_2 = invz * invz
            d00, d02 = -invz * fx, x * invz_2 * fx
            d11, d12 = -invz * fy, y * invz_2 * fy
            X, Y, Z = self.X1[:, 0], self.X1[:, 1], self.X1[:, 2]
            G = [[M[r][1] * Z - M[r][2] * Y, M[r][2] * X - M[r][0] * Z, M[r][0] * Y - M[r][1] * X,
                  -M[r][0] + zero, -M[r][1] + zero, -M[r][2] + zero, -((M[r][0] * X + M[r][1] * Y) + M[r][2] * Z)] for r in range(3)]
            B0 = [d00 * G[0][c] + d02 * G[2][c] for c in range(7)]
            B1 = [d11 * G[1][c] + d12 * G[2][c] for c in range(7)]
            if self.fix_scale:
                B0[6], B1[6] = zero, zero
        return (A0, A1), (B0, B1)

    def jac_numeric(self, S):
        """BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:176-198) on the Sim3 vertex (the points are fixed)."""
        delta = 1e-9
        scalar = 1.0 / (2 * delta)
        A0, A1, B0, B1 = [], [], [], []
        for d in range(7):
            e = []
            for sign in (delta, -delta):
                add = [0.0] * 7
                add[d] = sign
                if self.fix_scale:
                    add[6] = 0.0  # oplusImpl
                (ea, _, _), (eb, _, _) = self.errors(sim3_mul(sim3_exp(add), S))
                e.append((ea, eb))
            A0.append(scalar * (e[0][0][0] - e[1][0][0]))
            A1.append(scalar * (e[0][0][1] - e[1][0][1]))
            B0.append(scalar * (e[0][1][0] - e[1][1][0]))
            B1.append(scalar * (e[0][1][1] - e[1][1][1]))
        return (A0, A1), (B0, B1)


def _interleave(a, b):
    """rows of a and b alternating: e12 then e21 of every pair."""
    out = np.empty((2 * a.shape[0],) + a.shape[1:])
    out[0::2], out[1::2] = a, b
    return out


def optimize_sim3(x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2, sim3_in, th2, fix_scale, reverse=False,
                  jacobian="analytic"):
    """-> dict: n_in (the return value), sim3 [8] float64 (qx qy qz qw tx ty tz s: the incoming S12 when the call returns 0
    early), bad [n] uint8 (0 kept, 1 erased after round one, 2 after round two), rounds, n_bad, per round iterations, trials,
    lam, chi2, last_rejected, last_rho, cls_chi2_12 / cls_chi2_21 (the chi2 each classification read), fresh_differs (whether
    a pair would classify otherwise on the chi2 recomputed at the estimate), and chi2_12 / chi2_21 [n]: what every pair holds
    at the end."""
    E = _Pairs(x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2, th2, fix_scale)
    n = E.n
    start = sim3_from_record(sim3_in)
    out = dict(n_in=0, sim3=np.array(list(start[0]) + list(start[1]) + [start[2]]), bad=np.zeros(n, np.uint8), rounds=0,
               n_bad=0, iterations=[], trials=[], lam=[], chi2=[], last_rejected=[], last_rho=[], cls_chi2_12=[],
               cls_chi2_21=[], fresh_differs=[], chi2_12=np.zeros(n), chi2_21=np.zeros(n))
    if n == 0:
        return out
    bad = np.zeros(n, np.uint8)
    s12, s21 = np.zeros(n), np.zeros(n)  # chi2 of what g2o holds in _error of every edge
    est = start
    max_it = 5  # optimizer.optimize(5) (:1263)
    for rnd in range(2):
        active = bad == 0
        act2 = np.repeat(active, 2)
        iters = trials = 0
        lam = cur = 0.0
        rejected, rho = False, 0.0
        ni, nBadLM = 2.0, 0
        for it in range(max_it):
            (ea, ca, P), (eb, cb, Q) = E.errors(est)
            s12, s21 = np.where(active, ca, s12), np.where(active, cb, s21)
            JA, JB = E.jac_analytic(est, P, Q) if jacobian == "analytic" else E.jac_numeric(est)
            cols = []
            with np.errstate(all="ignore"):
                for (J0, J1), e, c, w in ((JA, ea, ca, E.w1), (JB, eb, cb, E.w2)):
                    rho0, rho1 = E.huber(c)
                    wr = rho1 * w
                    we0, we1 = wr * e[0], wr * e[1]
                    col = [(J0[r] * wr) * J0[cc] + (J1[r] * wr) * J1[cc] for r, cc in TRI]
                    col += [J0[j] * we0 + J1[j] * we1 for j in range(7)]
                    col.append(rho0)
                    cols.append(np.stack(col, axis=1))
                S = _seq_sum(np.where(act2[:, None], _interleave(cols[0], cols[1]), 0.0), reverse)
            Hs = [float(S[k]) for k in range(28)]
            b = [-float(S[28 + j]) for j in range(7)]
            cur = ini = float(S[35])
            if it == 0:  # computeLambdaInit: tau = 1e-5
                lam = 1e-5 * max(0.0, *[abs(Hs[k]) for k in DIAG])
                ni, nBadLM = 2.0, 0
            rho, q = 0.0, 0
            while True:
                ok, x = solve_ldlt7(Hs, lam, b)
                if E.fix_scale:
                    x[6] = 0.0  # oplusImpl writes into the solver's x
                trial = sim3_mul(sim3_exp(x), est)
                (_, ca, _), (_, cb, _) = E.errors(trial)
                s12, s21 = np.where(active, ca, s12), np.where(active, cb, s21)
                with np.errstate(all="ignore"):
                    r0 = _interleave(E.huber(ca)[0], E.huber(cb)[0])
                    temp = float(_seq_sum(np.where(act2, r0, 0.0)[:, None], reverse)[0])
                if not ok:
                    temp = DBL_MAX
                scale = 0.0
                for j in range(7):
                    scale = scale + x[j] * (lam * x[j] + b[j])
                scale = scale + 1e-3
                with np.errstate(all="ignore"):
                    rho = float(np.float64(cur - temp) / np.float64(scale))
                trials += 1
                if rho > 0 and math.isfinite(temp):
                    tt = 2 * rho - 1
                    alpha = min(1.0 - tt * tt * tt, 2.0 / 3.0)
                    lam = lam * max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur = temp
                    est = trial
                    rejected = False
                else:
                    lam = lam * ni
                    ni = ni * 2
                    rejected = True
                q += 1
                if not (rho < 0 and q < 10):
                    break
            iters += 1
            if q == 10 or rho == 0:
                break
            if (ini - cur) * 1e3 < ini:  # Stop criterium (Raul), :154-161
                nBadLM += 1
            else:
                nBadLM = 0
            if nBadLM >= 3:
                break
        # classification (:1267-1284, :1302-1316): chi2() reads the stored _error
        with np.errstate(all="ignore"):
            over = active & ((s12 > E.th2) | (s21 > E.th2))
            (_, fa, _), (_, fb, _) = E.errors(est)
            fresh = active & ((fa > E.th2) | (fb > E.th2))
        bad = np.where(over, rnd + 1, bad).astype(np.uint8)
        out["rounds"] = rnd + 1
        for key, val in (("iterations", iters), ("trials", trials), ("lam", lam), ("chi2", cur), ("last_rejected", rejected),
                         ("last_rho", rho), ("cls_chi2_12", np.where(active, s12, np.nan)),
                         ("cls_chi2_21", np.where(active, s21, np.nan)), ("fresh_differs", bool((over != fresh).any()))):
            out[key].append(val)
        if rnd == 0:
            n_bad = int(over.sum())
            out["n_bad"] = n_bad
            max_it = 10 if n_bad > 0 else 5  # nMoreIterations (:1287-1291)
            if n - n_bad < MIN_PAIRS:  # return 0: g2oS12 stays what came in, the erasures stay (:1293-1294)
                out["bad"], out["chi2_12"], out["chi2_21"] = bad, s12, s21
                return out
    out["bad"], out["chi2_12"], out["chi2_21"] = bad, s12, s21
    out["n_in"] = int((bad == 0).sum())
    out["sim3"] = np.array(list(est[0]) + list(est[1]) + [est[2]])
    return out


# ---------------------------------------------------------------------------------------------------------------------
def scene(seed, n, fix_scale, outlier_fraction, noise_px=1.0, cam2=None, th2=TH2, start=(0.03, 0.03, 0.05)):
    """dict: x3dc1, x3dc2 [n, 3], obs1, obs2 [n, 2], inv_sigma2_1, inv_sigma2_2 [n] (float32), cam1, cam2 [4], sim3_in [13]
    (the planted S12 perturbed by `start` = sigma of the rotation [rad], of log s, of t [m]: a few degrees, a few percent,
    and the translation error Sim3Solver leaves), th2, fix_scale, sim3_true (R [3, 3], t, s in float64), planted [n] bool."""
    # (the offset picks scenes that keep out of the guard bands -- a property of this reference alone: tests/test_optimize_sim3_ref.py)
    rng = np.random.default_rng(SEED_OFFSET + 1000 * seed + n)
    cam1 = CAM_A
    cam2 = CAM_A if cam2 is None else np.asarray(cam2, f32)
    R = rodrigues(rng.normal(0, 0.1, 3))
    t = rng.normal(0, 0.3, 3)
    s = 1.0 if fix_scale else float(rng.uniform(0.8, 1.25))
    # X2 in front of camera 2 and inside its image; X1 = S12 X2
    z = rng.uniform(6, 40, n)
    px = rng.uniform(150, W_IMG - 150, n)
    py = rng.uniform(60, H_IMG - 60, n)
    X2 = np.stack([(px - cam2[2]) / cam2[0] * z, (py - cam2[3]) / cam2[1] * z, z], axis=1)
    X1 = s * X2 @ R.T + t
    X1f, X2f = X1.astype(f32), X2.astype(f32)
    o1, o2 = [], []
    for X, K, o in ((X1, cam1, o1), (X2, cam2, o2)):
        octave = rng.integers(0, LEVELS, n)
        sigma = float(SCALE) ** octave
        u = K[0] * X[:, 0] / X[:, 2] + K[2] + rng.normal(0, 1, n) * noise_px * sigma
        v = K[1] * X[:, 1] / X[:, 2] + K[3] + rng.normal(0, 1, n) * noise_px * sigma
        o += [np.stack([u, v], axis=1), octave, sigma]
    planted = rng.random(n) < outlier_fraction
    ang = rng.uniform(0, 2 * np.pi, n)
    side = rng.random(n) < 0.5
    for o, mine in ((o1, side), (o2, ~side)):  # gross: 30 px or more off, in one of the two images
        off = rng.uniform(30, 120, n) * o[2]
        o[0] = np.where((planted & mine)[:, None], o[0] + np.stack([off * np.cos(ang), off * np.sin(ang)], axis=1), o[0])
    dR = rodrigues(rng.normal(0, start[0], 3))
    ds = 1.0 if fix_scale else float(np.exp(rng.normal(0, start[1])))
    dt = rng.normal(0, start[2], 3)
    rec = np.concatenate([(dR @ R).reshape(9), dt + t, [ds * s]]).astype(f32)
    return dict(x3dc1=X1f, x3dc2=X2f, obs1=o1[0].astype(f32), obs2=o2[0].astype(f32), inv_sigma2_1=INV_LEVEL_SIGMA2[o1[1]],
                inv_sigma2_2=INV_LEVEL_SIGMA2[o2[1]], cam1=cam1.copy(), cam2=cam2.copy(), sim3_in=rec, th2=f32(th2),
                fix_scale=int(bool(fix_scale)), sim3_true=(R, t, s), planted=planted)


SEED_OFFSET = 4200

# the GPU test's problems (tests/test_gpu_optimize_sim3.py): every size with fix_scale 0 / 1 and 0 % / 20 % planted outliers
SIZES = (0, 1, 9, 10, 63, 64, 65, 129, 300)
OUTLIERS = (0.0, 0.2)
# per problem, the first seed whose scene keeps out of the guard bands and classifies and iterates alike in both summation
# orders and with both Jacobians (0 where not listed); tests/test_optimize_sim3_ref.py re-checks the conditions for every scene
SEEDS = {(9, 1, 0.0): 3, (10, 1, 0.0): 32, (63, 0, 0.0): 1, (63, 1, 0.0): 1, (64, 0, 0.2): 1, (64, 1, 0.2): 3, (65, 1, 0.0): 2,
         (65, 1, 0.2): 4, (129, 1, 0.0): 1, (300, 1, 0.2): 4}
# n = 14 of which round one leaves 9: the early return with five erasures (seed found by search: tests/test_optimize_sim3_ref.py)
EARLY = ("n14-to-9", 0)
# The stale-error search of tests/test_optimize_sim3_ref.py
STALE_SHAPES, STALE_SEEDS, STALE_SEED = (20, 64), 60, None


def gpu_scenes():
    """(id, scene) of every problem the GPU test runs."""
    out = []
    for n in SIZES:
        for fix in (0, 1):
            for of in OUTLIERS:
                out.append((f"n{n}-fix{fix}-out{int(of * 100)}", scene(SEEDS.get((n, fix, of), 0), n, fix, of)))
    if EARLY[1] is not None:
        out.append((EARLY[0], early_scene(EARLY[1])))
    return out


def early_scene(seed):
    """14 pairs of which 5 are planted outliers, with a second camera of its own."""
    sc = scene(seed, 14, 0, 0.0, cam2=CAM_B)
    rng = np.random.default_rng(seed)
    idx = rng.permutation(14)[:5]
    sc["obs1"][idx] += f32(60.0)
    sc["planted"][idx] = True
    return sc


def run(sc, reverse=False, jacobian="analytic"):
    return optimize_sim3(sc["x3dc1"], sc["x3dc2"], sc["obs1"], sc["obs2"], sc["inv_sigma2_1"], sc["inv_sigma2_2"], sc["cam1"],
                         sc["cam2"], sc["sim3_in"], sc["th2"], sc["fix_scale"], reverse=reverse, jacobian=jacobian)


def guard_violations(sc, res):
    """What of a scene lies inside the guard bands: a classification chi2 within GUARD_CHI2 (relative) of th2, or a depth
    (S12 X2, S12^-1 X1 at the planted transform) with |z| < GUARD_Z."""
    out = []
    th2 = float(sc["th2"])
    for r in range(res["rounds"]):
        for key in ("cls_chi2_12", "cls_chi2_21"):
            with np.errstate(all="ignore"):
                near = np.abs(res[key][r] / th2 - 1.0) <= GUARD_CHI2
            if near.any():
                out.append((key, r, np.flatnonzero(near).tolist()))
    R, t, s = sc["sim3_true"]
    z12 = s * sc["x3dc2"].astype(np.float64) @ R[2] + t[2]
    z21 = ((sc["x3dc1"].astype(np.float64) - t) @ R)[:, 2] / s
    for name, z in (("z12", z12), ("z21", z21)):
        if (np.abs(z) < GUARD_Z).any():
            out.append((name, np.flatnonzero(np.abs(z) < GUARD_Z).tolist()))
    return out
