"""Reference of Optimizer::PoseOptimization (src/Optimizer.cc:256-473) for orbfe_pose_optimization: a float64 restatement
of the one graph it builds -- one free VertexSE3Expmap, unary EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose
edges, Huber kernel, Levenberg on a dense 6 x 6 system -- written from

* Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp} (computeError, cam_project :290-306, linearizeOplus :266-288, :335-364),
* Thirdparty/g2o/g2o/types/se3quat.h (exp :223-257, operator* :104-110, map :217-220, normalizeRotation :280-285),
* Thirdparty/g2o/g2o/core/base_unary_edge.hpp:43-72 (constructQuadraticForm), robust_kernel_impl.cpp:78-91 (Huber),
* Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189, sparse_optimizer.cpp:100-114, :354-419,
* src/Converter.cc:37-71 (toSE3Quat, toCvMat) and Eigen's Quaternion <-> rotation-matrix conversions.

Per-edge arithmetic is elementwise numpy float64 (IEEE, no contraction: the same bits a scalar loop gives); the sums over
edges of H, b and the robust chi2 are strictly sequential in edge order (np.cumsum), or in reversed order with
reverse=True -- the difference of the two is the reordering noise the GPU tolerance is built on
(tests/test_pose_opt_ref.py).  Mono edges are carried as three-row edges whose third row is zero: adding +0.0 changes no
sum.  The 6 x 6 solve is an unpivoted LDL^T; a non-positive pivot is a failed factorisation.
"""
import math

import numpy as np

from frustum_ref import CX, CY, FX, FY, MBF, rodrigues

f32 = np.float32
K5 = (FX, FY, CX, CY, MBF)
SCALE, LEVELS = 1.2, 8
INV_LEVEL_SIGMA2 = np.array([1.0 / (f32(SCALE) ** (2 * l)) for l in range(LEVELS)], dtype=f32)  # mvInvLevelSigma2
DELTA_MONO = float(f32(math.sqrt(5.991)))    # const float deltaMono (Optimizer.cc:291)
DELTA_STEREO = float(f32(math.sqrt(7.815)))  # :292
THR_MONO, THR_STEREO = f32(5.991), f32(7.815)  # chi2Mono / chi2Stereo (:391-392)
DBL_MAX = float(np.finfo(np.float64).max)
GUARD_CHI2, GUARD_Z = 1e-3, 0.1


# ---------------------------------------------------------------------------------------------------------------------
# SE3Quat: (q = (x, y, z, w), t) in Python floats (binary64)
def quat_from_R(m):
    """Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other,3,3>)."""
    t = m[0][0] + m[1][1] + m[2][2]
    q = [0.0, 0.0, 0.0, 0.0]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2][1] - m[1][2]) * t
        q[1] = (m[0][2] - m[2][0]) * t
        q[2] = (m[1][0] - m[0][1]) * t
    else:
        i = 0
        if m[1][1] > m[0][0]:
            i = 1
        if m[2][2] > m[i][i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k][j] - m[j][k]) * t
        q[j] = (m[j][i] + m[i][j]) * t
        q[k] = (m[k][i] + m[i][k]) * t
    return q


def normalize_rotation(q):
    """se3quat.h:280-285."""
    if q[3] < 0:
        q = [-c for c in q]
    n = math.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [c / n for c in q]


def quat_mul(a, b):
    """Eigen quat_product: a * b."""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by,
            aw * by + ay * bw + az * bx - ax * bz,
            aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def quat_rotate(q, X, Y, Z):
    """Eigen QuaternionBase::_transformVector: uv = 2 (q.vec x v); v + w uv + q.vec x uv.  X, Y, Z: floats or arrays."""
    qx, qy, qz, qw = q
    uvx = qy * Z - qz * Y
    uvy = qz * X - qx * Z
    uvz = qx * Y - qy * X
    uvx = uvx + uvx
    uvy = uvy + uvy
    uvz = uvz + uvz
    return ((X + qw * uvx) + (qy * uvz - qz * uvy),
            (Y + qw * uvy) + (qz * uvx - qx * uvz),
            (Z + qw * uvz) + (qx * uvy - qy * uvx))


def quat_to_R(q):
    """Eigen QuaternionBase::toRotationMatrix."""
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1.0 - (tyy + tzz), txy - twz, txz + twy],
            [txy + twz, 1.0 - (txx + tzz), tyz - twx],
            [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]


def to_se3quat(Tcw):
    """Converter::toSE3Quat (src/Converter.cc:37-47): float -> double, Quaterniond(R), normalizeRotation."""
    T = np.asarray(Tcw, dtype=f32).reshape(4, 4)
    R = [[float(T[r, c]) for c in range(3)] for r in range(3)]
    return normalize_rotation(quat_from_R(R)), [float(T[r, 3]) for r in range(3)]


def to_cvmat(q, t):
    """Converter::toCvMat(SE3Quat) (src/Converter.cc:49-71): to_homogeneous_matrix, double -> float."""
    R = quat_to_R(q)
    out = np.zeros((4, 4), f32)
    for r in range(3):
        for c in range(3):
            out[r, c] = f32(R[r][c])
        out[r, 3] = f32(t[r])
    out[3, 3] = f32(1.0)
    return out


def _matmul3(A, B):
    return [[(A[r][0] * B[0][c] + A[r][1] * B[1][c]) + A[r][2] * B[2][c] for c in range(3)] for r in range(3)]


def se3_exp(x):
    """SE3Quat::exp (se3quat.h:223-257): x = (omega, upsilon); pow(theta, 3) taken as theta * theta * theta."""
    wx, wy, wz = x[0], x[1], x[2]
    ups = x[3:6]
    theta = math.sqrt(wx * wx + wy * wy + wz * wz)
    Om = [[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]]
    Om2 = _matmul3(Om, Om)
    I = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    if theta < 0.00001:
        R = [[(I[r][c] + Om[r][c]) + Om2[r][c] for c in range(3)] for r in range(3)]
        V = R
    else:
        a = math.sin(theta) / theta
        b = (1.0 - math.cos(theta)) / (theta * theta)
        c3 = (theta - math.sin(theta)) / (theta * theta * theta)
        R = [[(I[r][c] + a * Om[r][c]) + b * Om2[r][c] for c in range(3)] for r in range(3)]
        V = [[(I[r][c] + b * Om[r][c]) + c3 * Om2[r][c] for c in range(3)] for r in range(3)]
    t = [(V[r][0] * ups[0] + V[r][1] * ups[1]) + V[r][2] * ups[2] for r in range(3)]
    return normalize_rotation(quat_from_R(R)), t  # SE3Quat(Quaterniond, Vector3d) normalises


def se3_mul(a, b):
    """SE3Quat::operator* (se3quat.h:104-110): t = a.t + a.r * b.t; r = a.r * b.r; normalizeRotation."""
    qa, ta = a
    qb, tb = b
    rx, ry, rz = quat_rotate(qa, tb[0], tb[1], tb[2])
    return normalize_rotation(quat_mul(qa, qb)), [ta[0] + rx, ta[1] + ry, ta[2] + rz]


# ---------------------------------------------------------------------------------------------------------------------
def solve_ldlt(H, lam, b):
    """(H + lam I) x = b by unpivoted LDL^T on the upper triangle; (ok, x), ok False on a pivot <= 0 (or NaN)."""
    A = [[H[r][c] for c in range(6)] for r in range(6)]
    for j in range(6):
        A[j][j] = A[j][j] + lam
    L = [[0.0] * 6 for _ in range(6)]
    D = [0.0] * 6
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - (L[j][k] * L[j][k]) * D[k]
        if not d > 0.0:
            return False, [0.0] * 6
        D[j] = d
        for i in range(j + 1, 6):
            s = A[j][i]
            for k in range(j):
                s = s - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = s / d
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i] / D[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s
    return True, x


TRI = [(r, c) for r in range(6) for c in range(r, 6)]  # the 21 upper-triangle entries, row-major


class _Edges:
    def __init__(self, xw, u, v, ur, inv_sigma2, K5_):
        xw = np.asarray(xw, f32).reshape(-1, 3)
        self.n = len(xw)
        self.X, self.Y, self.Z = [xw[:, i].astype(np.float64) for i in range(3)]
        self.u = np.asarray(u, f32).astype(np.float64)
        self.v = np.asarray(v, f32).astype(np.float64)
        self.ur = np.asarray(ur, f32).astype(np.float64)
        self.w = np.asarray(inv_sigma2, f32).astype(np.float64)
        self.stereo = self.ur >= 0  # mvuRight[i] < 0: monocular (Optimizer.cc:307)
        self.fx, self.fy, self.cx, self.cy, self.bf = [float(f32(k)) for k in K5_]
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.dsqr = self.delta * self.delta

    def error(self, pose, jac):
        """chi2 [n] at `pose`, and with jac the rows J [3][6] and e [3] of every edge."""
        q, t = pose
        with np.errstate(all="ignore"):
            rx, ry, rz = quat_rotate(q, self.X, self.Y, self.Z)
            x, y, z = rx + t[0], ry + t[1], rz + t[2]  # SE3Quat::map: _r * xyz + _t
            # mono: obs - (x / z * fx + cx, y / z * fy + cy) (project2d + cam_project, types_six_dof_expmap.cpp:290-296)
            m0 = self.u - ((x / z) * self.fx + self.cx)
            m1 = self.v - ((y / z) * self.fy + self.cy)
            # stereo: const float invz = 1.0f / trans_xyz[2] (:299-306)
            invz_f = (1.0 / z).astype(f32).astype(np.float64)
            p0 = (x * invz_f) * self.fx + self.cx
            p1 = (y * invz_f) * self.fy + self.cy
            p2 = p0 - self.bf * invz_f
            e0 = np.where(self.stereo, self.u - p0, m0)
            e1 = np.where(self.stereo, self.v - p1, m1)
            e2 = np.where(self.stereo, self.ur - p2, 0.0)
            chi2 = (e0 * (self.w * e0) + e1 * (self.w * e1)) + e2 * (self.w * e2)
            if not jac:
                return chi2, None, None
            invz = 1.0 / z
            invz_2 = invz * invz
            fx, fy, bf = self.fx, self.fy, self.bf
            zero = np.zeros(self.n)
            J0 = [x * y * invz_2 * fx, -(1.0 + (x * x * invz_2)) * fx, y * invz * fx, -invz * fx, zero, x * invz_2 * fx]
            J1 = [(1.0 + y * y * invz_2) * fy, -x * y * invz_2 * fy, -x * invz * fy, zero, -invz * fy, y * invz_2 * fy]
            J2 = [J0[0] - bf * y * invz_2, J0[1] + bf * x * invz_2, J0[2], J0[3], zero, J0[5] - bf * invz_2]
            J2 = [np.where(self.stereo, a, 0.0) for a in J2]
        return chi2, (J0, J1, J2), (e0, e1, e2)


def _seq_sum(cols, reverse):
    """Strictly sequential sums of the columns of cols [n, k], first edge first (last first with reverse)."""
    if len(cols) == 0:
        return np.zeros(cols.shape[1])
    return np.cumsum(cols[::-1] if reverse else cols, axis=0)[-1]


def pose_optimization(xw, u, v, u_right, inv_sigma2, K5_, Tcw, reverse=False):
    """-> dict: n_inliers (the return value), Tcw [4,4] float32, outlier [n] uint8 (None when n < 3: untouched), rounds, and
    per round run: iterations, trials, lam, chi2 (robust chi2 of the estimate), edge_chi2 [n] (the classification chi2),
    last_rejected, last_rho, stale_gap (largest relative difference, over the round's inlier edges, between the chi2 g2o
    holds -- that of the last evaluated trial -- and the chi2 recomputed at the estimate: 0 unless the last trial was rejected)."""
    E = _Edges(xw, u, v, u_right, inv_sigma2, K5_)
    n = E.n
    start = to_se3quat(Tcw)
    out = dict(n_inliers=0, Tcw=np.asarray(Tcw, f32).reshape(4, 4).copy(), outlier=None, rounds=0, iterations=[], trials=[],
               lam=[], chi2=[], edge_chi2=[], last_rejected=[], last_rho=[], stale_gap=[])
    if n < 3:  # nInitialCorrespondences < 3 (Optimizer.cc:385)
        return out
    level = np.zeros(n, np.uint8)
    robust = True
    stored = np.zeros(n)  # chi2 of what g2o holds in _error of every edge
    est = start
    nBad = 0
    thr = np.where(E.stereo, THR_STEREO, THR_MONO).astype(f32)
    for rnd in range(4):
        est = start  # vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw)) (:399)
        active = level == 0
        iters = trials = 0
        lam = cur = 0.0
        rejected, rho = False, 0.0
        if active.any():  # (no active edge: _ivMap is empty, optimize() returns at once)
            ni, nBadLM = 2.0, 0
            for it in range(10):
                with np.errstate(all="ignore"):
                    chi2, J, e = E.error(est, True)
                    stored = np.where(active, chi2, stored)
                    over = (chi2 > E.dsqr) & robust  # Huber (robust_kernel_impl.cpp:78-91)
                    sq = np.sqrt(chi2)
                    rho0 = np.where(over, 2 * sq * E.delta - E.dsqr, chi2)
                    rho1 = np.where(over, E.delta / sq, 1.0)
                    wr = rho1 * E.w
                    we = [wr * e[r] for r in range(3)]
                    cols = [(J[0][r] * wr) * J[0][c] + (J[1][r] * wr) * J[1][c] + (J[2][r] * wr) * J[2][c] for r, c in TRI]
                    cols += [J[0][j] * we[0] + J[1][j] * we[1] + J[2][j] * we[2] for j in range(6)]
                    cols.append(rho0)
                    S = _seq_sum(np.where(active[:, None], np.stack(cols, axis=1), 0.0), reverse)
                H = [[0.0] * 6 for _ in range(6)]
                for k, (r, c) in enumerate(TRI):
                    H[r][c] = H[c][r] = float(S[k])
                b = [-float(S[21 + j]) for j in range(6)]  # b -= rho1 J^T Omega e
                cur = ini = float(S[27])
                if it == 0:  # computeLambdaInit: tau = 1e-5
                    lam = 1e-5 * max(0.0, *[abs(H[j][j]) for j in range(6)])
                    ni, nBadLM = 2.0, 0
                rho, q = 0.0, 0
                while True:
                    ok, x = solve_ldlt(H, lam, b)
                    trial = se3_mul(se3_exp(x), est)  # VertexSE3Expmap::oplusImpl
                    with np.errstate(all="ignore"):
                        chi2, _, _ = E.error(trial, False)
                        stored = np.where(active, chi2, stored)
                        over = (chi2 > E.dsqr) & robust
                        rho0 = np.where(over, 2 * np.sqrt(chi2) * E.delta - E.dsqr, chi2)
                        temp = float(_seq_sum(np.where(active, rho0, 0.0)[:, None], reverse)[0])
                    if not ok:
                        temp = DBL_MAX
                    scale = 0.0
                    for j in range(6):
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
        # classification (Optimizer.cc:403-463): outlier edges are recomputed at the estimate, inliers keep _error
        with np.errstate(all="ignore"):
            fresh, _, _ = E.error(est, False)
            cls = np.where(level == 1, fresh, stored)
            gap = np.abs(fresh - stored)[(level == 0) & (stored != 0)] / np.abs(stored[(level == 0) & (stored != 0)])
            stored = cls.copy()
            bad = cls.astype(f32) > thr  # (a NaN chi2 is an inlier)
        level = bad.astype(np.uint8)
        nBad = int(bad.sum())
        if rnd == 2:
            robust = False
        out["rounds"] = rnd + 1
        for key, val in (("iterations", iters), ("trials", trials), ("lam", lam), ("chi2", cur), ("edge_chi2", cls),
                         ("last_rejected", rejected), ("last_rho", rho),
                         ("stale_gap", float(gap.max(initial=0.0)))):
            out[key].append(val)
        if n < 10:  # optimizer.edges().size() < 10 (:462)
            break
    out["Tcw"] = to_cvmat(*est)
    out["outlier"] = level.copy()
    out["n_inliers"] = n - nBad
    return out


# ---------------------------------------------------------------------------------------------------------------------
def scene(seed, n, stereo_fraction, outlier_fraction, noise_px=1.0, all_outliers=False):
    """dict: xw [n,3], u, v, u_right, inv_sigma2 [n] (float32), octave, K5, Tcw (the perturbed start pose, float32 4x4),
    Tcw_true, planted [n] bool."""
    # (the offset picks scenes that keep out of the guard bands -- a property of this reference alone: tests/test_pose_opt_ref.py)
    rng = np.random.default_rng(SEED_OFFSET + 1000 * seed + n)
    R = rodrigues(rng.normal(0, 0.2, 3))
    t = rng.normal(0, 0.5, 3)
    Ttrue = np.eye(4)
    Ttrue[:3, :3], Ttrue[:3, 3] = R, t
    Ttrue = Ttrue.astype(f32)
    R, t = Ttrue[:3, :3].astype(np.float64), Ttrue[:3, 3].astype(np.float64)
    # points in front of the camera, inside the image
    z = rng.uniform(4, 40, n)
    px = rng.uniform(20, 1220, n)
    py = rng.uniform(20, 356, n)
    Pc = np.stack([(px - CX) / FX * z, (py - CY) / FY * z, z], axis=1)
    xw = ((Pc - t) @ R).astype(f32)  # R^T (Pc - t)
    Pc = xw.astype(np.float64) @ R.T + t
    octave = rng.integers(0, LEVELS, n)
    sigma = float(SCALE) ** octave
    uu = FX * Pc[:, 0] / Pc[:, 2] + CX + rng.normal(0, 1, n) * noise_px * sigma
    vv = FY * Pc[:, 1] / Pc[:, 2] + CY + rng.normal(0, 1, n) * noise_px * sigma
    rr = uu - MBF / Pc[:, 2] + rng.normal(0, 1, n) * noise_px * sigma * 0.5
    stereo = rng.random(n) < stereo_fraction
    planted = np.ones(n, bool) if all_outliers else rng.random(n) < outlier_fraction
    ang = rng.uniform(0, 2 * np.pi, n)
    off = rng.uniform(30, 120, n) * sigma  # gross: 30 px or more off
    uu = np.where(planted, uu + off * np.cos(ang), uu)
    vv = np.where(planted, vv + off * np.sin(ang), vv)
    rr = np.where(stereo, np.maximum(rr, 0.0), -1.0)
    dT = np.eye(4)
    dT[:3, :3] = rodrigues(rng.normal(0, 0.004, 3))  # a few tenths of a degree
    dT[:3, 3] = rng.normal(0, 0.03, 3)               # a few centimetres
    Tstart = (dT @ Ttrue.astype(np.float64)).astype(f32)
    return dict(xw=xw, u=uu.astype(f32), v=vv.astype(f32), u_right=rr.astype(f32), inv_sigma2=INV_LEVEL_SIGMA2[octave],
                octave=octave.astype(np.int32), K5=np.array(K5, f32), Tcw=Tstart, Tcw_true=Ttrue, planted=planted)


SEED_OFFSET = 7100

# the GPU test's problems (tests/test_gpu_pose_opt.py): every size with mono only / stereo only / mixed, 0 % and 20 % planted
SIZES = (2, 3, 9, 10, 63, 64, 65, 257, 2000)
KINDS = {"mono": 0.0, "stereo": 1.0, "mixed": 0.5}
OUTLIERS = (0.0, 0.2)
# per problem, the first seed whose scene keeps out of the guard bands and classifies alike in both summation orders (0 where
# not listed); tests/test_pose_opt_ref.py re-checks both conditions for every scene
SEEDS = {(63, "stereo", 0.0): 1, (257, "stereo", 0.0): 1, (2000, "mono", 0.0): 3, (2000, "mono", 0.2): 1,
         (2000, "stereo", 0.0): 11, (2000, "stereo", 0.2): 1, (2000, "mixed", 0.0): 1, (2000, "mixed", 0.2): 7}
# Above kPoseOptLdsEdges = 2048 edges (csrc/poseopt_kernels.h) the kernel re-reads the edge constants from global memory:
# the smallest size on that path, and the frame limit.  At 16384 edges and unit noise some 20 classification chi2 fall inside
# the guard band (density 0.025 of a chi2 of 2 degrees of freedom at 5.991, band 0.012 wide, 4 rounds), so no seed keeps clear
# of it; with a quarter of the noise the inliers' chi2 stay below 1 and only the planted outliers lie above the threshold.
BIG = (("n2049-mono-out20", 3, 2049, 0.0, 0.2, 1.0), ("n2049-stereo-out20", 2, 2049, 1.0, 0.2, 1.0),
       ("n2049-mixed-out20", 2, 2049, 0.5, 0.2, 1.0), ("n16384-mixed-out20-quiet", 0, 16384, 0.5, 0.2, 0.25))
# The stale-error search of tests/test_pose_opt_ref.py: seeds 0..199 of STALE_PROBLEM and seeds 0..29 of every other STALE_SHAPES
# problem (mono / stereo / mixed, 0 % and 20 % outliers).  No round ends on a rejected trial with |rho| > STALE_RHO: a last trial is rejected only at convergence,
# where the step is noise (|rho| < 1e-8, or cur == trial chi2 to the bit).  There the chi2 an inlier keeps and the chi2
# recomputed at the estimate differ by less than the GPU tolerance, so NO test tells a kernel that keeps the stale error
# from one that recomputes it; the rule is implemented as the reference states it and is not discriminated.
STALE_PROBLEM, STALE_SHAPES, STALE_RHO, STALE_SEED = (64, "mixed", 0.2), (10, 64), 1e-3, None


def gpu_scenes():
    """(id, scene) of every problem the GPU test runs."""
    out = []
    for n in SIZES:
        for kind, sf in KINDS.items():
            for of in OUTLIERS:
                out.append((f"n{n}-{kind}-out{int(of * 100)}", scene(SEEDS.get((n, kind, of), 0), n, sf, of)))
    for id_, seed, n, sf, of, noise in BIG:
        out.append((id_, scene(seed, n, sf, of, noise_px=noise)))
    return out


def run(sc, reverse=False):
    return pose_optimization(sc["xw"], sc["u"], sc["v"], sc["u_right"], sc["inv_sigma2"], sc["K5"], sc["Tcw"], reverse=reverse)


def guard_violations(sc, res):
    """What of a scene lies inside the guard bands: classification chi2 within 1e-3 (relative) of its threshold in any
    round, or a point with |z| < 0.1 at the true pose."""
    bad = []
    thr = np.where(sc["u_right"] >= 0, float(THR_STEREO), float(THR_MONO))
    for r, c in enumerate(res["edge_chi2"]):
        with np.errstate(all="ignore"):
            near = np.abs(c / thr - 1.0) <= GUARD_CHI2
        if near.any():
            bad.append(("chi2", r, np.flatnonzero(near).tolist()))
    T = sc["Tcw_true"].astype(np.float64)
    z = sc["xw"].astype(np.float64) @ T[2, :3] + T[2, 3]
    if (np.abs(z) < GUARD_Z).any():
        bad.append(("z", np.flatnonzero(np.abs(z) < GUARD_Z).tolist()))
    return bad
