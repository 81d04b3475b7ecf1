"""An independent NumPy float64 restatement of PnPsolver (src/PnPsolver.cc): EPnP (compute_pose), CheckInliers,
SetRansacParameters, iterate() with its real, stateful Refine() calls, and the replay of iterate() over precomputed
prefix-maximum Refine records.  The well-posed decompositions are numpy.linalg's; the null-space basis of the 4-point
problem is written here with its own Householder reflectors (reflector k maps its column to -sign(alpha) |x| e_1,
sign(0) = +1; ut rows 8 .. 11 = Q e_8 .. Q e_11), not LAPACK's Q.  Also the scenes of the GPU and CPU tests, the guards
that decide which records are compared by value, and the comparison itself."""
import math
from pathlib import Path

import numpy as np

OK, NONFINITE = 0, 1
F32 = np.float32


# ----------------------------------------------------------------------------------------------- EPnP
def null_basis4(M):
    """M [8, 12] -> (v1..v4) = Q e_11, Q e_10, Q e_9, Q e_8 of the Householder QR of M^T."""
    a = np.array(M.T, np.float64)  # 12 x 8
    refl = []
    for k in range(8):
        x = a[k:, k].copy()
        alpha, nrm = x[0], math.sqrt(float(np.dot(x, x)))
        v = x.copy()
        v[0] = alpha + nrm if alpha >= 0.0 else alpha - nrm
        vv = float(np.dot(v, v))
        refl.append((v, vv))
        if not vv > 0.0:
            continue
        a[k:, k:] -= np.outer(v, (2.0 / vv) * (v @ a[k:, k:]))
    out = []
    for j in (11, 10, 9, 8):
        e = np.zeros(12)
        e[j] = 1.0
        for k in range(7, -1, -1):
            v, vv = refl[k]
            if vv > 0.0:
                e[k:] -= v * (2.0 * float(np.dot(v, e[k:])) / vv)
        out.append(e)
    return np.array(out)


def control_points(pw):
    """:401-445, with the sign rule: every row of UCt has its component of largest magnitude positive."""
    n = len(pw)
    c0 = pw.sum(0) / n
    pw0 = pw - c0
    U, dc, _ = np.linalg.svd(pw0.T @ pw0)  # :436 (symmetric: U = V)
    cws = np.zeros((4, 3))
    cws[0] = c0
    for i in range(1, 4):
        r = U[:, i - 1]
        r = r if r[int(np.argmax(np.abs(r)))] >= 0 else -r
        cws[i] = c0 + math.sqrt(dc[i - 1] / n) * r  # :441-443
    return cws


def pinv3(cc):
    """cvInvert(CV_SVD) (:473): singular values <= 2 eps (w0 + w1 + w2) count as zero."""
    U, w, Vt = np.linalg.svd(cc)
    iw = np.where(w > 2.0 * np.finfo(float).eps * w.sum(), 1.0 / np.where(w > 0, w, 1.0), 0.0)
    return (Vt.T * iw) @ U.T


def compute_pose(pw, us, cam, full=False):
    """compute_pose (:544-598) on pw [n, 3], us [n, 2] (float64), cam = fu fv uc vc.  -> R [3, 3], t [3]; full: a dict with
    the three candidates and the quantities the guards read."""
    with np.errstate(all="ignore"):
        return _compute_pose(np.asarray(pw, np.float64), np.asarray(us, np.float64), [float(c) for c in cam], full)


def _compute_pose(pw, us, cam, full):
    fu, fv, uc, vc = cam
    n = len(pw)
    cws = control_points(pw)
    cc = (cws[1:4] - cws[0]).T  # :471
    ci = pinv3(cc)
    al = np.zeros((n, 4))
    al[:, 1:] = (pw - cws[0]) @ ci.T  # :480-483
    al[:, 0] = 1.0 - al[:, 1] - al[:, 2] - al[:, 3]
    M = np.zeros((2 * n, 12))  # :495-510
    for i in range(4):
        M[0::2, 3 * i] = al[:, i] * fu
        M[0::2, 3 * i + 2] = al[:, i] * (uc - us[:, 0])
        M[1::2, 3 * i + 1] = al[:, i] * fv
        M[1::2, 3 * i + 2] = al[:, i] * (vc - us[:, 1])
    if _PERTURB is not None:  # measure_noise(): every entry of M moved by at most one unit in the last place
        M = M * (1.0 + _PERTURB.integers(-1, 2, M.shape) * np.finfo(float).eps / 2)
    info = {}
    if not np.all(np.isfinite(M)):
        nan = np.full((3, 3), np.nan), np.full(3, np.nan)
        return (nan + ({"ill": True, "cands": []},)) if full else nan
    if n == 4:
        v = null_basis4(M)
        s = np.linalg.svd(M, compute_uv=False)
        info["sv8"] = s[7] / s[0] if s[0] > 0 else 0.0
    else:
        w, V = np.linalg.eigh(M.T @ M)  # ascending: column 0 is ut row 11
        v = V[:, :4].T
        if _PERTURB is not None:
            v = -v
        g = [(w[i + 1] - w[i]) / abs(w[i + 1]) if w[i + 1] != 0 else 0.0 for i in range(4)]
        info["gap"] = min(g)
    info["cond"] = np.linalg.cond(cc)
    # compute_L_6x10 (:881-926), compute_rho (:929-937)
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    L = np.zeros((6, 10))
    rho = np.zeros(6)
    for r, (a, b) in enumerate(pairs):
        dv = [v[k][3 * a:3 * a + 3] - v[k][3 * b:3 * b + 3] for k in range(4)]
        L[r] = [dv[0] @ dv[0], 2 * dv[0] @ dv[1], dv[1] @ dv[1], 2 * dv[0] @ dv[2], 2 * dv[1] @ dv[2], dv[2] @ dv[2],
                2 * dv[0] @ dv[3], 2 * dv[1] @ dv[3], 2 * dv[2] @ dv[3], dv[3] @ dv[3]]
        rho[r] = np.sum((cws[a] - cws[b]) ** 2)
    cands = []
    for which in (1, 2, 3):
        betas = _find_betas(L, rho, which)
        betas = _gauss_newton(L, rho, betas)
        cands.append(_R_and_t(v, betas, al, pw, us, cam))
    N = 0  # :591-593
    if cands[1][2] < cands[0][2]:
        N = 1
    if cands[2][2] < cands[N][2]:
        N = 2
    if full:
        # two of the three errors within 1e-9 relative: the choice of N could flip.  Where the two tied candidates are one
        # and the same pose (Gauss-Newton has converged to it from both starts: the rule with n >> 4) a flip changes
        # nothing and the item is compared by value all the same, which asks more than excluding it would
        order = sorted(range(3), key=lambda i: cands[i][2])
        flip = not np.all(np.isfinite([c[2] for c in cands]))
        for i in range(2):
            a, b = cands[order[i]], cands[order[i + 1]]
            if not flip and abs(b[2] - a[2]) <= 1e-9 * abs(b[2]):
                flip = not pose_close(np.concatenate([b[0].reshape(9), b[1]]), a[0], a[1], 1e-9)[0]
        info["flip"] = bool(flip)
        info["cands"] = cands
        info["ill"] = bool(info.get("sv8", 1.0) < 1e-6 or info.get("gap", 1.0) < 1e-6 or not info["cond"] <= 1e8)
        return cands[N][0], cands[N][1], info
    return cands[N][0], cands[N][1]


_PERTURB = None


def _lstsq(A, b):
    if _PERTURB is not None:
        return np.linalg.pinv(A) @ b
    return np.linalg.lstsq(A, b, rcond=None)[0]


def measure_noise(scenes):
    """The restatement against itself over the hypotheses and Refine records of the scenes: a second run with every entry of
    M moved by at most one unit in the last place, the eigenvectors of M^T M negated and numpy.linalg.pinv in the place of
    lstsq.  -> the largest relative difference of R (Frobenius) and t over the items that are finite and not excluded."""
    global _PERTURB
    worst = 0.0
    for _, cands in scenes:
        for c in cands:
            items = [np.asarray(s) for s in c["sets"]]
            counts = []
            for s in c["sets"]:
                r = ref_item(c, s)
                counts.append(int(r["mask"].sum()))
            for h in scan_records(counts, c["min_inliers"]):
                items.append(np.flatnonzero(ref_item(c, c["sets"][h])["mask"]))
            for idx in items:
                a = ref_item(c, idx)
                _PERTURB = np.random.default_rng(len(idx))
                try:
                    b = ref_item(c, idx)
                finally:
                    _PERTURB = None
                if not (a["finite"] and b["finite"]) or a["info"]["ill"] or a["info"]["flip"] or b["info"]["ill"] or b["info"]["flip"]:
                    continue
                worst = max(worst, pose_close(np.concatenate([b["R"].reshape(9), b["t"]]), a["R"], a["t"], 0.0)[1])
    return worst


def _find_betas(L, rho, which):
    b = np.zeros(4)
    if which == 1:  # :767-794
        b4 = _lstsq(L[:, [0, 1, 3, 6]], rho)
        sg = -1.0 if b4[0] < 0 else 1.0
        b[0] = math.sqrt(sg * b4[0])
        b[1:] = sg * b4[1:] / b[0]
        return b
    x = _lstsq(L[:, :3] if which == 2 else L[:, :5], rho)  # :799-858
    if x[0] < 0:
        b[0] = math.sqrt(-x[0])
        b[1] = math.sqrt(-x[2]) if x[2] < 0 else 0.0
    else:
        b[0] = math.sqrt(x[0])
        b[1] = math.sqrt(x[2]) if x[2] > 0 else 0.0
    if x[1] < 0:
        b[0] = -b[0]
    if which == 3:
        b[2] = x[3] / b[0]
    return b


def _gauss_newton(L, rho, betas):
    """:941-989.  qr_solve (:991-1083) is a least-squares solve; its eta is a scale factor that cancels."""
    b = betas.copy()
    for _ in range(5):
        A = np.stack([2 * L[:, 0] * b[0] + L[:, 1] * b[1] + L[:, 3] * b[2] + L[:, 6] * b[3],
                      L[:, 1] * b[0] + 2 * L[:, 2] * b[1] + L[:, 4] * b[2] + L[:, 7] * b[3],
                      L[:, 3] * b[0] + L[:, 4] * b[1] + 2 * L[:, 5] * b[2] + L[:, 8] * b[3],
                      L[:, 6] * b[0] + L[:, 7] * b[1] + L[:, 8] * b[2] + 2 * L[:, 9] * b[3]], axis=1)
        bb = np.array([b[0] * b[0], b[0] * b[1], b[1] * b[1], b[0] * b[2], b[1] * b[2], b[2] * b[2], b[0] * b[3], b[1] * b[3],
                       b[2] * b[3], b[3] * b[3]])
        r = rho - L @ bb
        if not (np.all(np.isfinite(A)) and np.all(np.isfinite(r))):
            return np.full(4, np.nan)
        b = b + _lstsq(A, r)
    return b


def _R_and_t(v, betas, al, pw, us, cam):
    """compute_R_and_t (:748-759) -> (R, t, reprojection error)."""
    fu, fv, uc, vc = cam
    if not np.all(np.isfinite(betas)):
        return np.full((3, 3), np.nan), np.full(3, np.nan), np.nan
    ccs = (betas[:, None] * v).sum(0).reshape(4, 3)  # :513-525
    pcs = al @ ccs  # :528-537
    if pcs[0, 2] < 0.0:  # :722-735
        ccs, pcs = -ccs, -pcs
    pc0, pw0 = pcs.mean(0), pw.mean(0)  # :648-710
    abt = (pcs - pc0).T @ (pw - pw0)
    if not np.all(np.isfinite(abt)):
        return np.full((3, 3), np.nan), np.full(3, np.nan), np.nan
    U, _, Vt = np.linalg.svd(abt)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R[2] = -R[2]
    t = pc0 - R @ pw0
    pc = pw @ R.T + t  # :627-644
    iz = 1.0 / pc[:, 2]
    ue, ve = uc + fu * pc[:, 0] * iz, vc + fv * pc[:, 1] * iz
    return R, t, float(np.mean(np.sqrt((us[:, 0] - ue) ** 2 + (us[:, 1] - ve) ** 2)))


def check_inliers(R, t, cam, p3d, p2d, max_err2):
    """CheckInliers (:323-354) with the reference's float / double mix -> (mask [n] bool, error2 [n] float32)."""
    fu, fv, uc, vc = [float(F32(c)) for c in cam]
    P = np.asarray(p3d, F32).astype(np.float64)
    q = np.asarray(p2d, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        Xc = (R[0, 0] * P[:, 0] + R[0, 1] * P[:, 1] + R[0, 2] * P[:, 2] + t[0]).astype(F32)
        Yc = (R[1, 0] * P[:, 0] + R[1, 1] * P[:, 1] + R[1, 2] * P[:, 2] + t[1]).astype(F32)
        iz = (1.0 / (R[2, 0] * P[:, 0] + R[2, 1] * P[:, 1] + R[2, 2] * P[:, 2] + t[2])).astype(F32)
        ue = uc + fu * Xc.astype(np.float64) * iz.astype(np.float64)
        ve = vc + fv * Yc.astype(np.float64) * iz.astype(np.float64)
        dx, dy = (q[:, 0] - ue).astype(F32), (q[:, 1] - ve).astype(F32)
        e2 = dx * dx + dy * dy
        return e2 < np.asarray(max_err2, F32), e2


# ----------------------------------------------------------------------------------------------- RANSAC
def set_ransac_parameters(N, probability=0.99, minInliers=8, maxIterations=300, minSet=4, epsilon=0.4, th2=5.991):
    """:127-164 with its float and int conversions -> (mRansacMinInliers, mRansacMaxIts, mRansacEpsilon)."""
    eps = F32(epsilon)
    n_min = int(F32(N) * eps)  # :141 int = int * float, truncated
    n_min = max(n_min, minInliers, minSet)
    if N > 0 and eps < F32(n_min) / F32(N):  # :148
        eps = F32(n_min) / F32(N)
    if n_min == N:
        its = 1
    else:
        with np.errstate(all="ignore"):
            q = np.log(1 - probability) / np.log(1 - float(eps) ** 3) if N > 0 else np.nan
        its = int(math.ceil(q)) if np.isfinite(q) else 1
    return n_min, max(1, min(its, maxIterations)), float(eps)


def sets_from_draws(n, draws):
    """:201-214: draws [H, 4] -> sets [H, 4]."""
    out = []
    for d in draws:
        avail = list(range(n))
        s = []
        for r in d:
            s.append(avail[r])
            avail[r] = avail[-1]
            avail.pop()
        out.append(s)
    return np.array(out, np.int32).reshape(-1, 4)


def to_f32_pose(R, t):
    return np.concatenate([np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64)]).astype(F32)


class Solver:
    """PnPsolver with the real, stateful iterate() / Refine() (:178-320); the 4-sets come from `sets` in order."""

    def __init__(self, p3d, p2d, sigma2, cam, sets, kp_idx=None, n_kp=None, params=(0.99, 10, 300, 4, 0.5, 5.991)):
        self.p3d, self.p2d = np.asarray(p3d, F32), np.asarray(p2d, F32)
        self.cam = np.asarray(cam, F32)
        self.N = len(self.p3d)
        self.sets = np.asarray(sets, np.int32).reshape(-1, 4)
        self.kp_idx = np.arange(self.N) if kp_idx is None else np.asarray(kp_idx)
        self.n_kp = self.N if n_kp is None else n_kp
        self.min_inliers, self.max_its, self.eps = set_ransac_parameters(self.N, *params)
        self.max_err = (np.asarray(sigma2, F32) * F32(params[5])).astype(F32)  # :163
        self.its = 0
        self.best_n, self.best_mask, self.best_T = 0, None, None
        self.refine_calls = 0

    def pose(self, idx):
        R, t = compute_pose(self.p3d[idx].astype(np.float64), self.p2d[idx].astype(np.float64), self.cam)
        if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
            return R, t, np.zeros(self.N, bool)
        return R, t, check_inliers(R, t, self.cam, self.p3d, self.p2d, self.max_err)[0]

    def _vb(self, mask):
        vb = np.zeros(self.n_kp, bool)
        vb[self.kp_idx[mask]] = True  # :242-247
        return vb

    def iterate(self, nIterations):
        """-> (Tcw [12] float32 or None, bNoMore, vbInliers, nInliers)"""
        if self.N < self.min_inliers:  # :186
            return None, True, np.zeros(0, bool), 0
        cur = 0
        while self.its < self.max_its or cur < nIterations:  # :195, || as written
            if self.its >= len(self.sets):
                raise IndexError("out of hypotheses")
            cur += 1
            R, t, mask = self.pose(self.sets[self.its])
            self.its += 1
            n = int(mask.sum())
            if n >= self.min_inliers:
                if n > self.best_n:
                    self.best_n, self.best_mask, self.best_T = n, mask, to_f32_pose(R, t)
                self.refine_calls += 1
                Rr, tr, rmask = self.pose(np.flatnonzero(self.best_mask))  # Refine (:275-320)
                if int(rmask.sum()) > self.min_inliers:
                    return to_f32_pose(Rr, tr), False, self._vb(rmask), int(rmask.sum())
        if self.its >= self.max_its:  # :254
            if self.best_n >= self.min_inliers:
                return self.best_T, True, self._vb(self.best_mask), self.best_n
            return None, True, np.zeros(0, bool), 0
        return None, False, np.zeros(0, bool), 0


def scan_records(counts, min_inliers):
    best, rec = 0, []
    for h, c in enumerate(counts):
        if c >= min_inliers and c > best:
            best = c
            rec.append(h)
    return rec


class Replay:
    """iterate() as a scan over precomputed results: per-hypothesis (count, mask, pose) and per-record (count, mask, pose),
    records = scan_records(counts)."""

    def __init__(self, N, min_inliers, max_its, counts, masks, poses, rec_hyp, rec_counts, rec_masks, rec_poses, kp_idx=None,
                 n_kp=None):
        self.N, self.min_inliers, self.max_its = N, min_inliers, max_its
        self.counts, self.masks, self.poses = counts, masks, poses
        self.rec_hyp, self.rec_counts, self.rec_masks, self.rec_poses = list(rec_hyp), rec_counts, rec_masks, rec_poses
        self.kp_idx = np.arange(N) if kp_idx is None else np.asarray(kp_idx)
        self.n_kp = N if n_kp is None else n_kp
        self.its, self.best_n, self.best_h, self.rec = 0, 0, -1, -1

    def _vb(self, mask):
        vb = np.zeros(self.n_kp, bool)
        vb[self.kp_idx[np.asarray(mask, bool)]] = True
        return vb

    def iterate(self, nIterations):
        if self.N < self.min_inliers:
            return None, True, np.zeros(0, bool), 0
        cur = 0
        while self.its < self.max_its or cur < nIterations:
            if self.its >= len(self.counts):
                raise IndexError("out of hypotheses")
            cur += 1
            h = self.its
            self.its += 1
            n = int(self.counts[h])
            if n >= self.min_inliers:
                if n > self.best_n:
                    self.best_n, self.best_h = n, h
                    self.rec = self.rec_hyp.index(h)
                if int(self.rec_counts[self.rec]) > self.min_inliers:
                    return self.rec_poses[self.rec], False, self._vb(self.rec_masks[self.rec]), int(self.rec_counts[self.rec])
        if self.its >= self.max_its:
            if self.best_n >= self.min_inliers:
                return self.poses[self.best_h], True, self._vb(self.masks[self.best_h]), self.best_n
            return None, True, np.zeros(0, bool), 0
        return None, False, np.zeros(0, bool), 0


# ----------------------------------------------------------------------------------------------- scenes
CAM = np.array([517.3, 516.5, 318.6, 255.3], F32)


def _rot(rng):
    ax = rng.normal(size=3)
    ax /= np.linalg.norm(ax)
    th = rng.uniform(0.05, 0.6)
    Kx = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


def make_candidate(seed, n, H, inlier_frac=0.7, noise=0.3, spread=True):
    """Points in a box at 2-10 m depth seen by a camera of pose (R, t); 1 - inlier_frac of them get gross errors (>= 50
    px).  The 4-sets are drawn among inliers and outliers alike but (spread) only among sets whose image points are well
    spread: the minimal problem is then well conditioned (tests/test_pnp_ref.py asserts the exclusion caps)."""
    rng = np.random.default_rng(seed)
    R, t = _rot(rng), rng.uniform(-0.5, 0.5, 3)
    pc = np.stack([rng.uniform(-2.5, 2.5, n), rng.uniform(-2, 2, n), rng.uniform(2, 10, n)], 1)
    pw = (pc - t) @ R  # R^T (pc - t)
    p3d = pw.astype(F32)
    pcf = p3d.astype(np.float64) @ R.T + t
    uv = np.stack([CAM[0] * pcf[:, 0] / pcf[:, 2] + CAM[2], CAM[1] * pcf[:, 1] / pcf[:, 2] + CAM[3]], 1)
    uv += rng.normal(scale=noise, size=uv.shape) if noise else 0.0
    truth = np.ones(n, bool)
    n_out = int(round(n * (1 - inlier_frac)))
    if n_out:
        bad = rng.choice(n, n_out, replace=False)
        ang = rng.uniform(0, 2 * np.pi, n_out)
        uv[bad] += rng.uniform(50, 200, n_out)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
        truth[bad] = False
    p2d = uv.astype(F32)
    sigma2 = (F32(1.2) ** (2 * rng.integers(0, 4, n))).astype(F32)
    sets = []
    while len(sets) < H:
        s = rng.choice(n, 4, replace=False)
        if spread and n > 8:
            d = p2d[s].astype(np.float64)
            dd = np.linalg.norm(d[:, None] - d[None], axis=2)[np.triu_indices(4, 1)]
            if dd.min() < 60.0:
                continue
        sets.append(s)
    return dict(p3d=p3d, p2d=p2d, sigma2=sigma2, max_err=(sigma2 * F32(5.991)).astype(F32), cam=CAM.copy(),
                sets=np.array(sets, np.int32).reshape(-1, 4), truth=truth, R=R, t=t,
                min_inliers=set_ransac_parameters(n, 0.99, 10, 300, 4, 0.5, 5.991)[0])


def gpu_scenes():
    """(id, [candidates]): N = 4, 5, 31, 32, 33, 63, 64, 65, 129; H = 1, 4, 5, 9 and 300; K = 1 and K = 3 with an empty
    candidate; Refine records of 4, 5, 64, 255, 256, 257, 600 inliers (the all-inlier candidates: a record is the inlier
    set of a hypothesis)."""
    sc = []
    for j, (n, H) in enumerate([(4, 1), (5, 4), (31, 5), (32, 9), (33, 4), (63, 5), (64, 9), (65, 4), (129, 5)]):
        sc.append((f"n{n}_h{H}", [make_candidate(100 + j, n, H)]))
    sc.append(("h300", [make_candidate(120, 100, 300)]))
    for j, n in enumerate([4, 5, 64, 255, 256, 257, 600]):  # every point an exact inlier: a record of n inliers
        c = make_candidate(140 + j, n, 3, inlier_frac=1.0, noise=0.0)
        c["min_inliers"] = 4
        sc.append((f"rec{n}", [c]))
    k3 = [make_candidate(160, 40, 5), make_candidate(161, 33, 0), make_candidate(162, 70, 9)]
    sc.append(("k3_empty", k3))
    return sc


def write_scene(path, cands, last="max_err"):
    """last: the sixth column of a correspondence, max_err (tests/cpp/pnp_cpu.cpp) or sigma2 (tests/cpp/test_pnp.cpp)"""
    with open(path, "w") as f:
        f.write(f"{len(cands)}\n")
        for c in cands:
            f.write(f"{len(c['p3d'])} {len(c['sets'])} {c['min_inliers']} " + " ".join(f"{float(x):.9g}" for x in c["cam"]) + "\n")
            for P, q, e in zip(c["p3d"], c["p2d"], c[last]):
                f.write(" ".join(f"{float(x):.9g}" for x in (*P, *q, e)) + "\n")
            for s in c["sets"]:
                f.write(" ".join(str(int(x)) for x in s) + "\n")


def read_result(path, cands):
    """-> (hyp, rec_off, rec_hyp, rec); hyp / rec = lists of (n_inliers, status, pose [12] float32, words uint32)."""
    lines = Path(path).read_text().split("\n")
    H, R = [int(x) for x in lines[0].split()]

    def item(ln):
        p = ln.split()
        return int(p[0]), int(p[1]), np.array([float(x) for x in p[2:14]], F32), np.array([int(x) for x in p[14:]], np.uint32)
    hyp = [item(lines[1 + h]) for h in range(H)]
    rec_off = [int(x) for x in lines[1 + H].split()]
    rec_hyp = [int(x) for x in lines[2 + H].split()]
    rec = [item(lines[3 + H + r]) for r in range(R)]
    return hyp, rec_off, rec_hyp, rec


def words_to_mask(words, n):
    w = np.asarray(words, np.uint32)
    return ((w[np.arange(n) >> 5] >> (np.arange(n) & 31).astype(np.uint32)) & 1).astype(bool)


def mask_to_words(mask):
    n = len(mask)
    w = np.zeros((n + 31) // 32, np.uint32)
    for i in np.flatnonzero(mask):
        w[i >> 5] |= np.uint32(1) << np.uint32(i & 31)
    return w


# ----------------------------------------------------------------------------------------------- comparison
def s_pnp():
    """The pose tolerance (relative, on R in the Frobenius norm and on t): profiles/pnp_tolerance.txt."""
    txt = (Path(__file__).resolve().parent.parent / "profiles" / "pnp_tolerance.txt").read_text()
    noise = float([ln for ln in txt.split("\n") if ln.startswith("s_pnp=")][0].split("=")[1])
    return max(2.0 * float(np.finfo(F32).eps), 16.0 * noise)


def ref_item(c, idx):
    """The restatement on correspondences idx of candidate c -> dict(R, t, info, mask, e2)."""
    R, t, info = compute_pose(c["p3d"][idx].astype(np.float64), c["p2d"][idx].astype(np.float64), c["cam"], full=True)
    fin = bool(np.all(np.isfinite(R)) and np.all(np.isfinite(t)))
    if fin:
        mask, e2 = check_inliers(R, t, c["cam"], c["p3d"], c["p2d"], c["max_err"])
    else:
        mask, e2 = np.zeros(len(c["p3d"]), bool), np.full(len(c["p3d"]), np.inf, F32)
    return dict(R=R, t=t, info=info, mask=mask, e2=e2, finite=fin)


def pose_close(pose, R, t, tol):
    p = np.asarray(pose, np.float64)
    dR = np.linalg.norm(p[:9].reshape(3, 3) - R) / np.linalg.norm(R)
    dt = np.linalg.norm(p[9:] - t) / max(np.linalg.norm(t), 1.0)
    return max(dR, dt) <= tol, max(dR, dt)


def compare_item(c, ref, got, tol, stats):
    """One hypothesis or record: got = (n_inliers, status, pose, words).  Counts into stats: items, excluded, decisions,
    guard (decisions not compared), worst (largest relative pose difference among the compared)."""
    n = len(c["p3d"])
    n_inl, status, pose, words = got
    stats["items"] += 1
    assert status == (OK if ref["finite"] else NONFINITE), (status, ref["finite"])
    assert np.all(np.isfinite(pose)) == ref["finite"]
    mask = words_to_mask(words, n)
    assert int(mask.sum()) == n_inl
    if not ref["finite"]:
        assert n_inl == 0 and not np.any(words)
        return
    info = ref["info"]
    if info["ill"] or info["flip"]:
        stats["excluded"] += 1
        if info["flip"] and not info["ill"]:
            assert any(pose_close(pose, R, t, tol)[0] for R, t, _ in info["cands"] if np.all(np.isfinite(R)))
        return
    ok, d = pose_close(pose, ref["R"], ref["t"], tol)
    stats["worst"] = max(stats["worst"], d)
    assert ok, ("pose differs from the restatement", d, tol)
    near = np.abs(ref["e2"].astype(np.float64) - c["max_err"]) <= 1e-6 * c["max_err"]
    stats["decisions"] += n
    stats["guard"] += int(near.sum())
    assert np.array_equal(mask[~near], ref["mask"][~near]), "inlier decisions differ"


def new_stats():
    return dict(items=0, excluded=0, decisions=0, guard=0, worst=0.0)


def check_caps(stats, what=""):
    assert stats["excluded"] <= 0.05 * stats["items"] + 1e-12 or stats["excluded"] == 0, (what, stats)
    assert stats["guard"] <= 0.001 * stats["decisions"] or stats["guard"] == 0, (what, stats)
