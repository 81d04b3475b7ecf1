"""Reference of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:483-814) and Optimizer::BundleAdjustment (:54-253) for
orbfe_local_bundle_adjustment / orbfe_bundle_adjustment: a float64 restatement of the graph both build, written from

* src/Optimizer.cc:538-687 (the graph), :689-777 (optimize(5), first classification, optimize(10), final classification),
* Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp} (computeError / isDepthPositive .h:94-104, :126-136, cam_project
  .cpp:141-157, linearizeOplus .cpp:103-139, :188-234), se3quat.h (through tests/pose_opt_ref.py),
* Thirdparty/g2o/g2o/core/base_binary_edge.hpp:54-120 (constructQuadraticForm), robust_kernel_impl.cpp:78-91 (Huber),
* Thirdparty/g2o/g2o/core/block_solver.hpp:502-590 (buildSystem, setLambda), :354-487 (solve),
* Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189, sparse_optimizer.cpp (optimize, terminate,
  initializeOptimization: a vertex without an active edge is not in the active set and keeps its estimate).

No Schur trick: the full system over the active free poses and the active points is assembled DENSE and solved with
numpy.linalg (cholesky decides whether the factorisation succeeded, solve gives the step); schur_solve() is the block
solver's route, kept for the self-check of tests/test_lba_ref.py.  Per-edge arithmetic is elementwise numpy float64; the
sums over edges run in edge order (a sequential loop), or in reversed edge order with reverse=True -- the
difference of the two is the reordering noise the GPU tolerance is built on.  A monocular edge is a three-row edge whose
third row is zero.  The stop flag is "raised before iteration k" (iterations counted over both rounds; k = 0: at entry).
chi2() of an edge is what the last computeActiveErrors the edge was active in left: the last Levenberg trial, accepted or
not; for a level-1 edge its round-one value.  isDepthPositive() is evaluated at the estimates of the moment.
"""
import math

import numpy as np

from frustum_ref import CX, CY, FX, FY, MBF, rodrigues
from pose_opt_ref import INV_LEVEL_SIGMA2, LEVELS, SCALE, quat_rotate, quat_to_R, se3_exp, se3_mul, to_se3quat

f32 = np.float32
DELTA_MONO = float(f32(math.sqrt(5.991)))    # const float thHuberMono (Optimizer.cc:601)
DELTA_STEREO = float(f32(math.sqrt(7.815)))  # :602
THR_MONO, THR_STEREO = 5.991, 7.815          # double literals (:714, :730)
DBL_MAX = float(np.finfo(np.float64).max)
END = dict(none=0, iterations=1, trials=2, rho_zero=3, no_progress=4, stop=5)
GUARD_CHI2, GUARD_Z, GUARD_RHO = 1e-6, 1e-6, 1e-9


class Graph:
    def __init__(self, sc):
        self.n_local = int(sc["n_local"])
        self.T = np.asarray(sc["Tcw"], f32).reshape(-1, 4, 4)
        self.nT = len(self.T)
        self.cam = np.asarray(sc["cam"], f32).reshape(-1, 5).astype(np.float64)
        self.ep = np.asarray(sc["edge_pose"], np.int64)
        self.ept = np.asarray(sc["edge_point"], np.int64)
        self.nE, self.nP = len(self.ep), len(np.asarray(sc["xw"]).reshape(-1, 3))
        self.u, self.v, self.ur, self.w = [np.asarray(sc[k], f32).astype(np.float64) for k in ("u", "v", "u_right", "inv_sigma2")]
        self.stereo = ~(self.ur < 0)  # mvuRight < 0: monocular (:627)
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.thr = np.where(self.stereo, THR_STEREO, THR_MONO)
        fixed = np.zeros(self.n_local, bool) if sc.get("local_is_fixed") is None else np.asarray(sc["local_is_fixed"]).astype(bool)
        self.free = np.zeros(self.nT, bool)
        self.free[:self.n_local] = ~fixed
        self.fx, self.fy, self.cx, self.cy, self.bf = [self.cam[self.ep, k] for k in range(5)]

    def errors(self, poses, pts, jac=False):
        """chi2 [E], z [E] (what isDepthPositive tests), and with jac the rows e [3], Jp [3][6], Jl [3][3] of every edge."""
        Q = np.array([p[0] for p in poses])[self.ep]
        Tt = np.array([p[1] for p in poses])[self.ep]
        X = pts[self.ept]
        q = [Q[:, k] for k in range(4)]
        with np.errstate(all="ignore"):
            rx, ry, rz = quat_rotate(q, X[:, 0], X[:, 1], X[:, 2])
            x, y, z = rx + Tt[:, 0], ry + Tt[:, 1], rz + Tt[:, 2]
            fx, fy, cx, cy, bf = self.fx, self.fy, self.cx, self.cy, self.bf
            invz_f = (1.0 / z).astype(f32).astype(np.float64)  # const float invz = 1.0f / trans_xyz[2] (.cpp:151)
            p0 = (x * invz_f) * fx + cx
            e0 = np.where(self.stereo, self.u - p0, self.u - ((x / z) * fx + cx))
            e1 = np.where(self.stereo, self.v - ((y * invz_f) * fy + cy), self.v - ((y / z) * fy + cy))
            e2 = np.where(self.stereo, self.ur - (p0 - bf * invz_f), 0.0)
            w = self.w
            chi2 = (e0 * (w * e0) + e1 * (w * e1)) + e2 * (w * e2)
            if not jac:
                return chi2, z
            z_2 = z * z
            zero = np.zeros(self.nE)
            J0 = [x * y / z_2 * fx, -(1 + (x * x / z_2)) * fx, y / z * fx, -1. / z * fx, zero, x / z_2 * fx]
            J1 = [(1 + y * y / z_2) * fy, -x * y / z_2 * fy, -x / z * fy, zero, -1. / z * fy, y / z_2 * fy]
            J2 = [J0[0] - bf * y / z_2, J0[1] + bf * x / z_2, J0[2], J0[3], zero, J0[5] - bf / z_2]
            J2 = [np.where(self.stereo, a, 0.0) for a in J2]
            R = quat_to_R(q)
            s = -1. / z
            a00, a02, a11, a12 = s * fx, s * (-x / z * fx), s * fy, s * (-y / z * fy)
            L0, L1, L2 = [], [], []
            for c in range(3):
                s0 = -fx * R[0][c] / z + fx * x * R[2][c] / z_2
                s1 = -fy * R[1][c] / z + fy * y * R[2][c] / z_2
                L0.append(np.where(self.stereo, s0, a00 * R[0][c] + a02 * R[2][c]))
                L1.append(np.where(self.stereo, s1, a11 * R[1][c] + a12 * R[2][c]))
                L2.append(np.where(self.stereo, s0 - bf * R[2][c] / z_2, 0.0))
        return chi2, z, (e0, e1, e2), (J0, J1, J2), (L0, L1, L2)

    def huber(self, chi2, robust):
        with np.errstate(all="ignore"):
            over = (chi2 > self.delta * self.delta) & robust
            sq = np.sqrt(chi2)
            return np.where(over, 2 * sq * self.delta - self.delta * self.delta, chi2), np.where(over, self.delta / sq, 1.0)

    def build(self, poses, pts, active, robust, reverse):
        """computeActiveErrors + buildSystem over the active edges -> chi2 [E], robust chi2, H, b, and the index maps."""
        chi2, z, e, Jp, Jl = self.errors(poses, pts, True)
        rho0, rho1 = self.huber(chi2, robust)
        act = np.flatnonzero(active)
        order = act[::-1] if reverse else act
        pose_on = np.zeros(self.nT, bool)
        pose_on[self.ep[act]] = True
        pose_on &= self.free
        pt_on = np.zeros(self.nP, bool)
        pt_on[self.ept[act]] = True
        pidx = np.full(self.nT, -1)
        pidx[pose_on] = np.arange(pose_on.sum())
        n6 = 6 * int(pose_on.sum())
        lidx = np.full(self.nP, -1)
        lidx[pt_on] = n6 + 3 * np.arange(pt_on.sum())
        dim = n6 + 3 * int(pt_on.sum())
        H, b = np.zeros((dim, dim)), np.zeros(dim)
        wr = rho1 * self.w
        J9 = np.stack([np.stack(list(Jp[r]) + list(Jl[r]), axis=1) for r in range(3)], axis=1)  # [E, 3, 9]
        E3 = np.stack(e, axis=1)
        with np.errstate(all="ignore"):
            blocks = np.einsum("eri,e,erj->eij", J9, wr, J9)
            rhs = -np.einsum("eri,e,er->ei", J9, wr, E3)
        for ed in order:  # sequential, first (or last) edge first
            j, p = self.ep[ed], self.ept[ed]
            ids = np.concatenate([6 * pidx[j] + np.arange(6) if pidx[j] >= 0 else np.zeros(0, int), lidx[p] + np.arange(3)]).astype(int)
            sel = np.arange(9) if pidx[j] >= 0 else np.arange(6, 9)
            H[np.ix_(ids, ids)] += blocks[ed][np.ix_(sel, sel)]
            b[ids] += rhs[ed][sel]
        rsum = np.cumsum(np.where(active, rho0, 0.0)[order])[-1] if len(order) else 0.0
        return chi2, float(rsum), H, b, pidx, lidx, n6

    def robust_chi2(self, poses, pts, active, robust, reverse):
        chi2, _ = self.errors(poses, pts)
        rho0, _ = self.huber(chi2, robust)
        act = np.flatnonzero(active)
        order = act[::-1] if reverse else act
        return chi2, float(np.cumsum(rho0[order])[-1]) if len(order) else 0.0


def dense_solve(H, lam, b):
    """(H + lam I) x = b -> (ok, x): ok False when the Cholesky factorisation fails (then x = 0)."""
    A = H + lam * np.eye(len(H))
    try:
        np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return False, np.zeros(len(b))
    if not np.isfinite(A).all():
        return False, np.zeros(len(b))
    return True, np.linalg.solve(A, b)


def schur_solve(H, lam, b, n6):
    """BlockSolver::solve (block_solver.hpp:354-487): invert every 3 x 3 Hll, Hschur = Hpp - sum Hpl Hll^-1 Hpl^T, poses by
    Cholesky, points by back-substitution."""
    A = H + lam * np.eye(len(H))
    nl = (len(H) - n6) // 3
    Hpp, Hpl = A[:n6, :n6].copy(), A[:n6, n6:]
    bs = b[:n6].copy()
    inv = []
    for i in range(nl):
        D = np.linalg.inv(A[n6 + 3 * i:n6 + 3 * i + 3, n6 + 3 * i:n6 + 3 * i + 3])
        inv.append(D)
        B = Hpl[:, 3 * i:3 * i + 3]
        Hpp -= B @ D @ B.T
        bs -= B @ (D @ b[n6 + 3 * i:n6 + 3 * i + 3])
    xp = np.linalg.solve(Hpp, bs) if n6 else np.zeros(0)
    xl = [inv[i] @ (b[n6 + 3 * i:n6 + 3 * i + 3] - Hpl[:, 3 * i:3 * i + 3].T @ xp) for i in range(nl)]
    return np.concatenate([xp] + xl) if nl else xp


def to_matrix(pose):
    """SE3Quat::to_homogeneous_matrix, float64."""
    T = np.eye(4)
    T[:3, :3] = np.array(quat_to_R(pose[0]))
    T[:3, 3] = pose[1]
    return T


def adjust(sc, reverse=False, stop_before=None, local=True, n_iterations=5, robust=True, schur=False):
    """-> dict: Tcw [n_local, 4, 4], xw [n_points, 3] float64, erase / level1 [E] uint8, edge_chi2 [E], rounds, stopped, and per
    round iterations, trials, termination, lam, chi2; diagnostics: rejected (trials rejected), min_rho (smallest |rho|),
    guard (smallest relative distance of a classification chi2 to its threshold and of a classification depth to 0),
    stale_decides (edges the final test erases on their round-one chi2 whose chi2 at the final estimates would pass)."""
    G = Graph(sc)
    poses = [to_se3quat(G.T[j]) for j in range(G.nT)]
    pts = np.asarray(sc["xw"], f32).reshape(-1, 3).astype(np.float64)
    level = np.zeros(G.nE, np.uint8)
    stored = np.zeros(G.nE)
    out = dict(rounds=0, stopped=0, iterations=[0, 0], trials=[0, 0], termination=[0, 0], lam=[0.0, 0.0], chi2=[0.0, 0.0], rejected=0,
               min_rho=np.inf, guard=np.inf, stale_decides=0)
    done = [0]

    def stop():
        s = stop_before is not None and done[0] >= stop_before
        if s:
            out["stopped"] = 1
        return s

    def optimize(max_it, rob, rnd):
        nonlocal poses, pts, stored
        active = level == 0
        it = trials = nBad = 0
        lam, ni, cur, end = 0.0, 2.0, 0.0, END["none"] if max_it > 0 else END["iterations"]
        while max_it > 0:
            if stop():
                end = END["stop"]
                break
            if not active.any():
                break
            done[0] += 1
            chi2, cur, H, b, pidx, lidx, n6 = G.build(poses, pts, active, rob, reverse)
            stored = np.where(active, chi2, stored)
            ini = cur
            if it == 0:
                lam, ni, nBad = 1e-5 * float(np.abs(np.diag(H)).max(initial=0.0)), 2.0, 0
            rho, q = 0.0, 0
            while True:
                ok, x = dense_solve(H, lam, b)
                if schur and ok:  # the block solver's route through the reduced system instead of the full dense solve
                    x = schur_solve(H, lam, b, n6)
                tp = [se3_mul(se3_exp(list(x[6 * pidx[j]:6 * pidx[j] + 6])), poses[j]) if pidx[j] >= 0 else poses[j] for j in range(G.nT)]
                tx = pts.copy()
                on = lidx >= 0
                tx[on] = pts[on] + x[n6:].reshape(-1, 3)
                chi2, temp = G.robust_chi2(tp, tx, active, rob, reverse)
                stored = np.where(active, chi2, stored)
                if not ok:
                    temp = DBL_MAX
                scale = float(np.cumsum(x * (lam * x + b))[-1]) + 1e-3
                with np.errstate(all="ignore"):
                    rho = float(np.float64(cur - temp) / np.float64(scale))
                out["min_rho"] = min(out["min_rho"], abs(rho))
                trials += 1
                if rho > 0 and math.isfinite(temp):
                    tt = 2 * rho - 1
                    lam = lam * max(1.0 / 3.0, min(1.0 - tt * tt * tt, 2.0 / 3.0))
                    ni, cur, poses, pts = 2.0, temp, tp, tx
                else:
                    lam, ni = lam * ni, ni * 2
                    out["rejected"] += 1
                q += 1
                if not (rho < 0 and q < 10 and not stop()):
                    break
            it += 1
            if q == 10:
                end = END["trials"]
                break
            if rho == 0:
                end = END["rho_zero"]
                break
            nBad = nBad + 1 if (ini - cur) * 1e3 < ini else 0
            if nBad >= 3:
                end = END["no_progress"]
                break
            if it >= max_it:
                end = END["iterations"]
                break
        out["rounds"] = rnd + 1
        for k, val in (("iterations", it), ("trials", trials), ("termination", end), ("lam", lam), ("chi2", cur)):
            out[k][rnd] = val

    def is_bad():
        _, z = G.errors(poses, pts)
        X = pts[G.ept]
        with np.errstate(all="ignore"):
            g = min(np.abs(stored / G.thr - 1.0).min(), (np.abs(z) / np.maximum(np.linalg.norm(X, axis=1), 1.0)).min())
        out["guard"] = min(out["guard"], float(g))
        return (stored > G.thr) | ~(z > 0.0)

    erase = np.zeros(G.nE, np.uint8)
    if local:
        if not stop():  # :689-691
            optimize(5, True, 0)
            if not stop():  # bDoMore
                level = is_bad().astype(np.uint8)
                optimize(10, False, 1)
            bad = is_bad()
            erase = np.where(bad, np.where(level != 0, 1, 2), 0).astype(np.uint8)
            fresh, z = G.errors(poses, pts)
            out["stale_decides"] = int(((level != 0) & (z > 0) & (fresh <= G.thr) & bad).sum())
    else:
        optimize(n_iterations, robust, 0)
    out.update(Tcw=np.stack([to_matrix(poses[j]) for j in range(G.n_local)]), xw=pts, erase=erase, level1=level.copy(),
               edge_chi2=stored.copy())
    return out


# ---------------------------------------------------------------------------------------------------------------------
def scene(seed, n_local, n_fixed, n_points, stereo_fraction=0.0, vis=None, vis_prob=0.7, noise_px=1.0, start_rot=0.002,
          start_trans=0.02, start_point=0.02, outliers=(), flip=None, near=None, local_is_fixed=None, min_obs=2):
    """A seeded scene: key frames along a baseline looking at a cloud 4 .. 20 m ahead.  Poses 0 .. n_local-1 are local, the rest
    fixed (at their true pose); the gauge is pinned by >= 2 fixed poses, or one plus stereo edges.  vis [nT, n_points] bool
    says who sees what (default: random with vis_prob, at least min_obs observers).  outliers: (pose, point, pixels) edges whose
    observation is moved that far; flip: a (fixed) pose turned to look away from the cloud -- its observations are the exact
    projections x / z of points BEHIND it, so its edges have a small chi2 and a negative depth.  Local poses and points start
    perturbed."""
    rng = np.random.default_rng(seed)
    nT = n_local + n_fixed
    Ttrue = np.zeros((nT, 4, 4))
    for j in range(nT):
        Tj = np.eye(4)
        Tj[:3, :3] = rodrigues(rng.normal(0, 0.03, 3))
        Tj[:3, 3] = [-0.4 * j + rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.05)]
        if flip == j:
            Tj = np.diag([-1.0, 1.0, -1.0, 1.0]) @ Tj
        Ttrue[j] = Tj
    Ttrue = Ttrue.astype(f32).astype(np.float64)
    z = rng.uniform(4, 20, n_points)
    X = np.stack([rng.uniform(-0.35, 0.35, n_points) * z - 0.2 * nT, rng.uniform(-0.2, 0.2, n_points) * z, z], axis=1)
    if near is not None:  # (pose, point, depth): the point sits that close in front of the pose, a little off its axis
        j, p, d = near
        X[p] = Ttrue[j, :3, :3].T @ (np.array([0.3 * d, -0.2 * d, d]) - Ttrue[j, :3, 3])
    if vis is None:
        vis = rng.random((nT, n_points)) < vis_prob
        for p in range(n_points):
            while vis[:, p].sum() < min(min_obs, nT):
                vis[rng.integers(nT), p] = True
    vis = np.array(vis, bool)
    for (j, p, _) in outliers:
        vis[j, p] = True
    ep, ept = [], []
    for p in range(n_points):
        for j in range(nT):
            if vis[j, p]:
                ep.append(j)
                ept.append(p)
    ep, ept = np.array(ep, np.int32), np.array(ept, np.int32)
    E = len(ep)
    Pc = np.einsum("eij,ej->ei", Ttrue[ep, :3, :3], X[ept]) + Ttrue[ep, :3, 3]
    octave = rng.integers(0, LEVELS, E)
    sigma = float(SCALE) ** octave
    uu = FX * Pc[:, 0] / Pc[:, 2] + CX + rng.normal(0, 1, E) * noise_px * sigma
    vv = FY * Pc[:, 1] / Pc[:, 2] + CY + rng.normal(0, 1, E) * noise_px * sigma
    rr = uu - MBF / Pc[:, 2] + rng.normal(0, 1, E) * noise_px * sigma * 0.5
    stereo = rng.random(E) < stereo_fraction
    planted = np.zeros(E, bool)
    for (j, p, px) in outliers:
        k = np.flatnonzero((ep == j) & (ept == p))[0]
        ang = rng.uniform(0, 2 * np.pi)
        uu[k] += px * np.cos(ang)
        vv[k] += px * np.sin(ang)
        planted[k] = True
    rr = np.where(stereo, np.maximum(rr, 0.0), -1.0)
    Tstart = Ttrue.copy()
    for j in range(n_local):
        if local_is_fixed is not None and local_is_fixed[j]:
            continue
        dT = np.eye(4)
        dT[:3, :3] = rodrigues(rng.normal(0, start_rot, 3))
        dT[:3, 3] = rng.normal(0, start_trans, 3)
        Tstart[j] = dT @ Ttrue[j]
    cam = np.tile(np.array([FX, FY, CX, CY, MBF], f32), (nT, 1))
    xw = (X + rng.normal(0, start_point, X.shape)).astype(f32)
    return dict(n_local=n_local, Tcw=Tstart.astype(f32), Tcw_true=Ttrue, cam=cam, xw=xw, xw_true=X, edge_pose=ep, edge_point=ept,
                u=uu.astype(f32), v=vv.astype(f32), u_right=rr.astype(f32), inv_sigma2=INV_LEVEL_SIGMA2[octave], planted=planted,
                local_is_fixed=None if local_is_fixed is None else np.asarray(local_is_fixed, np.uint8))


def pose_with_edges(nT, n_points, pose, k):
    """vis in which `pose` sees exactly the first k points and every other pose sees every point."""
    vis = np.ones((nT, n_points), bool)
    vis[pose, k:] = False
    return vis


def guard_ok(res):
    """the condition every comparison scene keeps: no classification chi2 within 1e-6 (relative) of its threshold, no
    classification depth within 1e-6 of 0, no rho within 1e-9 of 0."""
    return res["guard"] > GUARD_CHI2 and res["min_rho"] > GUARD_RHO


def _vis_pair(nT, n_points, shared):
    """poses 0 and 1 share exactly `shared` points (the first ones); the fixed poses see everything."""
    vis = np.ones((nT, n_points), bool)
    vis[0, shared:] = False
    vis[1, shared:] = False
    half = shared + (n_points - shared) // 2
    vis[0, shared:half] = True
    vis[1, half:] = True
    return vis


def gpu_scenes():
    """(id, scene, kind) of every problem tests/test_gpu_lba.py runs; kind "local" or ("global", n_iterations, robust)."""
    S = []
    S.append(("l1f2p6", scene(1, 1, 2, 6), "local"))
    S.append(("l2f1p8-stereo", scene(2, 2, 1, 8, stereo_fraction=1.0), "local"))
    S.append(("l3f2p40-mixed", scene(3, 3, 2, 40, stereo_fraction=0.5, outliers=((0, 3, 40), (1, 7, 60), (4, 9, 50))), "local"))
    S.append(("local-is-fixed", scene(4, 3, 1, 30, local_is_fixed=(0, 1, 0), outliers=((2, 5, 45),)), "local"))
    for k in (63, 64, 65):
        S.append((f"pose-edges-{k}", scene(10 + k, 2, 2, 70, vis=pose_with_edges(4, 70, 0, k)), "local"))
        S.append((f"pair-shares-{k}", scene(20 + k, 2, 2, 140, vis=_vis_pair(4, 140, k)), "local"))
    S.append(("pair-shares-0", scene(30, 2, 2, 40, vis=_vis_pair(4, 40, 0)), "local"))
    vis = np.ones((4, 20), bool)
    vis[1, 0] = False  # point 0: local pose 0 and the two fixed poses only
    S.append(("point-fixed-plus-one", scene(31, 2, 2, 20, vis=vis), "local"))
    S.append(("point-all-level1", scene(32, 2, 2, 30, outliers=tuple((j, 4, 150) for j in range(4))), "local"))
    vis = np.ones((5, 40), bool)
    vis[2, 6:] = False  # local pose 2 sees six points, every observation gross
    S.append(("pose-all-level1", scene(33, 3, 2, 40, vis=vis, outliers=tuple((2, p, 200) for p in range(6))), "local"))
    vis = np.ones((5, 30), bool)
    vis[4, 3:] = False  # the pose that looks away sees three points, all behind it
    S.append(("behind-camera", scene(34, 2, 3, 30, vis=vis, flip=4), "local"))
    # point 0 sits 6 cm in front of local pose 0: its edge passes both chi2 tests and the first depth test, and round two
    # carries the point behind the camera (seed found by search; tests/test_lba_ref.py pins what the edge does)
    S.append(("depth-final-only", scene(111, 2, 2, 30, near=(0, 0, 0.06)), "local"))
    S.append(("far-start", scene(35, 2, 2, 60, start_rot=0.02, start_trans=0.3, start_point=0.3), "local"))
    S.append(("far-start-outliers", scene(36, 3, 2, 50, stereo_fraction=0.5, start_rot=0.05, start_trans=0.5, start_point=0.5,
                                          outliers=tuple((j % 5, j, 80) for j in range(10))), "local"))
    S.append(("no-progress", scene(37, 2, 2, 30, noise_px=0.5, start_rot=0.0, start_trans=0.0, start_point=0.0), "local"))
    S.append(("l7f5p300", scene(38, 7, 5, 300, stereo_fraction=0.3, vis_prob=0.5,
                                outliers=tuple((p % 12, p, 70) for p in range(0, 300, 23))), "local"))
    for rob in (True, False):
        sc = scene(39, 2, 0, 50, stereo_fraction=0.5, local_is_fixed=(1, 0), outliers=((1, 3, 30),))
        S.append((f"global-20-{'robust' if rob else 'plain'}", sc, ("global", 20, rob)))
    return S


def run(sc, kind="local", reverse=False, stop_before=None, schur=False):
    if kind == "local":
        return adjust(sc, reverse=reverse, stop_before=stop_before, schur=schur)
    return adjust(sc, reverse=reverse, stop_before=stop_before, local=False, n_iterations=kind[1], robust=kind[2], schur=schur)
