"""Restatement of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:833-1104) for the tests of
orbfe_optimize_essential_graph: numpy float64, dense normal equations and numpy.linalg.cholesky, written from

* src/Optimizer.cc:862-899 (vertices: vScw, fixed iff pKF == pLoopKF, _fix_scale), :907-1040 (EdgeSim3, identity information,
  Sji = Sjw * Swi from vScw for the new loop connections and from the non-corrected Sim3 otherwise), :1043-1044
  (setUserLambdaInit(1e-16) at :847, optimize(20)), :1059-1067 (Tiw = [R | t / s]), :1092-1100 (the point correction),
* Thirdparty/g2o/g2o/types/sim3.h (Sim3(Vector7d) :70-142, log :148-230, inverse :233-236, operator* :266-272, map :144-146),
* Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h (oplusImpl :60-69, EdgeSim3::computeError :106-114),
* Thirdparty/g2o/g2o/core/base_binary_edge.hpp:131-200 (the numeric Jacobian, delta 1e-9),
* Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189, sparse_optimizer.cpp:234 (an edge between two fixed
  vertices is not active).

It carries both Jacobian forms (jac="analytic": J_j = -G, J_i = G Ad(S_j S_i^-1) with G the derivative of Sim3::log as it is
computed, on dense 7 x 7 matrices; jac="g2o": the central difference), two solver routes (dense; sparse=True: a block right-looking Cholesky on a dictionary of
7 x 7 blocks, which is also the independent symbolic elimination that counts blocks_L), a reverse=True run (the edges summed in
reversed order) and the engineered scenes."""
import math

import numpy as np

EPS = 0.00001
DBL_MAX = np.finfo(np.float64).max
END_ITERATIONS, END_TRIALS, END_RHO_ZERO, END_NO_PROGRESS = 1, 2, 3, 4


# ---- Sim3 = (q [x y z w], t [3], s) -------------------------------------------------------------------------------------------
def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def quat_to_R(q):
    x, y, z, w = q
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def quat_from_R(m):
    """Eigen::Quaterniond(Matrix3d)"""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4)
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return q


def rotate(q, v):
    """Eigen QuaternionBase::_transformVector"""
    uv = 2.0 * np.cross(q[:3], v)
    return v + q[3] * uv + np.cross(q[:3], uv)


def quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def sim3_mul(a, b):
    return quat_mul(a[0], b[0]), a[2] * rotate(a[0], b[1]) + a[1], a[2] * b[2]


def sim3_inverse(S):
    qc = np.array([-S[0][0], -S[0][1], -S[0][2], S[0][3]])
    return qc, rotate(qc, (-1.0 / S[2]) * S[1]), 1.0 / S[2]


def sim3_map(S, x):
    return S[2] * rotate(S[0], x) + S[1]


def _abc(sigma, s, theta, small):
    if abs(sigma) < EPS:
        C = 1.0
        if small:
            return 1.0 / 2.0, 1.0 / 6.0, C
        th2 = theta * theta
        return (1.0 - math.cos(theta)) / th2, (theta - math.sin(theta)) / (th2 * theta), C
    C = (s - 1.0) / sigma
    if small:
        s2 = sigma * sigma
        return ((sigma - 1.0) * s + 1.0) / s2, ((0.5 * s2 - sigma + 1.0) * s) / (s2 * sigma), C
    a, b = s * math.sin(theta), s * math.cos(theta)
    th2 = theta * theta
    c = th2 + sigma * sigma
    return (a * sigma + (1.0 - b) * theta) / (theta * c), (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / th2, C


def sim3_exp(u):
    """Sim3(const Vector7d&) (sim3.h:70-142)"""
    w, ups, sigma = np.asarray(u[:3], np.float64), np.asarray(u[3:6], np.float64), float(u[6])
    theta = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    Om = skew(w)
    Om2 = Om @ Om
    s = math.exp(sigma)
    small = theta < EPS
    A, B, C = _abc(sigma, s, theta, small)
    if small:
        R = np.eye(3) + Om + Om2
    else:
        R = np.eye(3) + math.sin(theta) / theta * Om + (1.0 - math.cos(theta)) / (theta * theta) * Om2
    W = A * Om + B * Om2 + C * np.eye(3)
    return quat_from_R(R), W @ ups, s


def log_branch(S):
    """which of the four branches of Sim3::log S takes: (|sigma| < eps, d > 1 - eps)"""
    R = quat_to_R(S[0])
    d = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    return abs(math.log(S[2])) < EPS, d > 1.0 - EPS


def sim3_log(S):
    """Sim3::log (sim3.h:148-230)"""
    sigma = math.log(S[2])
    R = quat_to_R(S[0])
    d = 0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0)
    dR = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    small = d > 1.0 - EPS
    theta = 0.0
    if small:
        w = 0.5 * dR
    else:
        theta = math.acos(d)
        w = theta / (2.0 * math.sqrt(1.0 - d * d)) * dR
    A, B, C = _abc(sigma, S[2], theta, small)
    Om = skew(w)
    W = A * Om + B * Om @ Om + C * np.eye(3)
    ups = np.linalg.solve(W, S[1])
    return np.array([w[0], w[1], w[2], ups[0], ups[1], ups[2], sigma])


def from_record(r):
    return np.array(r[:4], np.float64), np.array(r[4:7], np.float64), float(r[7])


def to_record(S):
    return np.concatenate([S[0], S[1], [S[2]]])


def sim3_from_Rts(R, t, s=1.0):
    return quat_from_R(np.asarray(R, np.float64)), np.asarray(t, np.float64).copy(), float(s)


# ---- the edge --------------------------------------------------------------------------------------------------------------
def edge_error(C, Si, Sj):
    """EdgeSim3::computeError (types_seven_dof_expmap.h:106-114)"""
    return sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inverse(Sj)))


def Ad(S):
    R, t, s = quat_to_R(S[0]), S[1], S[2]
    M = np.zeros((7, 7))
    M[:3, :3] = R
    M[3:6, :3] = skew(t) @ R
    M[3:6, 3:6] = s * R
    M[3:6, 6] = -t
    M[6, 6] = 1.0
    return M


def log_jacobian(E):
    """G = d f(E * Sim3(xi)) / d xi at 0 of f = Sim3::log AS IT IS COMPUTED, branch by branch (csrc/essgraph_math.h:
    ess_log_jacobian).  With E' = (R (I + xi_w^), t + s R xi_u, s e^xi_s):  d omega = M_w xi_w, d sigma = xi_s and, from
    upsilon = W^-1 t,  d upsilon = W^-1 (s R xi_u - dW upsilon),  W = A Omega + B Omega^2 + C I with the A, B, C of the branch
    taken -- including what a branch freezes: no sigma-derivative for |sigma| < eps, no theta-derivative for d > 1 - eps, and
    B = (sigma^2 / 2 - sigma + 1) s / sigma^3 of sim3.h:199 as written.  Where the branches are exact this is Jr^-1(log E)."""
    small_sigma, small_theta = log_branch(E)
    e = sim3_log(E)
    w, u, sigma, s = e[:3], e[3:6], e[6], E[2]
    R = quat_to_R(E[0])
    Om = skew(w)
    At = Bt = As = Bs = Cs = 0.0
    if small_theta:
        theta = 0.0
        Mw = 0.5 * (np.trace(R) * np.eye(3) - R.T)  # omega = deltaR(R) / 2
    else:
        theta = math.acos(0.5 * (R[0, 0] + R[1, 1] + R[2, 2] - 1.0))
        Mw = np.eye(3) + 0.5 * Om + (1.0 / theta ** 2 - (1.0 + math.cos(theta)) / (2.0 * theta * math.sin(theta))) * Om @ Om
    A, B, C = _abc(sigma, s, theta, small_theta)
    if not small_sigma:
        Cs = s / sigma - (s - 1.0) / sigma ** 2
    if small_sigma and not small_theta:
        At = math.sin(theta) / theta ** 2 - 2.0 * (1.0 - math.cos(theta)) / theta ** 3
        Bt = (1.0 - math.cos(theta)) / theta ** 3 - 3.0 * (theta - math.sin(theta)) / theta ** 4
    elif not small_sigma and small_theta:
        As = s / sigma - 2.0 * A / sigma
        Bs = 0.5 * s / sigma - 3.0 * B / sigma
    elif not small_sigma:
        a, b, c = s * math.sin(theta), s * math.cos(theta), theta ** 2 + sigma ** 2
        DA = theta * c
        At = ((b * sigma + a * theta + (1.0 - b)) - A * (c + 2.0 * theta ** 2)) / DA
        As = ((a * sigma + a - b * theta) - A * 2.0 * theta * sigma) / DA
        M = (b - 1.0) * sigma + a * theta
        Q = M / c
        Qt = ((-a * sigma + b * theta + a) - Q * 2.0 * theta) / c
        Qs = ((b * sigma + (b - 1.0) + a * theta) - Q * 2.0 * sigma) / c
        Bt = -Qt / theta ** 2 - 2.0 * B / theta
        Bs = (Cs - Qs) / theta ** 2
    W = A * Om + B * Om @ Om + C * np.eye(3)
    ou, o2u = Om @ u, Om @ (Om @ u)
    K = -A * skew(u) - B * (skew(ou) + Om @ skew(u))
    if not small_theta:
        K = K + np.outer(At * ou + Bt * o2u, w) / theta
    G = np.zeros((7, 7))
    G[:3, :3] = Mw
    G[3:6, :3] = -np.linalg.solve(W, K @ Mw)
    G[3:6, 3:6] = np.linalg.solve(W, s * R)
    G[3:6, 6] = -np.linalg.solve(W, As * ou + Bs * o2u + Cs * u)
    G[6, 6] = 1.0
    return e, G


def jac_analytic(C, Si, Sj, fix_scale):
    """E = C S_i S_j^-1.  S_j <- Sim3(d) S_j gives E Sim3(-d): J_j = -G;  S_i <- Sim3(d) S_i gives E Sim3(Ad(S_j S_i^-1) d):
    J_i = G Ad(S_j S_i^-1)"""
    E = sim3_mul(sim3_mul(C, Si), sim3_inverse(Sj))
    e, G = log_jacobian(E)
    Ji = G @ Ad(sim3_mul(Sj, sim3_inverse(Si)))
    Jj = -G
    if fix_scale:
        Ji[:, 6] = 0.0
        Jj[:, 6] = 0.0
    return e, Ji, Jj


def oplus(S, upd, fix_scale):
    """VertexSim3Expmap::oplusImpl (:60-69)"""
    u = np.array(upd, np.float64)
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), S)


def jac_numeric(C, Si, Sj, fix_scale, delta=1e-9):
    """BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:131-200): central difference, scalar = 1 / (2 delta)"""
    e = edge_error(C, Si, Sj)
    out = []
    for which in (0, 1):
        J = np.zeros((7, 7))
        for d in range(7):
            add = np.zeros(7)
            add[d] = delta
            p = edge_error(C, oplus(Si, add, fix_scale), Sj) if which == 0 else edge_error(C, Si, oplus(Sj, add, fix_scale))
            add[d] = -delta
            m = edge_error(C, oplus(Si, add, fix_scale), Sj) if which == 0 else edge_error(C, Si, oplus(Sj, add, fix_scale))
            J[:, d] = (1.0 / (2.0 * delta)) * (p - m)
        out.append(J)
    return e, out[0], out[1]


# ---- the block-sparse route and the symbolic elimination ------------------------------------------------------------------------
def block_pattern(sc):
    """free index per vertex, active edges, the set of lower blocks (row >= col) of H"""
    n = len(sc["sim3"])
    fixed = np.asarray(sc["is_fixed"], bool)
    free_of = np.full(n, -1)
    free_of[~fixed] = np.arange(int((~fixed).sum()))
    active = [e for e in range(len(sc["edge_i"])) if free_of[sc["edge_i"][e]] >= 0 or free_of[sc["edge_j"][e]] >= 0]
    blocks = {(f, f) for f in range(int((~fixed).sum()))}
    for e in active:
        fi, fj = free_of[sc["edge_i"][e]], free_of[sc["edge_j"][e]]
        if fi >= 0 and fj >= 0:
            blocks.add((max(fi, fj), min(fi, fj)))
    return free_of, active, blocks


def count_blocks_L(n_cols, blocks):
    """elimination game on the block graph: the lower blocks of the factor, diagonal included"""
    cols = [set() for _ in range(n_cols)]
    for r, c in blocks:
        if r != c:
            cols[c].add(r)
    total = 0
    for j in range(n_cols):
        rows = sorted(cols[j])
        total += 1 + len(rows)
        for a in range(len(rows)):
            for b in range(a + 1, len(rows)):
                cols[rows[a]].add(rows[b])
    return total


def sparse_cholesky_solve(H, b, n_cols):
    """right-looking block Cholesky of the dense-stored H on a dictionary of its non-zero 7 x 7 lower blocks -> (x, blocks_L);
    raises numpy.linalg.LinAlgError on a pivot that is not positive"""
    A = {}
    for c in range(n_cols):
        for r in range(c, n_cols):
            blk = H[7 * r:7 * r + 7, 7 * c:7 * c + 7]
            if r == c or np.any(blk != 0.0):
                A[(r, c)] = blk.copy()
    col_rows = [sorted(r for (r, c) in A if c == j and r > j) for j in range(n_cols)]
    for j in range(n_cols):
        Ljj = np.linalg.cholesky(A[(j, j)])
        A[(j, j)] = Ljj
        rows = sorted(set(col_rows[j]))
        col_rows[j] = rows
        for r in rows:
            A[(r, j)] = np.linalg.solve(Ljj, A[(r, j)].T).T
        for a, r2 in enumerate(rows):
            for r1 in rows[a:]:
                if (r1, r2) not in A:
                    A[(r1, r2)] = np.zeros((7, 7))
                    col_rows[r2].append(r1)
                A[(r1, r2)] = A[(r1, r2)] - A[(r1, j)] @ A[(r2, j)].T
    y = b.reshape(-1, 7).copy()
    for j in range(n_cols):
        y[j] = np.linalg.solve(A[(j, j)], y[j])
        for r in col_rows[j]:
            y[r] = y[r] - A[(r, j)] @ y[j]
    for j in range(n_cols - 1, -1, -1):
        for r in col_rows[j]:
            y[j] = y[j] - A[(r, j)].T @ y[r]
        y[j] = np.linalg.solve(A[(j, j)].T, y[j])
    return y.reshape(-1), len(A)


# ---- the optimisation -----------------------------------------------------------------------------------------------------------
def measurements(sc):
    """Sji = Sjw * Swi (src/Optimizer.cc:927-929 from vScw; :957-959 and the like from the non-corrected Sim3)"""
    S = [from_record(r) for r in sc["sim3"]]
    M = [from_record(r) for r in sc["sim3_meas"]]
    out = []
    for e in range(len(sc["edge_i"])):
        src = S if sc["edge_kind"][e] else M
        out.append(sim3_mul(src[sc["edge_j"][e]], sim3_inverse(src[sc["edge_i"][e]])))
    return out


def linearise(sc, est, meas, free_of, active, jac, order):
    nF = int(free_of.max()) + 1
    H, b = np.zeros((7 * nF, 7 * nF)), np.zeros(7 * nF)
    chi = {}
    fn = jac_analytic if jac == "analytic" else jac_numeric
    for e in order:
        i, j = sc["edge_i"][e], sc["edge_j"][e]
        err, Ji, Jj = fn(meas[e], est[i], est[j], sc["fix_scale"])
        chi[e] = float(err @ err)
        fi, fj = free_of[i], free_of[j]
        if fi >= 0:
            H[7 * fi:7 * fi + 7, 7 * fi:7 * fi + 7] += Ji.T @ Ji
            b[7 * fi:7 * fi + 7] -= Ji.T @ err
        if fj >= 0:
            H[7 * fj:7 * fj + 7, 7 * fj:7 * fj + 7] += Jj.T @ Jj
            b[7 * fj:7 * fj + 7] -= Jj.T @ err
        if fi >= 0 and fj >= 0:
            H[7 * fi:7 * fi + 7, 7 * fj:7 * fj + 7] += Ji.T @ Jj
            H[7 * fj:7 * fj + 7, 7 * fi:7 * fi + 7] += Jj.T @ Ji
    return H, b, chi


def run(sc, jac="analytic", sparse=False, reverse=False, n_iterations=None):
    """-> dict(sim3_out, Tiw, edge_chi2, iterations, trials, termination, lam, chi2_initial, chi2, n_free, blocks_A, blocks_L,
    solve_failures, host_syncs, min_gap: the smallest |currentChi - tempChi| / max(currentChi, 1) over all trials)"""
    n, nE = len(sc["sim3"]), len(sc["edge_i"])
    max_it = sc["n_iterations"] if n_iterations is None else n_iterations
    est = [from_record(r) for r in sc["sim3"]]
    meas = measurements(sc)
    free_of, active, blocks = block_pattern(sc)
    nF = int((free_of >= 0).sum())
    order = active[::-1] if reverse else active
    edge_chi2 = np.zeros(nE)
    for e in range(nE):
        err = edge_error(meas[e], est[sc["edge_i"][e]], est[sc["edge_j"][e]])
        edge_chi2[e] = float(err @ err)
    out = dict(iterations=0, trials=0, termination=END_ITERATIONS, lam=0.0, chi2_initial=0.0, chi2=0.0, n_free=nF, blocks_A=len(blocks) if nF else 0,
               blocks_L=count_blocks_L(nF, blocks) if nF else 0, solve_failures=0, min_gap=math.inf)
    lam, ni, it, n_bad, trials, end, cur = 0.0, 2.0, 0, 0, 0, 0, 0.0
    more = max_it > 0 and nF > 0 and len(active) > 0
    if more:
        end = 0
    while more:
        H, b, chi = linearise(sc, est, meas, free_of, active, jac, order)
        for e, c in chi.items():
            edge_chi2[e] = c
        cur = ini = sum(chi[e] for e in order)
        if it == 0:
            out["chi2_initial"] = cur
            lam, ni, n_bad = 1e-16, 2.0, 0
        rho, q = 0.0, 0
        while True:
            ok = True
            try:
                Hl = H + lam * np.eye(7 * nF)
                if sparse:
                    x, _ = sparse_cholesky_solve(Hl, b, nF)
                else:
                    Lc = np.linalg.cholesky(Hl)
                    x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
                if not np.all(np.isfinite(x)):
                    raise np.linalg.LinAlgError
            except np.linalg.LinAlgError:
                ok, x = False, np.zeros(7 * nF)
                out["solve_failures"] += 1
            if sc["fix_scale"]:
                x[6::7] = 0.0
            trial = list(est)
            for v in range(n):
                if free_of[v] >= 0:
                    trial[v] = sim3_mul(sim3_exp(x[7 * free_of[v]:7 * free_of[v] + 7]), est[v])
            tchi = {}
            for e in order:
                err = edge_error(meas[e], trial[sc["edge_i"][e]], trial[sc["edge_j"][e]])
                tchi[e] = float(err @ err)
                edge_chi2[e] = tchi[e]
            temp = sum(tchi[e] for e in order) if ok else DBL_MAX
            scale = float(x @ (lam * x + b)) + 1e-3
            rho = (cur - temp) / scale
            if ok:
                out["min_gap"] = min(out["min_gap"], abs(cur - temp) / max(cur, 1.0))
            trials += 1
            q += 1
            if rho > 0 and math.isfinite(temp):
                tt = 2 * rho - 1
                alpha = min(1.0 - tt * tt * tt, 2.0 / 3.0)
                lam = lam * max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = temp
                est = trial
            else:
                lam = lam * ni
                ni = ni * 2
            if not (rho < 0 and q < 10):
                break
        it += 1
        if q == 10:
            end = END_TRIALS
        elif rho == 0:
            end = END_RHO_ZERO
        else:
            n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
            if n_bad >= 3:
                end = END_NO_PROGRESS
            elif it >= max_it:
                end = END_ITERATIONS
        more = end == 0
    if end == 0:
        end = END_ITERATIONS
    out.update(iterations=it, trials=trials, termination=end, lam=lam, chi2=cur, host_syncs=it + trials + 1, edge_chi2=edge_chi2,
               sim3_out=np.array([to_record(S) for S in est]))
    out["Tiw"] = np.array([tiw(S) for S in est])
    return out


def tiw(S):
    """(:1059-1067)"""
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] = quat_to_R(S[0]).astype(np.float32)
    T[:3, 3] = (S[1] * (1.0 / S[2])).astype(np.float32)
    return T


def correct_points(sim3, sim3_out, xw, ref_vertex):
    """(:1092-1100)"""
    out = np.asarray(xw, np.float32).copy()
    for p, r in enumerate(ref_vertex):
        if r >= 0:
            P = sim3_map(from_record(sim3[r]), out[p].astype(np.float64))
            out[p] = sim3_map(sim3_inverse(from_record(sim3_out[r])), P).astype(np.float32)
    return out


def assembled(sc, lam=1e-6):
    """the first linearisation's H + lam I in block-CSC (lower triangle, the diagonal first) and b: the operands of
    orbfe_block_sparse_solve7 -> (colptr, rowidx, blocks [k, 7, 7], rhs, H dense)"""
    est = [from_record(r) for r in sc["sim3"]]
    free_of, active, blocks = block_pattern(sc)
    nF = int((free_of >= 0).sum())
    H, b, _ = linearise(sc, est, measurements(sc), free_of, active, "analytic", active)
    H = H + lam * np.eye(7 * nF)
    colptr, rowidx, vals = [0], [], []
    for c in range(nF):
        for r in sorted(r for (r, cc) in blocks if cc == c):
            rowidx.append(r)
            vals.append(H[7 * r:7 * r + 7, 7 * c:7 * c + 7].copy())
        colptr.append(len(rowidx))
    return np.array(colptr, np.int32), np.array(rowidx, np.int32), np.array(vals), b, H


# ---- the scenes -----------------------------------------------------------------------------------------------------------------
def _rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = math.radians(deg)
    K = skew(a)
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * K @ K


def _scene(S, M, fixed, edges, fix_scale=False, n_iterations=4):
    e = np.array(edges, np.int64).reshape(-1, 3)
    return dict(sim3=np.array([to_record(s) for s in S]), sim3_meas=np.array([to_record(s) for s in M]),
                is_fixed=np.array(fixed, np.uint8), edge_i=e[:, 0].astype(np.int32), edge_j=e[:, 1].astype(np.int32),
                edge_kind=e[:, 2].astype(np.uint8), fix_scale=bool(fix_scale), n_iterations=int(n_iterations))


def _trajectory(n, rng, radius, turn_at=None):
    """n camera poses Siw (scale 1) along an arc of the given radius, looking along the path with a little wobble; turn_at:
    the camera is turned by 170 degrees from that vertex on"""
    S = []
    for k in range(n):
        ang = 2.0 * math.pi * k / n
        Rwc = _rot([0, 1, 0], math.degrees(ang)) @ _rot(rng.normal(size=3), 3.0 * rng.normal())
        if turn_at is not None and k >= turn_at:
            Rwc = Rwc @ _rot([0, 1, 0], 170.0)
        Ow = np.array([radius * math.cos(ang), 0.3 * rng.normal(), radius * math.sin(ang)])
        Rcw = Rwc.T
        S.append(sim3_from_Rts(Rcw, -Rcw @ Ow, 1.0))
    return S


def _perturbed(S, rng, rot_deg, trans, log_scale):
    u = np.concatenate([math.radians(rot_deg) * rng.normal(size=3), trans * rng.normal(size=3), [log_scale * rng.normal()]])
    return sim3_mul(sim3_exp(u), S)


def scenes():
    """[(id, scene, discrete)]: discrete False = compared on continuous results only.  n_iterations is the largest value up to
    6 at which every Levenberg decision of the restatement stays clear of summation noise (run()['min_gap'] > 1e-9, asserted
    by tests/test_essgraph_ref.py): a pose graph that reaches its minimum to the last place decides its next trial on noise.
    A chain with a fixed vertex has a zero minimum, which Gauss-Newton reaches within a few steps, so the chains start from
    perturbed estimates and stop earlier."""
    out = []
    rng = np.random.default_rng(20260)
    # 1. chain of 5, vertex 0 fixed, no loop, rotations and scales consistent: the error takes the small-angle, small-sigma
    #    branch of log on every edge; the translations start off by decimetres and one step takes chi2 to ~0
    M = _trajectory(5, rng, 4.0)
    S = [M[0]] + [(m[0].copy(), m[1] + 0.2 * rng.normal(size=3), m[2]) for m in M[1:]]
    out.append(("chain5", _scene(S, M, [1, 0, 0, 0, 0], [(k, k + 1, 0) for k in range(4)], n_iterations=1), True))
    # 2. chain of 5 with the fixed vertex in the middle and a sixth vertex without edges
    M = _trajectory(6, rng, 4.0)
    S = [M[k] if k in (2, 5) else _perturbed(M[k], rng, 2.0, 0.1, 0.03) for k in range(6)]
    out.append(("chain5_mid_fixed_isolated", _scene(S, M, [0, 0, 1, 0, 0, 0], [(k, k + 1, 0) for k in range(4)], n_iterations=2), True))
    # 3. ring of 12: the last three vertices are corrected (scale 1.1, a 10-degree turn), a bundle of 2 x 2 new loop
    #    connections links the last two vertices to the first two
    M = _trajectory(12, rng, 5.0)
    M = [_perturbed(m, rng, 0.5, 0.05, 0.0) for m in M]
    corr = (quat_from_R(_rot([0.2, 1.0, 0.1], 10.0)), np.array([0.3, -0.1, 0.2]), 1.1)
    S = [sim3_mul(corr, M[k]) if k >= 9 else M[k] for k in range(12)]
    ring = [(k, k + 1, 0) for k in range(11)] + [(10, 0, 1), (10, 1, 1), (11, 0, 1), (11, 1, 1)]
    fixed = [1] + [0] * 11
    out.append(("ring12", _scene(S, M, fixed, ring, n_iterations=4), True))
    # 4. the same with fix_scale: the pivots of the scale rows are lambda itself
    out.append(("ring12_fix_scale", _scene(S, M, fixed, ring, fix_scale=True, n_iterations=3), True))
    # 5. duplicate edges between one pair (a loop connection that is also a tree edge) and an extra old loop edge
    out.append(("ring12_duplicates", _scene(S, M, fixed, ring + [(3, 4, 0), (10, 1, 0), (2, 7, 0)], n_iterations=4), True))
    # 6. chain of 150 with covisibility band 3, two loop bundles, a 60 m extent, a 170-degree turn on the edges 70 -> 71..
    M = _trajectory(150, rng, 30.0, turn_at=71)
    corr = (quat_from_R(_rot([0.1, 1.0, -0.2], 6.0)), np.array([3.0, -1.0, 2.0]), 1.05)
    S = [sim3_mul(corr, M[k]) if k >= 140 else M[k] for k in range(150)]
    big = [(k, k + d, 0) for k in range(150) for d in (1, 2, 3) if k + d < 150]
    big += [(148, 0, 1), (148, 1, 1), (149, 0, 1), (149, 1, 1), (145, 30, 1), (146, 31, 1)]
    out.append(("chain150_band3_two_loops", _scene(S, M, [1] + [0] * 149, big, n_iterations=4), True))
    # 7. the ring at the reference's optimize(20): continuous results only.  (It ends at iteration 2 with ten rejected trials,
    #    as g2o does there: after one step the edges sit in the branch sigma >= eps, d > 1 - eps of Sim3::log, whose B of
    #    sim3.h:199 makes the linearisation a poor model of the error)
    sc7 = dict(out[2][1])
    sc7["n_iterations"] = 20
    out.append(("ring12_20_iterations", sc7, False))
    return out
