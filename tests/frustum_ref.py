"""Reference of Frame::isInFrustum + MapPoint::PredictScale (src/Frame.cc:292-353) for the device map-point table:

* spec32: the arithmetic include/orbfe.h states for orbfe_project_in_frustum, operation by operation in numpy float32 (sums left
  to right, the norm and the dot product accumulated in float64 as cv::norm / Mat::dot do) -- what the kernel must equal bit
  for bit;
* ref64: the same formulas entirely in float64 -- the independent statement of the reference's geometry, against which both
  the spec and the kernel may differ only next to a threshold;
* scene(): a pose, map points and the KITTI camera of bench.py, built so that every rejection stage and every pyramid level
  occurs.
"""
import numpy as np

FX, FY, CX, CY, MBF = 718.856, 718.856, 607.1928, 185.2157, 386.1448  # KITTI 00-02 (bench.py: fx, bf)
BOUNDS = (0.0, 1241.0, 0.0, 376.0)  # mnMinX, mnMaxX, mnMinY, mnMaxY
LIMIT, SCALE, LEVELS = 0.5, 1.2, 8
GUARD = 1e-4
STAGES = ("skip", "bad", "depth", "image", "distance", "cosine")

f32 = np.float32


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th < 1e-12:
        return np.eye(3)
    k = np.asarray(w, np.float64) / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def scene(seed, n):
    """dict: Rcw [3,3], tcw [3], Ow [3] (float32), pos / normal [n,3], min_dist / max_dist [n], flags [n] (1 = bad, 2 = observed),
    skip [n], desc [n,32]."""
    # (the offset picks scenes that keep out of the guard bands below -- a property of ref64 alone: tests/test_frustum_ref.py)
    rng = np.random.default_rng(5900 + seed)
    R = rodrigues(rng.normal(0, 0.2, 3)).astype(f32)
    t = rng.normal(0, 0.5, 3).astype(f32)
    Ow = (-(R.T.astype(f32) @ t)).astype(f32)  # Frame::UpdatePoseMatrices (src/Frame.cc:277-283)
    pos = np.stack([rng.uniform(-12, 12, n), rng.uniform(-6, 6, n), rng.uniform(-4, 30, n)], axis=1).astype(f32)
    to_cam = Ow.astype(np.float64) - pos.astype(np.float64)
    dist = np.linalg.norm(to_cam, axis=1)
    rnd = rng.normal(0, 1, (n, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    biased = -to_cam / np.maximum(dist, 1e-9)[:, None] + 0.5 * rnd  # mNormalVector points from the camera to the point
    biased /= np.linalg.norm(biased, axis=1, keepdims=True)
    normal = np.where((rng.random(n) < 0.6)[:, None], biased, rnd).astype(f32)
    max_dist = (dist * rng.uniform(0.7, 4.0, n)).astype(f32)
    min_dist = (max_dist.astype(np.float64) / 1.2 ** 7 * rng.uniform(0.5, 1.5, n)).astype(f32)
    flags = ((rng.random(n) < 0.02).astype(np.uint8) * 1) | ((rng.random(n) < 0.8).astype(np.uint8) * 2)
    skip = (rng.random(n) < 0.03).astype(np.uint8)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    return dict(Rcw=R, tcw=t, Ow=Ow, pos=pos, normal=normal, min_dist=min_dist, max_dist=max_dist, flags=flags.astype(np.uint8),
                skip=skip, desc=desc)


def _stages(skip, bad, zc, u, v, dist, lo, hi, cos, limit, bounds):
    """first rejecting stage per point (index into STAGES, -1 = in view); comparisons in the reference's sense"""
    with np.errstate(invalid="ignore"):
        tests = [skip != 0, bad != 0, zc < 0, (u < bounds[0]) | (u > bounds[1]) | (v < bounds[2]) | (v > bounds[3]),
                 (dist < lo) | (dist > hi), cos < limit]
    stage = np.full(len(zc), -1, np.int32)
    for k in range(len(tests) - 1, -1, -1):
        stage[tests[k]] = k
    return stage


def _finish(stage, quotient, n_levels):
    with np.errstate(invalid="ignore"):
        c = np.ceil(quotient)
        level = np.where(c > 0, np.minimum(c, n_levels - 1), 0)
    level = np.where(stage < 0, level, 0)
    return np.nan_to_num(level).astype(np.int32)


def spec32(sc, skip=None, limit=LIMIT, bounds=BOUNDS, scale=SCALE, n_levels=LEVELS, K4=(FX, FY, CX, CY), mbf=MBF):
    """include/orbfe.h's arithmetic.  Returns a dict: in_view, level, view_cos, proj_x, proj_y, proj_xr, inv_z, dist (0 where not in
    view, as the library writes them), stage, and the raw u / v / zc / dist_all / cos_all / quotient for the guard bands."""
    R, t, Ow = sc["Rcw"].astype(f32), sc["tcw"].astype(f32), sc["Ow"].astype(f32)
    P, N = sc["pos"].astype(f32), sc["normal"].astype(f32)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    fx, fy, cx, cy = [f32(v) for v in K4]
    b = [f32(v) for v in bounds]
    with np.errstate(all="ignore"):
        cam = [((R[r, 0] * X + R[r, 1] * Y) + R[r, 2] * Z) + t[r] for r in range(3)]
        xc, yc, zc = cam
        invz = f32(1.0) / zc
        u = (fx * xc) * invz + cx
        v = (fy * yc) * invz + cy
        PO = [(P[:, i] - Ow[i]).astype(np.float64) for i in range(3)]
        dist = np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]).astype(f32)
        lo = f32(0.8) * sc["min_dist"].astype(f32)
        hi = f32(1.2) * sc["max_dist"].astype(f32)
        dot = (PO[0] * N[:, 0].astype(np.float64) + PO[1] * N[:, 1].astype(np.float64)) + PO[2] * N[:, 2].astype(np.float64)
        cos = (dot / dist.astype(np.float64)).astype(f32)
        ratio = sc["max_dist"].astype(f32) / dist
        logf = np.float64(f32(np.log(f32(scale))))  # mfLogScaleFactor is a float (include/Frame.h)
        quotient = np.log(ratio.astype(np.float64)) / logf
        xr = u - f32(mbf) * invz
    assert all(a.dtype == f32 for a in (xc, invz, u, v, dist, lo, hi, cos, ratio, xr))
    sk = np.zeros(len(X), np.uint8) if skip is None else np.asarray(skip, np.uint8)
    stage = _stages(sk, sc["flags"] & 1, zc, u, v, dist, lo, hi, cos, f32(limit), b)
    ok = stage < 0
    z = lambda a: np.where(ok, a, f32(0)).astype(f32)
    return dict(in_view=ok.astype(np.uint8), level=_finish(stage, quotient, n_levels), view_cos=z(cos), proj_x=z(u), proj_y=z(v),
                proj_xr=z(xr), inv_z=z(invz), dist=z(dist), stage=stage, u=u, v=v, zc=zc, dist_all=dist, cos_all=cos,
                quotient=quotient, lo=lo, hi=hi)


def ref64(sc, skip=None, limit=LIMIT, bounds=BOUNDS, scale=SCALE, n_levels=LEVELS, K4=(FX, FY, CX, CY), mbf=MBF):
    """src/Frame.cc:292-353 evaluated in float64 from the same float32 inputs."""
    R, t, Ow = sc["Rcw"].astype(np.float64), sc["tcw"].astype(np.float64), sc["Ow"].astype(np.float64)
    P, N = sc["pos"].astype(np.float64), sc["normal"].astype(np.float64)
    fx, fy, cx, cy = [float(f32(v)) for v in K4]
    b = [float(f32(v)) for v in bounds]
    with np.errstate(all="ignore"):
        Pc = P @ R.T + t
        zc = Pc[:, 2]
        u = fx * Pc[:, 0] / zc + cx
        v = fy * Pc[:, 1] / zc + cy
        PO = P - Ow
        dist = np.linalg.norm(PO, axis=1)
        lo = 0.8 * sc["min_dist"].astype(np.float64)
        hi = 1.2 * sc["max_dist"].astype(np.float64)
        cos = np.einsum("ij,ij->i", PO, N) / dist
        quotient = np.log(sc["max_dist"].astype(np.float64) / dist) / np.log(float(scale))
        xr = u - float(f32(mbf)) / zc
    sk = np.zeros(len(zc), np.uint8) if skip is None else np.asarray(skip, np.uint8)
    stage = _stages(sk, sc["flags"] & 1, zc, u, v, dist, lo, hi, cos, float(limit), b)
    return dict(in_view=(stage < 0).astype(np.uint8), level=_finish(stage, quotient, n_levels), stage=stage, u=u, v=v, zc=zc,
                dist_all=dist, cos_all=cos, quotient=quotient, proj_xr=xr, lo=lo, hi=hi)


def near_threshold(r64, limit=LIMIT, bounds=BOUNDS, guard=GUARD):
    """Points whose float64 values lie within a relative `guard` of one of isInFrustum's thresholds (zc, the four bounds, the
    two distances, the cosine): the only ones on which a float32 evaluation may decide otherwise."""
    with np.errstate(all="ignore"):
        u, v, zc, d, c = r64["u"], r64["v"], r64["zc"], r64["dist_all"], r64["cos_all"]
        scale_u = np.maximum(np.abs(u), bounds[1])
        scale_v = np.maximum(np.abs(v), bounds[3])
        near = np.abs(zc) < guard * np.maximum(1.0, np.abs(d))
        for bx in bounds[:2]:
            near |= np.abs(u - bx) < guard * scale_u
        for by in bounds[2:]:
            near |= np.abs(v - by) < guard * scale_v
        near |= np.abs(d - r64["lo"]) < guard * d
        near |= np.abs(d - r64["hi"]) < guard * d
        near |= np.abs(c - limit) < guard
    return near


def near_integer(r64, guard=GUARD):
    """Points whose float64 level quotient lies within `guard` of an integer: log has no correctly rounded form."""
    with np.errstate(invalid="ignore"):
        q = r64["quotient"]
        return np.abs(q - np.round(q)) < guard
