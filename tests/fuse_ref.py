"""Reference of the prologue of ORBmatcher::Fuse (src/ORBmatcher.cc:960-1006; the Sim3 overload :1135-1184) for the device
map-point table, n points against K key-frame poses:

* spec32: the arithmetic include/orbfe.h states for orbfe_project_fuse, operation by operation in numpy float32 (sums left to
  right, the norm and the dot product accumulated in float64 as cv::norm / Mat::dot do, the 60-degree compare in float64) --
  what the kernel must equal bit for bit;
* ref64: the same geometry entirely in float64 -- the independent statement of the reference's lines, against which both the
  spec and the kernel may differ only next to a threshold (near_threshold / near_integer: the GUARD bands);
* scene(): K poses around a point cloud on the KITTI camera of frustum_ref.py with K small key frames, built so that every
  rejection stage and every pyramid level occurs and the strict upper image bound is hit exactly.
"""
import numpy as np

from frustum_ref import BOUNDS, CX, CY, FX, FY, LEVELS, MBF, SCALE, rodrigues

GUARD = 1e-4
STAGES = ("skip", "bad", "in_keyframe", "depth", "image", "distance", "cosine")
SF = (np.float32(SCALE) ** np.arange(LEVELS)).astype(np.float32)  # mvScaleFactors
INV_SIGMA2 = (np.float32(1.0) / (SF * SF)).astype(np.float32)     # mvInvLevelSigma2
KF_POINTS = 300  # keypoints per key frame of a scene
ENGINEERED = 9   # points 0..7: one per level for pose 0; point 8: u == max_x for pose 0 (scenes of at least 16 points)

f32 = np.float32


def _pose(R, t):
    R = np.asarray(R, f32)
    t = np.asarray(t, f32)
    return dict(Rcw=R, tcw=t, Ow=(-(R.T @ t)).astype(f32))  # KeyFrame::SetPose: Ow = -Rcw^T tcw (src/KeyFrame.cc:75-80)


def _u_of(pose, P):
    """spec32's u of one float32 point (the search for u == max_x)."""
    R, t = pose["Rcw"], pose["tcw"]
    xc = ((R[0, 0] * P[0] + R[0, 1] * P[1]) + R[0, 2] * P[2]) + t[0]
    zc = ((R[2, 0] * P[0] + R[2, 1] * P[1]) + R[2, 2] * P[2]) + t[2]
    return f32(FX) * (xc * (f32(1.0) / zc)) + f32(CX)


def _on_upper_bound(pose, depth):
    """A float32 point in front of `pose` whose spec32 u equals mnMaxX exactly: start at the real solution on the optical row and
    walk the float32 neighbours of X."""
    Rd, td = pose["Rcw"].astype(np.float64), pose["tcw"].astype(np.float64)
    cam = np.array([(BOUNDS[1] - float(f32(CX))) / float(f32(FX)) * depth, 0.0, depth])
    P = (Rd.T @ (cam - td)).astype(f32)
    target = f32(BOUNDS[1])
    for _ in range(4096):
        u = _u_of(pose, P)
        if u == target:
            return P
        step = np.sign(float(target) - float(u)) * np.sign(float(pose["Rcw"][0, 0]))
        P[0] = np.nextafter(P[0], f32(np.inf) if step > 0 else f32(-np.inf))
    raise AssertionError("no float32 point projects onto the upper image bound")


def scene(seed, n, K):
    """dict: poses (K dicts of Rcw [3,3], tcw [3], Ow [3], float32), pos / normal [n,3], min_dist / max_dist [n], flags [n]
    (1 = bad), skip [K,n], in_kf [K,n] (the point observes key frame k), desc [n,32], frames (K dicts of x, y, octave, desc,
    u_right or None)."""
    # (the offset picks scenes that keep out of the guard bands -- a property of ref64 alone: tests/test_fuse_ref.py)
    rng = np.random.default_rng(7300 + seed)
    poses = [_pose(np.eye(3), np.zeros(3))]
    for _ in range(1, K):
        poses.append(_pose(rodrigues(rng.normal(0, 0.12, 3)), rng.normal(0, 0.6, 3)))
    pos = np.stack([rng.uniform(-12, 12, n), rng.uniform(-6, 6, n), rng.uniform(-4, 30, n)], axis=1).astype(f32)
    Ow0 = poses[0]["Ow"].astype(np.float64)
    to_cam = Ow0 - pos.astype(np.float64)
    dist = np.linalg.norm(to_cam, axis=1)
    rnd = rng.normal(0, 1, (n, 3))
    rnd /= np.linalg.norm(rnd, axis=1, keepdims=True)
    biased = -to_cam / np.maximum(dist, 1e-9)[:, None] + 0.5 * rnd  # mNormalVector points from the camera to the point
    biased /= np.linalg.norm(biased, axis=1, keepdims=True)
    normal = np.where((rng.random(n) < 0.7)[:, None], biased, rnd).astype(f32)
    max_dist = (dist * rng.uniform(0.7, 4.0, n)).astype(f32)
    min_dist = (max_dist.astype(np.float64) / 1.2 ** 7 * rng.uniform(0.5, 1.5, n)).astype(f32)
    flags = (rng.random(n) < 0.03).astype(np.uint8)
    skip = (rng.random((K, n)) < 0.03).astype(np.uint8)
    in_kf = rng.random((K, n)) < 0.05
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if n >= 16:
        # points 0..7: in front of pose 0, facing it, max_dist / dist = 1.2^(level - 0.5) -> level exactly; point 8: u == max_x
        for lv in range(LEVELS):
            pos[lv] = (f32(-3.0 + 0.8 * lv), f32(0.5 - 0.1 * lv), f32(6.0 + lv))
        pos[8] = _on_upper_bound(poses[0], 9.0)
        for i in range(ENGINEERED):
            d = float(np.linalg.norm(pos[i].astype(np.float64) - Ow0))
            ratio = 1.2 ** ((i if i < LEVELS else 3) - 0.5)
            normal[i] = ((pos[i].astype(np.float64) - Ow0) / d).astype(f32)
            max_dist[i] = f32(d * ratio)
            min_dist[i] = f32(d * ratio / 1.2 ** 7)
        flags[:ENGINEERED] = 0
        skip[0, :ENGINEERED] = 0
        in_kf[0, :ENGINEERED] = False
        # ... and every early stage at least once, on points that would otherwise be searched
        flags[ENGINEERED] = 1
        skip[0, ENGINEERED + 1] = 1
        in_kf[0, ENGINEERED + 2] = True
    sc = dict(poses=poses, pos=pos, normal=normal, min_dist=min_dist, max_dist=max_dist, flags=flags, skip=skip, in_kf=in_kf,
              desc=desc)
    sc["frames"] = _keyframes(rng, sc, spec32(sc, skip=np.zeros((K, n), np.uint8), in_kf=np.zeros((K, n), bool)))
    return sc


def _keyframes(rng, sc, pr):
    """K key frames of KF_POINTS keypoints: most sit near the projection of a point that passes the geometry (noise around one
    pixel per level, so that the chi-square gate of src/ORBmatcher.cc:1030-1054 passes some and fails some), at the predicted
    octave or the one below, with the point's descriptor and a few flipped bits; even key frames are stereo with a part of
    their keypoints monocular (u_right < 0)."""
    frames = []
    K, n = pr["valid"].shape
    for k in range(K):
        m = KF_POINTS
        x = rng.uniform(BOUNDS[0], BOUNDS[1] - 1, m).astype(f32)
        y = rng.uniform(BOUNDS[2], BOUNDS[3] - 1, m).astype(f32)
        octave = rng.integers(0, LEVELS, m).astype(np.int32)
        desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        ur = np.full(m, -1.0, f32)
        ok = np.flatnonzero(pr["valid"][k])
        src = rng.permutation(ok)[: min(len(ok), (3 * m) // 4)]
        j = np.arange(len(src))
        lv = pr["level"][k, src]
        sigma = 1.3 * SF[lv]
        x[j] = (pr["u"][k, src] + rng.normal(0, 1, len(src)) * sigma).astype(f32)
        y[j] = (pr["v"][k, src] + rng.normal(0, 1, len(src)) * sigma).astype(f32)
        octave[j] = np.clip(lv - rng.integers(0, 2, len(src)), 0, LEVELS - 1)
        flips = rng.integers(0, 256, (len(src), 32), dtype=np.uint8) & rng.integers(0, 256, (len(src), 32), dtype=np.uint8) & \
            rng.integers(0, 256, (len(src), 32), dtype=np.uint8)
        heavy = rng.random(len(src)) < 0.25  # a quarter of them too far for TH_LOW
        desc[j] = sc["desc"][src] ^ np.where(heavy[:, None], rng.integers(0, 256, (len(src), 32), dtype=np.uint8), flips & (flips >> 1))
        stereo = k % 2 == 0
        if stereo:
            ur[j] = np.where(rng.random(len(src)) < 0.7, pr["ur"][k, src] + rng.normal(0, 1, len(src)) * sigma, -1.0).astype(f32)
            rest = np.arange(len(src), m)
            ur[rest] = np.where(rng.random(len(rest)) < 0.5, x[rest] - rng.uniform(1, 40, len(rest)), -1.0).astype(f32)
        frames.append(dict(x=x, y=y, octave=octave, desc=desc, u_right=ur if stereo else None))
    return frames


def sim3_poses(sc, s):
    """The poses of `sc` as the Sim3 overload of Fuse decomposes them from Scw = [s R | s t] (src/ORBmatcher.cc:1121-1125), on the
    host in float32: scw = sqrt(sRcw.row(0).dot(sRcw.row(0))), Rcw = sRcw / scw, tcw = Scw(0..2, 3) / scw, Ow = -Rcw^T tcw."""
    out = []
    for p in sc["poses"]:
        sR = (f32(s) * p["Rcw"]).astype(f32)
        st = (f32(s) * p["tcw"]).astype(f32)
        scw = f32(np.sqrt(np.dot(sR[0].astype(np.float64), sR[0].astype(np.float64))))  # Mat::dot accumulates in double
        R = (sR / scw).astype(f32)
        t = (st / scw).astype(f32)
        out.append(dict(Rcw=R, tcw=t, Ow=(-(R.T @ t)).astype(f32)))
    return out


def _stages(skip, bad, inkf, zc, u, v, dist, lo, hi, dot, half, bounds):
    """first rejecting stage per point (index into STAGES, -1 = searched); comparisons in the reference's sense"""
    with np.errstate(invalid="ignore"):
        in_image = (u >= bounds[0]) & (u < bounds[1]) & (v >= bounds[2]) & (v < bounds[3])  # KeyFrame::IsInImage: strict above
        tests = [skip != 0, bad != 0, inkf, zc < 0, ~in_image, (dist < lo) | (dist > hi), dot < half]
    stage = np.full(len(zc), -1, np.int32)
    for k in range(len(tests) - 1, -1, -1):
        stage[tests[k]] = k
    return stage


def _level(stage, quotient, n_levels):
    with np.errstate(invalid="ignore"):
        c = np.ceil(quotient)
        level = np.where(c > 0, np.minimum(c, n_levels - 1), 0)
    return np.nan_to_num(np.where(stage < 0, level, 0)).astype(np.int32)


def _masks(sc, skip, in_kf):
    K, n = len(sc["poses"]), len(sc["pos"])
    sk = sc["skip"] if skip is None else np.asarray(skip)
    ik = sc["in_kf"] if in_kf is None else np.asarray(in_kf)
    return np.asarray(sk, np.uint8).reshape(K, n), np.asarray(ik, bool).reshape(K, n)


def _stack(rows):
    return {name: np.stack([r[name] for r in rows]) for name in rows[0]}


def spec32(sc, poses=None, skip=None, in_kf=None, bounds=BOUNDS, scale=SCALE, n_levels=LEVELS, K4=(FX, FY, CX, CY), mbf=MBF):
    """include/orbfe.h's arithmetic.  Returns a dict of [K, n] arrays: valid, u, v, ur, dist (0 where not valid, as the library
    writes them), level, stage."""
    poses = sc["poses"] if poses is None else poses
    sk, ik = _masks(sc, skip, in_kf)
    P, N = sc["pos"].astype(f32), sc["normal"].astype(f32)
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    fx, fy, cx, cy = [f32(v) for v in K4]
    b = [f32(v) for v in bounds]
    lo = f32(0.8) * sc["min_dist"].astype(f32)
    hi = f32(1.2) * sc["max_dist"].astype(f32)
    logf = np.float64(f32(np.log(f32(scale))))  # mfLogScaleFactor is a float
    rows = []
    for k, p in enumerate(poses):
        R, t, Ow = p["Rcw"].astype(f32), p["tcw"].astype(f32), p["Ow"].astype(f32)
        with np.errstate(all="ignore"):
            xc, yc, zc = [((R[r, 0] * X + R[r, 1] * Y) + R[r, 2] * Z) + t[r] for r in range(3)]
            invz = f32(1.0) / zc
            x = xc * invz
            y = yc * invz
            u = fx * x + cx
            v = fy * y + cy
            ur = u - f32(mbf) * invz
            PO = [(P[:, i] - Ow[i]).astype(np.float64) for i in range(3)]
            dist = np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]).astype(f32)
            dot = (PO[0] * N[:, 0].astype(np.float64) + PO[1] * N[:, 1].astype(np.float64)) + PO[2] * N[:, 2].astype(np.float64)
            half = np.float64(0.5) * dist.astype(np.float64)
            ratio = sc["max_dist"].astype(f32) / dist
            quotient = np.log(ratio.astype(np.float64)) / logf
        assert all(a.dtype == f32 for a in (xc, invz, x, u, v, ur, dist, lo, hi, ratio))
        stage = _stages(sk[k], sc["flags"] & 1, ik[k], zc, u, v, dist, lo, hi, dot, half, b)
        ok = stage < 0
        z = lambda a: np.where(ok, a, f32(0)).astype(f32)
        rows.append(dict(valid=ok.astype(np.uint8), u=z(u), v=z(v), ur=z(ur), dist=z(dist), level=_level(stage, quotient, n_levels),
                         stage=stage))
    return _stack(rows)


def ref64(sc, poses=None, skip=None, in_kf=None, bounds=BOUNDS, scale=SCALE, n_levels=LEVELS, K4=(FX, FY, CX, CY), mbf=MBF):
    """src/ORBmatcher.cc:960-1006 evaluated in float64 from the same float32 inputs.  [K, n] arrays: valid, level, stage and the raw
    u / v / ur / zc / dist / cos / quotient / lo / hi for the guard bands."""
    poses = sc["poses"] if poses is None else poses
    sk, ik = _masks(sc, skip, in_kf)
    P, N = sc["pos"].astype(np.float64), sc["normal"].astype(np.float64)
    fx, fy, cx, cy = [float(f32(v)) for v in K4]
    b = [float(f32(v)) for v in bounds]
    lo = 0.8 * sc["min_dist"].astype(np.float64)  # GetMinDistanceInvariance / GetMaxDistanceInvariance (src/MapPoint.cc)
    hi = 1.2 * sc["max_dist"].astype(np.float64)
    rows = []
    for k, p in enumerate(poses):
        R, t, Ow = p["Rcw"].astype(np.float64), p["tcw"].astype(np.float64), p["Ow"].astype(np.float64)
        with np.errstate(all="ignore"):
            Pc = P @ R.T + t                      # :969
            zc = Pc[:, 2]                         # :972
            u = fx * (Pc[:, 0] / zc) + cx         # :975-980
            v = fy * (Pc[:, 1] / zc) + cy
            ur = u - float(f32(mbf)) / zc         # :986
            PO = P - Ow                           # :990
            dist = np.linalg.norm(PO, axis=1)     # :991
            dot = np.einsum("ij,ij->i", PO, N)    # :1000
            quotient = np.log(sc["max_dist"].astype(np.float64) / dist) / np.log(float(scale))  # MapPoint::PredictScale
        stage = _stages(sk[k], sc["flags"] & 1, ik[k], zc, u, v, dist, lo, hi, dot, 0.5 * dist, b)
        rows.append(dict(valid=(stage < 0).astype(np.uint8), level=_level(stage, quotient, n_levels), stage=stage, u=u, v=v, ur=ur,
                         zc=zc, dist=dist, cos=dot / dist, quotient=quotient, lo=np.broadcast_to(lo, zc.shape).copy(),
                         hi=np.broadcast_to(hi, zc.shape).copy()))
    return _stack(rows)


def near_threshold(r64, bounds=BOUNDS, guard=GUARD):
    """(k, i) pairs whose float64 values lie within a relative `guard` of one of the prologue's thresholds (zc, the four bounds,
    the two distances, the 60-degree cosine): the only ones on which a float32 evaluation may decide otherwise."""
    with np.errstate(all="ignore"):
        u, v, zc, d, c = r64["u"], r64["v"], r64["zc"], r64["dist"], r64["cos"]
        scale_u = np.maximum(np.abs(u), bounds[1])
        scale_v = np.maximum(np.abs(v), bounds[3])
        near = np.abs(zc) < guard * np.maximum(1.0, np.abs(d))
        for bx in bounds[:2]:
            near |= np.abs(u - bx) < guard * scale_u
        for by in bounds[2:]:
            near |= np.abs(v - by) < guard * scale_v
        near |= np.abs(d - r64["lo"]) < guard * d
        near |= np.abs(d - r64["hi"]) < guard * d
        near |= np.abs(c - 0.5) < guard
    return near


def near_integer(r64, guard=GUARD):
    """(k, i) pairs whose float64 level quotient lies within `guard` of an integer: log has no correctly rounded form."""
    with np.errstate(invalid="ignore"):
        q = r64["quotient"]
        return np.abs(q - np.round(q)) < guard


def excluded(r64):
    """The guard bands of the comparison with ref64: pairs the early stages (skip, bad, in key frame) reject are never excluded."""
    early = (r64["stage"] >= 0) & (r64["stage"] <= 2)
    return (near_threshold(r64) | (near_integer(r64) & (r64["stage"] < 0))) & ~early
