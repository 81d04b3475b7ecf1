"""Reference of the prologues of the two tracking-thread searches that walk a frame's own map points, for the device map-point
table: SearchByProjection(CurrentFrame, LastFrame, th, bMono) (form "last", src/ORBmatcher.cc:1516-1550) and
SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (form "kf", :1665-1699), K jobs over concatenated lists.

* spec32: the arithmetic include/orbfe.h states for orbfe_project_last_frame / orbfe_project_keyframe, operation by operation
  in numpy float32 (sums left to right, the norm accumulated in float64 as cv::norm does) -- what the kernel must equal bit
  for bit;
* ref64: the same geometry entirely in float64 -- the independent statement of the reference's lines, against which both the
  spec and the kernel may differ only next to a threshold (near_threshold / near_integer: the GUARD bands, as in fuse_ref.py);
* scene(): K poses, each with its own list of points, on the KITTI camera of frustum_ref.py, and one current frame of
  CUR_POINTS keypoints.  Job 0 carries the engineered points (ENGINEERED, scenes whose job 0 holds at least 16 points).
"""
import numpy as np

from frustum_ref import BOUNDS, CX, CY, FX, FY, LEVELS, MBF, SCALE, rodrigues

GUARD = 1e-4
STAGES = {"last": ("skip", "depth", "image"), "kf": ("skip", "bad", "image", "distance")}
SF = (np.float32(SCALE) ** np.arange(LEVELS)).astype(np.float32)  # mvScaleFactors
INV_SIGMA2 = (np.float32(1.0) / (SF * SF)).astype(np.float32)     # mvInvLevelSigma2
CUR_POINTS = 300  # keypoints of the current frame of a scene
# positions in job 0 of the engineered points: 0..7 one per level (key-frame form) and per octave (last-frame form);
ON_BOUND = 8      # u == max_x exactly: accepted by both forms (the bounds are inclusive, unlike Fuse's)
BEHIND = 9        # zc < 0, projecting inside the image: the key-frame form keeps it, the last-frame form drops it
BAD = 10          # ORBFE_MP_BAD, in the image: the last-frame form keeps it, the key-frame form drops it
ZERO_DEPTH = 11   # xc == yc == zc == 0: 1/zc = inf, u = NaN -- rejected at the image test by both forms
SKIPPED = 12      # skip set on a point that would otherwise be searched
ENGINEERED = 13

f32 = np.float32


def _sums(R, t, P):
    """spec32's camera coordinates of float32 points [n, 3]"""
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    return [((R[r, 0] * X + R[r, 1] * Y) + R[r, 2] * Z) + t[r] for r in range(3)]


def _u_of(pose, P):
    xc, _, zc = _sums(pose["Rcw"], pose["tcw"], P[None, :])
    return (f32(FX) * xc * (f32(1.0) / zc) + f32(CX))[0]


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


def _world(pose, cam):
    """float32 world points of float64 camera coordinates [n, 3]"""
    Rd, td = pose["Rcw"].astype(np.float64), pose["tcw"].astype(np.float64)
    return ((cam - td) @ Rd).astype(f32)


def scene(seed, n, K):
    """n: the length of every job's list, or K lengths.  dict: poses (K dicts of Rcw [3,3], tcw [3], Ow [3], float32), offsets
    [K+1], and over the concatenated list pos / normal [N,3], min_dist / max_dist, flags (1 = bad, 2 = observed), skip,
    last_octave, angle (the last frame's / key frames' mvKeysUn angle), desc [N,32]; th / orb_dist [K]; mode (0 / 1 / 2, by
    seed); cur / cur_stereo: the current frame (x, y, octave, angle, desc, u_right)."""
    # (the offset picks scenes that keep out of the guard bands -- a property of ref64 alone: tests/test_track_ref.py)
    rng = np.random.default_rng(8100 + seed)
    counts = [int(n)] * K if np.isscalar(n) else [int(c) for c in n]
    assert len(counts) == K
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    N = int(offsets[-1])
    # pose 0: the translation is MADE from the zero-depth point, so that its three sums cancel exactly
    R0 = rodrigues(rng.normal(0, 0.12, 3)).astype(f32)
    Pz = np.array([0.3125, -0.21875, 0.53125], f32)
    X, Y, Z = Pz
    t0 = np.array([-((R0[r, 0] * X + R0[r, 1] * Y) + R0[r, 2] * Z) for r in range(3)], f32)
    poses = [dict(Rcw=R0, tcw=t0, Ow=(-(R0.T @ t0)).astype(f32))]
    for _ in range(1, K):
        R = rodrigues(rng.normal(0, 0.12, 3)).astype(f32)
        t = rng.normal(0, 0.6, 3).astype(f32)
        poses.append(dict(Rcw=R, tcw=t, Ow=(-(R.T @ t)).astype(f32)))  # Frame::UpdatePoseMatrices (src/Frame.cc:277-283)
    job = np.repeat(np.arange(K), counts)
    cam = np.stack([rng.uniform(-12, 12, N), rng.uniform(-6, 6, N), rng.uniform(-4, 30, N)], axis=1)
    pos = np.zeros((N, 3), f32)
    for k in range(K):
        pos[job == k] = _world(poses[k], cam[job == k])
    Ow = np.stack([p["Ow"] for p in poses] + [np.zeros(3, f32)])[job].astype(np.float64).reshape(N, 3)
    dist = np.linalg.norm(pos.astype(np.float64) - Ow, axis=1)
    normal = rng.normal(0, 1, (N, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(f32)
    max_dist = (dist * rng.uniform(0.7, 4.0, N)).astype(f32)
    min_dist = (max_dist.astype(np.float64) / 1.2 ** 7 * rng.uniform(0.5, 1.5, N)).astype(f32)
    flags = ((rng.random(N) < 0.03).astype(np.uint8) * 1) | ((rng.random(N) < 0.8).astype(np.uint8) * 2)
    skip = (rng.random(N) < 0.03).astype(np.uint8)
    last_octave = rng.integers(0, LEVELS, N).astype(np.int32)
    angle = rng.uniform(0, 360, N).astype(f32)
    desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    if counts[0] >= 16:
        p0 = poses[0]
        for lv in range(LEVELS):
            pos[lv] = _world(p0, np.array([[-3.0 + 0.8 * lv, 0.5 - 0.1 * lv, 6.0 + lv]]))[0]
            last_octave[lv] = lv
        pos[ON_BOUND] = _on_upper_bound(p0, 9.0)
        pos[BEHIND] = _world(p0, np.array([[0.4, -0.2, -7.0]]))[0]
        pos[BAD] = _world(p0, np.array([[1.0, 0.3, 8.0]]))[0]
        pos[ZERO_DEPTH] = Pz
        pos[SKIPPED] = _world(p0, np.array([[-1.0, 0.2, 7.0]]))[0]
        for i in range(ENGINEERED):
            d = float(np.linalg.norm(pos[i].astype(np.float64) - p0["Ow"].astype(np.float64)))
            ratio = 1.2 ** ((i if i < LEVELS else 3) - 0.5)  # max_dist / dist -> the level exactly
            max_dist[i] = f32(d * ratio)
            min_dist[i] = f32(d * ratio / 1.2 ** 7)
        flags[:ENGINEERED] = 2
        skip[:ENGINEERED] = 0
        flags[BAD] = 3
        skip[SKIPPED] = 1
    sc = dict(poses=poses, offsets=offsets, pos=pos, normal=normal, min_dist=min_dist, max_dist=max_dist, flags=flags, skip=skip,
              last_octave=last_octave, angle=angle, desc=desc, mode=seed % 3,
              th=np.array([f32(10.0) if k % 2 == 0 else f32(3.0) for k in range(K)], f32),
              orb_dist=np.array([100 if k % 2 == 0 else 64 for k in range(K)], np.int32))
    sc["cur"] = current_frame(rng, sc, stereo=False)
    sc["cur_stereo"] = current_frame(rng, sc, stereo=True)
    return sc


def current_frame(rng, sc, stereo, m=CUR_POINTS, offset=None):
    """The current frame: most keypoints sit near the projection of a point that one of the two forms searches (noise well inside
    the smallest window, or -- offset = (lo, hi) -- at lo .. hi times th = 7 windows' radius from it), at the point's octave /
    level or a neighbour, with the point's descriptor and a few flipped bits and its angle plus a common rotation, so that the
    rotation histogram keeps most and drops some; the rest is clutter."""
    N = len(sc["pos"])
    x = rng.uniform(BOUNDS[0], BOUNDS[1] - 1, m).astype(f32)
    y = rng.uniform(BOUNDS[2], BOUNDS[3] - 1, m).astype(f32)
    octave = rng.integers(0, LEVELS, m).astype(np.int32)
    ang = rng.uniform(0, 360, m).astype(f32)
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    ur = np.full(m, -1.0, f32)
    if N:
        zero = np.zeros(N, np.uint8)
        last, kf = spec32(sc, "last", skip=zero), spec32(sc, "kf", skip=zero)
        ok = np.flatnonzero((last["valid"] != 0) | (kf["valid"] != 0))
        src = rng.permutation(ok)[: min(len(ok), (3 * m) // 4)]
        j = np.arange(len(src))
        raw = spec32(sc, "last", skip=zero, raw=True)
        # (half of the points both forms search sit at the key-frame form's level, the others at the last frame's octave)
        lv = np.where((kf["valid"][src] != 0) & ((rng.random(len(src)) < 0.5) | (last["valid"][src] == 0)), kf["level"][src],
                      sc["last_octave"][src])
        if offset is None:
            dx, dy = rng.normal(0, 0.7, len(src)), rng.normal(0, 0.7, len(src))
        else:
            # (the windows are squares: the offset along x alone puts the keypoint outside)
            rad = rng.uniform(offset[0], offset[1], len(src)) * 7.0 * SF[sc["last_octave"][src]]
            dx, dy = rad * rng.choice([-1.0, 1.0], len(src)), rad * rng.uniform(-0.5, 0.5, len(src))
        x[j] = (raw["u"][src] + dx).astype(f32)
        y[j] = (raw["v"][src] + dy).astype(f32)
        octave[j] = np.clip(lv + rng.integers(-1, 2, len(src)), 0, LEVELS - 1)
        flips = rng.integers(0, 256, (len(src), 32), dtype=np.uint8) & rng.integers(0, 256, (len(src), 32), dtype=np.uint8) & \
            rng.integers(0, 256, (len(src), 32), dtype=np.uint8)
        heavy = rng.random(len(src)) < 0.2  # a fifth of them too far for TH_HIGH
        desc[j] = sc["desc"][src] ^ np.where(heavy[:, None], rng.integers(0, 256, (len(src), 32), dtype=np.uint8), flips & (flips >> 1))
        turned = rng.random(len(src)) < 0.15  # outside the three leading histogram bins
        ang[j] = np.mod(sc["angle"][src] - 25.0 + np.where(turned, rng.uniform(60, 300, len(src)), rng.normal(0, 3, len(src))), 360.0).astype(f32)
        if stereo:
            ur[j] = np.where(rng.random(len(src)) < 0.7, raw["ur"][src] + rng.normal(0, 1.5, len(src)), -1.0).astype(f32)
    if stereo:
        rest = np.arange(min(len(ur), (3 * m) // 4), m)
        ur[rest] = np.where(rng.random(len(rest)) < 0.5, x[rest] - rng.uniform(1, 40, len(rest)), -1.0).astype(f32)
    keep = (x >= BOUNDS[0]) & (x < BOUNDS[1]) & (y >= BOUNDS[2]) & (y < BOUNDS[3])
    x, y = np.where(keep, x, f32(5.0)), np.where(keep, y, f32(5.0))  # (a frame holds no keypoint outside its bounds)
    return dict(x=x, y=y, octave=octave, angle=ang, desc=desc, u_right=ur if stereo else None)


def _stages(form, skip, bad, zc, u, v, dist, lo, hi, bounds):
    """first rejecting stage per point (index into STAGES[form], -1 = searched).  The image test keeps u >= min_x && u <= max_x &&
    v >= min_y && v <= max_y: the reference's four rejects with a NaN coordinate rejected too (include/orbfe.h)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        out_image =~((u >= bounds[0]) & (u <= bounds[1]) & (v >= bounds[2]) & (v <= bounds[3]))
        if form == "last":
            tests = [skip != 0, (1.0 / zc) < 0, out_image]  # invzc < 0 (:1524): true for zc = -0 as well
        else:
            tests = [skip != 0, bad != 0, out_image, (dist < lo) | (dist > hi)]
    stage = np.full(len(zc), -1, np.int32)
    for k in range(len(tests) - 1, -1, -1):
        stage[tests[k]] = k
    return stage


def _level(stage, quotient, n_levels):
    with np.errstate(invalid="ignore"):
        c = np.ceil(quotient)
        level = np.where(c > 0, np.minimum(c, n_levels - 1), 0)
    return np.nan_to_num(np.where(stage < 0, level, 0)).astype(np.int32)


def _job_of(sc):
    return np.repeat(np.arange(len(sc["poses"])), np.diff(sc["offsets"]))


def spec32(sc, form, skip=None, th=None, raw=False, bounds=BOUNDS, scale=SCALE, n_levels=LEVELS, K4=(FX, FY, CX, CY), mbf=MBF):
    """include/orbfe.h's arithmetic over the concatenated list.  form "last": valid, u, v, inv_z, ur, radius (th: one float,
    default 7); form "kf": valid, u, v, inv_z, level, dist; both with stage.  The fields are 0 where valid is, as the library
    writes them (raw: as computed)."""
    N = len(sc["pos"])
    sk = sc["skip"] if skip is None else np.asarray(skip, np.uint8)
    P = sc["pos"].astype(f32)
    fx, fy, cx, cy = [f32(v) for v in K4]
    b = [f32(v) for v in bounds]
    lo = f32(0.8) * sc["min_dist"].astype(f32)
    hi = f32(1.2) * sc["max_dist"].astype(f32)
    logf = np.float64(f32(np.log(f32(scale))))  # mfLogScaleFactor is a float
    job = _job_of(sc)
    out = {name: np.zeros(N, f32) for name in ("u", "v", "inv_z", "ur", "radius", "dist")}
    out.update(valid=np.zeros(N, np.uint8), level=np.zeros(N, np.int32), stage=np.zeros(N, np.int32))
    for k, p in enumerate(sc["poses"]):
        m = job == k
        if not m.any():
            continue
        R, t, Ow = p["Rcw"].astype(f32), p["tcw"].astype(f32), p["Ow"].astype(f32)
        Pk = P[m]
        with np.errstate(all="ignore"):
            xc, yc, zc = _sums(R, t, Pk)
            invz = f32(1.0) / zc
            u = (fx * xc) * invz + cx
            v = (fy * yc) * invz + cy
            ur = u - f32(mbf) * invz
            PO = [(Pk[:, i] - Ow[i]).astype(np.float64) for i in range(3)]
            dist = np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]).astype(f32)
            ratio = sc["max_dist"].astype(f32)[m] / dist
            quotient = np.log(ratio.astype(np.float64)) / logf
        assert all(a.dtype == f32 for a in (xc, invz, u, v, ur, dist, lo, hi, ratio))
        stage = _stages(form, sk[m], sc["flags"][m] & 1, zc, u, v, dist, lo[m], hi[m], b)
        ok = stage < 0
        z = (lambda a: a.astype(f32)) if raw else (lambda a: np.where(ok, a, f32(0)).astype(f32))
        out["valid"][m], out["stage"][m] = ok, stage
        out["u"][m], out["v"][m], out["inv_z"][m] = z(u), z(v), z(invz)
        if form == "last":
            tk = f32(7.0 if th is None else th)
            out["ur"][m] = z(ur)
            out["radius"][m] = z(tk * SF[np.where(ok, sc["last_octave"][m], 0)])
        else:
            out["level"][m] = _level(stage, quotient, n_levels)
            out["dist"][m] = z(dist)
    keys = ("valid", "u", "v", "inv_z", "ur", "radius", "stage") if form == "last" else ("valid", "u", "v", "inv_z", "level", "dist", "stage")
    return {name: out[name] for name in keys}


def ref64(sc, form, skip=None, th=None, bounds=BOUNDS, scale=SCALE, n_levels=LEVELS, K4=(FX, FY, CX, CY), mbf=MBF):
    """src/ORBmatcher.cc:1516-1550 / :1665-1699 evaluated in float64 from the same float32 inputs: valid, level, stage and the raw
    u / v / ur / inv_z / radius / zc / dist / quotient / lo / hi for the guard bands."""
    N = len(sc["pos"])
    sk = sc["skip"] if skip is None else np.asarray(skip, np.uint8)
    P = sc["pos"].astype(np.float64)
    fx, fy, cx, cy = [float(f32(v)) for v in K4]
    b = [float(f32(v)) for v in bounds]
    lo = 0.8 * sc["min_dist"].astype(np.float64)  # GetMinDistanceInvariance / GetMaxDistanceInvariance (src/MapPoint.cc)
    hi = 1.2 * sc["max_dist"].astype(np.float64)
    job = _job_of(sc)
    out = {name: np.zeros(N, np.float64) for name in ("u", "v", "inv_z", "ur", "radius", "zc", "dist", "quotient")}
    out.update(valid=np.zeros(N, np.uint8), level=np.zeros(N, np.int32), stage=np.zeros(N, np.int32), lo=lo, hi=hi)
    for k, p in enumerate(sc["poses"]):
        m = job == k
        if not m.any():
            continue
        R, t, Ow = p["Rcw"].astype(np.float64), p["tcw"].astype(np.float64), p["Ow"].astype(np.float64)
        with np.errstate(all="ignore"):
            Pc = P[m] @ R.T + t
            zc = Pc[:, 2]
            invz = 1.0 / zc
            u = fx * Pc[:, 0] * invz + cx
            v = fy * Pc[:, 1] * invz + cy
            PO = P[m] - Ow
            dist = np.linalg.norm(PO, axis=1)
            quotient = np.log(sc["max_dist"].astype(np.float64)[m] / dist) / np.log(float(scale))  # MapPoint::PredictScale
        stage = _stages(form, sk[m], sc["flags"][m] & 1, zc, u, v, dist, lo[m], hi[m], b)
        out["valid"][m], out["stage"][m] = stage < 0, stage
        out["u"][m], out["v"][m], out["inv_z"][m], out["zc"][m], out["dist"][m], out["quotient"][m] = u, v, invz, zc, dist, quotient
        out["ur"][m] = u - float(f32(mbf)) * invz
        out["radius"][m] = float(f32(7.0 if th is None else th)) * SF[sc["last_octave"][m]].astype(np.float64)
        if form == "kf":
            out["level"][m] = _level(stage, quotient, n_levels)
    return out


def near_threshold(r64, form, bounds=BOUNDS, guard=GUARD):
    """points whose float64 values lie within a relative `guard` of one of the prologue's thresholds (zc = 0, the four bounds, and
    for the key-frame form the two distances): the only ones on which a float32 evaluation may decide otherwise."""
    with np.errstate(all="ignore"):
        u, v, zc, d = r64["u"], r64["v"], r64["zc"], r64["dist"]
        scale_u = np.maximum(np.abs(u), bounds[1])
        scale_v = np.maximum(np.abs(v), bounds[3])
        near = np.abs(zc) < guard * np.maximum(1.0, np.abs(d))
        for bx in bounds[:2]:
            near |= np.abs(u - bx) < guard * scale_u
        for by in bounds[2:]:
            near |= np.abs(v - by) < guard * scale_v
        if form == "kf":
            near |= np.abs(d - r64["lo"]) < guard * d
            near |= np.abs(d - r64["hi"]) < guard * d
    return near


def near_integer(r64, guard=GUARD):
    """points whose float64 level quotient lies within `guard` of an integer: log has no correctly rounded form."""
    with np.errstate(invalid="ignore"):
        q = r64["quotient"]
        return np.abs(q - np.round(q)) < guard


def excluded(r64, form):
    """The guard bands of the comparison with ref64; points an early stage (skip, bad) rejects are never excluded."""
    early = (r64["stage"] >= 0) & (r64["stage"] <= (0 if form == "last" else 1))
    band = near_threshold(r64, form)
    if form == "kf":
        band = band | (near_integer(r64) & (r64["stage"] < 0))
    return band & ~early


def on_threshold_by_design(sc):
    """The two points of a scene that are PUT on a threshold (u == max_x, zc == 0): inside a guard band by construction."""
    m = np.zeros(len(sc["pos"]), bool)
    if sc["offsets"][1] >= 16:
        m[[ON_BOUND, ZERO_DEPTH]] = True
    return m
