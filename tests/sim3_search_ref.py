"""Reference of the prologue of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1298-1340 for the leg KF1 -> KF2, :1379-1420 for
KF2 -> KF1) for the device map-point table: many legs over concatenated slot lists, a leg being one direction of one candidate.

* spec32: the arithmetic include/orbfe.h states for orbfe_project_sim3, operation by operation in numpy float32 (sums left to
  right, the norm accumulated in float64 as cv::norm does) with the stage that rejects each point -- what the kernel must equal
  bit for bit;
* ref64: the same geometry entirely in float64 -- the independent statement of the reference's lines, against which both the
  spec and the kernel may differ only next to a threshold (excluded: the GUARD bands, as in track_ref.py);
* scene(): KF1 with n1 keypoints and K = len(n2s) candidates with n2s[k] keypoints on the KITTI camera of frustum_ref.py; the
  legs 2k (KF1 -> KF2_k) and 2k + 1 (KF2_k -> KF1) of every candidate; the key frames' keypoints.  Leg 0 carries the engineered
  points (ENGINEERED, scenes whose KF1 holds at least 16 keypoints); candidate 0 is a pure rotation and scale about KF1's
  centre (t12 = t21 = 0), so that a point at KF1's centre has c2 == 0 exactly.
"""
import numpy as np

from frustum_ref import BOUNDS, CX, CY, FX, FY, LEVELS, SCALE, rodrigues

GUARD = 1e-4
STAGES = ("noslot", "skip", "bad", "depth", "image", "distance")
SF = (np.float32(SCALE) ** np.arange(LEVELS)).astype(np.float32)  # mvScaleFactors
# positions in KF1's list of the engineered points: 0..7 one valid point per level of leg 0;
ON_MAX = 8        # u == max_x exactly: rejected, the bound is strict (KeyFrame::IsInImage)
ON_MIN = 9        # u == min_x exactly: accepted
BEHIND = 10       # c2.z < 0, projecting inside the image
ZERO = 11         # c2 == 0: invz = inf, u = NaN -- rejected at the image test
BAD = 12          # ORBFE_MP_BAD
NOSLOT = 13       # slot -1
SKIPPED = 14      # skip set on a point that would otherwise pass
ENGINEERED = 15

f32 = np.float32


def _sums(R, t, X, Y, Z):
    return [((R[r, 0] * X + R[r, 1] * Y) + R[r, 2] * Z) + t[r] for r in range(3)]


def _project32(leg, P):
    """spec32's c2, u, v of float32 points [n, 3]"""
    with np.errstate(all="ignore"):
        c1 = _sums(leg["Rw"], leg["tw"], P[:, 0], P[:, 1], P[:, 2])
        c2 = _sums(leg["sR"], leg["t"], *c1)
        invz = f32(1.0) / c2[2]
        x, y = c2[0] * invz, c2[1] * invz
        u, v = f32(FX) * x + f32(CX), f32(FY) * y + f32(CY)
    assert all(a.dtype == f32 for a in c1 + c2 + [invz, x, y, u, v])
    return c2, u, v


def _world(leg, c2):
    """float32 world points whose float64 target-camera coordinates are c2 [n, 3]"""
    Rw, tw, sR, t = [leg[k].astype(np.float64) for k in ("Rw", "tw", "sR", "t")]
    c1 = np.linalg.solve(sR, (c2 - t).T).T
    return ((c1 - tw) @ Rw).astype(f32)


def _on_bound(leg, target, depth):
    """A float32 point in front of the leg's target whose spec32 u equals `target` exactly: start at the real solution on the
    optical row and try the float32 neighbours of X (256 either side), for Z and its next float32 neighbours in turn."""
    c2 = np.array([[(float(target) - float(f32(CX))) / float(f32(FX)) * depth, 0.0, depth]])
    P0 = _world(leg, c2)[0]
    steps = np.arange(-256, 257, dtype=np.int32)
    for _ in range(64):
        P = np.repeat(P0[None, :], len(steps), axis=0)
        P[:, 0] = (P[:, 0].view(np.int32) + steps * (1 if P0[0] > 0 else -1)).view(f32)  # (neighbouring floats of one sign)
        u = _project32(leg, P)[1]
        hit = np.flatnonzero(u == f32(target))
        if len(hit):
            return P[hit[len(hit) // 2]].copy()
        P0[2] = np.nextafter(P0[2], f32(np.inf))
    raise AssertionError("no float32 point projects onto the image bound")


def make_leg(Rw, tw, sR, t):
    return dict(Rw=np.asarray(Rw, f32).reshape(3, 3), tw=np.asarray(tw, f32).reshape(3), sR=np.asarray(sR, f32).reshape(3, 3),
                t=np.asarray(t, f32).reshape(3))


def scene(seed, n1, n2s):
    """dict: legs (2K dicts of Rw [3,3], tw [3], sR [3,3], t [3], float32; leg 2k = KF1 -> KF2_k, 2k + 1 = KF2_k -> KF1), sim3 (K
    tuples s12, R12, t12 and the poses, for loop_closing.sim3_legs), the table (pos / normal [N,3], min_dist / max_dist, flags
    (1 = bad), desc [N,32]: table row = slot), slot1 [n1] and slot2 (K lists) with -1 = no map point, skip1 [K, n1] / skip2 (K
    lists) = vbAlreadyMatched, and kf1 / kf2 (K): the key frames' keypoints (x, y, octave, desc; keypoint i holds slot*[i])."""
    rng = np.random.default_rng(9300 + seed)
    n2s = [int(c) for c in n2s]
    K = len(n2s)
    R1 = rodrigues(rng.normal(0, 0.1, 3)).astype(f32)
    t1 = rng.normal(0, 0.5, 3).astype(f32)
    if n1 >= 16:  # KF1's translation is MADE from the ZERO point, so that the three sums of c1 cancel exactly
        Pz = np.array([0.3125, -0.21875, 0.53125], f32)
        t1 = np.array([-((R1[r, 0] * Pz[0] + R1[r, 1] * Pz[1]) + R1[r, 2] * Pz[2]) for r in range(3)], f32)
    legs, sim3 = [], []
    for k in range(K):
        s12 = f32(rng.uniform(0.9, 1.1))
        R12 = rodrigues(rng.normal(0, 0.06, 3)).astype(f32)
        t12 = np.zeros(3, f32) if k == 0 else rng.normal(0, 0.4, 3).astype(f32)
        # (the composition of loop_closing.sim3_legs; the key frame KF2_k is where the Sim3 says it is, up to rounding)
        sR12 = (s12 * R12).astype(f32)
        sR21 = ((1.0 / np.float64(s12)) * R12.T.astype(np.float64)).astype(f32)
        p = (sR21 * t12[None, :]).astype(f32)
        t21 = -((p[:, 0] + p[:, 1]).astype(f32) + p[:, 2]).astype(f32)
        R2 = (R12.T.astype(np.float64) @ R1.astype(np.float64)).astype(f32)
        t2 = (sR21.astype(np.float64) @ t1.astype(np.float64) + t21).astype(f32)
        legs += [make_leg(R1, t1, sR21, t21), make_leg(R2, t2, sR12, t12)]
        sim3.append(dict(s12=s12, R12=R12, t12=t12, R1w=R1, t1w=t1, R2w=R2, t2w=t2))
    counts = [n1] + n2s
    N = int(sum(counts))
    owner = np.repeat(np.arange(K + 1), counts)  # 0: a point of KF1's list, k + 1: of KF2_k's
    cam = np.stack([rng.uniform(-12, 12, N), rng.uniform(-6, 6, N), rng.uniform(-4, 30, N)], axis=1)
    pos = np.zeros((N, 3), f32)
    dist = np.ones(N)
    for o in range(K + 1):
        m = owner == o
        if not m.any() or K == 0:
            continue
        leg = legs[0] if o == 0 else legs[2 * (o - 1) + 1]
        pos[m] = _world(leg, cam[m])
        dist[m] = np.linalg.norm(cam[m], axis=1)
    normal = rng.normal(0, 1, (N, 3))
    normal = (normal / np.linalg.norm(normal, axis=1, keepdims=True)).astype(f32)
    max_dist = (dist * rng.uniform(0.7, 4.0, N)).astype(f32)
    min_dist = (max_dist.astype(np.float64) / 1.2 ** 7 * rng.uniform(0.5, 1.5, N)).astype(f32)
    flags = (rng.random(N) < 0.03).astype(np.uint8) | np.uint8(2)
    desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    slot = np.arange(N, dtype=np.int32)
    slot[rng.random(N) < 0.1] = -1
    skip = (rng.random(N) < 0.05).astype(np.uint8)
    if n1 >= 16 and K > 0:
        L0 = legs[0]
        for lv in range(LEVELS):
            pos[lv] = _world(L0, np.array([[-3.0 + 0.8 * lv, 0.5 - 0.1 * lv, 6.0 + lv]]))[0]
        pos[ON_MAX] = _on_bound(L0, BOUNDS[1], 9.0)
        pos[ON_MIN] = _on_bound(L0, BOUNDS[0], 9.0)
        pos[BEHIND] = _world(L0, np.array([[0.4, -0.2, -7.0]]))[0]
        pos[ZERO] = Pz
        pos[BAD] = _world(L0, np.array([[1.0, 0.3, 8.0]]))[0]
        pos[NOSLOT] = _world(L0, np.array([[1.5, 0.3, 8.0]]))[0]
        pos[SKIPPED] = _world(L0, np.array([[-1.0, 0.2, 7.0]]))[0]
        c2 = _project32(L0, pos[:ENGINEERED])[0]
        for i in range(ENGINEERED):
            d = max(float(np.sqrt(sum(float(c[i]) ** 2 for c in c2))), 1.0)
            ratio = 1.2 ** ((i if i < LEVELS else 3) - 0.5)  # max_dist / dist -> the level exactly
            max_dist[i] = f32(d * ratio)
            min_dist[i] = f32(d * ratio / 1.2 ** 7)
        flags[:ENGINEERED] = 2
        slot[:ENGINEERED] = np.arange(ENGINEERED)
        skip[:ENGINEERED] = 0
        flags[BAD] = 3
        slot[NOSLOT] = -1
        skip[SKIPPED] = 1
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    skip1 = np.zeros((K, n1), np.uint8)
    for k in range(K):
        skip1[k] = skip[:n1] if k == 0 else np.roll(skip[:n1], 3 * k)
        if n1 >= 16:
            skip1[k, :ENGINEERED] = skip[:ENGINEERED]
    sc = dict(legs=legs, sim3=sim3, pos=pos, normal=normal, min_dist=min_dist, max_dist=max_dist, flags=flags, desc=desc,
              slot1=slot[:n1].copy(), slot2=[slot[off[k + 1]:off[k + 2]].copy() for k in range(K)], skip1=skip1,
              skip2=[skip[off[k + 1]:off[k + 2]].copy() for k in range(K)], n1=int(n1), n2s=n2s)
    sc["kf1"], sc["kf2"] = key_frames(rng, sc)
    return sc


def leg_lists(sc):
    """(slots, skips) per leg, in leg order"""
    slots, skips = [], []
    for k in range(len(sc["n2s"])):
        slots += [sc["slot1"], sc["slot2"][k]]
        skips += [sc["skip1"][k], sc["skip2"][k]]
    return slots, skips


def key_frames(rng, sc):
    """The keypoints of KF1 and of every KF2_k; keypoint i of a key frame holds the map point slot*[i].  A search needs a keypoint
    of the TARGET near a projection: most keypoints of KF2_k sit on the projection of a point of KF1's list, at the predicted
    octave or a neighbour, with that point's descriptor and a few flipped bits (a fifth of them too many for TH_HIGH), and
    KF1's keypoints likewise for the points of KF2_0's list; the rest is clutter.  The second loop makes mutual pairs."""
    K = len(sc["n2s"])
    none = None

    def frame(m, leg, slots):
        x = rng.uniform(BOUNDS[0], BOUNDS[1] - 1, m).astype(f32)
        y = rng.uniform(BOUNDS[2], BOUNDS[3] - 1, m).astype(f32)
        octave = rng.integers(0, LEVELS, m).astype(np.int32)
        desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        if leg is not None and m and len(slots):
            pr = spec32_leg(sc, leg, slots, none)
            ok = np.flatnonzero(pr["valid"] != 0)
            src = rng.permutation(ok)[: min(len(ok), (3 * m) // 4)]
            j = rng.permutation(m)[: len(src)]
            x[j] = (pr["u"][src] + rng.normal(0, 0.7, len(src))).astype(f32)
            y[j] = (pr["v"][src] + rng.normal(0, 0.7, len(src))).astype(f32)
            octave[j] = np.clip(pr["level"][src] + rng.integers(-1, 2, len(src)), 0, LEVELS - 1)
            flips = rng.integers(0, 256, (len(src), 32), dtype=np.uint8) & rng.integers(0, 256, (len(src), 32), dtype=np.uint8) & \
                rng.integers(0, 256, (len(src), 32), dtype=np.uint8)
            heavy = rng.random(len(src)) < 0.2  # a fifth of them too far for TH_HIGH
            desc[j] = sc["desc"][slots[src]] ^ np.where(heavy[:, None], rng.integers(0, 256, (len(src), 32), dtype=np.uint8), flips)
        keep = (x >= BOUNDS[0]) & (x < BOUNDS[1]) & (y >= BOUNDS[2]) & (y < BOUNDS[3])
        x, y = np.where(keep, x, f32(5.0)), np.where(keep, y, f32(5.0))  # (a frame holds no keypoint outside its bounds)
        return dict(x=x, y=y, octave=octave, desc=desc)

    kf2 = [frame(sc["n2s"][k], sc["legs"][2 * k], sc["slot1"]) for k in range(K)]
    kf1 = frame(sc["n1"], sc["legs"][1] if K else None, sc["slot2"][0] if K else np.zeros(0, np.int32))
    # mutual pairs: where KF2_k's keypoint j was placed for KF1's point i1, give keypoint j the map point whose projection into
    # KF1 lies at KF1's keypoint i1 -- cheaply: the same map point, seen by both key frames
    for k in range(K):
        pr = spec32_leg(sc, sc["legs"][2 * k], sc["slot1"], none)
        ok = np.flatnonzero(pr["valid"] != 0)
        for i1 in ok[::2]:
            d = np.abs(kf2[k]["x"] - pr["u"][i1]) + np.abs(kf2[k]["y"] - pr["v"][i1])
            if len(d) == 0 or d.min() > 3.0:
                continue
            j = int(np.argmin(d))
            if sc["slot2"][k][j] < 0 or (len(sc["pos"]) and sc["slot1"][i1] < 0):
                continue
            s = sc["slot2"][k][j]
            if s < ENGINEERED + 1 and sc["n1"] >= 16:
                continue
            # the candidate's own map point becomes a twin of KF1's: same place and ranges, its own descriptor near KF1's keypoint's
            s1 = sc["slot1"][i1]
            for name in ("pos", "normal", "min_dist", "max_dist"):
                sc[name][s] = sc[name][s1]
            sc["flags"][s] = 2
            back = spec32_leg(sc, sc["legs"][2 * k + 1], np.array([s], np.int32), none)
            if back["valid"][0]:
                kf1["x"][i1], kf1["y"][i1] = back["u"][0], back["v"][0]
                kf1["octave"][i1] = back["level"][0]
                kf1["desc"][i1] = sc["desc"][s]
    return kf1, kf2


def _stage_of(tests, n):
    stage = np.full(n, -1, np.int32)
    for k in range(len(tests) - 1, -1, -1):
        stage[tests[k]] = k
    return stage


def _level(stage, quotient, n_levels):
    with np.errstate(invalid="ignore"):
        c = np.ceil(quotient)
        level = np.where(c > 0, np.minimum(c, n_levels - 1), 0)
    return np.nan_to_num(np.where(stage < 0, level, 0)).astype(np.int32)


def _gather(sc, slots):
    s = np.where(slots >= 0, slots, 0)
    return sc["pos"][s].astype(f32), sc["min_dist"][s].astype(f32), sc["max_dist"][s].astype(f32), (sc["flags"][s] & 1)


def spec32_leg(sc, leg, slots, skip, bounds=BOUNDS, scale=SCALE, n_levels=LEVELS, raw=False):
    """include/orbfe.h's arithmetic for one leg: valid, u, v, level, dist, stage (index into STAGES, -1 = searched).  The
    fields are 0 where valid is, as the library writes them (raw: as computed)."""
    slots = np.asarray(slots, np.int32)
    n = len(slots)
    sk = np.zeros(n, np.uint8) if skip is None else np.asarray(skip, np.uint8)
    P, mn, mx, bad = _gather(sc, slots) if n else (np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros(0, f32), np.zeros(0, np.uint8))
    b = [f32(v) for v in bounds]
    logf = np.float64(f32(np.log(f32(scale))))  # mfLogScaleFactor is a float
    c2, u, v = _project32(leg, P)
    with np.errstate(all="ignore"):
        d = [c.astype(np.float64) for c in c2]
        dist = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(f32)
        lo, hi = f32(0.8) * mn, f32(1.2) * mx
        ratio = mx / dist
        quotient = np.log(ratio.astype(np.float64)) / logf
        in_image = (u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])
        tests = [slots < 0, sk != 0, bad != 0, c2[2] < 0, ~in_image, (dist < lo) | (dist > hi)]
    assert all(a.dtype == f32 for a in (dist, lo, hi, ratio))
    stage = _stage_of(tests, n)
    ok = stage < 0
    z = (lambda a: a.astype(f32)) if raw else (lambda a: np.where(ok, a, f32(0)).astype(f32))
    return dict(valid=ok.astype(np.uint8), u=z(u), v=z(v), level=_level(stage, quotient, n_levels), dist=z(dist), stage=stage)


def ref64_leg(sc, leg, slots, skip, bounds=BOUNDS, scale=SCALE, n_levels=LEVELS):
    """src/ORBmatcher.cc:1300-1337 evaluated in float64 from the same float32 inputs: valid, level, stage and the raw u / v / z /
    dist / quotient / lo / hi for the guard bands."""
    slots = np.asarray(slots, np.int32)
    n = len(slots)
    sk = np.zeros(n, np.uint8) if skip is None else np.asarray(skip, np.uint8)
    P, mn, mx, bad = _gather(sc, slots) if n else (np.zeros((0, 3), f32), np.zeros(0, f32), np.zeros(0, f32), np.zeros(0, np.uint8))
    Rw, tw, sR, t = [leg[k].astype(np.float64) for k in ("Rw", "tw", "sR", "t")]
    b = [float(f32(v)) for v in bounds]
    with np.errstate(all="ignore"):
        c2 = (P.astype(np.float64) @ Rw.T + tw) @ sR.T + t
        z = c2[:, 2]
        u = float(f32(FX)) * (c2[:, 0] / z) + float(f32(CX))
        v = float(f32(FY)) * (c2[:, 1] / z) + float(f32(CY))
        dist = np.linalg.norm(c2, axis=1)
        lo, hi = 0.8 * mn.astype(np.float64), 1.2 * mx.astype(np.float64)
        quotient = np.log(mx.astype(np.float64) / dist) / np.log(float(scale))  # MapPoint::PredictScale
        in_image = (u >= b[0]) & (u < b[1]) & (v >= b[2]) & (v < b[3])
        tests = [slots < 0, sk != 0, bad != 0, z < 0, ~in_image, (dist < lo) | (dist > hi)]
    stage = _stage_of(tests, n)
    return dict(valid=(stage < 0).astype(np.uint8), level=_level(stage, quotient, n_levels), stage=stage, u=u, v=v, z=z, dist=dist,
                quotient=quotient, lo=lo, hi=hi)


def _cat(parts):
    return {name: np.concatenate([p[name] for p in parts]) for name in parts[0]} if parts else {}


def spec32(sc, skips="scene", **kw):
    """spec32_leg over every leg of the scene, concatenated in leg order (skips: "scene" = the scene's masks, None = none)"""
    slots, sk = leg_lists(sc)
    return _cat([spec32_leg(sc, sc["legs"][l], slots[l], sk[l] if skips == "scene" else None, **kw) for l in range(len(slots))])


def ref64(sc, skips="scene", **kw):
    slots, sk = leg_lists(sc)
    return _cat([ref64_leg(sc, sc["legs"][l], slots[l], sk[l] if skips == "scene" else None, **kw) for l in range(len(slots))])


def excluded(r64, bounds=BOUNDS, guard=GUARD):
    """The guard bands of the comparison with ref64: points whose float64 values lie within a relative `guard` of a threshold
    (z = 0, the four bounds, the two distances) and accepted points whose level quotient lies within `guard` of an integer (log
    has no correctly rounded form).  Points an early stage (no slot, skip, bad) rejects are never excluded."""
    with np.errstate(all="ignore"):
        u, v, z, d = r64["u"], r64["v"], r64["z"], r64["dist"]
        near = np.abs(z) < guard * np.maximum(1.0, np.abs(d))
        for bx in bounds[:2]:
            near |= np.abs(u - bx) < guard * np.maximum(np.abs(u), bounds[1])
        for by in bounds[2:]:
            near |= np.abs(v - by) < guard * np.maximum(np.abs(v), bounds[3])
        near |= np.abs(d - r64["lo"]) < guard * d
        near |= np.abs(d - r64["hi"]) < guard * d
        q = r64["quotient"]
        near |= (np.abs(q - np.round(q)) < guard) & (r64["stage"] < 0)
    early = (r64["stage"] >= 0) & (r64["stage"] <= 2)
    return near & ~early


def on_threshold_by_design(sc):
    """The three points of a scene that are PUT on a threshold (u == max_x, u == min_x, c2 == 0), over the concatenated legs:
    inside a guard band by construction."""
    slots, _ = leg_lists(sc)
    m = np.zeros(sum(len(s) for s in slots), bool)
    if sc["n1"] >= 16 and slots:
        m[[ON_MAX, ON_MIN, ZERO]] = True
    return m
