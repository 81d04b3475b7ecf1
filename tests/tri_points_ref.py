"""Sequential numpy restatement of where CreateNewMapPoints' triangulated points are born (include/orbfe.h:
orbfe_triangulated_points_select), and the engineered inputs of its tests.  It consumes `status` and `x3d` -- the per-pair
outcome is tests/triangulate_ref.py's business -- and walks the reference's two loops as they stand:

  src/LocalMapping.cc:283   for every neighbour, in order
  src/ORBmatcher.cc:800-803 a keypoint of key frame 1 that has a MapPoint is not searched: with matches taken at entry, a
                            pair whose i1 was given a point by an earlier neighbour is skipped
  src/LocalMapping.cc:333   for every matched pair, ascending in idx1; the `continue`s of :338-481 are status != CREATED
  :484-492                  MapPoint(x3D, mpCurrentKeyFrame), AddObservation twice, AddMapPoint twice
  :494                      ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333) on two observations: both medians are the
                            self-distance 0, `median < BestMedian` is strict, so the first in mObservations' order wins -- in
                            the handle's rows that order is ascending mnId
  :496                      UpdateNormalAndDepth (src/MapPoint.cc:360-404): the observations' unit vectors added in row order,
                            divided by n = 2; dist from the reference key frame, which is key frame 1
"""
import numpy as np

f32 = np.float32
CREATED = 1
N_LEVELS = 8
SCALE = (f32(1.2) ** np.arange(N_LEVELS, dtype=f32)).astype(f32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _term(P, C):
    """normali / cv::norm(normali) (:381-385): -> (unit vector float32 [3], norm as float64)"""
    d = (P.astype(f32) - C.astype(f32)).astype(f32)
    dd = d.astype(np.float64)
    nrm = np.sqrt((dd[0] * dd[0] + dd[1] * dd[1]) + dd[2] * dd[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        a = f32(np.float64(1.0) / nrm)  # Mat / double: the matrix times (float)(1 / s)
        return (d * a).astype(f32), nrm


def normal_range(P, c1, c2, first_is_2, level_scale, top_scale):
    t1, n1 = _term(P, c1)
    t2, _ = _term(P, c2)
    a, b = (t2, t1) if first_is_2 else (t1, t2)
    with np.errstate(invalid="ignore"):
        normal = (((f32(0.0) + a).astype(f32) + b).astype(f32) * f32(1.0 / 2.0)).astype(f32)
    hi = f32(f32(n1) * f32(level_scale))
    lo = f32(hi / f32(top_scale))
    return normal, lo, hi


def select(match12, status, x3d, kf1_id, kf2_ids, centre1, centre2, octave1, scale):
    K = len(kf2_ids)
    octave1 = np.asarray(octave1, np.int32).reshape(-1)
    n1 = len(octave1)
    match12 = np.asarray(match12, np.int32).reshape(K, n1)
    status = np.asarray(status, np.uint8).reshape(K, n1)
    x3d = np.asarray(x3d, f32).reshape(K, n1, 3)
    centre1, centre2 = np.asarray(centre1, f32).reshape(3), np.asarray(centre2, f32).reshape(K, 3)
    has_point = np.zeros(n1, bool)  # mpCurrentKeyFrame->GetMapPoint(idx1), for the keypoints this call touches
    out = dict(created_k=[], created_i1=[], created_i2=[], pos=[], normal=[], min_dist=[], max_dist=[], desc_from=[])
    for k in range(K):
        for i1 in range(n1):
            if match12[k, i1] < 0 or has_point[i1] or status[k, i1] != CREATED:
                continue
            has_point[i1] = True
            P = x3d[k, i1]
            first_is_2 = int(kf2_ids[k]) < int(kf1_id)
            normal, lo, hi = normal_range(P, centre1, centre2[k], first_is_2, scale[octave1[i1]], scale[len(scale) - 1])
            for key, v in (("created_k", k), ("created_i1", i1), ("created_i2", int(match12[k, i1])), ("pos", P.copy()), ("normal", normal),
                           ("min_dist", lo), ("max_dist", hi), ("desc_from", 1 if first_is_2 else 0)):
                out[key].append(v)
    m = len(out["created_k"])
    res = {key: np.asarray(out[key], np.int32) for key in ("created_k", "created_i1", "created_i2")}
    res["pos"] = np.asarray(out["pos"], f32).reshape(m, 3)
    res["normal"] = np.asarray(out["normal"], f32).reshape(m, 3)
    res["min_dist"], res["max_dist"] = np.asarray(out["min_dist"], f32), np.asarray(out["max_dist"], f32)
    res["desc_from"] = np.asarray(out["desc_from"], np.uint8)
    res["n_created"] = m
    return res


# ---- engineered inputs: status / x3d by hand, one property per case -------------------------------------------------
def _case(name, n1, kf1_id, kf2_ids, pairs, seed, centre1=(0.25, -0.5, 0.125), far=False, octave=None):
    """pairs: (k, i1, i2, status).  Positions a few units in front of the centres (far: the whole scene 1e3 from the origin,
    where float rounding of 1.0 / nrm and of P - C matters)."""
    rng = np.random.default_rng(seed)
    K = len(kf2_ids)
    shift = f32([1000.0, -1000.0, 1000.0]) if far else f32([0, 0, 0])
    c1 = (f32(centre1) + shift).astype(f32)
    c2 = (c1 + rng.uniform(-1.5, 1.5, (K, 3)).astype(f32)).astype(f32).reshape(K, 3)
    match12 = np.full((K, n1), -1, np.int32)
    status = np.zeros((K, n1), np.uint8)
    x3d = np.zeros((K, n1, 3), f32)
    for k, i1, i2, st in pairs:
        match12[k, i1], status[k, i1] = i2, st
        if st == CREATED:
            x3d[k, i1] = (c1 + f32([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(2, 7)])).astype(f32)
    oc = rng.integers(0, N_LEVELS, n1).astype(np.int32) if octave is None else np.asarray(octave, np.int32)
    return dict(name=name, n1=n1, K=K, kf1_id=kf1_id, kf2_ids=np.asarray(kf2_ids, np.int64), centre1=c1, centre2=c2, match12=match12,
                status=status, x3d=x3d, octave1=oc)


def cases():
    L, R = 2, 6  # LOW_PARALLAX, REPROJ_1: pairs that left the loop
    dense = [(k, i1, (i1 * 7 + k) % 90, CREATED if (i1 + k) % 3 else L) for k in range(3) for i1 in range(80) if (i1 + 2 * k) % 4]
    return [
        _case("no_neighbour", 5, 4, [], [], 1),
        _case("none_created", 6, 4, [9, 2], [(0, 1, 3, L), (1, 1, 2, R), (1, 4, 0, L)], 2),
        _case("one_pair", 4, 4, [9], [(0, 2, 5, CREATED)], 3),
        # i1 = 3 is CREATED by neighbours 0 and 2: the lower wins, keypoint 8 of neighbour 2 gets nothing
        _case("contested", 6, 10, [11, 12, 13], [(0, 3, 7, CREATED), (2, 3, 8, CREATED), (1, 3, 1, L), (2, 5, 2, CREATED), (0, 0, 0, CREATED)], 4),
        # the loser of an earlier neighbour does not hide a later one: neighbour 0 fails i1 = 2, neighbour 1 makes it
        _case("later_neighbour_wins", 5, 10, [3, 30], [(0, 2, 1, R), (1, 2, 4, CREATED), (1, 0, 0, CREATED)], 5),
        _case("empty_middle", 8, 10, [11, 12, 13], [(0, 1, 1, CREATED), (0, 6, 2, CREATED), (1, 2, 3, L), (2, 0, 4, CREATED), (2, 7, 5, CREATED)], 6),
        # mnIds below and above key frame 1's: desc_from and the order of the normal's sum flip
        _case("ids_both_sides", 6, 10, [3, 30], [(0, 0, 2, CREATED), (1, 1, 3, CREATED), (0, 4, 0, CREATED), (1, 5, 1, CREATED)], 7),
        _case("far_from_origin", 12, 10, [3, 30], [(k, i1, i1, CREATED) for k in range(2) for i1 in range(k, 12, 2)], 8, far=True),
        _case("octave_ends", 4, 10, [3, 30], [(0, 0, 0, CREATED), (0, 1, 1, CREATED), (1, 2, 2, CREATED), (1, 3, 3, CREATED)], 9,
              octave=[0, N_LEVELS - 1, N_LEVELS - 1, 0]),
        _case("dense", 80, 10, [3, 30, 11], dense, 10),
    ]
