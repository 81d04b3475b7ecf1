"""Sequential numpy restatement of where stereo / RGB-D map points are born, written from the reference's lines and
independent of csrc/stereopoints_host.h: Tracking::StereoInitialization (src/Tracking.cc:563-578, mode ALL), the
depth-sorted loop of Tracking::CreateNewKeyFrame (:1182-1234, KEYFRAME) and of Tracking::UpdateLastFrame (:899-949,
TEMPORAL), Frame::UnprojectStereo (src/Frame.cc:713-727), MapPoint::UpdateNormalAndDepth for a row of one entry
(src/MapPoint.cc:360-404; the Frame constructor :53-64 is the same expression) and the counts of
Tracking::NeedNewKeyFrame (:1100-1114).  np.float32 operations one at a time; np.float64 where include/orbfe.h says so.

Also the engineered frames both test files run (frames()): each is built so that the named branch alone decides the
outcome."""
import numpy as np

ALL, KEYFRAME, TEMPORAL = 0, 1, 2
MODES = (ALL, KEYFRAME, TEMPORAL)
F32, F64 = np.float32, np.float64
N_LEVELS = 8
SCALE = np.array([F32(1.2) ** k for k in range(N_LEVELS)], dtype=np.float32)
K4 = (F32(458.654), F32(457.296), F32(367.215), F32(248.375))  # fx fy cx cy
WIDTH, HEIGHT = 752.0, 480.0


def select(x, y, octave, depth, occupied, stale, pose, th_depth, mode, scale, centre):
    """-> dict of created_idx, pos, normal, min_dist, max_dist, cleared, n_created, n_walked.  pose: a CameraPoseC (Rcw, Ow,
    fx, fy, cx, cy are read)."""
    n = len(depth)
    th = F32(th_depth)
    cand = [(F32(depth[i]), i) for i in range(n) if depth[i] > 0]  # (:1184-1191); NaN > 0 is False
    if mode != ALL:
        cand = sorted(cand)  # pair<float, int> (:1195)
    Rcw = np.array(list(pose.Rcw), dtype=np.float32).reshape(3, 3)
    Rwc = Rcw.T
    Ow = np.array(list(pose.Ow), dtype=np.float32)
    fx, fy, cx, cy = F32(pose.fx), F32(pose.fy), F32(pose.cx), F32(pose.cy)
    invfx, invfy = F32(1.0) / fx, F32(1.0) / fy
    C = np.asarray(centre, dtype=np.float32)
    top = F32(scale[len(scale) - 1])
    out = dict(created_idx=[], pos=[], normal=[], min_dist=[], max_dist=[], cleared=np.zeros(n, np.uint8))
    n_points = 0
    with np.errstate(all="ignore"):
        for z, i in cand:
            create = True
            if mode != ALL and occupied is not None and occupied[i]:  # pMP with Observations() >= 1 (:1204-1211)
                create = False
            if create:
                if mode == KEYFRAME and stale is not None and stale[i]:
                    out["cleared"][i] = 1  # mvpMapPoints[i] = NULL (:1210)
                u, v = F32(x[i]), F32(y[i])
                xc = ((u - cx) * z) * invfx
                yc = ((v - cy) * z) * invfy
                P = np.zeros(3, np.float32)
                for r in range(3):  # mRwc * x3Dc + mOw: one gemm with beta = 1, double accumulator
                    s = F64(Rwc[r, 0]) * F64(xc)
                    s = s + F64(Rwc[r, 1]) * F64(yc)
                    s = s + F64(Rwc[r, 2]) * F64(z)
                    s = s + F64(Ow[r])
                    P[r] = F32(s)
                d = [P[k] - C[k] for k in range(3)]
                nrm = np.sqrt((F64(d[0]) * F64(d[0]) + F64(d[1]) * F64(d[1])) + F64(d[2]) * F64(d[2]))
                a = F32(F64(1.0) / nrm)
                one = F32(F64(1.0) / F64(1))
                normal = [(F32(0.0) + d[k] * a) * one for k in range(3)]
                hi = F32(nrm) * F32(scale[octave[i]])
                lo = hi / top
                out["created_idx"].append(i)
                out["pos"].append(P)
                out["normal"].append(np.array(normal, np.float32))
                out["min_dist"].append(lo)
                out["max_dist"].append(hi)
            n_points += 1  # in either branch (:1224, :1228)
            if mode != ALL and z > th and n_points > 100:  # (:1231)
                break
    m = len(out["created_idx"])
    out["created_idx"] = np.array(out["created_idx"], np.int32)
    out["pos"] = np.array(out["pos"], np.float32).reshape(m, 3)
    out["normal"] = np.array(out["normal"], np.float32).reshape(m, 3)
    out["min_dist"] = np.array(out["min_dist"], np.float32)
    out["max_dist"] = np.array(out["max_dist"], np.float32)
    out["n_created"], out["n_walked"] = m, n_points
    return out


def count_close(depth, has_point, outlier, th_depth):
    th = F32(th_depth)
    tracked = non_tracked = 0
    for i in range(len(depth)):
        z = F32(depth[i])
        if z > 0 and z < th:  # (:1106)
            if has_point[i] and not outlier[i]:
                tracked += 1
            else:
                non_tracked += 1
    return tracked, non_tracked


def same_bits(a, b, nan_by_place=True):
    """Equal shapes and equal bits.  nan_by_place: a NaN equals a NaN -- IEEE 754 leaves sign and payload of a NaN that an
    operation produces to the implementation (x86 and gfx950 differ), so between host and device only its place is
    compared.  Two results of one CPU are compared with nan_by_place=False: every bit."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    if not nan_by_place:
        return bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


# ---- poses ----

def rotation(seed):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, a, b, c = q
    return np.array([[1 - 2 * (b * b + c * c), 2 * (a * b - c * w), 2 * (a * c + b * w)],
                     [2 * (a * b + c * w), 1 - 2 * (a * a + c * c), 2 * (b * c - a * w)],
                     [2 * (a * c - b * w), 2 * (b * c + a * w), 1 - 2 * (a * a + b * b)]], dtype=np.float32)


def make_pose(seed=3, t=(0.3, -0.2, 0.5)):
    import orb_slam2_annotate_amd as amd
    return amd.camera_pose(rotation(seed), np.array(t, np.float32), K4, 40.0, (0.0, WIDTH, 0.0, HEIGHT), 1.2, N_LEVELS)


# ---- engineered frames ----

def _frame(name, depth, th, occupied=None, stale=None, seed=0, pose_t=(0.3, -0.2, 0.5), rgbd=()):
    depth = np.asarray(depth, dtype=np.float32)
    n = len(depth)
    rng = np.random.default_rng(1000 + seed)
    x = rng.uniform(5.0, WIDTH - 5.0, n).astype(np.float32)
    y = rng.uniform(5.0, HEIGHT - 5.0, n).astype(np.float32)
    octave = rng.integers(0, N_LEVELS, n).astype(np.int32)
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    with np.errstate(all="ignore"):
        u_right = np.where(depth > 0, x - np.float32(40.0) / depth, np.float32(-1.0)).astype(np.float32)
    for i in rgbd:  # an RGB-D "u - mbf / d" left of the image: mvuRight < 0 at a positive depth
        u_right[i] = np.float32(-3.5)
    occ = np.zeros(n, np.uint8) if occupied is None else np.asarray(occupied, np.uint8)
    st = np.zeros(n, np.uint8) if stale is None else np.asarray(stale, np.uint8)
    assert not (occ & st).any()
    return dict(name=name, n=n, x=x, y=y, octave=octave, desc=desc, depth=depth, u_right=u_right, occupied=occ, stale=st,
                th=np.float32(th), pose_t=pose_t, seed=seed)


def _shuffled(values, seed):
    v = np.asarray(values, dtype=np.float32)
    return v[np.random.default_rng(seed).permutation(len(v))]


def frames():
    TH = 10.0
    out = []
    rng = np.random.default_rng(7)
    for n in (0, 1, 63, 64, 65, 130):  # sizes; about a quarter of the depths are no candidates
        d = rng.uniform(0.5, 30.0, n)
        d[rng.random(n) < 0.25] = -1.0
        occ = (rng.random(n) < 0.3).astype(np.uint8)
        st = ((rng.random(n) < 0.2) & (occ == 0)).astype(np.uint8)
        out.append(_frame(f"n{n}", d, TH, occ, st, seed=n))
    # equal z at several i: the order is by i
    out.append(_frame("ties", [2.0, 1.0, 2.0, 1.0, 3.0, 2.0, 1.0, 3.0, 2.0, 1.0, 2.0, 3.0], TH, seed=20))
    # exactly 100 candidates, all beyond th: nPoints never exceeds 100, no early stop
    out.append(_frame("exact100_far", _shuffled(np.linspace(20.0, 40.0, 100), 21), TH, seed=21))
    # 101 candidates, the 101st beyond th: it is handled and the walk stops at j = 100
    out.append(_frame("stop101", _shuffled(list(np.linspace(1.0, 9.0, 100)) + [15.0], 22), TH, seed=22))
    # the same with two more far ones behind it, which the stop leaves out
    out.append(_frame("stop101_tail", _shuffled(list(np.linspace(1.0, 9.0, 100)) + [15.0, 16.0, 17.0], 23), TH, seed=23))
    # the 101st equal to th: z > th is false, the walk goes on to the 102nd
    out.append(_frame("eq_th", _shuffled(list(np.linspace(1.0, 9.0, 100)) + [TH, 16.0, 17.0], 24), TH, seed=24))
    # more than 100 close points, then far ones: stops at the first far one
    out.append(_frame("close_then_far", _shuffled(list(np.linspace(1.0, 9.0, 105)) + [15.0, 16.0, 17.0, 18.0, 19.0], 25), TH, seed=25))
    # occupied entries inside and outside the walked prefix; stale entries likewise
    d = np.array(list(np.linspace(1.0, 9.0, 105)) + [15.0, 16.0, 17.0, 18.0, 19.0], np.float32)
    occ = np.zeros(110, np.uint8)
    occ[[0, 7, 50, 104, 105, 107, 109]] = 1
    st = np.zeros(110, np.uint8)
    st[[1, 8, 51, 106, 108]] = 1
    perm = np.random.default_rng(26).permutation(110)
    out.append(_frame("occupied_stale", d[perm], TH, occ[perm], st[perm], seed=26))
    # depths 0, -1, NaN, +inf: +inf is a candidate and sorts last; here it is occupied, so no point is made of it
    d = np.array([0.0, -1.0, np.nan, np.inf, 2.0, -0.0, 1.0, np.nan, 3.0, -np.inf], np.float32)
    occ = np.zeros(10, np.uint8)
    occ[3] = 1
    out.append(_frame("special_depths", d, TH, occ, seed=27))
    # +inf created: its position is not finite
    out.append(_frame("inf_created", d, TH, seed=28))
    # every candidate occupied: mode ALL must not read the mask
    d = rng.uniform(0.5, 30.0, 40)
    out.append(_frame("all_occupied", d, TH, np.ones(40, np.uint8), seed=29))
    # an RGB-D-like frame: mvuRight < 0 at a positive depth
    d = rng.uniform(0.5, 8.0, 30)
    out.append(_frame("rgbd_negative_uright", d, TH, seed=30, rgbd=(2, 11, 29)))
    # a pose far from the origin: the double accumulation shows in the last place
    d = rng.uniform(0.5, 30.0, 70)
    out.append(_frame("far_pose", d, TH, (rng.random(70) < 0.3).astype(np.uint8), seed=31, pose_t=(1e3, -1e3, 1e3)))
    return out


def frame_pose(f):
    return make_pose(3 + f["seed"], f["pose_t"])
