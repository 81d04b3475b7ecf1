"""orbfe_triangulate_matches* (LocalMapping::CreateNewMapPoints' per-pair loop on the device) against the float64 restatement
tests/triangulate_ref.py: pair counts at the wave and workgroup edges as K = 1 and K = 3 with monocular, stereo and mixed
keypoints, one full-size scene, and the properties of the call (determinism, multi = single, resident = host views, raw
positions, refusals, the chain behind SearchForTriangulationMulti)."""
import numpy as np
import pytest

import triangulate_ref as tr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


@pytest.fixture(scope="module")
def scenes():
    """every scene with its reference result, computed once"""
    return {id_: (sc, tr.run(sc)) for id_, sc in tr.gpu_scenes()}


def operands(amd, sc, resident=False):
    def view(f):
        v = amd.FrameView(f["x"], f["y"], f["octave"], np.zeros((f["n"], 32), np.uint8), (0.0, 640.0, 0.0, 480.0),
                          angle=np.zeros(f["n"], np.float32), u_right=f["u_right"])
        return v.upload() if resident else v

    def cam(c, f):
        return amd.KeyFrameCamera(c["Tcw"], c["Ow"], c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], depth=f["depth"],
                                  x_raw=f["x_raw"], y_raw=f["y_raw"], invfx=c["invfx"], invfy=c["invfy"])
    return (view(sc["kf1"]), cam(sc["cam1"], sc["kf1"]), [view(f) for f in sc["kf2"]],
            [cam(c, f) for c, f in zip(sc["cams2"], sc["kf2"])])


def call(amd, sc, resident=False):
    v1, c1, v2, c2 = operands(amd, sc, resident)
    return amd.triangulate_matches_multi(v1, c1, v2, c2, sc["match12"], tr.SCALE_FACTORS, tr.LEVEL_SIGMA2, tr.RATIO_FACTOR)


@pytest.mark.parametrize("id_", [id_ for id_, _ in tr.specs()])
def test_scene_equals_the_reference(amd, scenes, id_):
    sc, r = scenes[id_]
    x3d, status, created, winner = call(amd, sc, resident=(id_ == tr.FULL_ID))
    tr.compare(id_, r, status, x3d, created, winner, tr.s_tri())


def test_raw_positions_change_only_the_unprojected_points(amd, scenes):
    sc, r = scenes[tr.RAW_ID]
    plain = dict(sc, kf1=dict(sc["kf1"], x_raw=None, y_raw=None), kf2=[dict(f, x_raw=None, y_raw=None) for f in sc["kf2"]])
    xr, sr, _, _ = call(amd, sc)
    xp, sp, _, _ = call(amd, plain)
    both = (sr == tr.CREATED) & (sp == tr.CREATED)
    moved = both & (xr != xp).any(axis=-1)
    unproj = np.zeros_like(both)
    unproj[r["k"], r["i1"]] = r["unp1"] | r["unp2"]
    assert moved.any() and not (moved & ~unproj).any()
    assert np.array_equal(sr[~unproj], sp[~unproj])
    tr.compare("plain", tr.run(plain), sp, xp, (sp == tr.CREATED).sum(axis=1), None, tr.s_tri())


def test_two_calls_give_identical_bytes_and_resident_equals_host_views(amd, scenes):
    sc, _ = scenes["mixed-K3-p257"]
    a, b, c = call(amd, sc), call(amd, sc), call(amd, sc, resident=True)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_multi_equals_single_calls(amd, scenes):
    for id_ in ("mixed-K3-p257", "stereo-K3-p65"):
        sc, _ = scenes[id_]
        x3d, status, created, _ = call(amd, sc)
        v1, c1, v2, c2 = operands(amd, sc)
        for k in range(sc["K"]):
            xs, ss, ns = amd.triangulate_matches(v1, c1, v2[k], c2[k], sc["match12"][k], tr.SCALE_FACTORS, tr.LEVEL_SIGMA2,
                                                 tr.RATIO_FACTOR)
            assert xs.tobytes() == x3d[k].tobytes() and ss.tobytes() == status[k].tobytes() and ns == created[k], (id_, k)


def test_refusals_leave_the_thread_usable(amd, scenes):
    import ctypes as C
    from orb_slam2_annotate_amd import _lib
    sc, r = scenes["mixed-K1-p65"]
    v1, c1, v2, c2 = operands(amd, sc)
    args = lambda m, lv=tr.LEVEL_SIGMA2: (v1, c1, v2, c2, m, tr.SCALE_FACTORS, lv, tr.RATIO_FACTOR)

    def refused(*a):
        with pytest.raises(amd.OrbfeError) as ei:
            amd.triangulate_matches_multi(*a)
        assert ei.value.code == _lib.ERR_INVALID
    live = np.argwhere(sc["match12"] >= 0)
    bad = sc["match12"].copy(); bad[tuple(live[0])] = sc["kf2"][0]["n"]
    refused(*args(bad))  # a match outside n2
    bad = sc["match12"].copy(); bad[tuple(live[0])] = -2
    refused(*args(bad))
    refused(v1, c1, v2, c2, sc["match12"], tr.SCALE_FACTORS[:3], tr.LEVEL_SIGMA2[:3], tr.RATIO_FACTOR)  # an octave outside the table
    st = [p for p in range(len(r["k"])) if r["st1"][p]]
    assert st
    nodepth = amd.KeyFrameCamera(c1.Tcw.reshape(3, 4), c1.Ow, c1.fx, c1.fy, c1.cx, c1.cy, c1.mb, c1.mbf)
    refused(v1, nodepth, v2, c2, sc["match12"], tr.SCALE_FACTORS, tr.LEVEL_SIGMA2, tr.RATIO_FACTOR)  # a stereo keypoint, no depth
    # NULL arrays, straight at the C-ABI
    L = _lib.load()
    cc1, cc2 = c1.c, c2[0].c
    m = np.ascontiguousarray(sc["match12"][0])
    x3d, status, created = np.zeros((sc["n1"], 3), np.float32), np.zeros(sc["n1"], np.uint8), C.c_int32(0)
    good = [0, C.byref(v1.c), C.byref(cc1), C.byref(v2[0].c), C.byref(cc2), _lib.ptr(m), _lib.ptr(tr.SCALE_FACTORS),
            _lib.ptr(tr.LEVEL_SIGMA2), tr.N_LEVELS, float(tr.RATIO_FACTOR), _lib.ptr(x3d), _lib.ptr(status), C.byref(created)]
    for i in (1, 2, 3, 4, 5, 6, 7, 10, 11, 12):
        a = list(good); a[i] = None
        assert L.orbfe_triangulate_matches(*a) == _lib.ERR_INVALID, i
    assert L.orbfe_triangulate_matches(*good) == 0
    x, s, n, w = call(amd, sc)  # a later valid call on the same thread
    tr.compare("after", r, s, x, n, w, tr.s_tri())


def test_chain_behind_search_for_triangulation_multi(amd):
    """SearchForTriangulationMulti on resident frames of one rendered scene, its match12 straight into
    triangulate_matches_multi; the neighbours look 10 degrees aside so that no pair sits at the parallax threshold."""
    from orb_slam2_annotate_amd import synth
    from test_gpu_matcher import _nodes, _resident
    K = 3
    fr = synth.render_sequence(40, 1 + K, 640, 480, step=1.0)
    ext = amd.ORBextractor(1000, 1.2, 8, 20, 7).extract_batch(np.stack(fr))
    frames = [_resident(amd, k, d, _nodes(d, 13, 60)) for k, d in ext]
    F12 = [(np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32) * (0.01 + 0.002 * k)) for k in range(K)]
    eps = [(5000.0 - 100 * k, 240.0 + k) for k in range(K)]
    has = [np.zeros(f.N, np.uint8) for f in frames]
    cnt, match = amd.ORBmatcher(0.6, True).SearchForTriangulationMulti(frames[0], has[0], frames[1:], has[1:], F12, eps,
                                                                       tr.SCALE_FACTORS, tr.LEVEL_SIGMA2, False)
    assert cnt.sum() > 20
    rng = np.random.default_rng(5)
    cam1 = tr._camera(np.eye(3), np.zeros(3))
    cams2 = []
    for k in range(K):
        a = np.deg2rad(10.0 + 3 * k)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        cams2.append(tr._camera(R, np.array([1.0 + 0.3 * k, 0.05 * k, 0.2])))

    def fd(i):
        k = ext[i][0]
        return dict(n=len(k), x=k["x"].astype(np.float32), y=k["y"].astype(np.float32), octave=k["octave"].astype(np.int32),
                    u_right=None, depth=None, x_raw=None, y_raw=None)
    sc = dict(n1=frames[0].N, K=K, kind="mono", cam1=cam1, cams2=cams2, kf1=fd(0), kf2=[fd(1 + k) for k in range(K)],
              match12=np.ascontiguousarray(match, dtype=np.int32))
    cam = lambda c: amd.KeyFrameCamera(c["Tcw"], c["Ow"], c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"],
                                       invfx=c["invfx"], invfy=c["invfy"])
    x3d, status, created, winner = amd.triangulate_matches_multi(frames[0], cam(cam1), frames[1:], [cam(c) for c in cams2], match,
                                                                 tr.SCALE_FACTORS, tr.LEVEL_SIGMA2, tr.RATIO_FACTOR)
    r = tr.run(sc)
    print("chain: pairs", int(cnt.sum()), "guard", tr.guard_violations(sc, r), "statuses", np.bincount(r["pair_status"], minlength=10))
    tr.compare("chain", r, status, x3d, created, winner, tr.s_tri())
    for f in frames:
        f.close()
