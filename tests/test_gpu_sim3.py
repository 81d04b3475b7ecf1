"""orbfe_sim3_ransac* (every RANSAC hypothesis of Sim3Solver in one launch) and the Sim3Solver class against the float64
restatement tests/sim3_ref.py: pair counts at the mask-word, ballot and wave-trip edges times hypothesis counts around the
four-waves-per-workgroup edge, K = 3 with an empty candidate, fix_scale both ways, the engineered hypotheses, and the
properties of the call (determinism, multi = single, refusals, the class's replay, the chain into SearchBySim3)."""
import ctypes as C

import numpy as np
import pytest

import sim3_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


@pytest.fixture(scope="module")
def scenes():
    """every scene with its reference result, computed once"""
    return {id_: (sc, sr.run(sc)) for id_, sc in sr.gpu_scenes()}


def call(amd, sc):
    o = sr.operands(sc)
    return amd.sim3_ransac_multi(o["pair_off"], o["x1"], o["x2"], o["max1"], o["max2"], o["cam1"], o["cam2"], o["fix_scale"],
                                 o["hyp_off"], o["triples"])


@pytest.mark.parametrize("id_", [id_ for id_, _ in sr.specs()])
def test_scene_equals_the_reference(amd, scenes, id_):
    sc, r = scenes[id_]
    n_inl, status, sim3, words, word_off = call(amd, sc)
    ill, guard, differ = sr.compare(id_, sc, r, n_inl, status, sim3, words, word_off, sr.s_sim3())
    print(id_, "not compared (ill-conditioned or degenerate):", ill, "guard-band decisions:", guard, "of which differ:", differ)


def test_engineered_hypotheses(amd, scenes):
    for fix in (0, 1):
        sc, r = scenes[f"engineered-fix{fix}"]
        c = sc["cands"][0]
        n_inl, status, sim3, words, word_off = call(amd, sc)
        w = (c["n"] + 31) // 32
        by = {name: h for h, name in c["tags"].items()}
        for name in ("identity", "identity-permuted", "coincident"):
            h = by[name]
            assert status[h] == sr.NONFINITE and n_inl[h] == 0 and not words[h * w:(h + 1) * w].any(), name
            assert not np.isfinite(sim3[h]).all()
        assert status[by["collinear"]] == r["status"][by["collinear"]] == sr.OK and np.isfinite(sim3[by["collinear"]]).all()
        assert status[by["outliers"]] == sr.OK and n_inl[by["outliers"]] == r["n_inliers"][by["outliers"]]
        for name in ("inliers", "with-negative-z"):
            mask = sr.unpack(words[by[name] * w:(by[name] + 1) * w], c["n"])
            assert np.array_equal(mask, c["inlier"]) and mask[15] and c["x1"][15, 2] < 0, name
    sc, _ = scenes["n64-H5-fix0"]
    n_inl, _, _, words, _ = call(amd, sc)
    assert (n_inl == 64).all() and (words == 0xFFFFFFFF).all()  # every pair an inlier: two full words per hypothesis


def test_two_calls_give_identical_bytes_and_multi_equals_single_calls(amd, scenes):
    for id_ in ("K3-fix0", "K3-fix1"):
        sc, _ = scenes[id_]
        a, b = call(amd, sc), call(amd, sc)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        n_inl, status, sim3, words, word_off = a
        h0 = 0
        for k, c in enumerate(sc["cands"]):
            H = len(c["triples"])
            ns, ss, ms, ws = amd.sim3_ransac(c["x1"], c["x2"], c["max1"], c["max2"], c["cam1"], c["cam2"], sc["fix_scale"], c["triples"])
            assert ns.tobytes() == n_inl[h0:h0 + H].tobytes() and ss.tobytes() == status[h0:h0 + H].tobytes(), (id_, k)
            assert ms.tobytes() == sim3[h0:h0 + H].tobytes() and ws.tobytes() == words[word_off[k]:word_off[k + 1]].tobytes(), (id_, k)
            h0 += H


def test_refusals_leave_the_thread_usable(amd, scenes):
    from orb_slam2_annotate_amd import _lib
    sc, r = scenes["K3-fix0"]
    o = sr.operands(sc)

    def refused(**kw):
        a = dict(o, **kw)
        with pytest.raises(amd.OrbfeError) as ei:
            amd.sim3_ransac_multi(a["pair_off"], a["x1"], a["x2"], a["max1"], a["max2"], a["cam1"], a["cam2"], a["fix_scale"],
                                  a["hyp_off"], a["triples"])
        assert ei.value.code == _lib.ERR_INVALID
    n0 = sc["cands"][0]["n"]
    bad = o["pair_off"].copy(); bad[1], bad[2] = bad[2], bad[1]
    refused(pair_off=bad)  # not monotone
    bad = o["pair_off"].copy(); bad[-1] -= 1
    refused(pair_off=bad)  # does not end at N
    bad = o["hyp_off"].copy(); bad[-1] += 1
    refused(hyp_off=bad)  # does not end at H
    bad = o["hyp_off"].copy(); bad[0] = 1
    refused(hyp_off=bad)  # does not start at 0
    bad = o["triples"].copy(); bad[0, 1] = n0
    refused(triples=bad)  # an index outside [0, n_k)
    bad = o["triples"].copy(); bad[0, 1] = -1
    refused(triples=bad)
    bad = o["triples"].copy(); bad[3, 2] = bad[3, 0]
    refused(triples=bad)  # a repeated index
    for name in ("cam1", "cam2"):
        for v in (np.nan, np.inf):
            bad = o[name].copy(); bad[1, 2] = v
            refused(**{name: bad})
    # a candidate with fewer than 3 pairs that has hypotheses (and none without them is legal)
    two = dict(pair_off=np.array([0, 2], np.int32), x1=o["x1"][:2], x2=o["x2"][:2], max1=o["max1"][:2], max2=o["max2"][:2],
               cam1=o["cam1"][:1], cam2=o["cam2"][:1])
    refused(**two, hyp_off=np.array([0, 1], np.int32), triples=np.array([[0, 1, 0]], np.int32))
    out = amd.sim3_ransac_multi(two["pair_off"], two["x1"], two["x2"], two["max1"], two["max2"], two["cam1"], two["cam2"], False,
                                np.array([0, 0], np.int32), np.zeros((0, 3), np.int32))
    assert len(out[0]) == 0 and out[4].tolist() == [0, 0]
    # NULL arguments, straight at the C-ABI
    L = _lib.load()
    c = sc["cands"][0]
    H, w = len(c["triples"]), (c["n"] + 31) // 32
    n_inl, status, sim3, words = np.zeros(H, np.int32), np.zeros(H, np.uint8), np.zeros((H, 13), np.float32), np.zeros(H * w, np.uint32)
    keep = [np.ascontiguousarray(c[k]) for k in ("x1", "x2", "max1", "max2", "cam1", "cam2", "triples")]
    good = [0, c["n"]] + [_lib.ptr(a) for a in keep[:6]] + [0, H, _lib.ptr(keep[6]), _lib.ptr(n_inl), _lib.ptr(status),
                                                             _lib.ptr(sim3), _lib.ptr(words)]
    for i in (2, 3, 4, 5, 6, 7, 10, 11, 12, 13, 14):
        a = list(good); a[i] = None
        assert L.orbfe_sim3_ransac(*a) == _lib.ERR_INVALID, i
    assert L.orbfe_sim3_ransac(*good) == 0
    po, ho, wo = o["pair_off"], o["hyp_off"], np.zeros(4, np.int32)
    Ht, Wt = int(ho[-1]), int(sr.word_offsets(sc)[-1])
    outs = [np.zeros(Ht, np.int32), np.zeros(Ht, np.uint8), np.zeros((Ht, 13), np.float32), np.zeros(Wt, np.uint32)]
    goodm = [0, 3, int(po[-1]), Ht, _lib.ptr(po)] + [_lib.ptr(o[k]) for k in ("x1", "x2", "max1", "max2", "cam1", "cam2")] + \
            [0, _lib.ptr(ho), _lib.ptr(o["triples"])] + [_lib.ptr(a) for a in outs] + [_lib.ptr(wo)]
    for i in (4, 5, 6, 7, 8, 9, 10, 12, 13, 14, 15, 16, 17, 18):
        a = list(goodm); a[i] = None
        assert L.orbfe_sim3_ransac_multi(*a) == _lib.ERR_INVALID, i
    assert L.orbfe_sim3_ransac_multi(*goodm) == 0
    # the two pure host functions
    d = np.array([[0, 0, 0], [6, 5, 4], [3, 3, 3]], np.int32)
    assert np.array_equal(amd.sim3_triples_from_draws(7, d), sr.triples_from_draws(7, d))
    with pytest.raises(amd.OrbfeError):
        amd.sim3_triples_from_draws(7, np.array([[0, 6, 0]], np.int32))  # the second draw indexes a list of 6
    for n, mi, mx in ((100, 20, 300), (40, 20, 300), (25, 20, 300), (40, 20, 10), (20, 20, 300), (19, 20, 300), (0, 6, 300), (21, 20, 300)):
        assert amd.sim3_max_iterations(n, 0.99, mi, mx) == sr.max_iterations(n, 0.99, mi, mx), (n, mi, mx)
    # a later valid call on the same thread
    sr.compare("after", sc, r, *call(amd, sc), sr.s_sim3())


def _solvers(amd, sc):
    out = []
    for c in sc["cands"]:
        s = amd.Sim3Solver(c["indices1"], c["x1"], c["x2"], c["sigma2_1"], c["sigma2_2"], c["cam1"], c["cam2"], c["N1"], sc["fix_scale"])
        s.SetRansacParameters(0.99, sr.CLASS_MIN_INLIERS, 300)
        out.append(s)
    return out


@pytest.mark.parametrize("fix", (0, 1))
def test_class_round_robin_equals_the_reference_state_machine(amd, scenes, fix):
    sc, r = scenes[f"class-fix{fix}"]
    solvers = _solvers(amd, sc)
    with pytest.raises(RuntimeError):
        solvers[0].iterate(5)  # before evaluate_all
    for s, c in zip(solvers, sc["cands"]):
        assert np.array_equal(s.max_err1, c["max1"]) and np.array_equal(s.max_err2, c["max2"])
        assert s.n_hypotheses == len(c["triples"])
    amd.Sim3Solver.evaluate_all(solvers, [c["triples"] for c in sc["cands"]])
    assert sum(int(g.sum()) for g in r["guard"]) == 0  # no decision of these scenes is in the guard band: counts are equal
    refs, h0 = [], 0
    for c in sc["cands"]:
        H = len(c["triples"])
        refs.append(sr.RefSolver(r["n_inliers"][h0:h0 + H], r["masks"][h0:h0 + H], c["indices1"], c["N1"], sr.CLASS_MIN_INLIERS,
                                 sr.max_iterations(c["n"], 0.99, sr.CLASS_MIN_INLIERS, 300)))
        h0 += H
    # the caller's loop (src/LoopClosing.cc:342-404), going on after an acceptance as it does when OptimizeSim3 rejects it
    discarded = [False] * len(solvers)
    first_accept = {}
    rounds = 0
    while not all(discarded) and rounds < 200:
        rounds += 1
        for k, (s, ref) in enumerate(zip(solvers, refs)):
            if discarded[k]:
                continue
            T, no_more, vb, n = s.iterate(5)
            hr, no_more_r, vbr, nr = ref.iterate(5)
            assert ((T is None) == (hr is None)) and no_more == no_more_r and n == nr and np.array_equal(vb, vbr), (k, rounds)
            assert s.mnIterations == ref.iterations and s.mnBestInliers == ref.best_inliers
            if T is not None:
                first_accept.setdefault(k, (vb, T))
                assert T.dtype == np.float32 and np.array_equal(T[3], [0, 0, 0, 1])
                assert np.allclose(s.GetEstimatedScale() * s.GetEstimatedRotation(), T[:3, :3], rtol=1e-6, atol=0)
                assert np.array_equal(s.GetEstimatedTranslation(), T[:3, 3])
            if no_more:
                discarded[k] = True
    assert all(discarded) and rounds > 1
    assert discarded[2] and solvers[2].mnIterations == 0  # n < minInliers: bNoMore at once
    assert 0 not in first_accept  # 95 % outliers: never above minInliers
    good = sc["cands"][1]
    planted = np.zeros(good["N1"], bool)
    planted[good["indices1"][good["inlier"]]] = True
    assert np.array_equal(first_accept[1][0], planted)  # the first accepted inlier set of the good candidate
    s0, R, t = sr.planted(fix)
    assert np.allclose(first_accept[1][1][:3], np.concatenate([s0 * R, t[:, None]], axis=1), atol=1e-4)
    # find() on fresh solvers: the first acceptance again; a seed in place of triples is reproducible
    again = _solvers(amd, sc)
    amd.Sim3Solver.evaluate_all(again, [c["triples"] for c in sc["cands"]])
    T, vb, n = again[1].find()
    assert np.array_equal(T, first_accept[1][1]) and np.array_equal(vb, planted)
    t1 = amd.Sim3Solver.evaluate_all(again, 7)
    t2 = amd.Sim3Solver.evaluate_all(_solvers(amd, sc), 7)
    assert all(np.array_equal(a, b) for a, b in zip(t1, t2)) and [len(t) for t in t1] == [len(c["triples"]) for c in sc["cands"]]
    assert all((np.sort(t, axis=1)[:, 1:] != np.sort(t, axis=1)[:, :-1]).all() and t.min() >= 0 and t.max() < c["n"]
               for t, c in zip(t1[:2], sc["cands"]))


def test_chain_into_search_by_sim3(amd):
    """Two resident frames of one scene: key frame 2's keypoints are key frame 1's map points seen through the planted
    Sim3.  The accepted (s, R, t) projects both key frames' points for the existing SearchBySim3, which must accept the
    operands and find at least the planted inliers whose descriptors match (all of them: the descriptors are equal)."""
    rng = np.random.default_rng(11)
    n = 120
    c = sr.candidate(rng, n, 50, False, outliers=0.25)
    sc = dict(fix_scale=False, cands=[c])
    solver = amd.Sim3Solver(np.arange(n), c["x1"], c["x2"], c["sigma2_1"], c["sigma2_2"], c["cam1"], c["cam2"], n, False)
    solver.SetRansacParameters(0.99, 20, 300)
    amd.Sim3Solver.evaluate_all([solver], 3)
    T12, vb, n_in = solver.find()
    assert T12 is not None and np.array_equal(vb, c["inlier"])
    s12, R12, t12 = solver.GetEstimatedScale(), solver.GetEstimatedRotation().astype(np.float64), solver.GetEstimatedTranslation().astype(np.float64)

    def image(K, X):
        K = K.astype(np.float64)
        return K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]
    X1, X2 = c["x1"].astype(np.float64), c["x2"].astype(np.float64)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    frames = []
    for K, X in ((c["cam1"], X1), (c["cam2"], X2)):
        u, v = image(K, X)
        frames.append(amd.FrameView(u.astype(np.float32), v.astype(np.float32), np.zeros(n, np.int32), desc, (-2000.0, 3000.0, -2000.0, 3000.0),
                                    angle=np.zeros(n, np.float32)).upload())
    # every keypoint holds a map point whose descriptor is the keypoint's; pair i is keypoint i of both key frames
    X1in2 = (X1 - t12) @ R12 / s12        # key frame 1's points in camera 2 (sR^T (X - t) / s)
    X2in1 = s12 * X2 @ R12.T + t12        # key frame 2's points in camera 1
    u12, v12 = image(c["cam2"], X1in2)
    u21, v21 = image(c["cam1"], X2in1)
    ok1 = (X1in2[:, 2] > 0).astype(np.uint8)
    ok2 = (X2in1[:, 2] > 0).astype(np.uint8)
    SF = (1.2 ** np.arange(8)).astype(np.float32)
    level = np.zeros(n, np.int32)
    found, m12 = amd.ORBmatcher(0.75, True).SearchBySim3(frames[0], frames[1], SF, SF, ok1, u12.astype(np.float32), v12.astype(np.float32),
                                                         level, desc, ok2, u21.astype(np.float32), v21.astype(np.float32), level, desc, 7.5)
    assert (m12[c["inlier"]] == np.arange(n)[c["inlier"]]).all()  # map point i of key frame 1 is keypoint i of key frame 2
    print("chain: planted inliers", int(c["inlier"].sum()), "nFound", found)
    assert found >= int(c["inlier"].sum())
    for f in frames:
        f.close()
