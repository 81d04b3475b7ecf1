"""GPU: orbfe_initializer_reconstruct* (k_init_reconstruct.hip) and Initializer.Reconstruct / Initialize against the numpy
restatement tests/initializer_reconstruct_ref.py.  The shapes sit where the kernel can go wrong -- 1, 32, 33, 51, 52, 64, 65, 256,
257 and 300 inlier pairs cross the mask-word, the min(50, n - 1), the wave and the workgroup edges -- and every sized case is a
planar scene with the true H and a general scene with the true F, whose 7 and 3 wrong hypotheses are exercised with them.  The
seeds keep every pair and problem out of the guard bands, so n_good, pair_flags and every replay decision are compared for
EQUALITY; motions, points and the selected cosine within the allowance of profiles/initializer_reconstruct_tolerance.txt."""
import numpy as np
import pytest

import initializer_ref as ir
import initializer_reconstruct_ref as rr

pytestmark = pytest.mark.gpu

KEYS = ("hyp_off", "slot_off", "R", "t", "n_good", "cos_sel", "hyp_status", "x3d", "pair_flags", "problem_status", "n_inliers")


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as amd
    return amd


@pytest.fixture(scope="module")
def scenes():
    return {id_: (sc, r) for id_, sc, r in rr.scenes()}


def call_multi(amd, sc):
    o = rr.operands(sc)
    return amd.initializer_reconstruct_multi(o["pair_off"], o["pairs"], o["model_kind"], o["model"], o["K4"], o["sigma"],
                                             o["inlier_words"], o["in_word_off"])


def call_single(amd, p):
    return amd.initializer_reconstruct(p["pairs"], p["kind"], p["model"], p["K4"], p["sigma"], rr.ir_pack(p["mask"]))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_multi_equals_singles(amd, sc, out):
    dev = rr.split(sc, out)
    for k, (p, d) in enumerate(zip(sc["probs"], dev)):
        s = call_single(amd, p)
        for key in ("R", "t", "n_good", "cos_sel", "hyp_status", "x3d", "pair_flags"):
            assert same_bytes(d[key], s[key]), (k, key)
        assert (d["problem_status"], d["n_inliers"]) == (s["problem_status"], s["n_inliers"]), k


@pytest.mark.parametrize("id_", rr.IDS)
def test_scene_equals_the_restatement_and_itself(amd, scenes, id_):
    sc, r = scenes[id_]
    out = call_multi(amd, sc)
    worst = rr.compare(id_, sc, r, rr.split(sc, out))
    print(id_, "largest motion / point (relative) / cosine distances:", worst)
    again = call_multi(amd, sc)
    for key in KEYS:
        assert same_bytes(out[key], again[key]), key  # two calls: identical bytes
    assert_multi_equals_singles(amd, sc, out)


def test_mixed_multi_call_equals_the_single_calls_byte_for_byte(amd, scenes):
    """H and F problems of different sizes, an all-zero mask, a DEGENERATE problem and a problem without pairs in ONE call"""
    probs = []
    for id_ in ("n257", "n1", "zero-mask", "n33", "identity", "nonfinite", "n300", "rotation"):
        probs += scenes[id_][0]["probs"]
    empty = rr.problem(rr.MF, ir.fundamental(), np.zeros((0, 4), np.float32), np.zeros(0, bool))
    probs = probs[:3] + [empty] + probs[3:] + [dict(empty, kind=rr.MH, model=ir.plant("planar")[2])]
    sc = dict(probs=probs)
    out = call_multi(amd, sc)
    assert out["hyp_off"][-1] == sum(8 if p["kind"] == rr.MH else 4 for p in probs)
    assert_multi_equals_singles(amd, sc, out)
    rr.compare("mixed", sc, rr.run(sc), rr.split(sc, out))


def test_invalid_arguments_are_refused_and_the_thread_stays_usable(amd, scenes):
    from orb_slam2_annotate_amd import _lib
    L = _lib.load()
    sc, r = scenes["n33"]
    o = rr.operands(sc)
    K, N, W = 2, int(o["pair_off"][-1]), int(o["in_word_off"][-1])
    G, S = 12, 12 * 33
    outs = [np.zeros(K + 1, np.int32), np.zeros(K + 1, np.int32), np.zeros((G, 9)), np.zeros((G, 3)), np.zeros(G, np.int32), np.zeros(G),
            np.zeros(G, np.uint8), np.zeros((S, 3)), np.zeros(S, np.uint8), np.zeros(K, np.uint8), np.zeros(K, np.int32)]

    def args(**kw):
        a = dict(o, **kw)
        keep.append(a)
        return [0, K, N, W] + [_lib.ptr(np.ascontiguousarray(a[k])) if a[k] is not None else None
                               for k in ("pair_off", "pairs", "model_kind", "model", "K4", "sigma", "inlier_words", "in_word_off")] + \
               [_lib.ptr(x) for x in outs]
    keep = []
    good = args()
    assert L.orbfe_initializer_reconstruct_multi(*good) == 0
    for i in range(4, 23):  # every array NULL in turn
        a = list(good); a[i] = None
        assert L.orbfe_initializer_reconstruct_multi(*a) == _lib.ERR_INVALID, i

    def edited(key, idx, val):
        x = np.array(o[key], copy=True)
        x.reshape(-1)[idx] = val
        return args(**{key: x})
    bad = [edited("pair_off", 0, 1), edited("pair_off", 1, 70), edited("pair_off", 2, N - 1),     # start, decrease, end
           edited("in_word_off", 0, 1), edited("in_word_off", 1, 3), edited("in_word_off", 2, W + 1),
           edited("in_word_off", 1, 1),                                                           # not ceil(n_k / 32) words
           edited("model_kind", 0, 2), edited("model_kind", 1, -1),
           edited("model", 4, np.nan), edited("model", 9, np.inf), edited("K4", 2, np.nan), edited("K4", 5, np.inf),
           edited("K4", 0, 0.0), edited("K4", 5, 0.0),                                           # fx, fy == 0
           edited("sigma", 0, 0.0), edited("sigma", 1, -1.0), edited("sigma", 0, np.nan), edited("sigma", 1, np.inf)]
    for i, a in enumerate(bad):
        assert L.orbfe_initializer_reconstruct_multi(*a) == _lib.ERR_INVALID, i
    for k in (-1, 4097):
        a = list(good); a[1] = k
        assert L.orbfe_initializer_reconstruct_multi(*a) == _lib.ERR_INVALID, k
    a = list(good); a[0] = -1
    assert L.orbfe_initializer_reconstruct_multi(*a) == _lib.ERR_INVALID
    # a call without problems: ORBFE_OK, offsets written
    z = np.zeros(1, np.int32)
    none = [0, 0, 0, 0, _lib.ptr(z)] + [None] * 6 + [_lib.ptr(z), _lib.ptr(np.ones(1, np.int32)), _lib.ptr(np.ones(1, np.int32))] + [None] * 9
    assert L.orbfe_initializer_reconstruct_multi(*none) == 0
    # the single form
    p = sc["probs"][1]
    s_outs = [np.zeros((4, 9)), np.zeros((4, 3)), np.zeros(4, np.int32), np.zeros(4), np.zeros(4, np.uint8), np.zeros((4 * 33, 3)),
              np.zeros(4 * 33, np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.int32)]
    words = rr.ir_pack(p["mask"])
    sgood = [0, 33, _lib.ptr(p["pairs"]), rr.MF, _lib.ptr(p["model"]), _lib.ptr(p["K4"]), 1.0, _lib.ptr(words)] + [_lib.ptr(x) for x in s_outs]
    assert L.orbfe_initializer_reconstruct(*sgood) == 0
    for i in (2, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16):
        a = list(sgood); a[i] = None
        assert L.orbfe_initializer_reconstruct(*a) == _lib.ERR_INVALID, i
    for i, v in ((1, -1), (3, 2), (6, 0.0), (6, float("nan"))):
        a = list(sgood); a[i] = v
        assert L.orbfe_initializer_reconstruct(*a) == _lib.ERR_INVALID, (i, v)
    # a valid call succeeds afterwards on the same thread
    rr.compare("after", sc, r, rr.split(sc, call_multi(amd, sc)))


@pytest.mark.parametrize("kind", ("planar", "general"))
def test_chain_from_search_for_initialization(amd, kind):
    """The two frames of tests/test_gpu_initializer.py's chain test -> SearchForInitialization -> Initializer.Initialize.  On
    the 3-D scene it succeeds: R21 / t21 equal the restatement's run on the same matches and the class's model and mask, and the
    true motion up to scale; vbTriangulated equals the restatement's; the points reproject within th2 in both images.  On the
    planar scene the reference itself returns false: the plane of tests/initializer_ref.py leaves Faugeras' two-fold ambiguity
    standing (both members of the pair accept all 150 points, so secondBestGood == bestGood at :813), and the device and the
    restatement agree on exactly that; the true motion is one of the two tied hypotheses."""
    rng = np.random.default_rng(21)
    n, extra = 150, 40
    P = ir.points(rng, kind, n).astype(np.float32)
    desc1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    perm = rng.permutation(n + extra)
    keys2 = np.concatenate([P[:, 2:], np.stack([rng.uniform(0, 640, extra), rng.uniform(0, 480, extra)], axis=1)]).astype(np.float32)
    desc2 = np.concatenate([desc1, rng.integers(0, 256, (extra, 32), dtype=np.uint8)])
    keys2, desc2 = keys2[perm], desc2[perm]
    bounds = (-2000.0, 3000.0, -2000.0, 3000.0)
    mk = lambda k, d: amd.FrameView(k[:, 0].copy(), k[:, 1].copy(), np.zeros(len(k), np.int32), d, bounds, angle=np.zeros(len(k), np.float32))
    F1, F2 = mk(P[:, :2], desc1), mk(keys2, desc2)
    n_matches, m12 = amd.ORBmatcher(0.9, True).SearchForInitialization(F1, F2, P[:, :2].copy(), 100)
    assert n_matches >= 100
    N = int((m12 >= 0).sum())
    draws = np.stack([rng.integers(0, N - j, 200) for j in range(8)], axis=1)
    init = amd.Initializer(P[:, :2], 1.0, 200)
    ok, R21, t21, vP3D, vbTri = init.Initialize(keys2, m12, draws, ir.KCAM)
    found = init.FindModels(keys2, m12, draws)
    rec = init.Reconstruct(found, ir.KCAM)
    assert rec["success"] == ok and np.array_equal(rec["vbTriangulated"], vbTri) and same_bytes(rec["vP3D"], vP3D)
    assert found["choose_H"] == (kind == "planar")
    name, mk_ = ("H", rr.MH) if found["choose_H"] else ("F", rr.MF)
    p = rr.problem(mk_, found[name + "21"], found["pairs"], found["vbMatchesInliers" + name])
    pr = rr.run_problem(p)
    assert rr.guard_count([pr]) == (0, 0)
    sc = dict(probs=[p])
    d = dict(rec["hypotheses"])
    rr.compare("chain-" + kind, sc, [pr], [d])
    truth = (ir.R21, ir.T21 / np.linalg.norm(ir.T21))
    assert ok == pr["success"] == (kind == "general")
    if kind == "planar":
        top = np.argsort(d["n_good"])[-2:]
        assert (d["n_good"][top] == N).all()
        assert min(rr.motion_distance(d["R"][i], d["t"][i], *truth) for i in top) < 1e-4
        assert R21 is None and not vbTri.any() and not vP3D.any()
        return
    a = ir.allowance(rr.recorded()[0])
    assert rr.motion_distance(R21, t21, pr["R21"], pr["t21"]) <= a
    assert rr.motion_distance(R21, t21, *truth) < 1e-4
    first = found["mvMatches12"][:, 0]
    h = pr["hyps"][pr["best"]]
    want = np.zeros(n, bool)
    want[first] = (h["flags"] & rr.GOOD) != 0
    assert np.array_equal(vbTri, want) and vbTri.sum() >= 0.9 * N
    X = vP3D[vbTri].astype(np.float64)
    x1 = X @ ir.KCAM.T
    x2 = (X @ R21.T + t21) @ ir.KCAM.T
    m2 = m12[vbTri]
    e1 = ((x1[:, :2] / x1[:, 2:] - P[vbTri, :2]) ** 2).sum(1)
    e2 = ((x2[:, :2] / x2[:, 2:] - keys2[m2]) ** 2).sum(1)
    assert (e1 <= 4.0).all() and (e2 <= 4.0).all()  # th2 = 4 sigma^2
