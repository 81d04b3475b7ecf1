"""orbfe_initializer_ransac* (every H / F RANSAC hypothesis of Initializer::Initialize in one launch) and the Initializer class
against the float64 restatement tests/initializer_ref.py: pair counts at the mask-word, ballot and wave-trip edges, set counts
around the four-waves-per-workgroup edge, the reference's own 200 sets x 300 pairs, K = 3 with an empty problem in each place,
sigma 1 and 2, three scene kinds, the engineered sets, and the properties of the call (determinism, multi = single, refusals,
the chain from SearchForInitialization)."""
import numpy as np
import pytest

import initializer_ref as ir

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


@pytest.fixture(scope="module")
def scenes():
    """every scene with its reference result, computed once"""
    return {id_: (sc, ir.run(sc)) for id_, sc in ir.gpu_scenes()}


@pytest.fixture(scope="module")
def tol():
    s_model, s_score = ir.recorded()
    return ir.allowance(s_model), ir.allowance(s_score)


def call(amd, sc):
    o = ir.operands(sc)
    return amd.initializer_ransac_multi(o["pair_off"], o["pairs"], o["T1"], o["T2"], o["sigma"], o["hyp_off"], o["sets"])


@pytest.mark.parametrize("id_", [id_ for id_, _ in ir.specs()])
def test_scene_equals_the_reference(amd, scenes, tol, id_):
    sc, r = scenes[id_]
    c = ir.compare(id_, sc, r, *call(amd, sc), tol)
    ill, n_hyp, guard, n_dec = ir.caps(sc, r)
    print(id_, "not compared (ill-conditioned or degenerate):", c["ill"], "ill-conditioned among the defined:", ill, "of", n_hyp,
          "guard-band decisions:", c["guard"], "of", n_dec, "of which differ:", c["differ"], "largest model distance:", c["d_model"],
          "largest score distance:", c["d_score"], "allowance:", tol)
    if not ir.exempt(id_):
        assert ill <= ir.ILL_CAP * n_hyp
    assert guard <= ir.GUARD_CAP * n_dec


def test_engineered_sets(amd, scenes):
    for sigma in (1, 2):
        sc, r = scenes[f"engineered-s{sigma}"]
        p = sc["probs"][0]
        score, status, n_inl, model, h12, words, word_off = call(amd, sc)
        w = (p["n"] + 31) // 32
        wd = lambda h, m: words[(2 * h + m) * w:(2 * h + m + 1) * w]
        by = {name: h for h, name in p["tags"].items()}
        h = by["coincident"]  # H singular -> zero H12 -> NaN score -> NONFINITE, never selected
        assert status[h, ir.MH] == ir.NONFINITE and n_inl[h, ir.MH] == 0 and not wd(h, ir.MH).any()
        assert not h12[h].any() and np.isnan(score[h, ir.MH])
        for m in (ir.MH, ir.MF):
            best, s = amd.initializer.replay_scan(score, m)
            ref = ir.replay(r["score"], m)[0]  # (the all-inlier set and its permutation score the same but for rounding)
            assert best == ref or ir.score_distance(r["score"][best, m], r["score"][ref, m]) <= ir.allowance(ir.recorded()[1])
            assert best != h and status[best, m] == ir.OK
        for m in (ir.MH, ir.MF):  # collinear: whatever comes out is labelled consistently
            hc = by["collinear"]
            fin = np.isfinite(score[hc, m]) and np.isfinite(model[hc, m]).all() and (m == ir.MF or np.isfinite(h12[hc]).all())
            assert (status[hc, m] == ir.OK) == bool(fin)
        ho = by["outliers"]
        assert (status[ho] == ir.OK).all() and np.array_equal(n_inl[ho], r["n_inliers"][ho])
        # the all-inlier set and its permutation find the scene's inliers under F, but for pair 32: one of its two chi-squares
        # lies between 3.841 and 5.991, so it is no inlier, and the other image's term still adds to the score
        for name in ("inliers", "inliers-permuted"):
            h = by[name]
            mask = ir.unpack(wd(h, ir.MF), p["n"])
            expect = p["inlier"].copy()
            expect[32] = False
            assert mask[expect].all() and not mask[32] and not (mask != r["masks"][h][ir.MF]).any(), name  # (an outlier displaced
            # along its epipolar line may pass: the restatement's mask says which)
            c1, c2 = ir.chi_f(model[h:h + 1, ir.MF], p["pairs"][32:33].astype(np.float64), p["sigma"])
            lo, hi = sorted((float(c1[0, 0]), float(c2[0, 0])))
            assert lo < ir.TH_F < hi < ir.TH_SCORE_F
            rest = np.arange(p["n"]) != 32
            alone = ir.score_of(*ir.chi_f(model[h:h + 1, ir.MF], p["pairs"][rest].astype(np.float64), p["sigma"]), ir.TH_F, ir.TH_SCORE_F)[1][0]
            assert score[h, ir.MF] - alone == pytest.approx(ir.TH_SCORE_F - lo, rel=1e-6)
    for sigma in (1, 2):  # every pair an inlier: two full words, 64 inliers
        sc, _ = scenes[f"planar-n64-S1-s{sigma}"]
        score, status, n_inl, model, h12, words, word_off = call(amd, sc)
        assert n_inl[0, ir.MH] == 64 and (words[:2] == 0xFFFFFFFF).all() and status[0, ir.MH] == ir.OK


def test_two_calls_give_identical_bytes_and_multi_equals_single_calls(amd, scenes):
    for id_ in ("K3-empty-first", "K3-empty-middle", "K3-empty-last", "engineered-s1"):
        sc, _ = scenes[id_]
        a, b = call(amd, sc), call(amd, sc)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        score, status, n_inl, model, h12, words, word_off = a
        h0 = 0
        for k, p in enumerate(sc["probs"]):
            H = len(p["sets"])
            s1, st1, n1, m1, i1, w1 = amd.initializer_ransac(p["pairs"], p["T1"], p["T2"], p["sigma"], p["sets"])
            sl = slice(h0, h0 + H)
            assert s1.tobytes() == score[sl].tobytes() and st1.tobytes() == status[sl].tobytes() and n1.tobytes() == n_inl[sl].tobytes(), (id_, k)
            assert m1.tobytes() == model[sl].tobytes() and i1.tobytes() == h12[sl].tobytes(), (id_, k)
            assert w1.tobytes() == words[word_off[k]:word_off[k + 1]].tobytes(), (id_, k)
            h0 += H


def test_refusals_leave_the_thread_usable(amd, scenes, tol):
    from orb_slam2_annotate_amd import _lib
    sc, r = scenes["K3-empty-middle"]
    o = ir.operands(sc)

    def refused(**kw):
        a = dict(o, **kw)
        with pytest.raises(amd.OrbfeError) as ei:
            amd.initializer_ransac_multi(a["pair_off"], a["pairs"], a["T1"], a["T2"], a["sigma"], a["hyp_off"], a["sets"])
        assert ei.value.code == _lib.ERR_INVALID
    n0 = sc["probs"][0]["n"]
    bad = o["pair_off"].copy(); bad[1], bad[3] = bad[3], bad[1]
    refused(pair_off=bad)  # not monotone
    bad = o["pair_off"].copy(); bad[-1] -= 1
    refused(pair_off=bad)  # does not end at N
    bad = o["pair_off"].copy(); bad[0] = 1
    refused(pair_off=bad)  # does not start at 0
    bad = o["hyp_off"].copy(); bad[-1] += 1
    refused(hyp_off=bad)  # does not end at H
    bad = o["hyp_off"].copy(); bad[0] = 1
    refused(hyp_off=bad)  # does not start at 0
    bad = o["hyp_off"].copy(); bad[1], bad[3] = bad[3], bad[1]
    refused(hyp_off=bad)
    bad = o["sets"].copy(); bad[0, 7] = n0
    refused(sets=bad)  # an index outside [0, n_k)
    bad = o["sets"].copy(); bad[0, 3] = -1
    refused(sets=bad)
    bad = o["sets"].copy(); bad[2, 7] = bad[2, 0]
    refused(sets=bad)  # a repeated index
    for name in ("T1", "T2"):
        for v in (np.nan, np.inf):
            bad = o[name].copy(); bad[2, 1] = v
            refused(**{name: bad})
    for v in (np.nan, np.inf, 0.0, -1.0):
        bad = o["sigma"].copy(); bad[0] = v
        refused(sigma=bad)
    # a problem with fewer than 8 pairs that has sets (and one without pairs and sets is legal)
    seven = dict(pair_off=np.array([0, 7], np.int32), pairs=o["pairs"][:7], T1=o["T1"][:1], T2=o["T2"][:1], sigma=o["sigma"][:1])
    refused(**seven, hyp_off=np.array([0, 1], np.int32), sets=np.array([[0, 1, 2, 3, 4, 5, 6, 0]], np.int32))
    none = amd.initializer_ransac_multi(np.array([0, 0], np.int32), np.zeros((0, 4), np.float32), o["T1"][:1], o["T2"][:1], o["sigma"][:1],
                                        np.array([0, 0], np.int32), np.zeros((0, 8), np.int32))
    assert len(none[0]) == 0 and none[6].tolist() == [0, 0]
    # NULL arguments, straight at the C-ABI
    L = _lib.load()
    p = sc["probs"][0]
    H, w = len(p["sets"]), (p["n"] + 31) // 32
    outs = [np.zeros((H, 2)), np.zeros((H, 2), np.uint8), np.zeros((H, 2), np.int32), np.zeros((H, 18)), np.zeros((H, 9)), np.zeros(2 * H * w, np.uint32)]
    keep = [np.ascontiguousarray(p["pairs"]), np.ascontiguousarray(p["T1"]), np.ascontiguousarray(p["T2"]), np.ascontiguousarray(p["sets"])]
    good = [0, p["n"], _lib.ptr(keep[0]), _lib.ptr(keep[1]), _lib.ptr(keep[2]), float(p["sigma"]), H, _lib.ptr(keep[3])] + [_lib.ptr(a) for a in outs]
    for i in (2, 3, 4, 7, 8, 9, 10, 11, 12, 13):
        a = list(good); a[i] = None
        assert L.orbfe_initializer_ransac(*a) == _lib.ERR_INVALID, i
    assert L.orbfe_initializer_ransac(*good) == 0
    po, ho, wo = o["pair_off"], o["hyp_off"], np.zeros(4, np.int32)
    Ht, Wt = int(ho[-1]), int(ir.word_offsets(sc)[-1])
    outs = [np.zeros((Ht, 2)), np.zeros((Ht, 2), np.uint8), np.zeros((Ht, 2), np.int32), np.zeros((Ht, 18)), np.zeros((Ht, 9)), np.zeros(Wt, np.uint32)]
    goodm = [0, 3, int(po[-1]), Ht, _lib.ptr(po)] + [_lib.ptr(o[k]) for k in ("pairs", "T1", "T2", "sigma")] + \
            [_lib.ptr(ho), _lib.ptr(o["sets"])] + [_lib.ptr(a) for a in outs] + [_lib.ptr(wo)]
    for i in range(4, 18):
        a = list(goodm); a[i] = None
        assert L.orbfe_initializer_ransac_multi(*a) == _lib.ERR_INVALID, i
    assert L.orbfe_initializer_ransac_multi(*goodm) == 0
    # the two pure host functions
    d = np.array([[0] * 8, [9, 8, 7, 6, 5, 4, 3, 2], [3, 3, 3, 3, 3, 2, 1, 0]], np.int32)
    assert np.array_equal(amd.initializer_sets_from_draws(10, d), ir.sets_from_draws(10, d))
    with pytest.raises(amd.OrbfeError):
        amd.initializer_sets_from_draws(10, np.array([[0, 0, 0, 0, 0, 0, 0, 3]], np.int32))  # the 8th draw indexes a list of 3
    keys = np.random.default_rng(5).uniform(0, 640, (333, 2)).astype(np.float32)
    assert np.allclose(amd.initializer_normalize(keys), ir.normalize(keys), rtol=1e-13, atol=0)
    with pytest.raises(amd.OrbfeError):
        amd.initializer_normalize(np.zeros((0, 2), np.float32))
    assert L.orbfe_initializer_normalize(3, None, _lib.ptr(np.zeros(4))) == _lib.ERR_INVALID
    assert L.orbfe_initializer_sets_from_draws(10, 1, None, _lib.ptr(np.zeros(8, np.int32))) == _lib.ERR_INVALID
    # a later valid call on the same thread
    ir.compare("after", sc, r, *call(amd, sc), tol)


@pytest.mark.parametrize("kind", ("planar", "general"))
def test_chain_from_search_for_initialization(amd, kind):
    """Two frames of one scene (key points and descriptors made here; frame 2 holds frame 1's points seen from the second
    camera, shuffled, among unmatched ones) -> SearchForInitialization -> Initializer.FindModels: the planar scene chooses H
    (RH > 0.40), the 3-D scene F, and the chosen model and mask equal the restatement's on the same matches and sets."""
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
    prev = P[:, :2].copy()
    n_matches, m12 = amd.ORBmatcher(0.9, True).SearchForInitialization(F1, F2, prev, 100)
    assert n_matches >= 100  # Tracking.cc asks for 100 before it calls Initialize
    N = int((m12 >= 0).sum())
    draws = np.stack([rng.integers(0, N - j, 200) for j in range(8)], axis=1)
    init = amd.Initializer(P[:, :2], 1.0, 200)
    out = init.FindModels(keys2, m12, draws)
    # the restatement on the same matches
    mv = out["mvMatches12"]
    pairs = np.concatenate([P[mv[:, 0], :2], keys2[mv[:, 1]]], axis=1)
    sc = dict(probs=[dict(kind=kind, n=N, pairs=pairs, T1=ir.normalize(P[:, :2]), T2=ir.normalize(keys2), sigma=1.0,
                          sets=ir.sets_from_draws(N, draws), tags={}, between=None)])
    r = ir.run(sc)
    assert np.array_equal(out["mvSets"], sc["probs"][0]["sets"])
    bH, SH = ir.replay(r["score"], ir.MH)
    bF, SF = ir.replay(r["score"], ir.MF)
    RH, choose_H = ir.choose(SH, SF)
    print(kind, "matches", N, "SH", out["SH"], "SF", out["SF"], "RH", out["RH"], "restatement RH", RH)
    assert out["choose_H"] == choose_H == (kind == "planar")
    m, best, name = (ir.MH, bH, "H") if choose_H else (ir.MF, bF, "F")
    assert out["best" + name] == best
    assert ir.model_distance(out[name + "21"][None], r["model"][best, m][None])[0] <= ir.allowance(ir.recorded()[0])
    diff = out["vbMatchesInliers" + name] != r["masks"][best][m]
    assert not (diff & ~r["guard"][best][m]).any()
    assert out["RH"] == pytest.approx(RH, rel=1e-6)
