"""CPU: properties of the float64 restatement tests/initializer_ref.py of Initializer::FindHomography / FindFundamental, its own
noise (recorded in profiles/initializer_tolerance.txt) and the two caps on every scene of the GPU test."""
import numpy as np
import pytest

import initializer_ref as ir


@pytest.fixture(scope="module")
def scenes():
    return [(id_, sc, ir.run(sc)) for id_, sc in ir.gpu_scenes()]


def _up_to_scale(a, b):
    return float(ir.model_distance(a[None], b[None])[0])


def test_planar_scene_recovers_the_generating_homography_with_all_pairs_inliers(scenes):
    seen = 0
    for id_, sc, r in scenes:
        for k, p in enumerate(sc["probs"]):
            if p["kind"] not in ("planar", "rotation"):
                continue
            Hgen = ir.plant(p["kind"])[2]
            for h in np.nonzero(r["prob"] == k)[0]:
                assert r["status"][h, ir.MH] == ir.OK and not r["ill"][h, ir.MH], (id_, h)
                assert _up_to_scale(r["model"][h, ir.MH], Hgen) < 1e-5, (id_, h)  # float32 coordinates: 6e-8 of ~500 px
                assert _up_to_scale(r["h12"][h], np.linalg.inv(Hgen)) < 1e-5, (id_, h)
                assert r["masks"][h][ir.MH].all() and r["n_inliers"][h, ir.MH] == p["n"], (id_, h)
                assert r["score"][h, ir.MH] == pytest.approx(2 * ir.TH_H * p["n"], rel=1e-4)
                seen += 1
    assert seen > 50


def test_general_scene_recovers_a_rank_two_fundamental_matrix(scenes):
    Fgen = ir.fundamental()
    seen = 0
    for id_, sc, r in scenes:
        for k, p in enumerate(sc["probs"]):
            if p["kind"] != "general" or p["n"] == 0:
                continue
            for h in np.nonzero(r["prob"] == k)[0]:
                F = r["model"][h, ir.MF]
                if r["status"][h, ir.MF] != ir.OK or r["ill"][h, ir.MF]:
                    continue
                assert abs(np.linalg.det(F / np.linalg.norm(F))) < 1e-12, (id_, h)  # after the rank-2 step
                st = p["sets"][h - int(np.nonzero(r["prob"] == k)[0][0])]
                if not p["inlier"][st].all() or p["tags"]:
                    continue  # a contaminated set fits its own 8 pairs, not the scene
                x = p["pairs"].astype(np.float64)[p["inlier"]]
                if p["between"] is not None:
                    x = x[np.arange(len(x)) != int(p["inlier"][:32].sum())]  # (pair 32 is displaced on purpose)
                x1, x2 = np.c_[x[:, :2], np.ones(len(x))], np.c_[x[:, 2:], np.ones(len(x))]
                res = np.abs(np.einsum("ni,ij,nj->n", x2, F / np.linalg.norm(F), x1)) / 500.0 ** 2
                assert res.max() < 1e-6 and _up_to_scale(F, Fgen) < 1e-2, (id_, h, float(res.max()))
                seen += 1
    assert seen > 10


def test_negating_the_null_vector_changes_no_score_or_mask(scenes):
    for id_, sc, r in scenes:
        rr = ir.run(sc, negate=True)
        assert np.array_equal(r["status"], rr["status"]), id_
        assert np.array_equal(r["score"][:, ir.MH], rr["score"][:, ir.MH], equal_nan=True), id_  # -H: every quotient is the same
        ok = (r["status"] == ir.OK) & ~r["ill"]
        assert (ir.score_distance(rr["score"][ok], r["score"][ok]) < 1e-9).all(), id_  # F: numpy's 3 x 3 SVD of -Fpre rounds anew
        for h in range(len(r["status"])):
            for m in (ir.MH, ir.MF):
                if ok[h, m]:
                    diff = r["masks"][h][m] != rr["masks"][h][m]
                    assert not (diff & ~r["guard"][h][m]).any(), (id_, h, m)


def test_sets_from_draws_is_the_pop_back_loop():
    rng = np.random.default_rng(3)
    for n in (8, 9, 50):
        d = np.stack([rng.integers(0, n - j, 60) for j in range(8)], axis=1)
        s = ir.sets_from_draws(n, d)
        assert all(len(set(row)) == 8 for row in s.tolist()) and s.min() >= 0 and s.max() < n
    # always the current last element: n-1, n-2, ...; always the first: 0, then what swap-with-back put there
    assert ir.sets_from_draws(10, [[9, 8, 7, 6, 5, 4, 3, 2]]).tolist() == [[9, 8, 7, 6, 5, 4, 3, 2]]
    assert ir.sets_from_draws(10, [[0] * 8]).tolist() == [[0, 9, 8, 7, 6, 5, 4, 3]]
    assert ir.sets_from_draws(8, [[7, 0, 5, 0, 3, 0, 1, 0]]).tolist() == [[7, 0, 5, 6, 3, 4, 1, 2]]
    with pytest.raises(AssertionError):
        ir.sets_from_draws(10, [[0, 0, 0, 0, 0, 0, 0, 3]])  # the 8th draw indexes a list of 3


def test_replay_keeps_the_first_of_two_equal_best_scores(scenes):
    sc = dict(ir.gpu_scenes())["general-n65-S3-sets"]
    p = dict(sc["probs"][0])
    p["sets"] = np.concatenate([p["sets"], p["sets"]])  # every set twice
    r = ir.run(dict(probs=[p]))
    for m in (ir.MH, ir.MF):
        assert np.array_equal(r["score"][:3, m], r["score"][3:, m])
        best, s = ir.replay(r["score"], m)
        assert 0 <= best < 3 and s == r["score"][:, m].max()
    # hand-made: strict >, NaN never taken, nothing above 0 leaves the model empty
    sc_ = np.array([[1.0, 0.0], [np.nan, np.nan], [3.0, 0.0], [3.0, -1.0], [2.0, 0.0]])
    assert ir.replay(sc_, 0) == (2, 3.0) and ir.replay(sc_, 1) == (-1, 0.0)
    assert ir.choose(3.0, 0.0) == (1.0, True) and ir.choose(0.0, 0.0)[1] is False and ir.choose(2.0, 3.0) == (0.4, False)


def test_float32_transcription_of_the_scoring_loops_agrees_with_the_float64_score(scenes):
    """the first three sets of every scene through the literal float32 loops; the figure is recorded as f32_score"""
    worst = 0.0
    for id_, sc, r in scenes:
        for k, p in enumerate(sc["probs"]):
            hs = np.nonzero(r["prob"] == k)[0][:3]
            for h in hs:
                for m in (ir.MH, ir.MF):
                    if r["status"][h, m] != ir.OK or r["ill"][h, m] or r["score"][h, m] < 1.0:
                        continue
                    s32 = ir.score_float32(r["model"][h, m], r["h12"][h], p["pairs"], p["sigma"], m == ir.MH)
                    worst = max(worst, abs(s32 - r["score"][h, m]) / r["score"][h, m])
    print("largest relative difference of the float32 score:", worst)
    assert 0 < worst < 1e-2
    rec = dict(t.split("=") for t in ir.TOLERANCE_FILE.read_text().split() if "=" in t)
    assert float(rec["f32_score"]) == pytest.approx(worst, rel=0.5)


def test_reference_noise_is_measured_and_recorded(scenes):
    """s_model / s_score: the largest relative difference of H21 / F21 (Frobenius, unit norm, sign fixed) and of the score of a
    finite, well-conditioned hypothesis between the restatement and itself with each set's 8 pairs reversed, and with the null
    vector negated."""
    s_model = s_score = 0.0
    for id_, sc, r in scenes:
        for kw in (dict(reverse=True), dict(negate=True)):
            rr = ir.run(sc, **kw)
            ok = (r["status"] == ir.OK) & (rr["status"] == ir.OK) & ~r["ill"] & ~rr["ill"]
            if ok.any():
                s_model = max(s_model, float(ir.model_distance(rr["model"][ok], r["model"][ok]).max()))
                same = np.array([[np.array_equal(r["masks"][h][m], rr["masks"][h][m]) for m in (0, 1)] for h in range(len(ok))])
                if (ok & same).any():
                    s_score = max(s_score, float(ir.score_distance(rr["score"][ok & same], r["score"][ok & same]).max()))
    print("s_model", s_model, "s_score", s_score)
    rec_model, rec_score = ir.recorded()
    assert s_model > 0 and s_score > 0
    assert rec_model / 2 <= s_model <= rec_model * 2 and rec_score / 2 <= s_score <= rec_score * 2


def test_every_gpu_scene_keeps_within_the_two_caps(scenes):
    for id_, sc, r in scenes:
        ill, n_hyp, guard, n_dec = ir.caps(sc, r)
        print(id_, "ill-conditioned", ill, "of", n_hyp, "guard-band decisions", guard, "of", n_dec)
        if not ir.exempt(id_):
            assert ill <= ir.ILL_CAP * n_hyp, (id_, ill, n_hyp)
        assert guard <= ir.GUARD_CAP * n_dec, (id_, guard, n_dec)


def test_scene_list_covers_the_edges_and_the_engineered_cases(scenes):
    ids = {id_ for id_, _, _ in scenes}
    for kind in ir.KINDS:
        for sigma in (1, 2):
            assert {n for n in ir.PAIR_COUNTS if any(i.startswith(f"{kind}-n{n}-") and i.endswith(f"-s{sigma}") for i in ids)} == set(ir.PAIR_COUNTS)
    assert {f"general-n65-S{S}-sets" for S in ir.SET_COUNTS} <= ids and "general-n300-S200" in ids
    by = {id_: (sc, r) for id_, sc, r in scenes}
    assert [[p["n"] for p in by[i][0]["probs"]].index(0) for i in ("K3-empty-first", "K3-empty-middle", "K3-empty-last")] == [0, 1, 2]
    for sigma in (1, 2):
        sc, r = by[f"engineered-s{sigma}"]
        p = sc["probs"][0]
        tag = {name: h for h, name in p["tags"].items()}
        h = tag["coincident"]  # H singular -> zero H12 -> NaN score
        assert (p["pairs"][:8] == p["pairs"][0]).all() and not r["h12"][h].any() and np.isnan(r["score"][h, ir.MH])
        assert r["status"][h, ir.MH] == ir.NONFINITE and r["n_inliers"][h, ir.MH] == 0
        assert ir.replay(r["score"], ir.MH)[0] != h
        assert r["ill"][tag["collinear"]].all()
        assert not p["inlier"][list(ir.ENGINEERED["outliers"])].any() and p["inlier"][list(ir.ENGINEERED["inliers"])].all()
        # pair 32 under the all-inlier set's F: one chi-square in (3.841, 5.991), the other below 3.841 -- not an inlier, and
        # the other image's term is in the score
        h = tag["inliers"]
        c1, c2 = ir.chi_f(r["model"][h:h + 1, ir.MF], p["pairs"][32:33].astype(np.float64), p["sigma"])
        lo, hi = sorted((float(c1[0, 0]), float(c2[0, 0])))
        assert lo < ir.TH_F < hi < ir.TH_SCORE_F, (lo, hi)
        assert not r["masks"][h][ir.MF][32]
        rest = np.arange(p["n"]) != 32
        alone = ir.score_of(*ir.chi_f(r["model"][h:h + 1, ir.MF], p["pairs"][rest].astype(np.float64), p["sigma"]), ir.TH_F, ir.TH_SCORE_F)[1][0]
        assert r["score"][h, ir.MF] - alone == pytest.approx(ir.TH_SCORE_F - lo, rel=1e-9)
    sc, r = by["planar-n64-S1-s1"]  # a set of all inliers in an all-inlier scene: two full words
    assert r["n_inliers"][0, ir.MH] == 64 and r["masks"][0][ir.MH].all()
