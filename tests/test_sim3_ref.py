"""CPU tests of tests/sim3_ref.py, the float64 restatement of Sim3Solver the GPU test compares with: known answers, the
reference's NaN case, SetRansacParameters, the selection without replacement, iterate's state on hand-made counts, and the
restatement's own noise and the two caps the GPU tolerance is built on (profiles/sim3_tolerance.txt)."""
from pathlib import Path

import numpy as np
import pytest

import sim3_ref as sr

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def scenes():
    return [(id_, sc, sr.run(sc)) for id_, sc in sr.gpu_scenes()]


def _three(fix_scale, s=None):
    s0, R, t = sr.planted(fix_scale)
    s = s0 if s is None else s
    X2 = np.array([[0.5, 0.2, 3.0], [-0.4, 0.3, 2.5], [0.1, -0.6, 4.0]])
    return s, R, t, (s * X2 @ R.T + t)[None], X2[None]


def test_planted_transform_comes_back_from_three_exact_pairs():
    s, R, t, P1, P2 = _three(False)
    r = sr.solve(P1, P2, False)
    assert np.abs(r["R"][0] - R).max() < 1e-13 and np.abs(r["t"][0] - t).max() < 1e-13 and abs(r["s"][0] - s) < 1e-13
    assert np.abs(r["T12"][0] - np.concatenate([s * R, t[:, None]], axis=1)).max() < 1e-13
    assert np.abs(r["T21"][0] - np.concatenate([R.T / s, -(R.T @ t)[:, None] / s], axis=1)).max() < 1e-13
    assert r["gap"][0] > 0.1


def test_fix_scale_forces_unit_scale():
    s, R, t, P1, P2 = _three(False)  # pairs that differ by s = 1.3
    r = sr.solve(P1, P2, True)
    assert r["s"][0] == 1.0 and np.abs(r["R"][0] - R).max() < 1e-13  # the rotation does not depend on the scale


def test_identical_sets_give_nan_and_no_inliers(scenes):
    _, _, _, _, P2 = _three(False)
    for fix in (False, True):
        r = sr.solve(P2, P2.copy(), fix)
        assert np.isnan(r["R"][0]).all() and np.isnan(r["t"][0]).all()
    for id_, sc, r in scenes:
        if id_.startswith("engineered"):
            tags = sc["cands"][0]["tags"]
            for h, name in tags.items():
                if name.startswith("identity") or name == "coincident":
                    assert r["status"][h] == sr.NONFINITE and r["n_inliers"][h] == 0 and not r["masks"][h].any(), (id_, name)
            h = [h for h, name in tags.items() if name == "inliers"][0]
            assert np.array_equal(r["masks"][h], sc["cands"][0]["inlier"]), id_  # every planted inlier and nothing else
            assert sc["cands"][0]["x1"][15, 2] < 0 and r["masks"][h][15]  # negative z, judged by the formula all the same
            h = [h for h, name in tags.items() if name == "outliers"][0]
            assert r["status"][h] == sr.OK and r["n_inliers"][h] < 6
    all_in = [r for id_, sc, r in scenes if id_.startswith("n64-H5")]
    assert all_in and all((r["n_inliers"] == 64).all() for r in all_in)  # every pair an inlier: a full ballot


def test_negated_eigenvector_gives_the_same_rotation():
    s, R, t, P1, P2 = _three(False)
    a, b = sr.solve(P1, P2, False), sr.solve(P1, P2, False, negate=True)
    assert np.abs(a["R"] - b["R"]).max() < 1e-14 and np.abs(a["t"] - b["t"]).max() < 1e-14


def test_max_iterations_against_hand_computed_values():
    # epsilon = 20/100 = 0.2f: ceil(log(0.01) / log(1 - 0.008)) = ceil(4.60517 / 0.00803217) = 574 -> min(., 300)
    assert sr.max_iterations(100, 0.99, 20, 300) == 300
    # epsilon = 0.5: ceil(4.60517 / 0.133531) = ceil(34.49) = 35
    assert sr.max_iterations(40, 0.99, 20, 300) == 35
    # epsilon = 0.8: ceil(4.60517 / 0.717440) = ceil(6.42) = 7
    assert sr.max_iterations(25, 0.99, 20, 300) == 7
    assert sr.max_iterations(40, 0.99, 20, 10) == 10
    assert sr.max_iterations(20, 0.99, 20, 300) == 1  # N == minInliers (:134)
    assert sr.max_iterations(19, 0.99, 20, 300) == 1  # N < minInliers: answered before the formula
    assert sr.max_iterations(0, 0.99, 6, 300) == 1
    assert sr.max_iterations(21, 0.99, 20, 300) == 3  # epsilon = 0.952381f: ceil(4.60517 / 1.99) = 3


def test_triples_from_draws_against_a_literal_list_pop():
    n = 7
    draws = np.array([[0, 0, 0], [6, 5, 4], [6, 0, 0], [3, 3, 3], [0, 5, 0]])
    # by hand: [0..6]; (0,0,0): 0, then 6 stands at 0 -> 6, then 5 -> 5.  (6,5,4): 6, 5, 4.  (6,0,0): 6, 0, then 5 at 0 -> 5.
    # (3,3,3): 3, then 6 at 3 -> 6, then 5 at 3 -> 5.  (0,5,0): 0 (6 moves to 0), [6,1,2,3,4,5][5] = 5, then 6.
    assert sr.triples_from_draws(n, draws).tolist() == [[0, 6, 5], [6, 5, 4], [6, 0, 5], [3, 6, 5], [0, 5, 6]]
    rng = np.random.default_rng(1)
    d = np.stack([rng.integers(0, 50 - i, 200) for i in range(3)], axis=1)
    t = sr.triples_from_draws(50, d)
    assert ((t[:, 0] != t[:, 1]) & (t[:, 0] != t[:, 2]) & (t[:, 1] != t[:, 2])).all() and t.min() >= 0 and t.max() < 50


def _solver(counts, min_inliers, max_its=None, N=30, N1=40):
    counts = np.array(counts)
    masks = [np.arange(N) < c for c in counts]
    return sr.RefSolver(counts, masks, np.arange(N) + 5, N1, min_inliers, len(counts) if max_its is None else max_its)


def test_iterate_replay_on_hand_made_counts():
    # return on the first count > min; == min does not return
    s = _solver([3, 20, 20, 21, 25], 20)
    h, no_more, vb, n = s.iterate(5)
    assert (h, no_more, n) == (3, False, 21) and vb.sum() == 21 and vb[5:26].all() and s.iterations == 4
    # state carried across calls: the next call goes on behind it, and a later acceptance follows the earlier one
    h, no_more, vb, n = s.iterate(5)
    assert (h, no_more, n) == (4, False, 25) and s.iterations == 5 and s.best_inliers == 25
    h, no_more, vb, n = s.iterate(5)
    assert h is None and no_more and n == 0 and not vb.any()
    # bNoMore on exactly the last iteration, not before
    s = _solver([1, 2, 3, 4, 5, 6], 20)
    assert s.iterate(5)[:2] == (None, False) and s.iterations == 5
    assert s.iterate(5)[:2] == (None, True) and s.iterations == 6
    # a hypothesis below the best so far is not taken even if it is above min
    s = _solver([25, 22, 25], 20)
    assert s.iterate(1)[0] == 0 and s.iterate(1)[0] is None and s.iterate(1)[0] == 2 and s.best == 2  # >= takes the tie
    # N < minInliers: bNoMore at once, nothing is counted
    s = _solver([30, 30], 31)
    assert s.iterate(5)[:2] == (None, True) and s.iterations == 0
    # a NONFINITE hypothesis has 0 inliers and is the best so far by >= while the best is 0
    s = _solver([0, 0, 7], 6)
    assert s.iterate(2)[0] is None and s.best == 1 and s.iterate(2)[0] == 2


def test_reference_noise_is_measured_and_recorded(scenes):
    """s_sim3: the largest relative difference of R (Frobenius), t and s of a finite, well-conditioned hypothesis between the
    restatement and itself with the three pairs reversed, and with the eigenvector negated."""
    s = 0.0
    for id_, sc, r in scenes:
        for kw in (dict(reverse=True), dict(negate=True)):
            rr = sr.run(sc, **kw)
            assert np.array_equal(r["status"], rr["status"]), id_
            ok = (r["status"] == sr.OK) & (r["gap"] >= sr.ILL_GAP)
            for err, mag in sr.sim3_errors(rr["sim3"][ok], r["sim3"][ok]):
                if len(err):
                    s = max(s, float((err / mag).max()))
    rec = dict(line.split("=") for line in (ROOT / "profiles" / "sim3_tolerance.txt").read_text().split() if "=" in line)
    assert s > 0 and float(rec["s_sim3"]) == pytest.approx(s, rel=1e-6, abs=0)


def test_every_gpu_scene_keeps_within_the_two_caps(scenes):
    for id_, sc, r in scenes:
        ill, n_hyp, guard, n_dec = sr.caps(sc, r)
        assert ill <= sr.ILL_CAP * n_hyp, (id_, ill, n_hyp)
        assert guard <= sr.GUARD_CAP * n_dec, (id_, guard, n_dec)


def test_scene_sizes_are_the_word_ballot_and_workgroup_edges(scenes):
    ids = {id_ for id_, _, _ in scenes}
    for fix in (0, 1):
        for n in sr.PAIR_COUNTS:
            for H in sr.HYP_COUNTS:
                assert f"n{n}-H{H}-fix{fix}" in ids
    for id_, sc, r in scenes:
        if id_.startswith("K3"):
            assert [len(c["triples"]) for c in sc["cands"]] == [37, 0, 5] and len({c["n"] for c in sc["cands"]}) == 3
        assert all(len(set(c["max1"].tolist())) > 1 for c in sc["cands"])  # mixed octaves: maxErr varies per pair
