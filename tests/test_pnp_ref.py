"""CPU: the NumPy restatement tests/pnp_ref.py pinned by hand -- a noise-free scene recovers its pose, the canonical 4-point
basis spans the null space of M, the || loop of iterate(), SetRansacParameters -- and the proof that iterate() with its real,
stateful Refine() calls equals the replay over precomputed prefix-maximum records."""
from pathlib import Path

import numpy as np
import pytest

import pnp_ref as pr

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("n", [5, 6, 40, 300])
def test_noise_free_scene_recovers_its_pose(n):
    """(n = 4 is left out on purpose: five Gauss-Newton steps from the linearisations do not reach the pose from every
    4-set, in the reference as here, which is why RANSAC scores each hypothesis; the h300 scenes cover n = 4.)"""
    c = pr.make_candidate(7 + n, n, 1, inlier_frac=1.0, noise=0.0)
    # exact image points of the float32 world points, kept in float64
    pc = c["p3d"].astype(np.float64) @ c["R"].T + c["t"]
    uv = np.stack([float(c["cam"][0]) * pc[:, 0] / pc[:, 2] + float(c["cam"][2]),
                   float(c["cam"][1]) * pc[:, 1] / pc[:, 2] + float(c["cam"][3])], 1)
    idx = np.arange(n)
    R, t = pr.compute_pose(c["p3d"][idx].astype(np.float64), uv[idx], c["cam"])
    assert np.abs(R - c["R"]).max() < 1e-7 and np.abs(t - c["t"]).max() < 1e-6


def test_canonical_basis_spans_the_null_space_of_M():
    rng = np.random.default_rng(3)
    for _ in range(20):
        M = rng.normal(size=(8, 12))
        v = pr.null_basis4(M)
        assert np.abs(v @ v.T - np.eye(4)).max() < 1e-13
        assert np.abs(M @ v.T).max() < 1e-12
        Vt = np.linalg.svd(M)[2]
        P = Vt[8:].T @ Vt[8:]
        assert np.abs(v.T @ v - P).max() < 1e-12  # the projectors are equal
    # a continuous function of M where M has rank 8 and no reflector meets alpha = 0
    M = rng.normal(size=(8, 12))
    assert np.abs(pr.null_basis4(M) - pr.null_basis4(M + 1e-9 * rng.normal(size=(8, 12)))).max() < 1e-6
    # sign(0) = +1: the first reflector of a column (0, x) is that of (+0, x), v = (|x|, x)
    M[0, 0] = 0.0
    N = M.copy()
    N[0, 0] = 1e-300
    assert np.abs(pr.null_basis4(M) - pr.null_basis4(N)).max() < 1e-12


def test_set_ransac_parameters():
    got = {N: pr.set_ransac_parameters(N, 0.99, 10, 300, 4, 0.5, 5.991)[:2] for N in (4, 10, 19, 20, 21, 100)}
    # N = 4: minInliers 10 > N, epsilon 2.5, the log of a negative number: iterate() returns at :186 before the count is read
    # N = 10: minInliers == N gives 1.  N = 19: epsilon = 10 / 19 in float, ceil(log(0.01) / log(1 - eps^3)) = 30.
    # N = 20, 21: int(N * 0.5) = 10, epsilon 0.5: ceil(4.605 / 0.1335) = 35.  N = 100: minInliers 50, epsilon 0.5: 35.
    assert got == {4: (10, 1), 10: (10, 1), 19: (10, 30), 20: (10, 35), 21: (10, 35), 100: (50, 35)}
    from orb_slam2_annotate_amd import relocalization
    for N in got:
        assert relocalization.ransac_parameters(N, 0.99, 10, 300, 4, 0.5, 5.991) == got[N]


def test_loop_condition_is_or():
    """:195: the first iterate(5) runs until mnIterations reaches mRansacMaxIts unless a Refine succeeds."""
    c = pr.make_candidate(11, 60, 40, inlier_frac=0.2, noise=0.0)  # 12 inliers < minInliers = 30: nothing ever qualifies
    s = pr.Solver(c["p3d"], c["p2d"], c["sigma2"], c["cam"], c["sets"])
    assert s.min_inliers == 30 and s.max_its == 35
    T, no_more, vb, n = s.iterate(5)
    assert s.its == 35 and no_more and T is None and n == 0
    s2 = pr.Solver(c["p3d"], c["p2d"], c["sigma2"], c["cam"], c["sets"][:10])
    with pytest.raises(IndexError):
        s2.iterate(5)


SEEDS = [(500, 100, 300, 0.7, 0.0), (600, 120, 300, 0.7, 0.3), (601, 80, 300, 0.55, 0.5), (602, 50, 300, 0.6, 1.0),
         (603, 64, 300, 0.52, 0.8)]


@pytest.mark.parametrize("seed,n,H,frac,noise", SEEDS)
def test_stateful_iterate_equals_the_replay_over_prefix_maximum_records(seed, n, H, frac, noise):
    c = pr.make_candidate(seed, n, H, inlier_frac=frac, noise=noise)
    for params in [(0.99, 10, 300, 4, 0.5, 5.991), (0.99, 10, 300, 4, 0.9, 5.991)]:
        a = pr.Solver(c["p3d"], c["p2d"], c["sigma2"], c["cam"], c["sets"], params=params)
        hyp = [a.pose(s) for s in c["sets"]]
        counts = [int(m.sum()) for _, _, m in hyp]
        rec = pr.scan_records(counts, a.min_inliers)
        recs = [a.pose(np.flatnonzero(hyp[h][2])) for h in rec]
        b = pr.Replay(a.N, a.min_inliers, a.max_its, counts, [m for _, _, m in hyp], [pr.to_f32_pose(R, t) for R, t, _ in hyp], rec,
                      [int(m.sum()) for _, _, m in recs], [m for _, _, m in recs], [pr.to_f32_pose(R, t) for R, t, _ in recs])
        for _ in range(3):
            try:
                ra = a.iterate(5)
            except IndexError:
                with pytest.raises(IndexError):
                    b.iterate(5)
                break
            rb = b.iterate(5)
            assert ra[1] == rb[1] and ra[3] == rb[3] and np.array_equal(ra[2], rb[2])
            assert (ra[0] is None) == (rb[0] is None) and (ra[0] is None or np.array_equal(ra[0], rb[0]))
            assert a.its == b.its
        assert a.refine_calls >= len([h for h in rec if h < a.its]) or a.refine_calls == 0


def test_committed_scenes_stay_within_the_exclusion_caps():
    """the restatement ALONE: at most 5 % of a scene's items excluded by the guards"""
    for id_, cands in pr.gpu_scenes():
        items = excluded = 0
        for c in cands:
            for s in c["sets"]:
                r = pr.ref_item(c, s)
                items += 1
                excluded += bool(r["finite"] and (r["info"]["ill"] or r["info"]["flip"]))
        assert excluded <= 0.05 * items, (id_, excluded, items)


def test_reference_noise_is_measured_and_recorded():
    noise = pr.measure_noise(pr.gpu_scenes())
    txt = (ROOT / "profiles" / "pnp_tolerance.txt").read_text()
    rec = float([ln for ln in txt.split("\n") if ln.startswith("s_pnp=")][0].split("=")[1])
    print("measured", noise, "recorded", rec)
    assert noise <= rec * 1.0000001  # the recorded figure is this run's
    assert pr.s_pnp() == max(2.0 * float(np.finfo(np.float32).eps), 16.0 * rec)
