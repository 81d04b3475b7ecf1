"""GPU: orbfe_pnp_* (k_pnp_ransac, k_pnp_refine) and the Python PnPsolver against the NumPy restatement tests/pnp_ref.py, under
the tolerance of profiles/pnp_tolerance.txt and the exclusion caps of pnp_ref.compare_item / check_caps."""
import numpy as np
import pytest

import pnp_ref as pr

pytestmark = pytest.mark.gpu

SCENES = pr.gpu_scenes()


def _cat(cands):
    off = np.concatenate([[0], np.cumsum([len(c["p3d"]) for c in cands])]).astype(np.int32)
    ho = np.concatenate([[0], np.cumsum([len(c["sets"]) for c in cands])]).astype(np.int32)
    return (off, np.concatenate([c["p3d"] for c in cands]), np.concatenate([c["p2d"] for c in cands]),
            np.concatenate([c["max_err"] for c in cands]), np.stack([c["cam"] for c in cands]), ho,
            np.concatenate([c["sets"].reshape(-1, 4) for c in cands]))


@pytest.fixture(scope="module")
def solved():
    """every scene through orbfe_pnp_solve_multi, once"""
    import orb_slam2_annotate_amd as amd
    return {id_: amd.pnp_solve_multi(*_cat(cands), [c["min_inliers"] for c in cands]) for id_, cands in SCENES}


@pytest.mark.parametrize("id_", [s[0] for s in SCENES])
def test_hypotheses_and_records_equal_the_restatement(solved, id_):
    cands = dict(SCENES)[id_]
    r = solved[id_]
    tol, st = pr.s_pnp(), pr.new_stats()
    h = rr = 0
    for k, c in enumerate(cands):
        n, w = len(c["p3d"]), (len(c["p3d"]) + 31) // 32
        counts = []
        for j, s in enumerate(c["sets"]):
            words = r["mask_words"][r["word_off"][k] + j * w: r["word_off"][k] + (j + 1) * w]
            pr.compare_item(c, pr.ref_item(c, s), (int(r["n_inliers"][h]), int(r["status"][h]), r["pose"][h], words), tol, st)
            counts.append(int(r["n_inliers"][h]))
            h += 1
        rec = pr.scan_records(counts, c["min_inliers"])
        h0 = h - len(c["sets"])
        assert [int(x) - h0 for x in r["rec_hyp"][r["rec_off"][k]:r["rec_off"][k + 1]]] == rec
        for j, hh in enumerate(rec):  # Refine on the kernel's own mask of that hypothesis
            mask = pr.words_to_mask(r["mask_words"][r["word_off"][k] + hh * w: r["word_off"][k] + (hh + 1) * w], n)
            words = r["rec_mask_words"][r["rec_word_off"][k] + j * w: r["rec_word_off"][k] + (j + 1) * w]
            pr.compare_item(c, pr.ref_item(c, np.flatnonzero(mask)),
                            (int(r["rec_n_inliers"][rr]), int(r["rec_status"][rr]), r["rec_pose"][rr], words), tol, st)
            rr += 1
    print(id_, st)
    if st["items"] >= 20:
        pr.check_caps(st, id_)
    else:
        assert st["excluded"] == 0 and st["guard"] == 0, st


@pytest.mark.parametrize("n_rec", [4, 5, 64, 255, 256, 257, 600])
def test_refine_records_of_every_size(n_rec):
    """A record of exactly n_rec correspondences (the workgroup's 256-lane trips: below, at and above one trip) of a
    600-point candidate, its indices spread over the candidate."""
    import orb_slam2_annotate_amd as amd
    c = pr.make_candidate(300 + n_rec, 600, 1, inlier_frac=1.0, noise=0.2)
    mask = np.zeros(600, bool)
    mask[np.random.default_rng(n_rec).choice(600, n_rec, replace=False)] = True
    if n_rec == 4:  # a well-spread minimal set
        mask[:] = False
        mask[c["sets"][0]] = True
    ni, st, pose, wo, words = amd.pnp_refine_multi([0, 600], c["p3d"], c["p2d"], c["max_err"], c["cam"], [0, 1], pr.mask_to_words(mask))
    stats = pr.new_stats()
    pr.compare_item(c, pr.ref_item(c, np.flatnonzero(mask)), (int(ni[0]), int(st[0]), pose[0], words), pr.s_pnp(), stats)
    print(n_rec, stats, int(ni[0]))
    assert stats["excluded"] == 0 and stats["guard"] == 0
    if n_rec >= 64:
        assert ni[0] >= 590  # the refined pose explains the scene


def test_multi_equals_single_calls_and_runs_are_identical():
    import orb_slam2_annotate_amd as amd
    cands = dict(SCENES)["k3_empty"]
    a = amd.pnp_ransac_multi(*_cat(cands))
    b = amd.pnp_ransac_multi(*_cat(cands))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    h = 0
    for k, c in enumerate(cands):
        ni, st, pose, words = amd.pnp_ransac(c["p3d"], c["p2d"], c["max_err"], c["cam"], c["sets"])
        H = len(c["sets"])
        assert ni.tobytes() == a[0][h:h + H].tobytes() and st.tobytes() == a[1][h:h + H].tobytes()
        assert pose.tobytes() == a[2][h:h + H].tobytes()
        assert words.tobytes() == a[4][a[3][k]:a[3][k + 1]].tobytes()
        h += H


def test_degenerate_sets_give_a_status_and_no_fault():
    """Two identical points in a set, and four coplanar points: statuses are compared, values are not."""
    import orb_slam2_annotate_amd as amd
    c = pr.make_candidate(400, 40, 2)
    c["p3d"][1], c["p2d"][1] = c["p3d"][0], c["p2d"][0]
    c["p3d"][4:8, 2] = np.float32(1.0)  # coplanar in the world
    c["p3d"][4:8, :2] = np.array([[0, 0], [1, 0], [0, 1], [1, 1]], np.float32)
    c["sets"] = np.array([[0, 1, 2, 3], [4, 5, 6, 7]], np.int32)
    ni, st, pose, words = amd.pnp_ransac(c["p3d"], c["p2d"], c["max_err"], c["cam"], c["sets"])
    for j in range(2):
        ref = pr.ref_item(c, c["sets"][j])
        assert int(st[j]) == (pr.OK if ref["finite"] else pr.NONFINITE)
        assert bool(np.all(np.isfinite(pose[j]))) == ref["finite"]
        if not ref["finite"]:
            assert ni[j] == 0 and not words[j].any()


def _exact_scene(seed=500, n=100, H=300):
    return pr.make_candidate(seed, n, H, inlier_frac=0.7, noise=0.0)


def test_replayed_iterate_equals_the_restatement_and_finds_the_true_inliers():
    """70 % exact inliers, gross outliers (>= 50 px): the replayed iterate() equals the restatement's stateful iterate() in
    bNoMore, the inlier set, nInliers, and in the pose within the tolerance; the inlier set is the true one."""
    import orb_slam2_annotate_amd as amd
    c = _exact_scene()
    kp = np.arange(len(c["p3d"])) * 2 + 1
    s = amd.PnPsolver(c["p3d"], c["p2d"], c["sigma2"], c["cam"], c["sets"], kp_indices=kp, n_keypoints=2 * len(kp) + 3)
    s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    ref = pr.Solver(c["p3d"], c["p2d"], c["sigma2"], c["cam"], c["sets"], kp_idx=kp, n_kp=2 * len(kp) + 3)
    assert (s.mRansacMinInliers, s.mRansacMaxIts) == (ref.min_inliers, ref.max_its)
    T, no_more, vb, n = s.iterate(5)
    Tr, no_more_r, vbr, nr = ref.iterate(5)
    assert no_more == no_more_r and n == nr and np.array_equal(vb, vbr) and T is not None and Tr is not None
    Tr = Tr.astype(np.float64)
    ok, d = pr.pose_close(np.concatenate([T[:3, :3].reshape(9), T[:3, 3]]), Tr[:9].reshape(3, 3), Tr[9:], pr.s_pnp())
    assert ok, (d, pr.s_pnp())
    truth = np.zeros(2 * len(kp) + 3, bool)
    truth[kp[c["truth"]]] = True
    assert np.array_equal(vb, truth) and n == int(c["truth"].sum())


def test_chain_into_pose_optimization():
    """Tracking::Relocalization (:1513-1530): the inliers and the pose of PnPsolver feed PoseOptimization."""
    import orb_slam2_annotate_amd as amd
    from orb_slam2_annotate_amd import optimizer
    c = pr.make_candidate(600, 120, 300, inlier_frac=0.7, noise=0.3)
    s = amd.PnPsolver(c["p3d"], c["p2d"], c["sigma2"], c["cam"], c["sets"])
    s.SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991)
    T, no_more, vb, n = s.iterate(5)
    assert T is not None and not no_more and n >= 0.9 * c["truth"].sum()
    K5 = np.array([*c["cam"], 40.0], np.float32)
    m = int(vb.sum())
    n_in, T_out, flags, stats, chi2 = optimizer.pose_optimization_batch([0, m], c["p3d"][vb], c["p2d"][vb, 0], c["p2d"][vb, 1],
                                                                       -np.ones(m, np.float32), 1.0 / c["sigma2"][vb], [K5], [T])
    assert n_in[0] >= 0.9 * m
    assert np.abs(T_out[0][:3, :3] - c["R"]).max() < 5e-3 and np.abs(T_out[0][:3, 3] - c["t"]).max() < 5e-2
