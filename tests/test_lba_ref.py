"""CPU: self-checks of the restatement of LocalBundleAdjustment / BundleAdjustment (tests/lba_ref.py) and of the scenes the GPU
test compares on: the Jacobians against central differences, the Schur route against the full dense system, a noise-free
scene staying put, planted gross outliers found exactly, and the condition every comparison scene keeps."""
import numpy as np
import pytest

import lba_ref as lr
from pose_opt_ref import se3_exp, se3_mul, to_se3quat


@pytest.fixture(scope="module")
def results():
    return {id_: (sc, kind, lr.run(sc, kind)) for id_, sc, kind in lr.gpu_scenes()}


def test_jacobians_equal_central_differences():
    sc = lr.scene(5, 2, 2, 12, stereo_fraction=0.5)
    G = lr.Graph(sc)
    poses = [to_se3quat(G.T[j]) for j in range(G.nT)]
    pts = sc["xw"].astype(np.float64)

    def err(ps, xs):
        Q = np.array([p[0] for p in ps])[G.ep]
        Tt = np.array([p[1] for p in ps])[G.ep]
        X = xs[G.ept]
        x, y, z = lr.quat_rotate([Q[:, k] for k in range(4)], X[:, 0], X[:, 1], X[:, 2])
        x, y, z = x + Tt[:, 0], y + Tt[:, 1], z + Tt[:, 2]
        p0 = x / z * G.fx + G.cx
        return np.stack([G.u - p0, G.v - (y / z * G.fy + G.cy), np.where(G.stereo, G.ur - (p0 - G.bf / z), 0.0)], axis=1)
    _, _, _, Jp, Jl = G.errors(poses, pts, True)
    h = 1e-6
    for k in range(6):
        d = np.zeros(6)
        d[k] = h
        plus = [se3_mul(se3_exp(list(d)), p) for p in poses]
        minus = [se3_mul(se3_exp(list(-d)), p) for p in poses]
        num = (err(plus, pts) - err(minus, pts)) / (2 * h)
        for r in range(3):
            assert np.allclose(num[:, r], Jp[r][k], rtol=1e-5, atol=1e-4), (k, r)
    for k in range(3):
        d = np.zeros(3)
        d[k] = h
        num = (err(poses, pts + d) - err(poses, pts - d)) / (2 * h)
        for r in range(3):
            assert np.allclose(num[:, r], Jl[r][k], rtol=1e-5, atol=1e-4), (k, r)


def test_schur_route_equals_the_dense_system():
    sc = lr.scene(6, 3, 2, 25, stereo_fraction=0.3)
    G = lr.Graph(sc)
    poses = [to_se3quat(G.T[j]) for j in range(G.nT)]
    _, _, H, b, _, _, n6 = G.build(poses, sc["xw"].astype(np.float64), np.ones(G.nE, bool), True, False)
    lam = 1e-5 * np.abs(np.diag(H)).max()
    ok, x = lr.dense_solve(H, lam, b)
    assert ok and n6 == 18
    xs = lr.schur_solve(H, lam, b, n6)
    assert np.allclose(xs, x, rtol=1e-8, atol=1e-12 * np.abs(x).max())


def test_noise_free_scene_stays_put():
    sc = lr.scene(7, 2, 2, 30, noise_px=0.0, start_rot=0.0, start_trans=0.0, start_point=0.0)
    res = lr.adjust(sc)
    assert not res["erase"].any()
    assert np.abs(res["Tcw"] - sc["Tcw_true"][:2]).max() < 1e-5 and np.abs(res["xw"] - sc["xw"]).max() < 1e-3


def test_planted_gross_outliers_are_erased_exactly_and_the_poses_recovered():
    outl = tuple((j % 5, 3 * j + 1, 120) for j in range(8))
    sc = lr.scene(9, 3, 2, 60, noise_px=0.2, outliers=outl, vis_prob=1.0)  # every pose sees every point: one bad edge of five
    res = lr.adjust(sc)
    assert np.array_equal(res["erase"] != 0, sc["planted"])
    assert np.abs(res["Tcw"] - sc["Tcw_true"][:3]).max() < 5e-3


def test_every_comparison_scene_keeps_the_condition(results):
    """no chi2 within 1e-6 (relative) of a threshold and no depth within 1e-6 of 0 at either classification, no rho within 1e-9
    of 0; and at least two fixed poses, or one plus stereo edges"""
    for id_, (sc, kind, res) in results.items():
        assert lr.guard_ok(res), (id_, res["guard"], res["min_rho"])
        G = lr.Graph(sc)
        assert (~G.free).sum() >= 2 or ((~G.free).sum() == 1 and G.stereo.any()), id_


def test_the_engineered_scenes_are_what_their_names_say(results):
    sc, _, res = results["point-all-level1"]
    on4 = sc["edge_point"] == 4
    assert res["level1"][on4].all() and not res["level1"][~on4].all()
    sc, _, res = results["pose-all-level1"]
    assert res["level1"][sc["edge_pose"] == 2].all()
    sc, _, res = results["behind-camera"]
    flipped = sc["edge_pose"] == 4
    assert (res["erase"][flipped] == 1).all() and (res["edge_chi2"][flipped] < 5.991).all()  # the depth alone decides
    assert results["l3f2p40-mixed"][2]["rejected"] >= 1
    assert results["l7f5p300"][2]["stale_decides"] >= 1  # level 1 on the round-one chi2; at the final estimates it would pass
    assert results["no-progress"][2]["termination"][1] == lr.END["no_progress"]
    assert results["local-is-fixed"][2]["Tcw"].shape == (3, 4, 4)
    for k in (63, 64, 65):
        sc = results[f"pose-edges-{k}"][0]
        assert (sc["edge_pose"] == 0).sum() == k
        sc = results[f"pair-shares-{k}"][0]
        assert len(np.intersect1d(sc["edge_point"][sc["edge_pose"] == 0], sc["edge_point"][sc["edge_pose"] == 1])) == k
    sc = results["pair-shares-0"][0]
    assert len(np.intersect1d(sc["edge_point"][sc["edge_pose"] == 0], sc["edge_point"][sc["edge_pose"] == 1])) == 0
    sc = results["point-fixed-plus-one"][0]
    assert sorted(sc["edge_pose"][sc["edge_point"] == 0].tolist()) == [0, 2, 3]
    sc, _, res = results["depth-final-only"]
    e0 = np.flatnonzero((sc["edge_pose"] == 0) & (sc["edge_point"] == 0))[0]
    # level 0 after round one, a chi2 far below the threshold at the final test: only !isDepthPositive() erases it
    assert res["level1"][e0] == 0 and res["erase"][e0] == 2 and res["edge_chi2"][e0] < 1.0
    assert results["far-start-outliers"][2]["stale_decides"] >= 1


@pytest.mark.parametrize("k", [0, 2, 5, 8])
def test_stop_flag_raised_before_iteration_k(results, k):
    sc, kind, full = results["l3f2p40-mixed"]
    res = lr.run(sc, kind, stop_before=k)
    assert res["stopped"] == 1 and sum(res["iterations"]) == min(k, sum(full["iterations"]))
    if k == 0:
        assert res["rounds"] == 0 and not res["erase"].any() and np.array_equal(res["xw"], sc["xw"].astype(np.float64))
    elif k <= 5:
        assert res["iterations"][1] == 0 and not res["level1"].any() and (res["erase"] != 1).all()
