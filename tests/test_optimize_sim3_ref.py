"""CPU tests of tests/optimize_sim3_ref.py, the float64 restatement of Optimizer::OptimizeSim3 the GPU test compares with:
known answers, the two-round rules, the conditions on the GPU test's scenes, the reordering noise the GPU tolerance is built
on and the distance to g2o's numeric Jacobian (profiles/optimize_sim3_tolerance.txt), and the stale-error search.

The stale-error search (seeds 0 .. STALE_SEEDS-1 of every STALE_SHAPES size, fix_scale 0 / 1, 0 % / 20 % outliers, with the
scenes' start and with a five times harder one) finds NO round that ends on a rejected trial AND classifies a pair otherwise
on the recomputed chi2 (STALE_SEED = None).  Rounds that end on a rejected trial do occur, but only after ten rejections in a
row, when lambda has grown by 2^45 and the rejected step is noise: the stale and the recomputed chi2 then differ far inside
the GPU tolerance, and no test discriminates the rule "a classification reads the error of the last evaluated trial".  It is
implemented as the reference states it."""
import numpy as np
import pytest

import optimize_sim3_check as chk
import optimize_sim3_ref as osr


@pytest.fixture(scope="module")
def scenes():
    return [(id_, sc, osr.run(sc)) for id_, sc in osr.gpu_scenes()]


def _rts_error(sim3, sc):
    R, t, s = osr.sim3_to_Rts(sim3)
    Rt, tt, st = sc["sim3_true"]
    return max(np.abs(R - Rt).max(), np.abs(t - tt).max(), abs(s - st))


def test_zero_noise_recovers_the_planted_transform_and_erases_exactly_the_planted():
    # tolerance: X1, X2 rounded to float32 at depths of up to 40 m (2e-6 m) and observations at ~1000 px (6e-5 px over 700 px)
    for fix in (0, 1):
        sc = osr.scene(0, 200, fix, 0.2, noise_px=0.0)
        for jac in ("analytic", "numeric"):
            r = osr.run(sc, jacobian=jac)
            assert r["rounds"] == 2 and r["n_bad"] == int(sc["planted"].sum())
            assert np.array_equal(r["bad"] != 0, sc["planted"]) and r["n_in"] == int((~sc["planted"]).sum())
            assert _rts_error(r["sim3"], sc) < 1e-4, (fix, jac, _rts_error(r["sim3"], sc))


def test_no_pair_nothing_happens():
    sc = osr.scene(0, 0, 0, 0.0)
    r = osr.run(sc)
    assert r["n_in"] == 0 and r["rounds"] == 0 and r["iterations"] == [] and len(r["bad"]) == 0
    q, t, s = osr.sim3_from_record(sc["sim3_in"])
    assert np.array_equal(r["sim3"], np.array(q + t + [s]))


def test_nine_pairs_run_round_one_and_return_zero_with_the_incoming_transform():
    sc = osr.scene(0, 9, 0, 0.2)
    r = osr.run(sc)
    assert r["rounds"] == 1 and r["iterations"][0] >= 1 and r["n_in"] == 0
    assert r["n_bad"] == int((r["bad"] == 1).sum()) > 0  # the erasures of round one stay
    q, t, s = osr.sim3_from_record(sc["sim3_in"])
    assert np.array_equal(r["sim3"], np.array(q + t + [s]))


def test_fourteen_pairs_of_which_nine_survive_return_zero():
    sc = osr.early_scene(osr.EARLY[1])
    r = osr.run(sc)
    assert r["rounds"] == 1 and r["n_in"] == 0 and r["n_bad"] == 5
    assert int((r["bad"] == 1).sum()) == 5 and np.array_equal(r["bad"] != 0, sc["planted"])
    q, t, s = osr.sim3_from_record(sc["sim3_in"])
    assert np.array_equal(r["sim3"], np.array(q + t + [s]))


def test_second_round_runs_five_iterations_without_erasures_and_up_to_ten_with(scenes):
    seen = set()
    for id_, sc, r in scenes:
        if r["rounds"] < 2:
            continue
        assert r["iterations"][0] <= 5, id_
        assert r["iterations"][1] <= (10 if r["n_bad"] > 0 else 5), id_
        seen.add(r["n_bad"] > 0)
    assert seen == {False, True}
    # (neither cap is the binding rule in these scenes: the stop rule -- three iterations that gain less than 0.1 % -- ends
    # the second round after three or four iterations; the caps are the loop bounds of the restatement and of the kernel)


def test_fix_scale_keeps_the_scale_bit_for_bit():
    for seed, n in ((0, 64), (1, 129)):
        sc = osr.scene(seed, n, 1, 0.2)
        for jac in ("analytic", "numeric"):
            r = osr.run(sc, jacobian=jac)
            assert r["rounds"] == 2 and r["sim3"][7] == float(sc["sim3_in"][12]), jac
    sc = osr.scene(0, 64, 0, 0.2)
    assert osr.run(sc)["sim3"][7] != float(sc["sim3_in"][12])


def test_stale_error_search():
    found, rejected = None, 0
    for start in ((0.03, 0.03, 0.05), (0.15, 0.15, 0.5)):
        for n in osr.STALE_SHAPES:
            for fix in (0, 1):
                for of in osr.OUTLIERS:
                    for seed in range(osr.STALE_SEEDS):
                        r = osr.run(osr.scene(seed, n, fix, of, start=start))
                        rejected += any(r["last_rejected"])
                        if found is None and any(a and b for a, b in zip(r["last_rejected"], r["fresh_differs"])):
                            found = (start, n, fix, of, seed)
    assert found == osr.STALE_SEED
    assert rejected > 0  # rounds that end on a rejected trial were among the searched


def test_every_gpu_scene_meets_the_conditions_on_the_scenes(scenes):
    """No guard violation, and the same bad[], n_in, iterations and trials for forward / reversed sums and for the analytic /
    numeric Jacobian: a property of the reference alone, for which the seeds of optimize_sim3_ref.SEEDS were chosen."""
    assert [id_ for id_, _, _ in scenes] == [id_ for id_, _ in osr.gpu_scenes()] and len(scenes) == 37
    for id_, sc, r in scenes:
        assert not osr.guard_violations(sc, r), id_
        for kw in (dict(reverse=True), dict(jacobian="numeric"), dict(reverse=True, jacobian="numeric")):
            x = osr.run(sc, **kw)
            assert np.array_equal(r["bad"], x["bad"]) and r["n_in"] == x["n_in"], (id_, kw)
            assert r["iterations"] == x["iterations"] and r["trials"] == x["trials"] and r["rounds"] == x["rounds"], (id_, kw)


def measure(scenes):
    s_sim3 = s_chi2 = j_gap = 0.0
    for id_, sc, r in scenes:
        rr, rn = osr.run(sc, reverse=True), osr.run(sc, jacobian="numeric")
        s_sim3 = max(s_sim3, float(np.abs(r["sim3"] - rr["sim3"]).max()))
        j_gap = max(j_gap, float(np.abs(r["sim3"] - rn["sim3"]).max()))
        for key in ("chi2_12", "chi2_21"):
            a, b = r[key], rr[key]
            assert np.array_equal(a == 0, b == 0), id_
            s_chi2 = max(s_chi2, float((np.abs(a - b)[a != 0] / np.abs(a[a != 0])).max(initial=0.0)))
    return dict(s_sim3=s_sim3, s_chi2=s_chi2, j_gap=j_gap)


def test_reordering_noise_and_jacobian_gap_are_measured_and_recorded(scenes):
    """s_sim3 / s_chi2: the reference against itself with the H / b / chi2 sums in reversed order.  j_gap: analytic against
    g2o's numeric Jacobian -- the distance to g2o's own numerics, recorded and quoted in DESIGN 4.O, not a tolerance."""
    rec = chk.recorded()
    for key, val in measure(scenes).items():
        assert rec[key] == pytest.approx(val, rel=1e-6, abs=0), key
