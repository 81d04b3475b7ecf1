"""CPU: the restatement of Optimizer::OptimizeEssentialGraph (tests/essgraph_ref.py) checked against itself: log against exp on
the four branches of Sim3::log, the analytic Jacobians against a central difference of the restated error, the symbolic
elimination against the sparse route's own fill, the scenes' distance from summation noise, and the analytic form of the
Jacobians against g2o's difference quotient (delta 1e-9) over whole runs."""
import math

import numpy as np
import pytest

import essgraph_ref as er
from essgraph_check import TOLERANCE_FILE, agrees, recorded

SCENES = er.scenes()


@pytest.mark.parametrize("u,branch", [
    ([0.3, -0.2, 0.5, 1.0, 2.0, 3.0, 0.2], (False, False)),
    ([1e-7, 0.0, -2e-7, 1.0, 2.0, 3.0, 0.2], (False, True)),
    ([0.3, -0.2, 0.5, 1.0, 2.0, 3.0, 1e-7], (True, False)),
    ([1e-7, 0.0, 1e-7, 1.0, -2.0, 3.0, 0.0], (True, True)),
    ([2.0, 1.5, -1.2, 30.0, -20.0, 10.0, -0.8], (False, False)),
])
def test_log_inverts_exp_on_every_branch(u, branch):
    u = np.array(u)
    S = er.sim3_exp(u)
    assert er.log_branch(S) == branch
    # exp and log round a handful of times each; the 3 x 3 solve is well conditioned: 1e-12 of the largest component
    assert np.abs(er.sim3_log(S) - u).max() <= 1e-12 * max(1.0, np.abs(u).max())


def _random_edge(rng, err_scale):
    Si = er.sim3_exp(rng.normal(size=7) * [1, 1, 1, 10, 10, 10, 0.3])
    Sj = er.sim3_exp(rng.normal(size=7) * [1, 1, 1, 10, 10, 10, 0.3])
    C = er.sim3_mul(er.sim3_exp(np.asarray(err_scale) * rng.normal(size=7)), er.sim3_mul(Sj, er.sim3_inverse(Si)))
    return C, Si, Sj


@pytest.mark.parametrize("err_scale,branch", [
    ([0.5, 0.5, 0.5, 3, 3, 3, 0.2], (False, False)),      # the general branch, metres in upsilon
    ([0.5, 0.5, 0.5, 3, 3, 3, 0.0], (True, False)),       # |sigma| < eps: upsilon is solved with the coefficients of sigma = 0
    ([0.0, 0.0, 0.0, 3, 3, 3, 0.0], (True, True)),        # both small: an edge between two consistent key frames of scale 1
    ([0.0, 0.0, 0.0, 3, 3, 3, 0.2], (False, True)),       # a consistent rotation under a scale correction
    ([1e-3, 1e-3, 1e-3, 3, 3, 3, 0.0], (True, True)),     # a small but visible angle: omega = deltaR / 2, A and B frozen
    ([1e-3, 1e-3, 1e-3, 1, 1, 1, 0.05], (False, True)),   # the same under a scale error: B of sim3.h:199, ~ 1 / sigma^3
])
@pytest.mark.parametrize("fix_scale", [False, True])
def test_analytic_jacobian_equals_the_central_difference(err_scale, branch, fix_scale):
    """delta 1e-6.  The analytic form differentiates Sim3::log as it is computed, branch by branch, so only the difference
    quotient's own error is allowed: truncation delta^2 |f(3)| / 6 and rounding 1e-16 |e| / delta, both below 1e-8 of the
    largest entry while the higher derivatives are of the order of J.  In the branch sigma >= eps, d > 1 - eps they are not:
    B = (sigma^2 / 2 - sigma + 1) s / sigma^3 (sim3.h:199, the closed form without its '- 1') makes upsilon vary like
    theta^2 / sigma^3 and every derivative by sigma gains another 1 / sigma, so the truncation term is delta^2 / sigma^2 of J.
    A draw of that branch with |sigma| < 0.01 is passed over (1e-8 there), and the bound is 2e-5 of max(1, |J|) throughout:
    three orders above the quotient's error, two below the 5e-3 (upsilon / 2 in column 6) by which a Jacobian of the true
    logarithm misses in the |sigma| < eps branch."""
    rng = np.random.default_rng(7)
    checked = 0
    for _ in range(8):
        C, Si, Sj = _random_edge(rng, err_scale)
        E = er.sim3_mul(er.sim3_mul(C, Si), er.sim3_inverse(Sj))
        assert er.log_branch(E) == branch
        if branch == (False, True) and abs(math.log(E[2])) < 0.01:
            continue
        _, Ji, Jj = er.jac_analytic(C, Si, Sj, fix_scale)
        _, Ni, Nj = er.jac_numeric(C, Si, Sj, fix_scale, delta=1e-6)
        tol = 2e-5 * max(1.0, np.abs(Ni).max(), np.abs(Nj).max())
        print(branch, fix_scale, np.abs(Ji - Ni).max(), np.abs(Jj - Nj).max(), tol)
        assert np.abs(Ji - Ni).max() <= tol and np.abs(Jj - Nj).max() <= tol
        if fix_scale:
            assert not Ji[:, 6].any() and not Jj[:, 6].any() and not Ni[:, 6].any() and not Nj[:, 6].any()
        checked += 1
    assert checked >= 4


@pytest.fixture(scope="module")
def runs():
    return {id_: er.run(sc) for id_, sc, _ in SCENES}


def test_symbolic_elimination_counts_the_fill_of_the_sparse_route():
    for id_, sc, _ in SCENES[:5]:
        free_of, active, blocks = er.block_pattern(sc)
        nF = int((free_of >= 0).sum())
        H, b, _ = er.linearise(sc, [er.from_record(r) for r in sc["sim3"]], er.measurements(sc), free_of, active, "analytic", active)
        x, blocks_L = er.sparse_cholesky_solve(H + 1e-6 * np.eye(7 * nF), b, nF)
        assert blocks_L == er.count_blocks_L(nF, blocks), id_
        assert np.abs(x - np.linalg.solve(H + 1e-6 * np.eye(7 * nF), b)).max() <= 1e-9 * max(1.0, np.abs(x).max()), id_


def test_scenes_decide_well_above_summation_noise(runs):
    """every accept / reject of the restatement's run is decided by more than 1e-9 of max(currentChi, 1): a scene that is not
    is changed here, on the CPU, before it reaches a GPU"""
    for id_, sc, discrete in SCENES:
        if discrete:
            print(id_, runs[id_]["min_gap"])
            assert runs[id_]["min_gap"] > 1e-9, (id_, runs[id_]["min_gap"])


def test_scenes_reach_the_branches_they_are_built_for(runs):
    seen = {}
    for id_, sc, _ in SCENES:
        S, meas = [er.from_record(r) for r in sc["sim3"]], er.measurements(sc)
        seen[id_] = {er.log_branch(er.sim3_mul(er.sim3_mul(meas[e], S[sc["edge_i"][e]]), er.sim3_inverse(S[sc["edge_j"][e]])))
                     for e in range(len(sc["edge_i"]))}
    assert seen["chain5"] == {(True, True)}
    assert (False, False) in seen["ring12"] and (True, True) in seen["ring12"]
    assert runs["ring12"]["blocks_L"] > runs["ring12"]["blocks_A"]  # fill rows
    assert runs["ring12"]["chi2"] > 1e-3                             # a non-zero minimum
    assert runs["chain5"]["chi2"] < 1e-20 < runs["chain5"]["chi2_initial"]
    assert runs["chain5_mid_fixed_isolated"]["n_free"] == 5
    big = SCENES[5][1]
    assert runs["chain150_band3_two_loops"]["n_free"] > 64 and runs["chain150_band3_two_loops"]["blocks_L"] > 256
    assert np.abs(big["sim3"][:, 4:7]).max() > 25.0
    # the 170-degree relative rotation of the edge 70 -> 71
    q = er.sim3_mul(er.from_record(big["sim3_meas"][71]), er.sim3_inverse(er.from_record(big["sim3_meas"][70])))[0]
    assert 2.0 * math.degrees(math.acos(min(1.0, abs(q[3]) / np.linalg.norm(q)))) > 160.0


def test_analytic_and_g2o_form_take_the_same_decisions(runs):
    """the same iteration and trial counts; the largest difference of sim3_out is j_gap in profiles/essential_graph_tolerance.txt,
    the documented distance to g2o's numerics.  Both forms end the ring at iteration 2 with ten rejected trials: after the
    first step its edges sit in the branch sigma >= eps, d > 1 - eps of Sim3::log (sim3.h:199).  A Jacobian of the true
    logarithm took 4 iterations / 4 trials there and parted from g2o by 0.05; the one used differentiates what is computed."""
    measured = {}
    bad = []
    for id_, sc, discrete in SCENES:
        if not discrete or id_.startswith("chain150"):  # (the 150-vertex scene costs 13 s in the difference-quotient form)
            continue
        g = er.run(sc, jac="g2o")
        measured[f"{id_}.j_gap"] = float(np.abs(g["sim3_out"] - runs[id_]["sim3_out"]).max())
        print(id_, "analytic", runs[id_]["iterations"], runs[id_]["trials"], "g2o", g["iterations"], g["trials"], measured[f"{id_}.j_gap"])
        if (g["iterations"], g["trials"]) != (runs[id_]["iterations"], runs[id_]["trials"]):
            bad.append((id_, runs[id_]["iterations"], runs[id_]["trials"], g["iterations"], g["trials"]))
    rec = {k: v for k, v in recorded().items() if k.endswith(".j_gap")}
    assert set(rec) == set(measured), f"{TOLERANCE_FILE.name} lists other scenes than the test measures"
    off = {k: (measured[k], rec[k]) for k in rec if not agrees(measured[k], rec[k])}
    assert not off, f"{TOLERANCE_FILE.name} disagrees with what is measured: {off}"
    assert not bad, bad
