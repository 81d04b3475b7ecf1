"""CPU: properties of the float64 restatement tests/initializer_reconstruct_ref.py of ReconstructH / ReconstructF / CheckRT: the
seeds keep every scene free of guard-band cases, its own noise (recorded in profiles/initializer_reconstruct_tolerance.txt), the
planted motion, the engineered cases and a float32 transcription of CheckRT's decisions."""
import numpy as np
import pytest

import initializer_ref as ir
import initializer_reconstruct_ref as rr


@pytest.fixture(scope="module")
def scenes():
    return rr.scenes()


def test_seeds_are_the_first_without_a_guard_band_case(scenes):
    for id_, sc, r in scenes:
        assert rr.guard_count(r) == (0, 0), id_
        assert rr.find_seed(id_) == rr.SEEDS[id_], id_


def test_reference_noise_is_measured_and_recorded(scenes):
    """s_motion / s_point / s_cos: the largest |R - R'|_F + |t - t'| of matched hypotheses, |X - X'|_inf / |X| of a counted
    point and relative difference of the selected cosine between the restatement and itself with the rows of every 4 x 4 A
    reversed, and with the singular vectors of the 3 x 3 SVD negated.  The decisions must not move at all."""
    s = [0.0, 0.0, 0.0]
    for id_, sc, r in scenes:
        for kw in (dict(reverse=True), dict(negate=True)):
            for a, b in zip(r, rr.run(sc, **kw)):
                assert a["status"] == b["status"] and a["success"] == b["success"], id_
                if a["status"] == rr.DEGENERATE:
                    continue
                perm = rr.match(np.array([h["R"] for h in b["hyps"]]), np.array([h["t"] for h in b["hyps"]]), a["hyps"], 4)
                for i, j in enumerate(perm):
                    hb, ha = b["hyps"][i], a["hyps"][j]
                    s[0] = max(s[0], rr.motion_distance(hb["R"], hb["t"], ha["R"], ha["t"]))
                    assert np.array_equal(hb["flags"], ha["flags"]), (id_, kw)
                    c = (ha["flags"] & rr.COUNTED) != 0
                    if c.any():
                        s[1] = max(s[1], float((np.abs(hb["X"][c] - ha["X"][c]).max(1) / np.linalg.norm(ha["X"][c], axis=1)).max()))
                    if ha["n_good"]:
                        s[2] = max(s[2], abs(hb["cos_sel"] - ha["cos_sel"]) / abs(ha["cos_sel"]))
    print("s_motion", s[0], "s_point", s[1], "s_cos", s[2])
    for got, rec in zip(s, rr.recorded()):
        assert rec / 2 <= got <= rec * 2, (s, rr.recorded())
    assert s[1] > 0 and s[2] > 0


def test_restatement_recovers_the_planted_motion(scenes):
    seen = 0
    for id_, sc, r in scenes:
        for p, pr in zip(sc["probs"], r):
            if p["truth"] is None or pr["status"] == rr.DEGENERATE or not p["mask"].any():
                continue
            R, t = p["truth"]
            d = [rr.motion_distance(h["R"], h["t"], R, t) for h in pr["hyps"]]
            j = int(np.argmin(d))
            assert d[j] < 1e-4, (id_, d)  # float32 coordinates
            assert pr["hyps"][j]["n_good"] == int(p["mask"].sum()) - (1 if id_ == "nonfinite" else 0), id_
            for h in pr["hyps"]:
                assert abs(np.linalg.det(h["R"]) - 1.0) < 1e-9 and abs(np.linalg.norm(h["t"]) - 1.0) < 1e-12, id_
            if pr["success"]:
                assert pr["best"] == j, id_
                seen += 1
    assert seen >= 9


def test_engineered_cases_are_what_they_claim(scenes):
    by = {id_: (sc, r) for id_, sc, r in scenes}
    assert all(pr["n_inliers"] == 0 and not any(h["n_good"] for h in pr["hyps"]) and not pr["success"] for pr in by["zero-mask"][1])
    sc, r = by["interleaved"]
    assert all(p["mask"][31] != p["mask"][33] and p["mask"].sum() == 66 for p in sc["probs"]) and r[1]["success"]
    sc, r = by["rotation"]  # H degenerate; under F every pair is counted by two hypotheses and none is good
    assert r[0]["status"] == rr.DEGENERATE and r[1]["status"] == rr.P_OK and not r[1]["success"]
    assert sorted(h["n_good"] for h in r[1]["hyps"]) == [0, 0, 80, 80]
    assert not any((h["flags"] & rr.GOOD).any() for h in r[1]["hyps"])
    assert all(h["cos_sel"] >= rr.COS_TH for h in r[1]["hyps"] if h["n_good"])
    assert by["identity"][1][0]["status"] == rr.DEGENERATE
    sc, r = by["few"]  # 40 accepted pairs do not reach minTriangulated
    assert max(h["n_good"] for h in r[1]["hyps"]) == 40 and not r[1]["success"] and not r[0]["success"]
    assert rr.replay_f(40, [h["n_good"] for h in r[1]["hyps"]], r[1]["par"], minTriangulated=30)[0]  # ... and nothing else
    for n in (51, 52):  # the selection index min(50, n - 1): the last and the last but one of the ascending order
        pr = by[f"n{n}"][1][1]
        h = pr["hyps"][pr["best"]]
        assert h["n_good"] == n
        c = np.sort(h["cos"][(h["flags"] & rr.COUNTED) != 0])
        assert h["cos_sel"] == c[50] and (c[50] == c[-1]) == (n == 51)
    sc, r = by["nonfinite"]  # pair 7: x3D[3] == 0 under all four hypotheses
    for h in r[0]["hyps"]:
        assert not np.isfinite(h["X"][7]).any() and h["flags"][7] == 0
    assert r[0]["success"] and r[0]["hyps"][r[0]["best"]]["n_good"] == 119
    sc, r = by["low-parallax"]  # false through `parallax > minParallax` alone
    pr = r[0]
    g = [h["n_good"] for h in pr["hyps"]]
    assert not pr["success"] and 0 < max(pr["par"]) < 1.0
    assert rr.replay_f(300, g, pr["par"], minParallax=0.5)[0]
    j = int(np.argmax(g))
    assert g[j] == 300 and ((pr["hyps"][j]["flags"] & rr.GOOD) != 0).all()
    # the plane of tests/initializer_ref.py keeps Faugeras' two-fold ambiguity: two hypotheses accept every pair
    pr = by["n300"][1][0]
    assert sorted(h["n_good"] for h in pr["hyps"])[-2:] == [300, 300] and not pr["success"]
    assert by["planar-unique"][1][0]["success"]


def test_float32_transcription_of_check_rt_decides_as_the_float64_one(scenes):
    """CheckRT's tests after the triangulation in float32 arithmetic (the reference's precision) against the float64 ones, on
    the guard-band-free scenes: the same flags, hence the same counts and replay decisions."""
    pairs = 0
    for id_, sc, r in scenes:
        for pr, p32 in zip(r, rr.run(sc, f32=True)):
            assert pr["status"] == p32["status"] and pr["success"] == p32["success"] and pr["best"] == p32["best"], id_
            for a, b in zip(pr["hyps"], p32["hyps"]):
                assert np.array_equal(a["flags"], b["flags"]), id_
                pairs += int((a["flags"] != 0).sum())
    assert pairs > 3000


def test_scene_list_covers_the_sizes_at_the_edges(scenes):
    ids = [id_ for id_, _, _ in scenes]
    assert [f"n{n}" for n in (1, 32, 33, 51, 52, 64, 65, 256, 257, 300)] == ids[:10]
    for id_, sc, r in scenes[:10]:
        assert [p["kind"] for p in sc["probs"]] == [rr.MH, rr.MF] and all(p["mask"].all() for p in sc["probs"])
    assert ir.KCAM[0, 0] == rr.K4[0]
