"""Frame::ComputeStereoMatches on engineered edge cases, CPU only: the oracle against an independent numpy restatement
of src/Frame.cc:512-686 (tests/stereo_edges.py), and proof that every case reaches the branch it was built for.

Per-branch totals (left keypoints leaving the per-keypoint loop by that exit; orc_stereo_branch_counts):

    exit                     rendered (*)   engineered + seams   200 seeded
    invalid_record                0               4                115
    row_out_of_range              0               2                 41
    empty_row                     0              25               1558
    maxu_negative                 0               1                  0
    no_candidate                450               6               5742
    hamming_above_th           3111               5               2675
    iniu_negative                 0               1                  0
    endu_past_cols                0               2                307
    guard_cy_low                  0               2                276
    guard_cy_high                 0               1                290
    guard_cxl_low                 0               2                202
    guard_cxl_high                0               1                  1
    guard_cxr_low                 0               2                379
    bestinc_low_end             114               4                 86
    bestinc_high_end            128               1                126
    delta_out_of_range            0               0                  0
    delta_nan_passed              0               0                  0
    disparity_out_of_range        3               2                 90
    disparity_clamped             0               2                  0
    accepted                   2630            1749               2015
    median_removed              420             176                385

(*) the four cases of test_compute_stereo_matches (two rendered scenes at 1241x376 / 2000 features and 752x480 / 1200):
6436 left keypoints, 2875 SAD refinements.  The rare exits of the engineered column are asserted below
(ENGINEERED_TOTALS), so a change to a case shows up here.  No exit the rendered cases miss stays at 0 there.

The two zero rows cannot be reached by any input; stereo_edges.py's docstring has the proof and
test_parabola_fit_is_bounded_and_exact checks its steps on every fit of the case set.  The right-image patch guard
(guard_cxr_low) IS reachable: round(uR0 / scale) in 0..9 passes `iniu < 0` and the strip's first patch starts at a
negative column.
"""
import numpy as np
import pytest

import oracle_lib as orc
import stereo_edges as se


@pytest.fixture(scope="module")
def world():
    """every case with the oracle's and the restatement's answers, computed once"""
    P = se.Pyramids()
    out = {}
    for group, cases in (("engineered", se.engineered_cases() + se.seam_cases()), ("random", se.random_cases())):
        for c in cases:
            u_o, d_o = P.oracle(c)
            counts = orc.stereo_branch_counts()
            u_n, d_n, trace = P.restatement(c)
            out[c.name] = dict(case=c, group=group, oracle=(u_o.copy(), d_o.copy()), counts=counts, numpy=(u_n, d_n),
                               trace=trace)
    return out


ENGINEERED_TOTALS = dict(invalid_record=4, row_out_of_range=2, maxu_negative=1, iniu_negative=1, endu_past_cols=2,
                         guard_cy_low=2, guard_cy_high=1, guard_cxl_low=2, guard_cxl_high=1, guard_cxr_low=2,
                         bestinc_low_end=4, bestinc_high_end=1, delta_out_of_range=0, delta_nan_passed=0,
                         disparity_out_of_range=2, disparity_clamped=2)


def _totals(world, group):
    tot = dict.fromkeys(se.EXITS, 0)
    for w in world.values():
        if w["group"] == group:
            for k, v in w["counts"].items():
                tot[k] += v
    return tot


def test_level_7_is_89_by_56():
    o = orc.Oracle(1000, se.SCALE, se.NLEVELS, 20, 7)
    assert o.level_sizes(se.W, se.H)[7] == (89, 56)
    assert o.level_sizes(se.W, se.H)[0] == (se.W, se.H)


def test_oracle_equals_restatement_bit_for_bit(world):
    assert sum(w["group"] == "random" for w in world.values()) == 200
    for name, w in world.items():
        (u_o, d_o), (u_n, d_n) = w["oracle"], w["numpy"]
        assert u_o.dtype == u_n.dtype == np.float32
        assert np.array_equal(u_o, u_n) and np.array_equal(d_o, d_n), name
        assert not np.isnan(u_o).any() and not np.isnan(d_o).any(), name
        # "no stereo" is -1 in both arrays or in neither
        assert np.array_equal(u_o == -1, d_o == -1), name


def test_oracle_counters_equal_the_restatements_trace(world):
    """the counters are the oracle's; the trace is the restatement's: two tallies of the same exits"""
    for name, w in world.items():
        assert w["counts"] == se.branch_counts_of(w["trace"]), name
        assert sum(v for k, v in w["counts"].items() if k not in ("disparity_clamped", "median_removed",
                                                                  "delta_nan_passed")) == len(w["case"].kpL), name


def test_every_named_case_reaches_its_branch(world):
    """what keeps the GPU test honest: an engineered keypoint leaves by the exit it was built for, with the
    intermediate values the construction promises, and the oracle's counter for that exit is above 0 in that case"""
    checked = 0
    for name, w in world.items():
        for i, exit_, fields in w["case"].expect:
            t = w["trace"][i]
            if exit_ is not None:
                assert t["exit"] == exit_, (name, i, t)
                assert w["counts"][exit_] > 0, (name, exit_)
            for k, v in fields.items():
                got = bool(t.get(k)) if isinstance(v, bool) else t.get(k)
                assert got == v, (name, i, k, v, got)
                if k in ("clamped", "median_removed") and v:
                    assert w["counts"]["disparity_clamped" if k == "clamped" else "median_removed"] > 0, name
            checked += 1
    assert checked > 250


def test_no_branch_counter_is_zero_over_the_engineered_set(world):
    tot = _totals(world, "engineered")
    for k in se.EXITS:
        if k in se.UNREACHABLE:
            assert tot[k] == 0, k    # see test_parabola_fit_is_bounded_and_exact
        else:
            assert tot[k] > 0, k
    for k, v in ENGINEERED_TOTALS.items():
        assert tot[k] == v, (k, tot[k])
    rnd = _totals(world, "random")
    for k in se.UNREACHABLE:
        assert rnd[k] == 0, k


def test_engineered_outcomes_are_visible_in_the_output(world):
    """a few outcomes spelled out, so the cases cannot drift into ones where both answers are -1"""
    u, d = world["hamming_tie_first_wins"]["oracle"]
    i_first, i_second = (e[0] for e in world["hamming_tie_first_wins"]["case"].expect)
    assert u[i_first] >= 0 and abs(u[i_first] - 193.0) < 1.0
    assert not abs(u[i_second] - 113.0) < 1.0                   # the true match came second and lost
    w = world["disparity_ends_and_clamp"]
    i = w["case"].expect[0][0]
    uL = np.float32(w["case"].kpL[i]["x"])
    # `uL-0.01` is a double expression (:663).  For every uL a clamp can see here -- disparity == 0 needs bestuR == uL, at
    # octave 0 an integer plus deltaR == 0 -- the float form uL - 0.01f rounds to the same float (checked for every integer
    # below 320 and every scale * integer of the eight levels), so this pins the value, not the form
    assert w["oracle"][0][i] == np.float32(np.float64(uL) - 0.01)
    assert w["oracle"][1][i] == np.float32(se.MBF) / np.float32(0.01)
    u, _ = world["median_zero"]["oracle"]
    assert (u == -1).all()
    u, _ = world["median_run_at_threshold"]["oracle"]
    assert [bool(v >= 0) for v in u] == [True, False, True, True, False, True, True]
    u, _ = world["median_even_upper_middle"]["oracle"]
    assert (u >= 0).all()
    u, _ = world["crowded_row"]["oracle"]
    for i, _, f in world["crowded_row"]["case"].expect:
        assert abs(u[i] - 193.0) < 1.0


def test_parabola_fit_is_bounded_and_exact(world):
    """deltaR = (dist1 - dist3) / (2 (dist1 + dist3 - 2 dist2)) over every fit of the case set.

    The operands are integers <= 61710, so dist1 - dist3, dist1 + dist3 (< 2^17), 2 dist2 and the denominator (< 2^18)
    are exact in float: of the operations only the division rounds, and a float division is correctly rounded, so the
    float32 value must EQUAL the float64 value rounded to float32 (a double quotient of two floats rounds to the same
    float: 53 >= 2 * 24 + 2).  A contraction or a reciprocal-multiply would show as a 1-ulp difference.
    Measured over the case set: largest deviation 0 ulp, largest |deltaR| 0.5; bound asserted: 0 ulp, 0.5."""
    n, worst, largest = 0, 0.0, 0.0
    for name, w in world.items():
        for t in w["trace"]:
            if "fit" not in t:
                continue
            d1, d2, d3 = t["fit"]
            assert d1 > d2 and d3 >= d2, (name, t)              # the first minimum won, and it is not at -5
            f32 = orc.stereo_delta_r(d1, d2, d3)
            assert f32 == t["deltaR"], (name, t)
            num, s, den = d1 - d3, d1 + d3, 2.0 * (d1 + d3 - 2.0 * d2)
            for v in (num, s, 2.0 * d2, den):
                assert np.float64(np.float32(v)) == v           # exact steps
            f64 = np.float64(num) / np.float64(den)
            ulp = np.spacing(np.float32(abs(f64))) if f64 != 0 else np.float32(0)
            dev = abs(np.float64(f32) - f64) / ulp if ulp else abs(np.float64(f32) - f64)
            assert dev <= 0.5, (name, t)                        # the float64 value rounded
            worst = max(worst, float(abs(np.float64(f32) - np.float64(np.float32(f64)))))
            largest = max(largest, abs(float(f32)))
            n += 1
    assert n > 3500
    assert worst == 0.0      # measured: 0
    assert largest <= 0.5    # measured: 0.5 (dist3 == dist2, the next shift ties the minimum)


def test_counters_change_no_result():
    """the same call twice, and interleaved with a different one: results and counters depend on the call alone"""
    P = se.Pyramids()
    cases = se.engineered_cases()
    a, b = cases[3], cases[9]
    u1, d1 = P.oracle(a)
    c1 = orc.stereo_branch_counts()
    P.oracle(b)
    assert orc.stereo_branch_counts() != c1
    u2, d2 = P.oracle(a)
    assert np.array_equal(u1, u2) and np.array_equal(d1, d2) and orc.stereo_branch_counts() == c1
    out = (orc.C.c_int64 * 2)(-7, -7)
    assert orc.lib().orc_stereo_branch_counts(out, 1) == len(orc.STEREO_BRANCHES) and out[1] == -7
    assert orc.STEREO_BRANCHES == se.EXITS
