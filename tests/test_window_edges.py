"""The Frame grid and the window searches on engineered edge cases, CPU only: the oracle (oracle/orb_oracle.c) against the
independent restatement of tests/window_edges.py -- results and branch tallies -- and proof that every named case takes the
branch it names.  tests/test_gpu_window_edges.py runs the same cases through the kernels."""
import math
from collections import Counter

import numpy as np
import pytest

import oracle_lib as orc
import window_edges as we


@pytest.fixture(scope="module")
def world():
    """every case with the oracle's and the restatement's answers and tallies, computed once"""
    out = {}
    for group, cases in (("named", we.named_cases()), ("seeded", we.seeded_cases())):
        for c in cases:
            assert c.name not in out, c.name
            ro, To = we.run_oracle(c)
            rr, Tr = we.run_restatement(c)
            out[c.name] = dict(case=c, group=group, oracle=ro, counts=+To, restatement=rr, tally=+Tr)
    return out


def test_case_set_has_200_seeded_cases_per_search(world):
    for k in we.KINDS:
        assert sum(w["group"] == "seeded" and w["case"].kind == k for w in world.values()) == 200, k
        assert any(w["group"] == "named" and w["case"].kind == k for w in world.values()), k


def test_oracle_equals_restatement_arrays_and_counts(world):
    for name, w in world.items():
        assert w["oracle"] == w["restatement"], name


def test_oracle_counters_equal_the_restatements_tally(world):
    """the counters are the oracle's, the tally is the restatement's: two records of the same decisions"""
    for name, w in world.items():
        assert w["counts"] == w["tally"], (name, dict(w["counts"] - w["tally"]), dict(w["tally"] - w["counts"]))
        assert set(w["counts"]) <= set(orc.WINDOW_BRANCHES), name


def test_every_named_case_takes_the_branch_it_names(world):
    checked = 0
    for name, w in world.items():
        if w["group"] != "named":
            continue
        c = w["case"]
        for branch, count in c.expect.items():
            assert branch in orc.WINDOW_BRANCHES, (name, branch)
            assert w["counts"][branch] == count, (name, branch, count, w["counts"][branch])
            checked += 1
        if c.want is not None:
            assert we.outcome(c, w["oracle"]) == list(c.want), (name, w["oracle"])
            checked += 1
    assert checked > 250


def test_no_counter_is_zero_over_the_named_set(world):
    """a condition on the inputs: every exit and decision the oracle counts is taken by some engineered case"""
    tot = Counter()
    for w in world.values():
        if w["group"] == "named":
            tot.update(w["counts"])
    for k in orc.WINDOW_BRANCHES:
        assert tot[k] > 0, k


def test_seeded_cases_are_not_trivial(world):
    tot = Counter()
    for w in world.values():
        if w["group"] == "seeded":
            tot.update(w["counts"])
    for k in ("accepted", "blocked", "tie_ignored", "ratio_reject", "init_overwrite", "init_refused", "hist_pruned", "stereo_reject",
              "chi2_mono_reject", "chi2_stereo_reject", "sim3_mutual", "sim3_one_way_only", "clamp_minx", "clamp_maxy"):
        assert tot[k] > 20, (k, tot[k])


def _strip(c, res, n0):
    """a result on a padded frame, cut back to the case's own features (the filler must have stayed unmatched)"""
    if c.kind in ("mappoints", "lastframe", "reloc", "sim3proj"):
        assert all(v == -1 for v in res[1][n0:]), c.name
        return [res[0], res[1][:n0]]
    return res


@pytest.mark.parametrize("form", ["crowded", "large"])
def test_filler_of_the_grid_forms_is_seen_by_no_named_case(world, form):
    """pad_frame() turns a case's frame into the crowded-cell and the n > 8192 form; the case must not notice"""
    for name, w in world.items():
        if w["group"] != "named":
            continue
        c = w["case"]
        res, counts = we.run_oracle(we.padded_case(c, form))
        assert _strip(c, res, len(c.frame["x"])) == w["oracle"], name
        assert +counts == w["counts"], name
    assert len(we.pad_frame(c.frame, "large")["x"]) > 8192


def test_rounding_cell_is_inside_the_cell_range_of_every_window_that_returns_it(world):
    """the argument of window_edges.py's docstring, on every (window, returned feature) pair of the area cases"""
    n = 0
    for w in world.values():
        c = w["case"]
        if c.kind != "area":
            continue
        f = c.frame
        minx, _, miny, _ = [np.float32(b) for b in f["bounds"]]
        _, winv, hinv = we.py_grid(f["x"], f["y"], f["bounds"])
        for (x, y, r, _, _), got in zip(c.args["q"], w["oracle"][0]):
            x, y, r = np.float32(x), np.float32(y), np.float32(r)
            for i in got:
                px = we.c_round(float((f["x"][i] - minx) * winv))
                py = we.c_round(float((f["y"][i] - miny) * hinv))
                assert math.floor(float((x - minx - r) * winv)) <= px <= math.ceil(float((x - minx + r) * winv))
                assert math.floor(float((y - miny - r) * hinv)) <= py <= math.ceil(float((y - miny + r) * hinv))
                n += 1
    assert n > 3000
    # the features the grid drops although a window contains them: columns -1 and 64, row 48
    c = next(w for w in world.values() if w["case"].name == "grid_rounding")
    assert sorted(set(range(21)) - set(c["oracle"][0][0]) - set(c["oracle"][0][1])) == [1, 3, 4, 6, 20]


def test_constructions_hold_the_float_facts_they_claim():
    f32 = np.float32
    assert f32(0.8) * f32(50) > f32(40) and not f32(40) > f32(f32(0.8) * f32(50)) or f32(f32(0.8) * f32(50)) >= f32(40)
    assert f32(f32(50) * f32(0.9)) == f32(45.0)              # init ratio at equality: 45 < 45.0f is false
    assert f32(f32(0.1) * f32(20)) == f32(2.0) and f32(f32(0.1) * f32(10)) == f32(1.0)
    u, mbf, iz = we.fma_triple()
    assert f32(u - f32(mbf * iz)) != f32(np.float64(u) - np.float64(mbf) * np.float64(iz))
    assert [we.rot_bin(a, 0.0) for a in (15.0, 45.0, 345.0, 0.0, 359.0)] == [1, 2, 12, 0, 12]
    assert we.c_round(0.5) == 1 and we.c_round(-0.5) == -1 and we.c_round(2.5) == 3


def test_counters_change_no_result_and_belong_to_the_last_call():
    cases = {c.name: c for c in we.named_cases()}
    a, b = cases["tenth_20_2_1"], cases["ratio_0.8_above_same_level"]
    r1, c1 = we.run_oracle(a)
    we.run_oracle(b)
    assert +Counter(orc.window_branch_counts()) != +c1
    r2, c2 = we.run_oracle(a)
    assert r1 == r2 and c1 == c2
    out = (orc.C.c_int64 * 2)(-7, -7)
    assert orc.lib().orc_window_branch_counts(out, 1) == len(orc.WINDOW_BRANCHES) and out[1] == -7
    orc.three_maxima([20, 1, 0])   # a search call of its own: the counters are reset and hold this call only
    got = +Counter(orc.window_branch_counts())
    assert got == Counter(max2_below_tenth=1)
