"""SearchByBoW (both forms), SearchForTriangulation and their rotation histogram on engineered edge cases, CPU only: the
oracle (oracle/orb_oracle.c) against the independent restatement of tests/bow_edges.py -- results and branch tallies --, proof
that every named case takes the branch it names, and proof that every wrong reading of bow_edges.VARIANTS is defeated by a
named case.  tests/test_gpu_bow_edges.py runs the same cases through the kernels."""
from collections import Counter

import numpy as np
import pytest

import bow_edges as be
import oracle_lib as orc

ALL_BRANCHES = set(orc.BOW_BRANCHES) | set(be.HIST_BRANCHES)


@pytest.fixture(scope="module")
def world():
    """every case with the oracle's and the restatement's answers and tallies, computed once"""
    out = {}
    for group, cases in (("named", be.named_cases()), ("seeded", be.seeded_cases())):
        for c in cases:
            assert c.name not in out, c.name
            ro, To = be.run_oracle(c)
            rr, Tr = be.run_restatement(c)
            out[c.name] = dict(case=c, group=group, oracle=ro, counts=+To, restatement=rr, tally=+Tr)
    return out


def test_case_set_has_200_seeded_cases_per_search(world):
    for k in be.KINDS:
        seeded = [w["case"] for w in world.values() if w["group"] == "seeded" and w["case"].kind == k]
        assert len(seeded) == 200, k
        assert any(w["group"] == "named" and w["case"].kind == k for w in world.values()), k
        for c in seeded:
            assert len(c.s1["desc"]) <= 400 and len(c.s2["desc"]) <= 400
            assert len(set(c.s1["nodes"].tolist())) <= 12 and len(set(c.s2["nodes"].tolist())) <= 12
    assert {w["case"].nnratio for w in world.values() if w["group"] == "named"} >= {0.6, 0.75, 0.8}


def test_oracle_equals_restatement_arrays_and_counts(world):
    for name, w in world.items():
        assert w["oracle"] == w["restatement"], name


def test_oracle_counters_equal_the_restatements_tally(world):
    """the counters are the oracle's, the tally is the restatement's: two records of the same decisions"""
    for name, w in world.items():
        assert w["counts"] == w["tally"], (name, dict(w["counts"] - w["tally"]), dict(w["tally"] - w["counts"]))
        assert set(w["counts"]) <= ALL_BRANCHES, name


def test_every_named_case_takes_the_branch_it_names(world):
    checked = 0
    for name, w in world.items():
        if w["group"] != "named":
            continue
        c = w["case"]
        for branch, count in c.expect.items():
            assert branch in ALL_BRANCHES, (name, branch)
            assert w["counts"][branch] == count, (name, branch, count, w["counts"][branch])
            checked += 1
        if c.want is not None:
            assert w["oracle"][1] == list(c.want), (name, w["oracle"])
            assert w["oracle"][0] == sum(v >= 0 for v in c.want), name
            checked += 1
    assert checked > 800


def test_no_counter_is_zero_over_the_named_set(world):
    """a condition on the inputs: every exit and decision the oracle counts is taken by some engineered case"""
    tot = Counter()
    for w in world.values():
        if w["group"] == "named":
            tot.update(w["counts"])
    for k in orc.BOW_BRANCHES + be.HIST_BRANCHES:
        assert tot[k] > 0, k


def test_every_case_defeats_the_variants_it_lists(world):
    n = 0
    for name, w in world.items():
        c = w["case"]
        for v in c.catches:
            assert v in be.VARIANTS, (name, v)
            assert be.run_restatement(c, v)[0] != w["restatement"], (name, v)
            n += 1
    assert n > 250


def test_every_variant_is_caught_by_a_named_case(world):
    caught = {v for w in world.values() if w["group"] == "named" for v in w["case"].catches}
    assert caught == set(be.VARIANTS), set(be.VARIANTS) - caught
    assert len(be.VARIANTS) == 22


def test_variant_none_is_the_restatement_itself(world):
    c = world["bow_frame_best_50_second_256"]["case"]
    assert be.run_restatement(c, None)[0] == be.run_restatement(c)[0] == [1, [0]]
    assert be.run_restatement(c, "low_inclusive_swapped")[0] == [0, [-1]]


def test_seeded_cases_are_not_trivial(world):
    """a condition on the generator"""
    tot = Counter()
    for w in world.values():
        if w["group"] == "seeded":
            tot.update(w["counts"])
    for k in ("accepted", "cand_claimed", "equal_best_becomes_second", "ratio_reject", "threshold_reject", "tri_replaced_equal",
              "tri_epipolar_reject", "tri_epipole_reject", "hist_pruned"):
        assert tot[k] > 20, (k, tot[k])


def test_ratio_rounding_search():
    """(float)best1 < nnratio * (float)best2 with a ROUNDED product: the pairs where the rounding decides"""
    p6, p8 = be.ratio_rounding_pairs(0.6), be.ratio_rounding_pairs(0.8)
    assert len(p6) == 13 and p6[:3] == [(3, 5), (6, 10), (9, 15)]
    assert len(p8) == 12 and p8[:3] == [(4, 5), (8, 10), (12, 15)]
    for r in (0.7, 0.75, 0.9):
        assert be.ratio_rounding_pairs(r) == [], r
    f32 = np.float32
    assert f32(f32(0.6) * f32(5)) == f32(3.0) and float(f32(0.6)) * 5 > 3.0
    for r, pairs in ((0.6, p6), (0.8, p8)):
        for b1, b2 in pairs:                       # each refuses, its neighbour passes
            assert not f32(b1) < f32(f32(r) * f32(b2)) and f32(b1) < f32(f32(r) * f32(b2 + 1))


def test_constructions_hold_the_float_facts_they_claim():
    f32 = np.float32
    for o in (0, 1):
        lim = f32(f32(100.0) * be.SF[o])
        for t in (be.nxt(lim, False), lim, be.nxt(lim)):
            dx, dy = be.sum_of_squares_operands(t)
            assert f32(f32(dx * dx) + f32(dy * dy)) == t
    s, d = be.float_gate_sigma()
    assert (float(d) < 3.84 * float(s)) != bool(d < f32(f32(3.84) * s))
    for sig in (be.SIGMA2[1], s):
        lo, hi = be.gate_floats(sig)
        assert float(lo) < 3.84 * float(sig) <= float(hi) and be.nxt(lo) == hi
        for t in (be.nxt(lo, False), lo, hi):
            la, lb, lc = be.dsqr_operands(t)
            num, den = be.epipolar_terms(0, 0, 0, 0, [0, 0, 0, 0, 0, 0, la, lb, lc])
            assert num == lc and f32(f32(num * num) / den) == t
    x1, y1, F, x2, y2, sg = be.fused_tuple()
    (n0, d0), (n1, d1) = be.epipolar_terms(x1, y1, x2, y2, F), be.epipolar_terms(x1, y1, x2, y2, F, True)
    a, b = f32(f32(n0 * n0) / d0), f32(f32(n1 * n1) / d1)
    assert (float(a) < 3.84 * float(sg)) != (float(b) < 3.84 * float(sg))
    hw = be.half_way_angles()
    assert len(hw) >= 9 and (15.0, 0.0, 1) in hw and (135.0, 0.0, 5) in hw
    for a1, a2, b in hw:
        assert be.rot_bin(a1, a2) == b and be._bin(a1, a2, "bin_half_to_even") == b - 1
    assert be.rot_bin(-0.0, 0.0) == 0 and be.rot_bin(100.0, be.nxt(100.0)) == 12 and be._bin(100.0, be.nxt(100.0), "bin_no_wrap") == 0


def test_batch_vocabulary_places_every_fitting_case(world):
    """the centroids are 128 bits apart pairwise; the oracle's transform puts every descriptor of a fitting case into the
    node it was built for (tests/test_gpu_bow_edges.py repeats this against the device FeatureVector)"""
    arrays, cent = be.batch_vocabulary_arrays()
    d = be._dist_matrix(cent, cent)
    assert (d + 256 * np.eye(len(cent), dtype=np.int64)).min() >= 120
    vo = orc.Vocabulary.from_arrays(arrays)
    fit = [w["case"] for w in world.values() if w["group"] == "named" and be.fits_batch(w["case"])]
    assert len(fit) > 100 and any(len(c.s2["desc"]) == 300 for c in fit)
    for c in fit:
        for desc, _, node in be.batch_frames(c, cent):
            used, _, weight, got = vo.transform(desc, 1)
            assert used == len(desc) and np.array_equal(got, node), c.name


def test_counters_change_no_result_and_belong_to_the_last_call():
    cases = {c.name: c for c in be.named_cases()}
    a, b = cases["hist_tenth_30_3_2"], cases["tri_den_zero_f12_zero"]
    r1, c1 = be.run_oracle(a)
    be.run_oracle(b)
    assert +Counter(orc.bow_branch_counts()) != +Counter({k: v for k, v in c1.items() if k in orc.BOW_BRANCHES})
    assert orc.window_branch_counts()["hist_pruned"] == 0 and c1["hist_pruned"] == 2
    r2, c2 = be.run_oracle(a)
    assert r1 == r2 and c1 == c2
    out = (orc.C.c_int64 * 2)(-7, -7)
    assert orc.lib().orc_bow_branch_counts(out, 1) == len(orc.BOW_BRANCHES) and out[1] == -7
