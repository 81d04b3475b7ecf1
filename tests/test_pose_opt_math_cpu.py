"""CPU: csrc/poseopt_math.h on csrc/g2o_math.h -- the arithmetic k_poseopt.hip compiles for the device -- as a stand-alone
program (tests/cpp/poseopt_cpu.cpp, built with -ffp-contract=off) that emulates the kernel's lane-strided partial sums and its
reduction order, on every scene of the GPU test and on the engineered cases of tests/pose_opt_check.py, against the
restatement (tests/pose_opt_ref.py) under the GPU test's pass condition."""
import numpy as np
import pytest

import pose_opt_check as chk
import pose_opt_ref as pr


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """id -> (scene, reference result, result of the program): one build, one run of the program, shared."""
    tmp = tmp_path_factory.mktemp("poseopt_cpu")
    exe = chk.build_program(tmp)
    ids, scenes = zip(*(pr.gpu_scenes() + chk.extra_scenes()))
    got = chk.run_program(exe, tmp, list(scenes))
    return {id_: (sc, pr.run(sc), g) for id_, sc, g in zip(ids, scenes, got)}


def test_the_device_arithmetic_on_the_cpu_meets_the_gpu_pass_condition(runs):
    for id_, (sc, ref, got) in runs.items():
        if len(sc["u"]) < 3:  # pose and flags untouched
            assert got[0] == 0 and np.array_equal(got[1], sc["Tcw"]) and (got[2] == 7).all() and got[3]["rounds"] == 0, id_
        chk.check_against(ref, got, id_)


def test_the_engineered_scenes_keep_out_of_the_guard_bands_and_take_their_paths(runs):
    for id_, _ in chk.extra_scenes():
        sc, ref, got = runs[id_]
        assert not pr.guard_violations(sc, ref), id_
    n = lambda id_: len(runs[id_][0]["u"])
    assert runs["x-n2"][1]["rounds"] == 0                                               # nothing touched
    assert [runs[k][1]["rounds"] for k in ("x-n3", "x-n9", "x-n10")] == [1, 1, 4]       # edges().size() < 10: one round
    assert [n(k) for k in ("x-n255", "x-n256", "x-n257")] == [255, 256, 257]            # a lane's second edge
    for k in ("x-mix-n40", "x-n257"):
        ur = runs[k][0]["u_right"]
        assert (ur >= 0).any() and (ur < 0).any(), k
    sc, ref, got = runs["x-all-outliers-n40"]                                           # the empty active set
    assert ref["n_inliers"] == 0 and ref["rounds"] == 4 and ref["iterations"][1:] == [0, 0, 0] and got[3]["iterations"][1:] == [0, 0, 0]

    sc, ref, got = runs["x-equal-points-n24"]                                           # the first solve meets a pivot of 0
    assert (sc["xw"] == sc["xw"][0]).all() and ref["rounds"] == 4 and ref["iterations"] == [1] * 4 and ref["trials"] == [10] * 4
    assert got[3]["iterations"] == [1] * 4 and got[3]["trials"] == [10] * 4 and got[3]["lam"] == [0.0] * 4
    assert np.array_equal(got[1], ref["Tcw"]) and not got[2].any() and not got[4].any()
