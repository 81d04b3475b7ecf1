"""orbfe_cpp::Sim3Solver (include/orbfe_classes.hpp) compiled with g++ against liborbfe.so (tests/cpp/test_sim3.cpp) on the class
scene of tests/test_gpu_sim3.py: the caller's round-robin of iterate(5) against the restatement's state machine."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sim3_ref as sr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_class_equals_the_reference_state_machine(tmp_path):
    exe = tmp_path / "test_sim3"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tests' / 'cpp'}",
                    str(ROOT / "tests/cpp/test_sim3.cpp"), "-o", str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    id_ = "class-fix0"
    sc = dict(sr.gpu_scenes())[id_]
    r = sr.run(sc)
    sr.write_scene(tmp_path / "scene.txt", sc)
    out = subprocess.run([str(exe), str(tmp_path / "scene.txt"), str(sr.CLASS_MIN_INLIERS)], check=True, capture_output=True,
                         text=True).stdout.splitlines()
    assert not [ln for ln in out if ln.startswith("error")], out
    assert [ln.split()[3] for ln in out if ln.startswith("solver")] == [str(len(c["triples"])) for c in sc["cands"]]
    assert "iterate_before_evaluate_throws 1" in out and "seeded 1 1 1" in out
    assert "estimate_before_any_hypothesis_throws 1" in out  # as the Python class
    # re-parameterised to fewer hypotheses, then to none: the estimate of the best hypothesis so far is kept, nothing stale is read
    assert [ln for ln in out if ln.startswith("reparameterised")] == ["reparameterised 1 1 1"], out
    # the C++ generator draws what the Python one draws
    from orb_slam2_annotate_amd.loop_closing import seeded_draws
    draws = [int(t) for t in [ln for ln in out if ln.startswith("draws")][0].split()[1:]]
    assert draws[:12] == seeded_draws(7, 100, 80, 4).reshape(-1).tolist()
    big = int(seeded_draws(0xFFFFFFFFFFFFFFFF, 0, 1000003, 1)[0, 0])
    assert draws[12:] == [big, int(seeded_draws(0, 0, 3, 1)[0, 0])]
    refs, h0 = [], 0
    for c in sc["cands"]:
        H = len(c["triples"])
        refs.append(sr.RefSolver(r["n_inliers"][h0:h0 + H], r["masks"][h0:h0 + H], c["indices1"], c["N1"], sr.CLASS_MIN_INLIERS,
                                 sr.max_iterations(c["n"], 0.99, sr.CLASS_MIN_INLIERS, 300)))
        h0 += H
    calls = [ln.split()[1:] for ln in out if ln.startswith("call")]
    assert len(calls) > 10
    s0, R, t = sr.planted(False)
    accepted = 0
    for tok in calls:
        k = int(tok[0])
        h, no_more, vb, n = refs[k].iterate(5)
        assert [int(x) for x in tok[1:8]] == [int(h is not None), int(no_more), n, int(vb.sum()), int(np.nonzero(vb)[0].sum()),
                                             refs[k].iterations, int(refs[k].best_inliers)], tok
        if h is not None:
            accepted += 1
            assert int(tok[8]) == 1  # T12 = [s R | t] of GetEstimated*
            T = np.array([float(x) for x in tok[9:21]]).reshape(3, 4)
            assert np.allclose(T, np.concatenate([s0 * R, t[:, None]], axis=1), atol=1e-4)
    assert accepted > 0 and all(ref.iterate(5)[1] for ref in refs)  # the program went on until every solver said bNoMore
