"""orbfe_cpp::PnPsolver (include/orbfe_classes.hpp, PnPReplay of include/orbfe_pnp_replay.hpp) compiled with g++ against
liborbfe.so (tests/cpp/test_pnp.cpp): the multi-candidate form and the caller's round-robin of iterate(5) against the
restatement's stateful iterate() -- a candidate whose Refine succeeds, one that reaches mRansacMaxIts without a qualifying
hypothesis, one with fewer correspondences than minInliers, and one that runs out of supplied hypotheses."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pnp_ref as pr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
PARAMS = (0.99, 10, 300, 4, 0.5, 5.991)


def test_cpp_class_equals_the_reference_state_machine(tmp_path):
    exe = tmp_path / "test_pnp"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tests' / 'cpp'}",
                    str(ROOT / "tests/cpp/test_pnp.cpp"), "-o", str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    few = pr.make_candidate(11, 60, 40, inlier_frac=0.2, noise=0.0)
    short = dict(few, sets=few["sets"][:10])
    cands = [pr.make_candidate(500, 100, 300, inlier_frac=0.7, noise=0.0), few, pr.make_candidate(12, 8, 0), short]
    pr.write_scene(tmp_path / "scene.txt", cands, last="sigma2")
    out = subprocess.run([str(exe), str(tmp_path / "scene.txt")], check=True, capture_output=True, text=True).stdout.splitlines()
    assert not [ln for ln in out if ln.startswith("error")], out
    assert "iterate_before_solve_throws 1" in out
    refs = [pr.Solver(c["p3d"], c["p2d"], c["sigma2"], c["cam"], c["sets"], kp_idx=2 * np.arange(len(c["p3d"])) + 1,
                      n_kp=2 * len(c["p3d"]) + 3, params=PARAMS) for c in cands]
    assert [ln.split()[1:] for ln in out if ln.startswith("solver")] == \
        [[str(k), str(r.N), str(r.min_inliers), str(r.max_its)] for k, r in enumerate(refs)]
    calls = [ln.split()[1:] for ln in out if ln.startswith("call")]
    seen = {k: [] for k in range(4)}
    for tok in calls:
        k = int(tok[0])
        try:
            T, no_more, vb, n = refs[k].iterate(5)
        except IndexError:
            assert int(tok[1]) == 1, tok
            seen[k].append("out")
            continue
        assert [int(x) for x in tok[1:8]] == [0, int(T is not None), int(no_more), n, int(vb.sum()), int(np.nonzero(vb)[0].sum()),
                                             refs[k].its], tok
        assert int(tok[8]) == len(vb)
        seen[k].append("pose" if T is not None else ("nomore" if no_more else "more"))
        if T is not None:
            Tc = np.array([float(x) for x in tok[9:21]]).reshape(3, 4)
            Tr = T.astype(np.float64)
            ok, d = pr.pose_close(np.concatenate([Tc[:, :3].reshape(9), Tc[:, 3]]), Tr[:9].reshape(3, 3), Tr[9:], pr.s_pnp())
            assert ok, (d, pr.s_pnp())
    assert seen == {0: ["pose"], 1: ["nomore"], 2: ["nomore"], 3: ["out"]}, seen
