"""orbfe_cpp::Initializer::Initialize / Reconstruct (include/orbfe_classes.hpp) compiled with g++ against liborbfe.so
(tests/cpp/test_initializer_reconstruct.cpp): Reconstruct returns the C-ABI's bytes, Initialize returns Reconstruct's, and the
decisions equal the restatement's on the model and mask the class chose."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import initializer_ref as ir
import initializer_reconstruct_ref as rr

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_initialize_equals_the_c_abi_and_the_restatement(tmp_path):
    exe = tmp_path / "test_initializer_reconstruct"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tests' / 'cpp'}",
                    str(ROOT / "tests/cpp/test_initializer_reconstruct.cpp"), "-o", str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"],
                   check=True)
    rng = np.random.default_rng(8)
    for kind, n, S in (("general", 129, 40), ("planar", 65, 20)):
        p = ir.problem(rng, kind, n, S, sigma=1.0, outliers=0.2 if kind == "general" else 0.0)
        draws = np.stack([rng.integers(0, n - j, S) for j in range(8)], axis=1)
        p["sets"] = ir.sets_from_draws(n, draws)
        ir.write_scene(tmp_path / "scene.txt", dict(probs=[p]))
        (tmp_path / "draws.txt").write_text(" ".join(str(int(v)) for v in draws.reshape(-1)))
        out = subprocess.run([str(exe), str(tmp_path / "scene.txt"), str(tmp_path / "draws.txt")] + [repr(float(v)) for v in rr.K4],
                             check=True, capture_output=True, text=True).stdout.splitlines()
        assert not [ln for ln in out if ln.startswith("error")], out
        line = {ln.split()[0]: ln.split()[1:] for ln in out}
        assert line["bytes_equal"] == ["1"] * 9 and line["initialize_equals_reconstruct"] == ["1"]
        ok, model_kind, best, pst, n_inl = (int(v) for v in line["decision"][:5])
        assert model_kind == (rr.MH if kind == "planar" else rr.MF)
        mask = np.array([int(v) for v in line["mask"]], bool)
        model = np.array([float(v) for v in line["model"]]).reshape(3, 3)
        pr = rr.run_problem(rr.problem(model_kind, model, p["pairs"], mask))
        assert rr.guard_count([pr]) == (0, 0)  # (this scene and these draws)
        assert (bool(ok), pst, n_inl) == (pr["success"], pr["status"], pr["n_inliers"])
        assert sorted(int(v) for v in line["n_good"]) == sorted(h["n_good"] for h in pr["hyps"])
        assert bool(ok) == (kind == "general")  # the plane keeps Faugeras' two-fold ambiguity: ReconstructH returns false
        vb = np.array([int(v) for v in line["vbTriangulated"]], bool)
        vP = np.array([float(v) for v in line["vP3D"]]).reshape(-1, 3)
        assert len(vb) == n + 1 and not vb[n] and not vP[n].any()
        if ok:
            a = ir.allowance(rr.recorded()[0])
            R21, t21 = np.array([float(v) for v in line["R21"]]).reshape(3, 3), np.array([float(v) for v in line["t21"]])
            assert rr.motion_distance(R21, t21, pr["R21"], pr["t21"]) <= a
            assert rr.motion_distance(R21, t21, ir.R21, ir.T21 / np.linalg.norm(ir.T21)) < 1e-3
            h = pr["hyps"][pr["best"]]
            assert np.array_equal(vb[:n], (h["flags"] & rr.GOOD) != 0)
            c = (h["flags"] & rr.COUNTED) != 0
            assert (np.abs(vP[:n][c] - h["X"][c]).max(axis=1) <= rr.point_tolerance(h["X"][c], rr.recorded()[1]) +
                    np.spacing(np.abs(h["X"][c]).max(axis=1).astype(np.float32))).all()  # (+ the rounding to float)
            assert float(line["decision"][5]) == pytest.approx(pr["parallax"], rel=1e-9)
