"""orbfe_cpp::Initializer (include/orbfe_classes.hpp) compiled with g++ against liborbfe.so (tests/cpp/test_initializer.cpp) on
scenes of tests/test_gpu_initializer.py: FindModels returns the C-ABI's bytes, and its picks equal the restatement's replay."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import initializer_ref as ir

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_cpp_class_equals_the_c_abi_and_the_restatement(tmp_path):
    exe = tmp_path / "test_initializer"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", f"-I{ROOT / 'tests' / 'cpp'}",
                    str(ROOT / "tests/cpp/test_initializer.cpp"), "-o", str(exe), f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    rng = np.random.default_rng(8)
    for kind, n, S in (("general", 129, 9), ("planar", 65, 5)):
        p = ir.problem(rng, kind, n, S, sigma=1.0, outliers=0.3 if kind == "general" else 0.0)
        draws = np.stack([rng.integers(0, n - j, S) for j in range(8)], axis=1)
        p["sets"] = ir.sets_from_draws(n, draws)
        keys1 = np.concatenate([p["pairs"][:, :2], [[5.0, 7.0]]]).astype(np.float32)  # (the program's unmatched key)
        p["T1"], p["T2"] = ir.normalize(keys1), ir.normalize(p["pairs"][:, 2:])
        sc = dict(probs=[p])
        ir.write_scene(tmp_path / "scene.txt", sc)
        (tmp_path / "draws.txt").write_text(" ".join(str(int(v)) for v in draws.reshape(-1)))
        out = subprocess.run([str(exe), str(tmp_path / "scene.txt"), str(tmp_path / "draws.txt")], check=True, capture_output=True,
                             text=True).stdout.splitlines()
        assert not [ln for ln in out if ln.startswith("error")], out
        line = {ln.split()[0]: ln.split()[1:] for ln in out}
        assert line["matches"] == [str(n), "sets_equal", "1"] and line["bytes_equal"] == ["1"] * 6 and line["short_draws_throw"] == ["1"]
        assert np.allclose([float(v) for v in line["T"]], np.concatenate([p["T1"], p["T2"]]), rtol=1e-13, atol=0)
        r = ir.run(sc)
        bH, SH = ir.replay(r["score"], ir.MH)
        bF, SF = ir.replay(r["score"], ir.MF)
        RH, choose_H = ir.choose(SH, SF)
        pick = line["pick"]
        assert (int(pick[0]), int(pick[1]), int(pick[5])) == (bH, bF, int(choose_H)) and choose_H == (kind == "planar")
        allow_m, allow_s = ir.allowance(ir.recorded()[0]), ir.allowance(ir.recorded()[1])
        assert ir.score_distance(float(pick[2]), SH) <= allow_s and ir.score_distance(float(pick[3]), SF) <= allow_s
        assert float(pick[4]) == pytest.approx(RH, rel=1e-6)
        for name, b, m in (("H", bH, ir.MH), ("F", bF, ir.MF)):
            if r["ill"][b, m]:
                continue
            got = np.array([float(v) for v in line[name + "21"]]).reshape(3, 3)
            assert ir.model_distance(got[None], r["model"][b, m][None])[0] <= allow_m, name
            mask = np.array([int(v) for v in line["mask" + name]], bool)
            assert not ((mask != r["masks"][b][m]) & ~r["guard"][b][m]).any(), name
