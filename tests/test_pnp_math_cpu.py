"""CPU: csrc/pnp_math.h -- the arithmetic the PnP kernels compile -- and the checks, layout and record scan of csrc/pnp_host.h
as a stand-alone program (tests/cpp/pnp_cpu.cpp, -ffp-contract=off) against the NumPy restatement tests/pnp_ref.py on every
scene of the GPU test, under the GPU test's pass condition.  This is the proof, without a device, that the Jacobi routines,
the canonical 4-point basis, the Gauss-Newton loop and the inlier test are right."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pnp_ref as pr

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cxx = hipcc if Path(hipcc).exists() else shutil.which("clang++") or shutil.which("g++")
    assert cxx, "no compiler to build the program with"
    out = tmp_path_factory.mktemp("pnp") / "pnp_cpu"
    subprocess.run([cxx, "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "tests" / "cpp"), str(ROOT / "tests" / "cpp" / "pnp_cpu.cpp"), "-o", str(out)], check=True)
    return out


def test_cpu_build_of_the_kernel_arithmetic_equals_the_reference(exe, tmp_path):
    tol = pr.s_pnp()
    total = pr.new_stats()
    for id_, cands in pr.gpu_scenes():
        pr.write_scene(tmp_path / "scene.txt", cands)
        subprocess.run([str(exe), str(tmp_path / "scene.txt"), str(tmp_path / "out.txt")], check=True, capture_output=True)
        hyp, rec_off, rec_hyp, rec = pr.read_result(tmp_path / "out.txt", cands)
        st = pr.new_stats()
        h = r = 0
        for k, c in enumerate(cands):
            n, counts, h0 = len(c["p3d"]), [], h
            for s in c["sets"]:
                pr.compare_item(c, pr.ref_item(c, s), hyp[h], tol, st)
                counts.append(hyp[h][0])
                h += 1
            want = pr.scan_records(counts, c["min_inliers"])
            assert [x - h0 for x in rec_hyp[rec_off[k]:rec_off[k + 1]]] == want
            for hh in want:
                mask = pr.words_to_mask(hyp[h0 + hh][3], n)
                pr.compare_item(c, pr.ref_item(c, np.flatnonzero(mask)), rec[r], tol, st)
                r += 1
        if st["items"] >= 20:
            pr.check_caps(st, id_)
        else:
            assert st["excluded"] == 0 and st["guard"] == 0, (id_, st)
        for key in ("items", "excluded", "decisions", "guard"):
            total[key] += st[key]
        total["worst"] = max(total["worst"], st["worst"])
    print(total, "tolerance", tol)
    assert total["items"] > 350
