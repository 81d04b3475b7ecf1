"""CPU: csrc/lba_math.h and csrc/lba_host.h -- the arithmetic, work items and schedule the kernels of k_lba.hip run -- as a
stand-alone program in the device's summation order (tests/cpp/lba_cpu.cpp) against the restatement (tests/lba_ref.py) on
the scenes of the GPU test: discrete results identical, continuous ones within the reordering noise."""
import subprocess

import numpy as np
import pytest

import lba_ref as lr
from lba_check import agrees, assert_discrete_equal, build_cpu_program, deviation, recorded, run_cpu, tolerance, write_scene


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_cpu_program(tmp_path_factory.mktemp("lbacpu"))


@pytest.fixture(scope="module")
def scenes():
    return [(id_, sc, kind, lr.run(sc, kind), lr.run(sc, kind, reverse=True), lr.run(sc, kind, schur=True)) for id_, sc, kind in lr.gpu_scenes()]


def test_cpu_program_equals_the_restatement(exe, scenes, tmp_path):
    """discrete results identical; continuous ones within 16 x the restatement's own deviation (or 4 float32 ulps).  The program
    differs from the restatement in the order of its sums AND in its solver (Schur complement and Cholesky instead of one
    dense solve), so the restatement's own deviation is the larger of forward-against-reversed edge order and dense-against-
    Schur route (lr.schur_solve), both measured here per scene"""
    measured = {}
    for id_, sc, kind, ref, rev, sch in scenes:
        got = run_cpu(exe, tmp_path, sc, kind)
        assert_discrete_equal(got, ref, id_)
        assert_discrete_equal(rev, ref, id_)
        assert_discrete_equal(sch, ref, id_)
        d, s_rev, s_sch = deviation(got, ref), deviation(rev, ref), deviation(sch, ref)
        s_ref = (max(s_rev[0], s_sch[0]), max(s_rev[1], s_sch[1]))
        tol = tolerance(sc, s_ref, (0.0, 0.0))
        print(f"{id_}: s_cpu {d[0]:.2e} / {d[1]:.2e}  s_ref {s_rev[0]:.2e} / {s_rev[1]:.2e}  schur route {s_sch[0]:.2e} / {s_sch[1]:.2e}  "
              f"allowed {tol[0]:.2e} / {tol[1]:.2e}")
        assert d[0] <= tol[0] and d[1] <= tol[1], (id_, d, tol)
        for name, val in (("s_ref", s_rev), ("s_schur", s_sch), ("s_cpu", d)):
            measured[f"{id_}.{name}_abs"], measured[f"{id_}.{name}_rel"] = val
    rec = recorded()
    assert set(rec) == set(measured), "profiles/lba_tolerance.txt lists other scenes than the test measures"
    off = {k: (measured[k], rec[k]) for k in rec if not agrees(measured[k], rec[k])}
    assert not off, f"profiles/lba_tolerance.txt disagrees with what is measured: {off}"


@pytest.mark.parametrize("k", [0, 1, 3, 5, 7])
def test_cpu_program_stop_flag_raised_before_iteration_k(exe, scenes, tmp_path, k):
    id_, sc, kind = scenes[2][:3]
    ref = lr.run(sc, kind, stop_before=k)
    got = run_cpu(exe, tmp_path, sc, kind, stop_before=k)
    assert_discrete_equal(got, ref, (id_, k))
    assert got["stopped"] == 1
    if k == 0:
        assert got["rounds"] == 0 and not got["erase"].any() and np.array_equal(got["xw"], sc["xw"].astype(np.float64))
    if k <= 5:
        assert got["iterations"][1] == 0 and not got["level1"].any()  # bDoMore is false: no first classification, no round two


def test_cpu_program_refuses_what_the_host_header_refuses(exe, scenes, tmp_path):
    sc = dict(scenes[0][1])
    sc["edge_point"] = sc["edge_point"][::-1].copy()
    write_scene(tmp_path / "bad.bin", sc)
    r = subprocess.run([str(exe), str(tmp_path / "bad.bin"), str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 1 and "grouped by point" in r.stdout, r.stdout
