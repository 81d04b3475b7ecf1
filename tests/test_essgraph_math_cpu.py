"""CPU: csrc/essgraph_math.h and csrc/essgraph_host.h -- the arithmetic, work items, tables and schedule the kernels of
k_essgraph.hip run -- as a stand-alone program in the device's summation order (tests/cpp/essgraph_cpu.cpp) against the
restatement (tests/essgraph_ref.py) on the scenes of the GPU test: discrete results identical, continuous ones within the
reordering noise."""
import subprocess

import numpy as np
import pytest

import essgraph_ref as er
from essgraph_check import (agrees, assert_discrete_equal, build_cpu_program, deviation, recorded, run_cpu, solve_cpu, tolerance,
                            write_scene)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_cpu_program(tmp_path_factory.mktemp("essgraphcpu"))


@pytest.fixture(scope="module")
def scenes():
    return [(id_, sc, disc, er.run(sc), er.run(sc, reverse=True), er.run(sc, sparse=True)) for id_, sc, disc in er.scenes()]


def test_cpu_program_equals_the_restatement(exe, scenes, tmp_path):
    """discrete results identical (scenes of the discrete set); continuous ones within 16 x the restatement's own deviation (or
    4 float32 ulps of the largest coordinate): the larger of forward-against-reversed edge order and dense-against-sparse
    route, both measured here per scene"""
    measured = {}
    for id_, sc, disc, ref, rev, spr in scenes:
        got = run_cpu(exe, tmp_path, sc)
        if disc:
            assert_discrete_equal(got, ref, id_)
            assert_discrete_equal(rev, ref, id_)
            assert_discrete_equal(spr, ref, id_)
        d, s_rev, s_spr = deviation(got, ref), deviation(rev, ref), deviation(spr, ref)
        s_ref = (max(s_rev[0], s_spr[0]), max(s_rev[1], s_spr[1]))
        tol = tolerance(sc, s_ref, (0.0, 0.0))
        print(f"{id_}: s_cpu {d[0]:.2e} / {d[1]:.2e}  s_ref {s_rev[0]:.2e} / {s_rev[1]:.2e}  sparse route {s_spr[0]:.2e} / {s_spr[1]:.2e}  "
              f"allowed {tol[0]:.2e} / {tol[1]:.2e}")
        assert d[0] <= tol[0] and d[1] <= tol[1], (id_, d, tol)
        assert np.array_equal(got["Tiw"], ref["Tiw"]) or np.abs(got["Tiw"] - ref["Tiw"]).max() <= tol[0], id_
        for name, val in (("s_ref", s_rev), ("s_sparse", s_spr), ("s_cpu", d)):
            measured[f"{id_}.{name}_abs"], measured[f"{id_}.{name}_rel"] = val
    rec = {k: v for k, v in recorded().items() if not k.endswith(".j_gap")}
    assert set(rec) == set(measured), "profiles/essential_graph_tolerance.txt lists other scenes than the test measures"
    off = {k: (measured[k], rec[k]) for k in rec if not agrees(measured[k], rec[k])}
    assert not off, f"profiles/essential_graph_tolerance.txt disagrees with what is measured: {off}"


def test_cpu_solver_equals_numpy_on_an_assembled_system(exe, scenes, tmp_path):
    for idx in (2, 5):
        id_, sc = scenes[idx][0], scenes[idx][1]
        colptr, rowidx, blocks, rhs, H = er.assembled(sc)
        x, ok, blocks_L = solve_cpu(exe, tmp_path, colptr, rowidx, blocks, rhs)
        assert ok == 1 and blocks_L == scenes[idx][3]["blocks_L"], id_
        want = np.linalg.solve(H, rhs)
        assert np.abs(x - want).max() <= tolerance(sc, (0.0, 0.0), (0.0, 0.0))[0], (id_, np.abs(x - want).max())


def test_cpu_solver_reports_a_negative_pivot_in_a_middle_column(exe, scenes, tmp_path):
    colptr, rowidx, blocks, rhs, _ = er.assembled(scenes[2][1])
    blocks = blocks.copy()
    blocks[colptr[5]][3, 3] = -1.0
    x, ok, _ = solve_cpu(exe, tmp_path, colptr, rowidx, blocks, rhs)
    assert ok == 0 and not x.any()


def test_cpu_program_refuses_what_the_host_header_refuses(exe, scenes, tmp_path):
    sc = dict(scenes[0][1])
    sc["edge_j"] = sc["edge_i"].copy()
    write_scene(tmp_path / "bad.bin", sc)
    r = subprocess.run([str(exe), "opt", str(tmp_path / "bad.bin"), str(tmp_path / "o.bin")], capture_output=True, text=True)
    assert r.returncode == 1 and "joins a vertex to itself" in r.stdout, r.stdout
