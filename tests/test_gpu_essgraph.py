"""GPU: orbfe_optimize_essential_graph, orbfe_block_sparse_solve7 and the point correction against the restatement
(tests/essgraph_ref.py) and the CPU program (tests/cpp/essgraph_cpu.cpp: the same header and host loop) on the engineered
scenes of essgraph_ref.scenes()."""
import numpy as np
import pytest

import essgraph_ref as er
from essgraph_check import (assert_discrete_equal, build_cpu_program, call_device, deviation, run_cpu, solve_cpu, tolerance)

pytestmark = pytest.mark.gpu

SCENES = er.scenes()
IDS = [s[0] for s in SCENES]


@pytest.fixture(scope="module")
def opt():
    from orb_slam2_annotate_amd import optimizer
    return optimizer


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build_cpu_program(tmp_path_factory.mktemp("essgraphcpu"))


@pytest.fixture(scope="module")
def world(exe, tmp_path_factory):
    """per scene: the restatement, its reversed-order run and the CPU program, computed once and left unchanged"""
    tmp = tmp_path_factory.mktemp("essgraphruns")
    return {id_: (sc, disc, er.run(sc), er.run(sc, reverse=True), run_cpu(exe, tmp, sc)) for id_, sc, disc in SCENES}


@pytest.mark.parametrize("id_", IDS)
def test_device_equals_restatement_and_cpu_program(opt, world, id_):
    """discrete results identical to both; sim3_out and edge_chi2 within max(16 x max(s_ref, s_cpu), 4 float32 ulps of the
    scene's largest coordinate); chi2 and lambda relative to max(|value|, 1).  Bit-equality with the CPU program is printed,
    not asserted: acos / log / exp may differ in the last place between the two libms."""
    sc, disc, ref, rev, cpu = world[id_]
    got = call_device(opt, sc)
    s_ref, s_cpu = deviation(rev, ref), deviation(cpu, ref)
    tol = tolerance(sc, s_ref, s_cpu)
    d_ref, d_cpu = deviation(got, ref), deviation(got, cpu)
    print(f"{id_}: device-ref {d_ref[0]:.2e} / {d_ref[1]:.2e}  device-cpu {d_cpu[0]:.2e} / {d_cpu[1]:.2e}  allowed {tol[0]:.2e} / {tol[1]:.2e}  "
          f"bit-equal to the CPU program: {np.array_equal(got['sim3_out'], cpu['sim3_out'])}")
    if disc:
        assert_discrete_equal(got, ref, id_)
    assert_discrete_equal(got, cpu, id_)
    assert got["host_syncs"] == got["iterations"] + got["trials"] + 1 and got["stopped"] == 0
    assert d_ref[0] <= tol[0] and d_ref[1] <= tol[1], (id_, d_ref, tol)
    assert d_cpu[0] <= tol[0] and d_cpu[1] <= tol[1], (id_, d_cpu, tol)


@pytest.mark.parametrize("id_", ["ring12", "chain150_band3_two_loops"])
def test_block_sparse_solve7_is_bit_equal_to_the_cpu_program(opt, world, exe, tmp_path, id_):
    sc, ref = world[id_][0], world[id_][2]
    colptr, rowidx, blocks, rhs, H = er.assembled(sc)
    x, ok, blocks_L = opt.block_sparse_solve7(colptr, rowidx, blocks, rhs)
    xc, okc, blc = solve_cpu(exe, tmp_path, colptr, rowidx, blocks, rhs)
    assert ok == 1 and okc == 1 and blocks_L == blc == ref["blocks_L"]
    assert np.array_equal(x, xc)  # only + - x / sqrt
    want = np.linalg.solve(H, rhs)
    assert np.abs(x - want).max() <= tolerance(sc, deviation(world[id_][3], ref), deviation(world[id_][4], ref))[0]


def test_block_sparse_solve7_reports_a_negative_pivot_in_a_middle_column(opt, world):
    colptr, rowidx, blocks, rhs, _ = er.assembled(world["chain150_band3_two_loops"][0])
    blocks = blocks.copy()
    blocks[colptr[70]][3, 3] = -1.0
    x, ok, _ = opt.block_sparse_solve7(colptr, rowidx, blocks, rhs)
    assert ok == 0 and not x.any()


def test_two_runs_give_the_same_bits(opt, world):
    sc = world["chain150_band3_two_loops"][0]
    a, b = call_device(opt, sc), call_device(opt, sc)
    assert np.array_equal(a["sim3_out"], b["sim3_out"]) and np.array_equal(a["edge_chi2"], b["edge_chi2"])
    assert a["chi2"] == b["chi2"] and a["lam"] == b["lam"] and np.array_equal(a["Tiw"], b["Tiw"])


def test_Tiw_is_R_and_t_over_s_of_sim3_out(opt, world):
    got = call_device(opt, world["ring12"][0])
    assert got["sim3_out"][9:, 7].min() > 1.01  # the corrected vertices keep a scale
    for rec, T in zip(got["sim3_out"], got["Tiw"]):
        assert np.array_equal(T, er.tiw(er.from_record(rec)))


def test_table_form_of_the_point_correction_equals_the_array_form_bit_for_bit(opt, world):
    import orb_slam2_annotate_amd as amd
    sc = world["ring12"][0]
    out = call_device(opt, sc)["sim3_out"]
    rng = np.random.default_rng(3)
    n = 200  # more than one workgroup
    xw = rng.normal(size=(n, 3)).astype(np.float32) * 5.0
    ref_vertex = rng.integers(0, 12, n).astype(np.int32)
    ref_vertex[::17] = -1
    got = opt.essential_graph_correct_points(sc["sim3"], out, xw, ref_vertex)
    want = er.correct_points(sc["sim3"], out, xw, ref_vertex)
    assert np.array_equal(got[ref_vertex < 0], xw[ref_vertex < 0])
    assert np.abs(got - want).max() <= 4 * 2.0 ** -23 * max(1.0, float(np.abs(want).max()))
    assert np.abs(got - xw)[ref_vertex >= 9].max() > 1e-2  # the corrected key frames move their points
    slot = rng.permutation(n + 9)[:n].astype(np.int32)
    mp = amd.MapPoints(n + 9)
    mp.update(slot, xw, np.tile(np.array([0, 0, 1], np.float32), (n, 1)), np.full(n, 0.1, np.float32), np.full(n, 100.0, np.float32),
              np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8))
    mp.essential_graph_correct(slot, sc["sim3"], out, ref_vertex)
    assert np.array_equal(mp.positions(slot), got)
    mp.close()


def test_an_edge_between_two_fixed_vertices_is_inert(opt, world):
    sc = dict(world["ring12"][0])
    base = call_device(opt, sc)
    fixed = sc["is_fixed"].copy()
    fixed[5] = 1
    sc["is_fixed"] = fixed
    sc2 = dict(sc)
    sc2["edge_i"] = np.append(sc["edge_i"], 0).astype(np.int32)
    sc2["edge_j"] = np.append(sc["edge_j"], 5).astype(np.int32)
    sc2["edge_kind"] = np.append(sc["edge_kind"], 0).astype(np.uint8)
    sc2["sim3_meas"] = sc["sim3_meas"].copy()
    sc2["sim3_meas"][5, 4] += 0.25  # the edge's measurement disagrees with the estimates: a chi2 of its own
    sc["sim3_meas"] = sc2["sim3_meas"]
    want = call_device(opt, sc)
    got = call_device(opt, sc2)
    assert np.array_equal(got["sim3_out"], want["sim3_out"]) and got["chi2"] == want["chi2"] and got["trials"] == want["trials"]
    assert np.array_equal(got["edge_chi2"][:-1], want["edge_chi2"])
    S, M = [er.from_record(r) for r in sc2["sim3"]], [er.from_record(r) for r in sc2["sim3_meas"]]
    e = er.edge_error(er.sim3_mul(M[5], er.sim3_inverse(M[0])), S[0], S[5])
    assert got["edge_chi2"][-1] > 1e-3 and abs(got["edge_chi2"][-1] - e @ e) <= 1e-9 * max(1.0, e @ e)
    assert base["n_free"] == want["n_free"] + 1


def test_no_iterations_returns_the_inputs(opt, world):
    sc = world["ring12"][0]
    got = call_device(opt, sc, n_iterations=0)
    assert np.array_equal(got["sim3_out"], sc["sim3"]) and got["iterations"] == 0 and got["trials"] == 0 and got["host_syncs"] == 1
    all_fixed = dict(sc)
    all_fixed["is_fixed"] = np.ones(12, np.uint8)
    got = call_device(opt, all_fixed)
    assert np.array_equal(got["sim3_out"], sc["sim3"]) and got["n_free"] == 0 and got["iterations"] == 0
    want = er.run(sc, n_iterations=0)["edge_chi2"]  # every edge is inactive: its chi2 is that of the inputs
    assert want[8] > 0.1 and np.abs(got["edge_chi2"] - want).max() <= 1e-12 * max(1.0, want.max())


def test_refused_inputs(opt, world):
    from orb_slam2_annotate_amd._lib import OrbfeError
    sc = world["chain5"][0]
    for change, text in ((dict(edge_j=sc["edge_i"]), "joins a vertex to itself"), (dict(edge_j=sc["edge_j"] + 9), "out of range"),
                         (dict(n_iterations=-1), "negative n_iterations")):
        bad = dict(sc)
        bad.update(change)
        with pytest.raises(OrbfeError, match=text):
            call_device(opt, bad)
    for col, val, text in ((7, 0.0, "scale of sim3 is not positive"), (5, np.nan, "not finite")):
        bad = dict(sc)
        bad["sim3"] = sc["sim3"].copy()
        bad["sim3"][2, col] = val
        with pytest.raises(OrbfeError, match=text):
            call_device(opt, bad)
