"""GPU: orbfe_local_bundle_adjustment / orbfe_bundle_adjustment / the table form against the restatement (tests/lba_ref.py)
on its engineered scenes: discrete results (erase[], level1[], iterations, trials, termination reasons) identical,
continuous ones within max(16 x max(s_ref, s_cpu), 4 float32 ulps), s_ref the restatement's forward-against-reversed
deviation and s_cpu the CPU program's deviation from the restatement, both measured here per scene."""
import ctypes as C

import numpy as np
import pytest

import lba_ref as lr
from lba_check import assert_discrete_equal, build_cpu_program, deviation, run_cpu, tolerance

pytestmark = pytest.mark.gpu

ARGS = ("edge_pose", "edge_point", "u", "v", "u_right", "inv_sigma2")


def device_run(sc, kind="local", stop_flag=None):
    import orb_slam2_annotate_amd as amd
    a = [sc["n_local"], sc["Tcw"], sc["cam"], sc["xw"]] + [sc[k] for k in ARGS]
    if kind == "local":
        T, x, erase, level1, st, chi2 = amd.local_bundle_adjustment(*a, local_is_fixed=sc.get("local_is_fixed"), stop_flag=stop_flag)
    else:
        T, x, st, chi2 = amd.bundle_adjustment(*a, n_iterations=kind[1], robust=kind[2], local_is_fixed=sc.get("local_is_fixed"))
        erase = level1 = np.zeros(len(sc["u"]), np.uint8)
    r = st["rounds"]
    pad = lambda v: [v[i] if i < r else type(v[0])(0) for i in range(2)]
    return dict(Tcw=T.copy(), xw=x.copy(), erase=erase.copy(), level1=level1.copy(), edge_chi2=chi2.copy(), rounds=r,
                stopped=st["stopped"], iterations=pad(st["iterations"]), trials=pad(st["trials"]), termination=pad(st["termination"]),
                lam=pad(st["lam"]), chi2=pad(st["chi2"]), host_syncs=st["host_syncs"])


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("lbagpu")
    exe = build_cpu_program(tmp)
    out = {}
    for id_, sc, kind in lr.gpu_scenes():
        ref, rev = lr.run(sc, kind), lr.run(sc, kind, reverse=True)
        cpu = run_cpu(exe, tmp, sc, kind)
        out[id_] = (sc, kind, ref, tolerance(sc, deviation(rev, ref), deviation(cpu, ref)), cpu)
    return out


IDS = [id_ for id_, _, _ in lr.gpu_scenes()]


@pytest.mark.parametrize("id_", IDS)
def test_device_equals_the_restatement(world, id_):
    sc, kind, ref, tol, cpu = world[id_]
    got = device_run(sc, kind)
    d = deviation(got, ref)
    print(f"{id_}: device {d[0]:.3e} / {d[1]:.3e}  allowed {tol[0]:.3e} / {tol[1]:.3e}  syncs {got['host_syncs']}")
    assert_discrete_equal(got, ref, id_)
    assert d[0] <= tol[0] and d[1] <= tol[1], (id_, d, tol)
    assert got["host_syncs"] == sum(got["iterations"]) + sum(got["trials"]) + 1
    # the CPU program runs the same header in the same summation orders: the same bits
    assert_discrete_equal(got, cpu, id_)
    for k in ("Tcw", "xw", "edge_chi2"):
        assert np.array_equal(got[k].view(np.uint8), np.ascontiguousarray(cpu[k]).view(np.uint8)), (id_, k, "device and CPU program differ")
    assert got["lam"] == cpu["lam"] and got["chi2"] == cpu["chi2"], id_


@pytest.mark.parametrize("id_", ["l3f2p40-mixed", "l7f5p300", "global-20-robust"])
def test_two_runs_give_the_same_bits(world, id_):
    sc, kind = world[id_][:2]
    a, b = device_run(sc, kind), device_run(sc, kind)
    for k in ("Tcw", "xw", "erase", "level1", "edge_chi2"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), (id_, k)
    assert a["lam"] == b["lam"] and a["chi2"] == b["chi2"]


def test_stop_flag_raised_before_the_call_leaves_everything_as_it_came(world):
    sc, kind = world["l3f2p40-mixed"][:2]
    got = device_run(sc, kind, stop_flag=C.c_int(1))
    ref = lr.run(sc, kind, stop_before=0)
    assert got["stopped"] == 1 and got["rounds"] == 0 and not got["erase"].any()
    assert np.array_equal(got["xw"], sc["xw"].astype(np.float64))
    assert np.array_equal(got["Tcw"], ref["Tcw"])  # the inputs through Converter::toSE3Quat and back
    assert np.abs(got["Tcw"] - sc["Tcw"][:sc["n_local"]]).max() < 1e-6


@pytest.mark.parametrize("id_", ["l3f2p40-mixed", "point-all-level1"])
def test_table_form_equals_the_array_form_bit_for_bit(world, id_):
    import orb_slam2_annotate_amd as amd
    sc, kind = world[id_][:2]
    n = len(sc["xw"])
    slot = (np.arange(n, dtype=np.int32) * 3 + 5)[::-1].copy()
    mp = amd.MapPoints(int(slot.max()) + 7)
    mp.update(slot, sc["xw"], np.tile(np.array([0, 0, 1], np.float32), (n, 1)), np.full(n, 0.1, np.float32), np.full(n, 100.0, np.float32),
              np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8))
    want = device_run(sc, kind)
    T, x, erase, level1, st, chi2 = mp.local_bundle_adjustment(slot, sc["n_local"], sc["Tcw"], sc["cam"], *[sc[k] for k in ARGS],
                                                               local_is_fixed=sc.get("local_is_fixed"))
    for got, k in ((T, "Tcw"), (x, "xw"), (erase, "erase"), (level1, "level1"), (chi2, "edge_chi2")):
        assert np.array_equal(np.ascontiguousarray(got).view(np.uint8), want[k].view(np.uint8)), (id_, k)
    # the table holds the optimised positions as floats: a second adjustment starts from them
    again = mp.local_bundle_adjustment(slot, sc["n_local"], sc["Tcw"], sc["cam"], *[sc[k] for k in ARGS],
                                       local_is_fixed=sc.get("local_is_fixed"))
    sc2 = dict(sc)
    sc2["xw"] = x.astype(np.float32)
    want2 = device_run(sc2, kind)
    assert np.array_equal(again[1].view(np.uint8), want2["xw"].view(np.uint8))


def test_refusals(world):
    import orb_slam2_annotate_amd as amd
    sc = world["l1f2p6"][0]
    bad = dict(sc)
    bad["edge_point"] = sc["edge_point"][::-1].copy()
    with pytest.raises(Exception, match="grouped by point"):
        device_run(bad)
    bad = dict(sc)
    bad["xw"] = sc["xw"].copy()
    bad["xw"][0, 0] = np.nan
    with pytest.raises(Exception, match="not finite"):
        device_run(bad)
    assert amd is not None
