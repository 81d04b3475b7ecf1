"""orbfe_optimize_sim3* (Optimizer::OptimizeSim3 in one launch, one wave per loop candidate) against the float64 restatement
tests/optimize_sim3_ref.py under the pass condition of tests/optimize_sim3_check.py: pair counts 0, 1, 9, 10, 14 -> 9 (the
early return), 63, 64, 65 (the wave edge), 129 and 300, outlier shares 0 and 0.2, fix_scale both ways; and the properties
of the call: determinism, multi = single, 256-byte line ends with sentinels, refusals, the chain from Sim3Solver.

Measured on an MI355X over the 37 scenes: largest |difference| of a sim3_out entry 7.1e-14 (allowed: 1.5e-12, or 4 float32
ulps of the entry where that is more), largest relative difference of a classification chi2 3.0e-12 (allowed 2.4e-11)."""
import ctypes as C

import numpy as np
import pytest

import optimize_sim3_check as chk
import optimize_sim3_ref as osr
import sim3_ref as sr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


@pytest.fixture(scope="module")
def scenes():
    """every scene with its reference result, computed once"""
    return {id_: (sc, osr.run(sc)) for id_, sc in osr.gpu_scenes()}


KEYS = ("x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "cam1", "cam2", "sim3_in", "th2", "fix_scale")


def single(amd, sc):
    return amd.optimize_sim3(*[sc[k] for k in KEYS])


def batch(scs):
    cat = lambda k, shape: np.concatenate([np.asarray(sc[k], np.float32).reshape(shape) for sc in scs])
    return dict(pair_off=np.concatenate([[0], np.cumsum([len(sc["x3dc1"]) for sc in scs])]).astype(np.int32),
                x3dc1=cat("x3dc1", (-1, 3)), x3dc2=cat("x3dc2", (-1, 3)), obs1=cat("obs1", (-1, 2)), obs2=cat("obs2", (-1, 2)),
                inv_sigma2_1=cat("inv_sigma2_1", -1), inv_sigma2_2=cat("inv_sigma2_2", -1), cam1=cat("cam1", (1, 4)),
                cam2=cat("cam2", (1, 4)), sim3_in=cat("sim3_in", (1, 13)), th2=np.array([sc["th2"] for sc in scs], np.float32),
                fix_scale=np.array([sc["fix_scale"] for sc in scs], np.uint8))


def multi(amd, b):
    return amd.optimize_sim3_multi(b["pair_off"], *[b[k] for k in KEYS])


def same_bits(a, b):
    return a[0] == b[0] and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a[1:3] + a[4:], b[1:3] + b[4:])) \
        and repr(a[3]) == repr(b[3])


@pytest.mark.parametrize("id_", [id_ for id_, _ in osr.gpu_scenes()])
def test_scene_equals_the_reference(amd, scenes, id_):
    sc, r = scenes[id_]
    got = single(amd, sc)
    print(id_, "deviation of sim3_out %.3e, of a classification chi2 %.3e (relative)" % chk.deviations(r, got))
    chk.check(r, got)
    if id_ == osr.EARLY[0]:
        assert got[0] == 0 and got[3]["rounds"] == 1 and int((got[2] == 1).sum()) == 5


def test_all_scenes_in_one_launch_and_the_measured_deviations(amd, scenes):
    ids = list(scenes)
    n_in, sim3, bad, st, c12, c21 = multi(amd, batch([scenes[i][0] for i in ids]))
    off = np.concatenate([[0], np.cumsum([len(scenes[i][0]["x3dc1"]) for i in ids])])
    d_sim3 = d_chi2 = 0.0
    for p, i in enumerate(ids):
        got = (int(n_in[p]), sim3[p], bad[off[p]:off[p + 1]], st[p], c12[off[p]:off[p + 1]], c21[off[p]:off[p + 1]])
        a, b = chk.check(scenes[i][1], got)
        d_sim3, d_chi2 = max(d_sim3, a), max(d_chi2, b)
        assert same_bits(got, single(amd, scenes[i][0])), i
    rec = chk.recorded()
    print("measured: sim3_out %.3e (16 x max(s_sim3, s_cpu) = %.3e), classification chi2 %.3e relative (16 x s_chi2 = %.3e)"
          % (d_sim3, 16 * max(rec["s_sim3"], rec["s_cpu"]), d_chi2, 16 * rec["s_chi2"]))


def test_two_calls_give_identical_bits(amd, scenes):
    for id_ in ("n300-fix0-out20", "n65-fix1-out0", osr.EARLY[0]):
        sc, _ = scenes[id_]
        assert same_bits(single(amd, sc), single(amd, sc)), id_


def test_multi_equals_single_calls_for_mixed_problems(amd):
    scs = [osr.scene(1, 0, 0, 0.0), osr.scene(2, 9, 1, 0.2, th2=7.5), osr.scene(3, 10, 0, 0.0, cam2=osr.CAM_B),
           osr.scene(4, 65, 1, 0.2, cam2=osr.CAM_B * np.float32(0.5)), osr.scene(5, 300, 0, 0.2, th2=12.0)]
    n_in, sim3, bad, st, c12, c21 = multi(amd, batch(scs))
    off = np.concatenate([[0], np.cumsum([len(sc["x3dc1"]) for sc in scs])])
    for p, sc in enumerate(scs):
        got = (int(n_in[p]), sim3[p], bad[off[p]:off[p + 1]], st[p], c12[off[p]:off[p + 1]], c21[off[p]:off[p + 1]])
        assert same_bits(got, single(amd, sc)), p
    assert st[0]["rounds"] == 0 and st[1]["rounds"] == 1 and st[4]["rounds"] == 2


@pytest.mark.parametrize("counts", [(15, 0, 16, 17), (31, 32, 0, 33), (255, 1, 0, 1), (0, 256, 1), (257, 0)])
def test_array_ends_around_a_256_byte_line_and_sentinels(amd, counts):
    """Pair records are 16 bytes (16 to a line), chi2 entries 8 (32 to a line), bad flags 1 (256 to a line): cumulative counts
    that end just before, on and after a line.  Everything past a call's own entries keeps the sentinel."""
    from orb_slam2_annotate_amd import _lib
    from orb_slam2_annotate_amd._lib import OptSim3StatsC, ptr
    scs = [osr.scene(7 + p, n, p & 1, 0.2) for p, n in enumerate(counts)]
    b = batch(scs)
    K, N, PAD = len(scs), int(b["pair_off"][-1]), 40
    out = np.full(8 * K + PAD, np.float64(-7.25))
    bad = np.full(N + PAD, 0xA5, np.uint8)
    c12, c21 = np.full(N + PAD, np.float64(-7.25)), np.full(N + PAD, np.float64(-7.25))
    n_in = np.full(K + PAD, -77, np.int32)
    st = (OptSim3StatsC * K)()
    rc = _lib.load().orbfe_optimize_sim3_multi(0, K, ptr(b["pair_off"]), *[ptr(np.ascontiguousarray(b[k])) for k in KEYS],
                                               ptr(out), ptr(bad), ptr(n_in), C.cast(st, C.c_void_p), ptr(c12), ptr(c21))
    assert rc == 0
    assert (out[8 * K:] == -7.25).all() and (bad[N:] == 0xA5).all() and (c12[N:] == -7.25).all() and (c21[N:] == -7.25).all()
    assert (n_in[K:] == -77).all()
    for p, sc in enumerate(scs):
        lo, hi = int(b["pair_off"][p]), int(b["pair_off"][p + 1])
        want = single(amd, sc)
        assert n_in[p] == want[0] and out[8 * p:8 * p + 8].tobytes() == want[1].tobytes(), p
        assert bad[lo:hi].tobytes() == want[2].tobytes() and (bad[lo:hi] <= 2).all(), p
        assert c12[lo:hi].tobytes() == want[4].tobytes() and c21[lo:hi].tobytes() == want[5].tobytes(), p
        if hi == lo:  # nothing runs: no round, n_in 0, the incoming transform
            q, t, s = osr.sim3_from_record(sc["sim3_in"])
            assert n_in[p] == 0 and st[p].rounds == 0 and np.array_equal(out[8 * p:8 * p + 8], np.array(q + t + [s]))


def test_refusals_carry_the_host_headers_message_and_leave_the_thread_usable(amd, scenes):
    from orb_slam2_annotate_amd import _lib
    scs = [scenes[i][0] for i in ("n10-fix0-out0", "n65-fix1-out20")]
    b = batch(scs)

    def refused(message, **kw):
        a = dict(b, **kw)
        with pytest.raises(amd.OrbfeError) as ei:
            multi(amd, a)
        assert ei.value.code == _lib.ERR_INVALID and message in str(ei.value), str(ei.value)
    refused("pair_off must not descend", pair_off=np.array([0, 80, 75], np.int32))
    refused("pair_off[0] must be 0", pair_off=np.array([1, 10, 75], np.int32))
    refused("th2 must be positive and finite", th2=np.array([10.0, 0.0], np.float32))
    refused("th2 must be positive and finite", th2=np.array([np.nan, 10.0], np.float32))
    refused("th2 must be positive and finite", th2=np.array([10.0, np.inf], np.float32))
    n = 16385
    z = lambda k: np.zeros((n, k), np.float32)
    with pytest.raises(amd.OrbfeError) as ei:
        amd.optimize_sim3(z(3), z(3), z(2), z(2), z(1), z(1), osr.CAM_A, osr.CAM_A, scs[0]["sim3_in"])
    assert ei.value.code == _lib.ERR_INVALID and "more than 16384 pairs" in str(ei.value)
    with pytest.raises(amd.OrbfeError) as ei:
        amd.optimize_sim3_multi(np.array([0, n], np.int32), z(3), z(3), z(2), z(2), z(1), z(1), osr.CAM_A, osr.CAM_A,
                                scs[0]["sim3_in"], [10.0], [0])
    assert "more than 16384 pairs in one problem" in str(ei.value)
    lib = _lib.load()
    assert lib.orbfe_optimize_sim3_multi(0, 1, None, *([None] * 17)) == _lib.ERR_INVALID
    assert b"NULL pair_off" in lib.orbfe_last_error()
    assert lib.orbfe_optimize_sim3_multi(0, -1, _lib.ptr(b["pair_off"]), *([None] * 17)) == _lib.ERR_INVALID
    assert b"negative problem count" in lib.orbfe_last_error()
    assert lib.orbfe_optimize_sim3_multi(-1, 0, _lib.ptr(b["pair_off"]), *([None] * 17)) == _lib.ERR_INVALID
    assert b"negative device" in lib.orbfe_last_error()
    # a later valid call on the same thread
    chk.check(scenes["n65-fix1-out20"][1], single(amd, scs[1]))


def test_chain_from_sim3solver(amd):
    """Sim3Solver.evaluate_all -> iterate -> its sim3[13] fed unchanged as sim3_in (the hand-over layout), on the good
    candidate of sim3_ref's class scene with exact projections as observations: the optimised transform is closer to the
    planted one than the RANSAC estimate was."""
    sc = dict(sr.gpu_scenes())["class-fix0"]
    c = sc["cands"][1]
    s = amd.Sim3Solver(c["indices1"], c["x1"], c["x2"], c["sigma2_1"], c["sigma2_2"], c["cam1"], c["cam2"], c["N1"], sc["fix_scale"])
    s.SetRansacParameters(0.99, sr.CLASS_MIN_INLIERS, 300)
    amd.Sim3Solver.evaluate_all([s], [c["triples"]])
    T, vb, n = s.find()
    assert T is not None
    rec = np.concatenate([s.GetEstimatedRotation().reshape(9), s.GetEstimatedTranslation(), [s.GetEstimatedScale()]]).astype(np.float32)
    keep = vb[c["indices1"]]
    x1, x2 = c["x1"][keep].astype(np.float64), c["x2"][keep].astype(np.float64)
    s0, R, t = sr.planted(0)
    # observations: the planted geometry seen by both cameras (X1 through camera 1, S12^-1 X1 ... = X2 through camera 2)
    proj = lambda X, K: np.stack([K[0] * X[:, 0] / X[:, 2] + K[2], K[1] * X[:, 1] / X[:, 2] + K[3]], axis=1)
    X1p = s0 * x2 @ R.T + t          # where the planted transform puts X2 in camera 1
    X2p = (x1 - t) @ R / s0          # and X1 in camera 2
    obs1, obs2 = proj(X1p, c["cam1"].astype(np.float64)), proj(X2p, c["cam2"].astype(np.float64))
    w = np.ones(len(x1), np.float32)
    n_in, out, bad, st, _, _ = amd.optimize_sim3(c["x1"][keep], c["x2"][keep], obs1, obs2, w, w, c["cam1"], c["cam2"], rec, 10.0, False)
    assert st["rounds"] == 2 and n_in >= 10
    Ro, to, so = amd.sim3_to_Rts(out)
    want = np.concatenate([s0 * R, t[:, None]], axis=1)
    before = np.abs(np.concatenate([float(rec[12]) * rec[:9].reshape(3, 3).astype(np.float64), rec[9:12, None]], axis=1) - want).max()
    after = np.abs(np.concatenate([so * Ro, to[:, None]], axis=1) - want).max()
    print("distance to the planted [sR | t]: RANSAC %.3e, optimised %.3e" % (before, after))
    assert after < before
