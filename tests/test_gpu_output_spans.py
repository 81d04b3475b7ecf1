"""The eight device round trips whose outputs come back as ONE span of the arena (csrc/arena.h: open_span / close_span /
down_span) -- Sim3 RANSAC, PnP RANSAC and Refine, Initializer RANSAC, Initializer reconstruct, pose optimisation on arrays and
on the map-point table, OptimizeSim3, triangulation -- at the smallest shapes at which a span can go wrong: K = 3 owners with
0, 2 and 1 items, one of them with 33 entries (two mask words) and one with the minimal number, a pose problem with n < 3
beside one with n = 5, and one call each with no items at all (the `n ? n : 1` carves).

Every array the Python wrappers allocate for a call is here the middle of a larger buffer filled with a sentinel byte.  After
the call the bytes around it are untouched, and what the call returned equals the Python reference of that call under the
comparison rule of that call's own GPU test."""
import numpy as np
import pytest

import initializer_ref as ir
import initializer_reconstruct_ref as rr
import optimize_sim3_check as osc
import optimize_sim3_ref as osr
import pnp_ref as pr
import pose_opt_ref as por
import sim3_ref as sr
import triangulate_ref as tr
from pose_opt_check import check_against
from frustum_ref import BOUNDS
from test_gpu_pose_opt import _table_problem
from test_gpu_triangulate import call as triangulate_call

pytestmark = pytest.mark.gpu

PAD, SENTINEL = 256, 0xA5


class GuardedNumpy:
    """numpy, but zeros(), full() and array() -- what the wrappers allocate their outputs with -- give the middle of a larger
    buffer"""

    def __init__(self):
        self.made = []

    def __getattr__(self, name):
        return getattr(np, name)

    def _alloc(self, shape, dtype, fill):
        dtype = np.dtype(dtype)
        nbytes = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
        buf = np.full(nbytes + 2 * PAD, SENTINEL, np.uint8)
        a = buf[PAD:PAD + nbytes].view(dtype).reshape(shape)
        a[...] = fill
        self.made.append((buf, nbytes))
        return a

    def zeros(self, shape, dtype=float):
        return self._alloc(shape, dtype, 0)

    def full(self, shape, fill_value, dtype=None):
        return self._alloc(shape, np.asarray(fill_value).dtype if dtype is None else dtype, fill_value)

    def array(self, obj, dtype=None):  # (the copy of a caller's flag array that a call then writes into)
        src = np.array(obj, dtype=dtype)
        a = self._alloc(src.shape, src.dtype, 0)
        a[...] = src
        return a

    def check(self, what):
        assert self.made, what
        for i, (buf, nbytes) in enumerate(self.made):
            assert (buf[:PAD] == SENTINEL).all() and (buf[PAD + nbytes:] == SENTINEL).all(), (what, "array", i, "of", len(self.made))


@pytest.fixture
def guard(monkeypatch):
    from orb_slam2_annotate_amd import initializer, local_mapping, loop_closing, map_points, optimizer, relocalization
    g = GuardedNumpy()
    for module in (initializer, local_mapping, loop_closing, map_points, optimizer, relocalization):
        monkeypatch.setattr(module, "np", g)
    return g


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


# ------------------------------------------------------------------------------------------------------------ Sim3Solver
def _sim3(amd, sc):
    o = sr.operands(sc)
    return amd.sim3_ransac_multi(o["pair_off"], o["x1"], o["x2"], o["max1"], o["max2"], o["cam1"], o["cam2"], o["fix_scale"],
                                 o["hyp_off"], o["triples"])


def test_sim3_ransac(amd, guard):
    sc = sr.scene(0, dict(fix_scale=0, cands=[dict(n=5, H=0, outliers=0.0), dict(n=33, H=2, outliers=0.0), dict(n=3, H=1, outliers=0.0)]))
    sr.compare("span", sc, sr.run(sc), *_sim3(amd, sc), sr.s_sim3())
    none = sr.scene(1, dict(fix_scale=1, cands=[dict(n=5, H=0, outliers=0.0), dict(n=3, H=0, outliers=0.0)]))
    n_inl, status, sim3, words, word_off = _sim3(amd, none)
    assert len(n_inl) == len(status) == len(sim3) == len(words) == 0 and word_off.tolist() == [0, 0, 0]
    guard.check("sim3_ransac_multi")


# ------------------------------------------------------------------------------------------------------------- PnPsolver
def _pnp(amd, cands):
    off = np.concatenate([[0], np.cumsum([len(c["p3d"]) for c in cands])]).astype(np.int32)
    ho = np.concatenate([[0], np.cumsum([len(c["sets"]) for c in cands])]).astype(np.int32)
    return amd.pnp_solve_multi(off, np.concatenate([c["p3d"] for c in cands]), np.concatenate([c["p2d"] for c in cands]),
                               np.concatenate([c["max_err"] for c in cands]), np.stack([c["cam"] for c in cands]), ho,
                               np.concatenate([c["sets"].reshape(-1, 4) for c in cands]), [c["min_inliers"] for c in cands])


def test_pnp_ransac_and_refine(amd, guard):
    """orbfe_pnp_solve_multi makes both round trips of pnp.hip: the hypotheses, then the Refine records.  Every point an exact
    inlier and min_inliers = 4, so that the 33-point candidate has records (the rule of tests/test_gpu_pnp.py)."""
    cands = [pr.make_candidate(700, 5, 0), pr.make_candidate(701, 33, 2, inlier_frac=1.0, noise=0.0),
             pr.make_candidate(702, 4, 1, inlier_frac=1.0, noise=0.0)]
    for c in cands:
        c["min_inliers"] = 4
    r = _pnp(amd, cands)
    tol, st = pr.s_pnp(), pr.new_stats()
    h = q = 0
    for k, c in enumerate(cands):
        n, w = len(c["p3d"]), (len(c["p3d"]) + 31) // 32
        counts = []
        for j, s in enumerate(c["sets"]):
            words = r["mask_words"][r["word_off"][k] + j * w: r["word_off"][k] + (j + 1) * w]
            pr.compare_item(c, pr.ref_item(c, s), (int(r["n_inliers"][h]), int(r["status"][h]), r["pose"][h], words), tol, st)
            counts.append(int(r["n_inliers"][h]))
            h += 1
        rec = pr.scan_records(counts, c["min_inliers"])
        h0 = h - len(c["sets"])
        assert [int(x) - h0 for x in r["rec_hyp"][r["rec_off"][k]:r["rec_off"][k + 1]]] == rec
        for j, hh in enumerate(rec):
            mask = pr.words_to_mask(r["mask_words"][r["word_off"][k] + hh * w: r["word_off"][k] + (hh + 1) * w], n)
            words = r["rec_mask_words"][r["rec_word_off"][k] + j * w: r["rec_word_off"][k] + (j + 1) * w]
            pr.compare_item(c, pr.ref_item(c, np.flatnonzero(mask)),
                            (int(r["rec_n_inliers"][q]), int(r["rec_status"][q]), r["rec_pose"][q], words), tol, st)
            q += 1
    print("pnp", st)
    assert q >= 2 and st["excluded"] == 0 and st["guard"] == 0, st
    none = _pnp(amd, [pr.make_candidate(703, 5, 0), pr.make_candidate(704, 4, 0)])
    assert len(none["n_inliers"]) == len(none["rec_hyp"]) == 0 and list(none["word_off"]) == list(none["rec_off"]) == [0, 0, 0]
    guard.check("pnp_solve_multi")


# ----------------------------------------------------------------------------------------------------------- Initializer
def _init(amd, sc):
    o = ir.operands(sc)
    return amd.initializer_ransac_multi(o["pair_off"], o["pairs"], o["T1"], o["T2"], o["sigma"], o["hyp_off"], o["sets"])


def test_initializer_ransac(amd, guard):
    s_model, s_score = ir.recorded()
    tol = ir.allowance(s_model), ir.allowance(s_score)
    rng = np.random.default_rng(ir.SEED)
    sc = dict(probs=[ir.problem(rng, "planar", 9, 0), ir.problem(rng, "planar", 33, 2, sigma=2.0), ir.problem(rng, "general", 8, 1)])
    c = ir.compare("span", sc, ir.run(sc), *_init(amd, sc), tol)
    print("initializer", c)
    none = dict(probs=[ir.problem(rng, "planar", 9, 0), ir.problem(rng, "general", 8, 0)])
    score, status, n_inl, model, h12, words, word_off = _init(amd, none)
    assert len(score) == len(status) == len(n_inl) == len(model) == len(h12) == len(words) == 0 and word_off.tolist() == [0, 0, 0]
    guard.check("initializer_ransac_multi")


def _reconstruct(amd, sc):
    o = rr.operands(sc)
    return amd.initializer_reconstruct_multi(o["pair_off"], o["pairs"], o["model_kind"], o["model"], o["K4"], o["sigma"],
                                             o["inlier_words"], o["in_word_off"])


def test_initializer_reconstruct(amd, guard):
    """An owner's items are its 8 (H) or 4 (F) motion hypotheses: a problem without pairs beside the 33-pair and the 1-pair
    scenes of tests/test_gpu_initializer_reconstruct.py, then two problems without pairs alone (no slot at all)."""
    scenes = {id_: sc for id_, sc, _ in rr.scenes()}
    empty = rr.problem(rr.MF, ir.fundamental(), np.zeros((0, 4), np.float32), np.zeros(0, bool))
    sc = dict(probs=[empty] + scenes["n33"]["probs"] + scenes["n1"]["probs"])
    print("reconstruct", rr.compare("span", sc, rr.run(sc), rr.split(sc, _reconstruct(amd, sc))))
    none = dict(probs=[empty, dict(empty, kind=rr.MH, model=ir.plant("planar")[2])])
    out = _reconstruct(amd, none)
    assert out["hyp_off"].tolist() == [0, 4, 12] and out["slot_off"].tolist() == [0, 0, 0] and len(out["x3d"]) == 0
    rr.compare("none", none, rr.run(none), rr.split(none, out))
    guard.check("initializer_reconstruct_multi")


# ------------------------------------------------------------------------------------------------------- PoseOptimization
def _pose_batch(amd, scs):
    off = np.cumsum([0] + [len(s["u"]) for s in scs]).astype(np.int32)
    cat = lambda k: np.concatenate([s[k] for s in scs])
    ni, T, flags, st, chi2 = amd.pose_optimization_batch(off, cat("xw"), cat("u"), cat("v"), cat("u_right"), cat("inv_sigma2"),
                                                         np.stack([s["K5"] for s in scs]), np.stack([s["Tcw"] for s in scs]))
    return [(int(ni[p]), T[p], flags[off[p]:off[p + 1]], st[p], chi2[off[p]:off[p + 1]]) for p in range(len(scs))]


def test_pose_optimization_batch(amd, guard):
    scs = [por.scene(60, 2, 0.5, 0.0), por.scene(61, 5, 0.5, 0.0), por.scene(62, 0, 0.5, 0.0)]
    for p, (sc, got) in enumerate(zip(scs, _pose_batch(amd, scs))):
        ref = por.run(sc)
        assert not por.guard_violations(sc, ref), p
        check_against(ref, got, f"span-{p}")
        if len(sc["u"]) < 3:  # pose and flags untouched
            assert got[0] == 0 and np.array_equal(got[1], sc["Tcw"]) and not got[2].any() and got[3]["rounds"] == 0
    none = [por.scene(63, 0, 0.5, 0.0), por.scene(64, 0, 0.5, 0.0)]
    for sc, got in zip(none, _pose_batch(amd, none)):
        check_against(por.run(sc), got, "none")
        assert got[0] == 0 and np.array_equal(got[1], sc["Tcw"]) and got[3]["rounds"] == 0
    guard.check("pose_optimization_batch")


def test_pose_optimization_on_the_table(amd, guard):
    """5 edges and 2 features on bad slots; then 2 edges, which is below the 3 an optimisation needs"""
    for seed, n, bad_edges in ((61, 5, [1, 4]), (60, 2, [0])):
        sc = por.scene(seed, n, 0.5, 0.0)
        ref = por.run(sc)
        mp, F, slots, match, pos_of = _table_problem(sc, bad_edges)
        ni, T, flags, st, chi2 = mp.pose_optimization(F, slots, match, sc["Tcw"], sc["K5"], por.INV_LEVEL_SIGMA2,
                                                      outlier=np.full(F.N, 9, np.uint8))
        has = pos_of >= 0
        assert (flags[~has] == 9).all()
        if n < 3:  # pose and flags untouched
            assert ni == 0 and np.array_equal(T, sc["Tcw"]) and (flags == 9).all() and st["rounds"] == 0
        check_against(ref, (ni, T, flags[has], st, chi2[has]), f"table-{n}")
        mp.close()
    # a frame without features beside three live slots: level, chi2 and edgeFeat are carved with one element each
    sc = por.scene(61, 5, 0.5, 0.0)
    mp = amd.MapPoints(8)
    z = np.zeros(3, np.float32)
    mp.update(np.arange(3, dtype=np.int32), sc["xw"][:3], np.zeros((3, 3), np.float32), z, z + 1, np.zeros((3, 32), np.uint8),
              np.full(3, 2, np.uint8))
    none = np.zeros(0, np.float32)
    F = amd.FrameView(none, none, np.zeros(0, np.int32), np.zeros((0, 32), np.uint8), BOUNDS, u_right=none)
    ni, T, flags, st, chi2 = mp.pose_optimization(F, np.arange(3, dtype=np.int32), np.zeros(0, np.int32), sc["Tcw"], sc["K5"],
                                                  por.INV_LEVEL_SIGMA2)
    assert F.N == 0 and ni == 0 and np.array_equal(T, sc["Tcw"]) and st["rounds"] == 0 and len(flags) == len(chi2) == 0
    mp.close()
    guard.check("pose_optimization_mappoints")


# ---------------------------------------------------------------------------------------------------------- OptimizeSim3
KEYS = ("x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "cam1", "cam2", "sim3_in", "th2", "fix_scale")


def _optsim3(amd, scs):
    cat = lambda k, shape: np.concatenate([np.asarray(sc[k], np.float32).reshape(shape) for sc in scs])
    off = np.concatenate([[0], np.cumsum([len(sc["x3dc1"]) for sc in scs])]).astype(np.int32)
    n_in, sim3, bad, st, c12, c21 = amd.optimize_sim3_multi(
        off, cat("x3dc1", (-1, 3)), cat("x3dc2", (-1, 3)), cat("obs1", (-1, 2)), cat("obs2", (-1, 2)), cat("inv_sigma2_1", -1),
        cat("inv_sigma2_2", -1), cat("cam1", (1, 4)), cat("cam2", (1, 4)), cat("sim3_in", (1, 13)),
        np.array([sc["th2"] for sc in scs], np.float32), np.array([sc["fix_scale"] for sc in scs], np.uint8))
    return [(int(n_in[p]), sim3[p], bad[off[p]:off[p + 1]], st[p], c12[off[p]:off[p + 1]], c21[off[p]:off[p + 1]]) for p in range(len(scs))]


def test_optimize_sim3(amd, guard):
    """the scenes of tests/test_gpu_optimize_sim3.py with 0, 10 and 1 pairs (10: the least that is optimised)"""
    scenes = dict(osr.gpu_scenes())
    scs = [scenes["n0-fix0-out0"], scenes["n10-fix1-out0"], scenes["n1-fix0-out0"]]
    for sc, got in zip(scs, _optsim3(amd, scs)):
        osc.check(osr.run(sc), got)
    none = [scenes["n0-fix0-out0"], scenes["n0-fix1-out0"]]
    for sc, got in zip(none, _optsim3(amd, none)):
        osc.check(osr.run(sc), got)
        assert got[0] == 0 and got[3]["rounds"] == 0
    guard.check("optimize_sim3_multi")


# ----------------------------------------------------------------------------------------------------------- triangulate
def test_triangulate(amd, guard):
    """K = 3 neighbours with 65 pairs, with 1 pair and with none (tests/test_gpu_triangulate.py's scenes)"""
    scenes = dict(tr.gpu_scenes(full=False))
    for id_ in ("mixed-K3-p65", "mixed-K3-p1", "mixed-K3-p0"):
        sc = scenes[id_]
        x3d, status, created, winner = triangulate_call(amd, sc)
        tr.compare(id_, tr.run(sc), status, x3d, created, winner, tr.s_tri())
    guard.check("triangulate_matches_multi")
