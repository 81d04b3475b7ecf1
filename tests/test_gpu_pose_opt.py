"""orbfe_pose_optimization* (csrc/k_poseopt.hip) against tests/pose_opt_ref.py, the cited float64 restatement of
Optimizer::PoseOptimization (src/Optimizer.cc:256-473).

Pass condition per problem: outlier[], the return value and stats.rounds identical; every Tcw_out entry within
max(16 * s_pose, 4 float32 ulps of the entry); edge_chi2 within 16 * s_chi2 relative -- s_pose / s_chi2 being the
reference's own reordering noise (profiles/pose_opt_tolerance.txt, measured by tests/test_pose_opt_ref.py).  The device's
tree sum is a third summation order and its sin / cos / sqrt differ from libm in the last place, hence the margin of 16.
No edge and no scene is skipped: the scenes keep out of the guard bands by construction (tests/test_pose_opt_ref.py)."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import frustum_ref as fr
import pose_opt_check as chk
import pose_opt_ref as pr
from pose_opt_check import check_against  # THE pass condition, shared with tests/test_pose_opt_math_cpu.py

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


_REF = {}


def ref_of(id_):
    """(scene, reference result), computed once and shared."""
    if not _REF:
        for k, sc in pr.gpu_scenes():
            _REF[k] = (sc, None)
    sc, r = _REF[id_]
    if r is None:
        r = pr.run(sc)
        _REF[id_] = (sc, r)
    return sc, r


def run_gpu(sc, outlier=None):
    import orb_slam2_annotate_amd as amd
    return amd.pose_optimization(sc["xw"], sc["u"], sc["v"], sc["u_right"], sc["inv_sigma2"], sc["K5"], sc["Tcw"], outlier=outlier)


@pytest.mark.parametrize("id_", [k for k, _ in pr.gpu_scenes()])
def test_against_the_reference(id_):
    sc, ref = ref_of(id_)
    sentinel = np.full(len(sc["u"]), 7, np.uint8)
    got = run_gpu(sc, outlier=sentinel)
    if len(sc["u"]) < 3:  # pose and flags untouched
        assert got[0] == 0 and np.array_equal(got[1], sc["Tcw"]) and (got[2] == 7).all() and got[3]["rounds"] == 0
    check_against(ref, got, id_)


def test_device_equals_the_cpu_program_of_the_same_header(tmp_path):
    """csrc/poseopt_math.h compiled for the host, in the kernel's summation order (tests/cpp/poseopt_cpu.cpp), against the
    device on n = 3 (one round), 10, 257 (a lane's second edge) and a mono / stereo mix: every discrete field identical,
    every float within the pass condition."""
    scenes = dict(chk.extra_scenes())
    ids = ("x-n3", "x-n10", "x-n257", "x-mix-n40")
    cpu = chk.run_program(chk.build_program(tmp_path), tmp_path, [scenes[k] for k in ids])
    for k, c in zip(ids, cpu):
        chk.check_same_run(c, run_gpu(scenes[k], outlier=np.full(len(scenes[k]["u"]), 7, np.uint8)), k)


def _same(a, b):
    return a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3] and \
        a[4].tobytes() == b[4].tobytes()


def test_two_calls_give_identical_bits():
    sc, _ = ref_of("n2000-mixed-out20")
    assert _same(run_gpu(sc), run_gpu(sc))


def test_batch_equals_single_calls_bit_for_bit():
    import orb_slam2_annotate_amd as amd
    scs = [ref_of("n257-mixed-out20")[0], pr.scene(0, 0, 0.5, 0.0), ref_of("n65-stereo-out0")[0]]
    off = np.cumsum([0] + [len(s["u"]) for s in scs]).astype(np.int32)
    cat = lambda k: np.concatenate([s[k] for s in scs])
    ni, T, flags, st, chi2 = amd.pose_optimization_batch(off, cat("xw"), cat("u"), cat("v"), cat("u_right"), cat("inv_sigma2"),
                                                         np.stack([s["K5"] for s in scs]), np.stack([s["Tcw"] for s in scs]))
    for p, s in enumerate(scs):
        one = run_gpu(s)
        lo, hi = off[p], off[p + 1]
        assert _same(one, (int(ni[p]), T[p], flags[lo:hi], st[p], chi2[lo:hi])), p
    assert ni[1] == 0 and st[1]["rounds"] == 0 and np.array_equal(T[1], scs[1]["Tcw"])


def test_batch_whose_problems_end_around_a_256_byte_line():
    """Per-problem edge counts 15, 16, 17, 3, 0 and 2: sixteen float4 edges are exactly one 256-byte line, so the edge, flag and
    chi2 arrays of the call end just before, on and just after a line, and 53 edges in all end inside one.  An array carved
    a line short would be overwritten by its neighbour."""
    import orb_slam2_annotate_amd as amd
    scs = [pr.scene(40 + p, n, 0.5, 0.2) for p, n in enumerate((15, 16, 17, 3, 0, 2))]
    assert all((s["u_right"] >= 0).any() and (s["u_right"] < 0).any() for s in scs[:3])  # mixed mono / stereo
    off = np.cumsum([0] + [len(s["u"]) for s in scs]).astype(np.int32)
    cat = lambda k: np.concatenate([s[k] for s in scs])
    ni, T, flags, st, chi2 = amd.pose_optimization_batch(off, cat("xw"), cat("u"), cat("v"), cat("u_right"), cat("inv_sigma2"),
                                                         np.stack([s["K5"] for s in scs]), np.stack([s["Tcw"] for s in scs]),
                                                         outlier=np.full(off[-1], 7, np.uint8))
    for p, s in enumerate(scs):
        lo, hi = off[p], off[p + 1]
        one = run_gpu(s, outlier=np.full(hi - lo, 7, np.uint8))
        assert _same(one, (int(ni[p]), T[p], flags[lo:hi], st[p], chi2[lo:hi])), p
        if hi - lo < 3:  # pose and flags untouched
            assert (flags[lo:hi] == 7).all() and ni[p] == 0 and st[p]["rounds"] == 0 and np.array_equal(T[p], s["Tcw"]), p
        else:
            assert (flags[lo:hi] <= 1).all() and st[p]["rounds"] > 0, p


def test_batch_across_the_lds_bound_equals_single_calls():
    """One problem above kPoseOptLdsEdges = 2048 sends the whole batch to the global-memory form of the kernel; the single
    call of the small problem takes the LDS form.  Both read the same floats and sum in the same order."""
    import orb_slam2_annotate_amd as amd
    scs = [ref_of("n2049-mixed-out20")[0], ref_of("n2000-mixed-out20")[0], ref_of("n64-stereo-out0")[0]]
    off = np.cumsum([0] + [len(s["u"]) for s in scs]).astype(np.int32)
    cat = lambda k: np.concatenate([s[k] for s in scs])
    ni, T, flags, st, chi2 = amd.pose_optimization_batch(off, cat("xw"), cat("u"), cat("v"), cat("u_right"), cat("inv_sigma2"),
                                                         np.stack([s["K5"] for s in scs]), np.stack([s["Tcw"] for s in scs]))
    for p, s in enumerate(scs):
        lo, hi = off[p], off[p + 1]
        assert _same(run_gpu(s), (int(ni[p]), T[p], flags[lo:hi], st[p], chi2[lo:hi])), p


def test_table_form_above_the_lds_bound():
    """2051 features (2049 edges + 2 on bad slots): the gather and the global-memory form in one launch."""
    sc, ref = ref_of("n2049-mixed-out20")
    mp, F, slots, match, pos_of = _table_problem(sc, [7, 2040])
    assert F.N == 2051
    ni, T, flags, st, chi2 = mp.pose_optimization(F, slots, match, sc["Tcw"], sc["K5"], pr.INV_LEVEL_SIGMA2,
                                                  outlier=np.full(F.N, 9, np.uint8))
    has = pos_of >= 0
    assert _same(run_gpu(sc), (ni, T, flags[has], st, chi2[has]))
    assert (flags[~has] == 9).all()
    check_against(ref, (ni, T, flags[has], st, chi2[has]), "table-2051")
    mp.close()


def _table_problem(sc, bad_edges):
    """The scene's edges as a table + frame + match: features in shuffled slots, two extra features matched to bad slots."""
    import orb_slam2_annotate_amd as amd
    n = len(sc["u"])
    rng = np.random.default_rng(5)
    pos_of = np.insert(np.arange(n), bad_edges, -1)  # feature -> edge of the scene, -1: a feature on a bad slot
    nf = len(pos_of)
    edge = np.where(pos_of >= 0, pos_of, 0)
    cap = nf + 9
    slots = rng.permutation(cap)[:nf].astype(np.int32)  # slot[] position p serves feature perm[p]
    perm = rng.permutation(nf)
    match = np.empty(nf, np.int32)
    match[perm] = np.arange(nf)
    mp = amd.MapPoints(cap)
    flags = np.where(pos_of[perm] >= 0, 2, 1 | 2).astype(np.uint8)
    z = np.zeros(nf, np.float32)
    mp.update(slots, sc["xw"][edge[perm]], np.zeros((nf, 3), np.float32), z, z + 1, np.zeros((nf, 32), np.uint8), flags)
    octave = np.where(pos_of >= 0, sc["octave"][edge], 0).astype(np.int32)
    ur = sc["u_right"][edge]
    F = amd.FrameView(sc["u"][edge], sc["v"][edge], octave, np.zeros((nf, 32), np.uint8), fr.BOUNDS, u_right=ur)
    return mp, F, slots, match, pos_of


def test_table_form_equals_array_form_and_leaves_bad_slots_alone():
    sc, _ = ref_of("n257-mixed-out20")
    mp, F, slots, match, pos_of = _table_problem(sc, [10, 200])
    sentinel = np.full(F.N, 9, np.uint8)
    ni, T, flags, st, chi2 = mp.pose_optimization(F, slots, match, sc["Tcw"], sc["K5"], pr.INV_LEVEL_SIGMA2, outlier=sentinel)
    one = run_gpu(sc)
    has = pos_of >= 0
    assert _same(one, (ni, T, flags[has], st, chi2[has]))
    assert (flags[~has] == 9).all() and (~has).sum() == 2
    mp.close()


@pytest.mark.parametrize("stereo", [False, True], ids=["mono", "stereo"])
@pytest.mark.parametrize("nf", [64, 65])
@pytest.mark.parametrize("n_slots", [63, 64, 65])
def test_table_form_whose_arrays_end_around_a_256_byte_line(n_slots, nf, stereo):
    """64 int32 / float entries are exactly one 256-byte line: slot[] and the frame's arrays end just before, on and just after
    one, a monocular frame stages no u_right at all.  min(nf, n_slots) edges; the other features have no match, the other
    slots no feature.  Equal to the array form on the same edges bit for bit."""
    import orb_slam2_annotate_amd as amd
    ne = min(nf, n_slots)
    kind = "stereo" if stereo else "mono"
    sc = pr.scene(pr.SEEDS.get((ne, kind, 0.2), 0), ne, pr.KINDS[kind], 0.2)  # (the scene of test_against_the_reference)
    rng = np.random.default_rng(100 * n_slots + nf)
    pos_of = np.full(nf, -1)  # feature -> edge of the scene, -1: a feature without a match
    pos_of[np.sort(rng.permutation(nf)[:ne])] = np.arange(ne)
    has = pos_of >= 0
    edge = np.where(has, pos_of, 0)
    cap = 70
    slots = rng.permutation(cap)[:n_slots].astype(np.int32)
    at = rng.permutation(n_slots)[:ne]  # slot[] position of edge k
    mp = amd.MapPoints(cap)
    z = np.zeros(ne, np.float32)
    mp.update(slots[at], sc["xw"], np.zeros((ne, 3), np.float32), z, z + 1, np.zeros((ne, 32), np.uint8), np.full(ne, 2, np.uint8))
    match = np.where(has, at[edge], -1).astype(np.int32)
    assert (sc["u_right"] >= 0).all() if stereo else (sc["u_right"] < 0).all()
    F = amd.FrameView(sc["u"][edge], sc["v"][edge], np.where(has, sc["octave"][edge], 0), np.zeros((nf, 32), np.uint8), fr.BOUNDS,
                      u_right=sc["u_right"][edge] if stereo else None)
    ni, T, flags, st, chi2 = mp.pose_optimization(F, slots, match, sc["Tcw"], sc["K5"], pr.INV_LEVEL_SIGMA2,
                                                  outlier=np.full(nf, 9, np.uint8))
    assert _same(run_gpu(sc), (ni, T, flags[has], st, chi2[has]))
    assert (flags[~has] == 9).all() and (chi2[~has] == 0).all() and (~has).sum() == nf - ne
    mp.close()


def test_invalid_arguments_return_before_a_launch():
    import orb_slam2_annotate_amd as amd
    from orb_slam2_annotate_amd import _lib
    L = _lib.load()
    sc, _ = ref_of("n10-mixed-out0")
    p = _lib.ptr
    a = [np.ascontiguousarray(sc[k]) for k in ("xw", "u", "v", "u_right", "inv_sigma2", "K5", "Tcw")]
    out, fl, ni = np.zeros(16, np.float32), np.zeros(10, np.uint8), C.c_int32(0)
    args = lambda n, arrs: (0, n, *[p(x) for x in arrs], p(out), p(fl), C.byref(ni), None, None)
    # The calling thread's stream is held by a stall kernel.  Every call that enqueues work also waits for it, behind the
    # stall; so a call that returns while the stall is still pending -- the idle query at the end -- has enqueued nothing.
    mp, F, slots, match, _ = _table_problem(sc, [])
    assert L.orbfe_debug_stall_thread_stream(0, 400000) == 0
    assert L.orbfe_pose_optimization(*args(-1, a)) == _lib.ERR_INVALID
    assert L.orbfe_pose_optimization(*args(16385, a)) == _lib.ERR_INVALID
    for k in range(7):
        assert L.orbfe_pose_optimization(*args(10, [None if i == k else x for i, x in enumerate(a)])) == _lib.ERR_INVALID, k
    assert L.orbfe_pose_optimization(0, 10, *[p(x) for x in a], None, p(fl), C.byref(ni), None, None) == _lib.ERR_INVALID
    assert L.orbfe_pose_optimization(0, 10, *[p(x) for x in a], p(out), None, C.byref(ni), None, None) == _lib.ERR_INVALID
    assert L.orbfe_pose_optimization(0, 10, *[p(x) for x in a], p(out), p(fl), None, None, None) == _lib.ERR_INVALID
    off = np.array([0, 6, 4, 10], np.int32)  # descends
    nis = np.zeros(3, np.int32)
    K, T = np.tile(a[5], 3), np.tile(a[6].reshape(-1), 3)
    outs = np.zeros(48, np.float32)
    assert L.orbfe_pose_optimization_batch(0, 3, p(off), *[p(x) for x in a[:5]], p(K), p(T), p(outs), p(fl), p(nis), None,
                                           None) == _lib.ERR_INVALID
    assert L.orbfe_pose_optimization_batch(0, 3, None, *[p(x) for x in a[:5]], p(K), p(T), p(outs), p(fl), p(nis), None,
                                           None) == _lib.ERR_INVALID
    for bad_off in ([0, 10], [0, 16385]):  # n_problems < 0; a problem of more than 16384 edges
        o2 = np.array(bad_off, np.int32)
        q = -1 if bad_off[1] == 10 else 1
        assert L.orbfe_pose_optimization_batch(0, q, p(o2), *[p(x) for x in a[:5]], p(K), p(T), p(outs), p(fl), p(nis), None,
                                               None) == _lib.ERR_INVALID
    with pytest.raises(amd.OrbfeError) as ei:  # a slot outside the table
        mp.pose_optimization(F, np.where(np.arange(len(slots)) == 3, mp.capacity, slots), match, sc["Tcw"], sc["K5"], pr.INV_LEVEL_SIGMA2)
    assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(amd.OrbfeError):  # a match outside slot[]
        mp.pose_optimization(F, slots, np.where(np.arange(F.N) == 2, len(slots), match), sc["Tcw"], sc["K5"], pr.INV_LEVEL_SIGMA2)
    with pytest.raises(amd.OrbfeError):  # an octave outside the level table
        mp.pose_optimization(F, slots, match, sc["Tcw"], sc["K5"], pr.INV_LEVEL_SIGMA2[:1])
    assert L.orbfe_debug_thread_stream_idle(0) == 0  # the stall is still pending: no call above waited behind it
    mp.close()


def test_search_local_points_then_pose_optimization():
    """The TrackLocalMap chain on a frustum_ref scene: match[] goes from one call into the other unchanged, and the result
    equals the reference fed the same match[]."""
    import orb_slam2_annotate_amd as amd
    n = 600
    sc = fr.scene(3, n)
    mp = amd.MapPoints(n)
    slots = np.arange(n, dtype=np.int32)
    mp.update(slots, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
    s32 = fr.spec32(sc)
    vis = np.flatnonzero(s32["in_view"])
    rng = np.random.default_rng(11)
    sf = np.array([fr.SCALE ** l for l in range(fr.LEVELS)], np.float32)
    # the frame: one feature on every visible point (a pixel of noise, the predicted level, its descriptor)
    x = (s32["proj_x"][vis] + rng.normal(0, 0.5, len(vis))).astype(np.float32)
    y = (s32["proj_y"][vis] + rng.normal(0, 0.5, len(vis))).astype(np.float32)
    ur = np.where(rng.random(len(vis)) < 0.5, s32["proj_xr"][vis], -1).astype(np.float32)
    F = amd.FrameView(x, y, s32["level"][vis].astype(np.int32), sc["desc"][vis], fr.BOUNDS, u_right=ur)
    pose = amd.camera_pose(sc["Rcw"], sc["tcw"], (fr.FX, fr.FY, fr.CX, fr.CY), fr.MBF, fr.BOUNDS, fr.SCALE, fr.LEVELS, Ow=sc["Ow"])
    nm, match, _ = mp.SearchLocalPoints(F, slots, pose, sf, th=3.0)
    assert nm > 100
    Tcw = np.eye(4, dtype=np.float32)
    Tcw[:3, :3], Tcw[:3, 3] = sc["Rcw"], sc["tcw"]
    K5 = np.array(pr.K5, np.float32)
    got = mp.pose_optimization(F, slots, match, Tcw, K5, pr.INV_LEVEL_SIGMA2)
    has = (match >= 0) & ((sc["flags"][np.maximum(match, 0)] & 1) == 0)
    ref = pr.pose_optimization(sc["pos"][match[has]], x[has], y[has], ur[has], pr.INV_LEVEL_SIGMA2[F.octave[has]], K5, Tcw)
    assert not pr.guard_violations(dict(u_right=ur[has], xw=sc["pos"][match[has]], Tcw_true=Tcw), ref)
    check_against(ref, (got[0], got[1], got[2][has], got[3], got[4][has]), "chain")
    mp.close()
