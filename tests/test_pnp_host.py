"""CPU: the PnP C-ABI without a device: the argument checks answer before any device call, a call with nothing to do is
ORBFE_OK, compute calls fail with ORBFE_ERR_HIP (no CPU fallback), orbfe_pnp_sets_from_draws equals the restatement."""
import numpy as np
import pytest

import pnp_ref as pr


def _amd():
    import orb_slam2_annotate_amd as amd
    from orb_slam2_annotate_amd import _lib
    return amd, _lib


def test_sets_from_draws_equals_the_restatement():
    amd, _lib = _amd()
    rng = np.random.default_rng(5)
    for n in (4, 5, 9, 64):
        draws = np.stack([rng.integers(0, n - i, 50) for i in range(4)], 1)
        got = amd.pnp_sets_from_draws(n, draws)
        assert np.array_equal(got, pr.sets_from_draws(n, draws))
        assert all(len(set(s)) == 4 for s in got.tolist())
    for n, d in [(3, [[0, 0, 0, 0]]), (5, [[5, 0, 0, 0]]), (5, [[0, 0, 0, 2]]), (5, [[-1, 0, 0, 0]])]:
        with pytest.raises(amd.OrbfeError) as ei:
            amd.pnp_sets_from_draws(n, d)
        assert ei.value.code == _lib.ERR_INVALID


def test_empty_calls_are_ok_without_a_device():
    amd, _lib = _amd()
    cam = np.array([[500, 500, 320, 240]], np.float32)
    ni, st, pose, wo, words = amd.pnp_ransac_multi([0, 0], np.zeros((0, 3)), np.zeros((0, 2)), np.zeros(0), cam, [0, 0], np.zeros((0, 4)))
    assert len(ni) == 0 and wo.tolist() == [0, 0]
    r = amd.pnp_solve_multi([0, 6], np.zeros((6, 3)), np.zeros((6, 2)), np.ones(6), cam, [0, 0], np.zeros((0, 4)), [4])
    assert len(r["n_inliers"]) == 0 and len(r["rec_hyp"]) == 0 and r["rec_off"].tolist() == [0, 0]
    ni, *_ = amd.pnp_refine_multi([0, 6], np.zeros((6, 3)), np.zeros((6, 2)), np.ones(6), cam, [0, 0], np.zeros(0, np.uint32))
    assert len(ni) == 0


def test_invalid_arguments_are_refused():
    amd, _lib = _amd()
    c = pr.make_candidate(1, 40, 3)
    cam = c["cam"][None]

    def bad(f, *a):
        with pytest.raises(amd.OrbfeError) as ei:
            f(*a)
        assert ei.value.code == _lib.ERR_INVALID

    P = (c["p3d"], c["p2d"], c["max_err"])
    bad(amd.pnp_ransac_multi, [1, 40], *P, cam, [0, 3], c["sets"])            # offsets do not start at 0
    bad(amd.pnp_ransac_multi, [0, 39], *P, cam, [0, 3], c["sets"])            # ... do not end at the total
    bad(amd.pnp_ransac_multi, [0, 40], *P, cam, [0, 2], c["sets"])            # hyp_off does not end at H
    bad(amd.pnp_ransac_multi, [0, 50, 40], *P, np.repeat(cam, 2, 0), [0, 3, 3], c["sets"])  # decreasing
    s = c["sets"].copy(); s[1, 2] = 40
    bad(amd.pnp_ransac_multi, [0, 40], *P, cam, [0, 3], s)                    # index outside [0, n_k)
    s = c["sets"].copy(); s[1, 2] = s[1, 0]
    bad(amd.pnp_ransac_multi, [0, 40], *P, cam, [0, 3], s)                    # repeated index
    k = cam.copy(); k[0, 1] = np.inf
    bad(amd.pnp_ransac_multi, [0, 40], *P, k, [0, 3], c["sets"])              # non-finite camera
    bad(amd.pnp_ransac_multi, [0, 3, 40], *P, np.repeat(cam, 2, 0), [0, 1, 3], np.zeros((3, 4), np.int32))  # n_k < 4 with hypotheses
    m = np.zeros(2, np.uint32); m[0] = 0b111
    bad(amd.pnp_refine_multi, [0, 40], *P, cam, [0, 1], m)                    # fewer than 4 bits
    m = np.zeros(2, np.uint32); m[0] = 0xF; m[1] = 1 << 8
    bad(amd.pnp_refine_multi, [0, 40], *P, cam, [0, 1], m)                    # a bit at n_k = 40
    bad(amd.pnp_solve_multi, [0, 40], *P, cam, [0, 3], c["sets"], [3])        # min_inliers below the minimal set


def test_compute_calls_fail_loudly_without_a_gpu():
    amd, _lib = _amd()
    if _lib.load().orbfe_device_count() > 0:
        pytest.skip("a GPU is present")
    c = pr.make_candidate(2, 40, 3)
    with pytest.raises(amd.OrbfeError) as ei:
        amd.pnp_ransac(c["p3d"], c["p2d"], c["max_err"], c["cam"], c["sets"])
    assert ei.value.code == _lib.ERR_HIP
    with pytest.raises(amd.OrbfeError) as ei:
        amd.PnPsolver(c["p3d"], c["p2d"], c["sigma2"], c["cam"], c["sets"]).iterate(5)
    assert ei.value.code == _lib.ERR_HIP


def test_null_arrays_and_candidate_range_are_refused_not_read():
    """the C-ABI itself: NULL arrays and n_candidates outside [0, 4096] answer ORBFE_ERR_INVALID before anything is read --
    also with a NULL min_inliers next to an n_candidates beyond the range"""
    import ctypes as C
    amd, _lib = _amd()
    from orb_slam2_annotate_amd._lib import check, ptr
    L = _lib.load()
    c = pr.make_candidate(3, 40, 3)
    off, ho, mi = np.array([0, 40], np.int32), np.array([0, 3], np.int32), np.array([10], np.int32)
    ni, st, pose, wo, words = np.zeros(3, np.int32), np.zeros(3, np.uint8), np.zeros(36, np.float32), np.zeros(2, np.int32), \
        np.zeros(6, np.uint32)
    good = [ptr(off), ptr(c["p3d"]), ptr(c["p2d"]), ptr(c["max_err"]), ptr(c["cam"]), ptr(ho), ptr(c["sets"]), ptr(ni), ptr(st),
            ptr(pose), ptr(wo), ptr(words)]

    def refused(f, *a):
        with pytest.raises(amd.OrbfeError) as ei:
            check(f(*a))
        assert ei.value.code == _lib.ERR_INVALID

    for i in range(len(good)):
        a = list(good)
        a[i] = None
        refused(L.orbfe_pnp_ransac_multi, 0, 1, 40, 3, *a)
        refused(L.orbfe_pnp_refine_multi, 0, 1, 40, 3, *a)
    for K in (-1, 4097, 1 << 30):
        refused(L.orbfe_pnp_ransac_multi, 0, K, 40, 3, *good)
        refused(L.orbfe_pnp_refine_multi, 0, K, 40, 3, *good)
    rec = [ptr(np.zeros(2, np.int32)), ptr(np.zeros(3, np.int32)), ptr(np.zeros(3, np.int32)), ptr(np.zeros(3, np.uint8)),
           ptr(np.zeros(36, np.float32)), ptr(np.zeros(2, np.int32)), ptr(np.zeros(6, np.uint32))]
    for K in (-1, 4097, 1 << 30):
        refused(L.orbfe_pnp_solve_multi, 0, K, 40, 3, *good[:7], None, *good[7:], *rec)
        refused(L.orbfe_pnp_solve_multi, 0, K, 40, 3, *good[:7], ptr(mi), *good[7:], *rec)
    refused(L.orbfe_pnp_solve_multi, 0, 1, 40, 3, *good[:7], None, *good[7:], *rec)
    for i in range(len(rec)):
        a = list(rec)
        a[i] = None
        refused(L.orbfe_pnp_solve_multi, 0, 1, 40, 3, *good[:7], ptr(mi), *good[7:], *a)
    refused(L.orbfe_pnp_ransac_multi, 0, 1, -1, 3, *good)
    refused(L.orbfe_pnp_ransac_multi, 0, 1, 40, -1, *good)
    refused(L.orbfe_pnp_ransac_multi, -1, 1, 40, 3, *good)
