"""CPU: pins tests/frustum_ref.py itself -- the float32 statement of orbfe_project_in_frustum (spec32) against the float64
statement of src/Frame.cc:292-353 (ref64) on the scenes the GPU tests use, and that those scenes reach every branch."""
import numpy as np
import pytest

import frustum_ref as fr

CASES = [(seed, n) for seed in (0, 1, 2) for n in (33, 2000, 4096)]


@pytest.fixture(scope="module")
def results():
    out = {}
    for seed, n in CASES:
        sc = fr.scene(seed, n)
        out[seed, n] = (sc, fr.spec32(sc, sc["skip"]), fr.ref64(sc, sc["skip"]))
    return out


@pytest.mark.parametrize("seed,n", CASES)
def test_spec32_agrees_with_ref64(results, seed, n):
    sc, s32, r64 = results[seed, n]
    assert np.array_equal(s32["stage"], r64["stage"]), np.flatnonzero(s32["stage"] != r64["stage"])
    assert np.array_equal(s32["in_view"], r64["in_view"])
    assert np.array_equal(s32["level"], r64["level"])
    ok = s32["in_view"] != 0
    if ok.any():
        assert np.abs(s32["proj_x"][ok] - r64["u"][ok]).max() < 2e-3
        assert np.abs(s32["proj_y"][ok] - r64["v"][ok]).max() < 2e-3
        assert np.abs(s32["proj_xr"][ok] - r64["proj_xr"][ok]).max() < 2e-3
        assert np.abs(s32["view_cos"][ok] - r64["cos_all"][ok]).max() < 1e-6
        assert np.abs(s32["dist"][ok] / r64["dist_all"][ok] - 1).max() < 1e-6


@pytest.mark.parametrize("seed,n", [c for c in CASES if c[1] >= 2000])
def test_scenes_reach_every_stage_and_level(results, seed, n):
    sc, s32, r64 = results[seed, n]
    for k, name in enumerate(fr.STAGES):
        assert (s32["stage"] == k).any(), f"no point is rejected at stage {name}"
    ok = s32["in_view"] != 0
    assert 0.22 <= ok.mean() <= 0.36, ok.mean()
    assert set(np.unique(s32["level"][ok]).tolist()) == set(range(fr.LEVELS))


@pytest.mark.parametrize("seed,n", CASES)
def test_guard_bands_are_nearly_empty(results, seed, n):
    sc, s32, r64 = results[seed, n]
    near = fr.near_threshold(r64)
    assert near.sum() <= max(0.0005 * n, 0), (near.sum(), n)
    ok = r64["in_view"] != 0
    assert (fr.near_integer(r64) & ok).sum() <= 0.0005 * n


def test_outputs_are_zero_outside_the_view():
    sc = fr.scene(0, 2000)
    s32 = fr.spec32(sc, sc["skip"])
    out = s32["in_view"] == 0
    for name in ("level", "view_cos", "proj_x", "proj_y", "proj_xr", "inv_z", "dist"):
        assert not s32[name][out].any(), name
    assert s32["proj_x"].dtype == np.float32 and s32["level"].dtype == np.int32


def test_skip_and_bad_come_first():
    sc = fr.scene(1, 2000)
    s32 = fr.spec32(sc, sc["skip"])
    assert (s32["stage"][sc["skip"] != 0] == 0).all()
    assert (s32["stage"][(sc["skip"] == 0) & ((sc["flags"] & 1) != 0)] == 1).all()
    free = fr.spec32(sc, None)
    assert free["in_view"].sum() > s32["in_view"].sum()
