"""CPU checks of tests/fuse_ref.py, the reference of the Fuse prologue the GPU tests compare against: its two statements of the
arithmetic agree away from the thresholds, and its scenes exercise what they claim to."""
import numpy as np
import pytest

import fuse_ref as fr

# the (seed, n, K) of every scene tests/test_gpu_fuse_mappoints.py builds
PROJECTION_SHAPES = [(n, K) for n in (1, 255, 256, 257, 700) for K in (1, 3, 20)]
GPU_SCENES = [(10 * K + i, n, K) for i, (n, K) in enumerate(PROJECTION_SHAPES)] + [(40, 700, 4), (41, 600, 3), (42, 500, 3), (43, 400, 2),
                                                                                   (44, 700, 4)]


@pytest.mark.parametrize("seed,n,K", GPU_SCENES)
def test_spec32_and_ref64_agree_outside_the_guard_bands(seed, n, K):
    sc = fr.scene(seed, n, K)
    s32, r64 = fr.spec32(sc), fr.ref64(sc)
    keep = ~fr.excluded(r64)
    assert np.array_equal(s32["valid"][keep], r64["valid"][keep])
    assert np.array_equal(s32["stage"][keep], r64["stage"][keep])
    assert np.array_equal(s32["level"][keep], r64["level"][keep])
    ok = keep & (r64["valid"] != 0)
    for name in ("u", "v", "ur", "dist"):
        assert np.allclose(s32[name][ok], r64[name][ok], rtol=1e-5, atol=2e-3), name
    # a property of ref64 alone: the scenes keep out of the bands
    assert fr.excluded(r64).mean() <= 0.02 or n < 16, fr.excluded(r64).mean()
    if n >= 16:
        assert fr.excluded(r64).sum() <= 0.02 * r64["valid"].size


@pytest.mark.parametrize("seed,n,K", [s for s in GPU_SCENES if s[1] >= 255])
def test_scenes_exercise_every_stage_level_and_the_strict_bound(seed, n, K):
    sc = fr.scene(seed, n, K)
    s32 = fr.spec32(sc)
    assert set(np.unique(s32["stage"])) == set(range(-1, len(fr.STAGES))), np.unique(s32["stage"])
    assert set(np.unique(s32["level"][s32["valid"] != 0])) == set(range(fr.LEVELS))
    assert s32["level"][0, :fr.LEVELS].tolist() == list(range(fr.LEVELS)) and s32["valid"][0, :fr.LEVELS].all()
    # point 8 projects onto mnMaxX exactly: KeyFrame::IsInImage rejects it, Frame::isInFrustum's u > max_x would not
    raw = fr.spec32(sc, bounds=(fr.BOUNDS[0], 1e9, fr.BOUNDS[2], fr.BOUNDS[3]))
    assert raw["u"][0, 8] == np.float32(fr.BOUNDS[1]) and raw["valid"][0, 8] == 1
    assert s32["stage"][0, 8] == fr.STAGES.index("image")
    assert (s32["valid"].mean(axis=1) > 0.02).all()


def test_keyframes_split_the_chi_square_gate():
    sc = fr.scene(40, 700, 4)
    assert [f["u_right"] is not None for f in sc["frames"]] == [True, False, True, False]
    for f in sc["frames"]:
        assert len(f["x"]) == fr.KF_POINTS and f["octave"].min() >= 0 and f["octave"].max() < fr.LEVELS
    assert (sc["frames"][0]["u_right"] < 0).any() and (sc["frames"][0]["u_right"] >= 0).any()


def test_sim3_poses_are_the_float32_decomposition():
    sc = fr.scene(43, 400, 2)
    for p, q in zip(sc["poses"], fr.sim3_poses(sc, 1.37)):
        assert q["Rcw"].dtype == np.float32 and np.allclose(q["Rcw"], p["Rcw"], atol=1e-6) and np.allclose(q["tcw"], p["tcw"], atol=1e-5)
