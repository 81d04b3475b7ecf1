"""CPU checks of tests/track_ref.py, the reference of the last-frame / key-frame SearchByProjection prologues the GPU tests compare
against: its two statements of the arithmetic agree away from the thresholds, and its scenes exercise what they claim to.

The guard-band cap.  At most 0.2 % of a scene's (job, point) pairs may lie inside the guard bands of ref64.  Two points of every
scene are PUT on a threshold (u == max_x and zc == 0, track_ref.on_threshold_by_design) and are therefore inside a band by
construction; at the sizes of these scenes (at most 300 points a job) they alone are 0.2 % .. 0.7 % of the pairs.  The cap of
0.2 % is asserted on all other pairs, and the cap tests/test_gpu_fuse_mappoints.py uses (2 %) on all pairs, those two included;
what the two points must give is asserted by name below and, on the GPU, by the bit-for-bit comparison with spec32."""
import numpy as np
import pytest

import track_ref as tr

# the (seed, n, K) of every scene tests/test_gpu_track_mappoints.py builds: the workgroup boundary, unequal jobs, an empty job
SIZES = (0, 1, 255, 256, 257, 300)
LAST_SCENES = [(i, n, 1) for i, n in enumerate(SIZES)]
KF_SCENES = [(11, 300, 1), (12, (300, 0, 257), 3), (13, (256, 1, 0, 255, 300), 5)]
GPU_SCENES = LAST_SCENES + KF_SCENES
CAP, CAP_ALL = 0.002, 0.02
IDS = [f"seed{s}-K{K}" for s, _, K in GPU_SCENES]


@pytest.mark.parametrize("form", ["last", "kf"])
@pytest.mark.parametrize("seed,n,K", GPU_SCENES, ids=IDS)
def test_spec32_and_ref64_agree_outside_the_guard_bands(seed, n, K, form):
    sc = tr.scene(seed, n, K)
    s32, r64 = tr.spec32(sc, form), tr.ref64(sc, form)
    out = tr.excluded(r64, form)
    keep = ~out
    assert np.array_equal(s32["valid"][keep], r64["valid"][keep])
    assert np.array_equal(s32["stage"][keep], r64["stage"][keep])
    ok = keep & (r64["valid"] != 0)
    names = ("u", "v", "ur", "radius") if form == "last" else ("u", "v", "dist")
    for name in names:
        assert np.allclose(s32[name][ok], r64[name][ok], rtol=1e-5, atol=2e-3), name
    assert np.allclose(s32["inv_z"][ok], r64["inv_z"][ok], rtol=1e-4)
    if form == "kf":
        assert np.array_equal(s32["level"][keep], r64["level"][keep])
    # a property of ref64 alone: the scenes keep out of the bands (the module's docstring)
    N = len(sc["pos"])
    assert (out & ~tr.on_threshold_by_design(sc)).sum() <= CAP * N, (int(out.sum()), N)
    assert out.sum() <= max(CAP_ALL * N, 2 if N >= 16 else 0), (int(out.sum()), N)


@pytest.mark.parametrize("seed,n,K", [s for s in GPU_SCENES if np.max(s[1]) >= 255], ids=[i for i, s in zip(IDS, GPU_SCENES) if np.max(s[1]) >= 255])
def test_scenes_exercise_every_stage_level_and_engineered_point(seed, n, K):
    sc = tr.scene(seed, n, K)
    last, kf = tr.spec32(sc, "last"), tr.spec32(sc, "kf")
    assert set(np.unique(last["stage"])) == set(range(-1, len(tr.STAGES["last"])))
    assert set(np.unique(kf["stage"])) == set(range(-1, len(tr.STAGES["kf"])))
    assert set(np.unique(kf["level"][kf["valid"] != 0])) == set(range(tr.LEVELS))
    assert set(np.unique(sc["last_octave"][last["valid"] != 0])) == set(range(tr.LEVELS))
    assert kf["level"][:tr.LEVELS].tolist() == list(range(tr.LEVELS)) and kf["valid"][:tr.LEVELS].all() and last["valid"][:tr.LEVELS].all()
    # u == max_x exactly, and accepted: these bounds are inclusive (KeyFrame::IsInImage's, which Fuse uses, are not)
    assert last["u"][tr.ON_BOUND] == np.float32(tr.BOUNDS[1]) and last["valid"][tr.ON_BOUND] == 1 and kf["valid"][tr.ON_BOUND] == 1
    # behind the camera, inside the image: the key-frame form has no depth test
    assert last["stage"][tr.BEHIND] == tr.STAGES["last"].index("depth") and kf["valid"][tr.BEHIND] == 1
    assert tr.spec32(sc, "kf", raw=True)["inv_z"][tr.BEHIND] < 0
    # a bad point: the last-frame form asks pMP and mvbOutlier only
    assert last["valid"][tr.BAD] == 1 and kf["stage"][tr.BAD] == tr.STAGES["kf"].index("bad")
    # zero depth: 1/zc = +inf, u = NaN, rejected at the image test by both
    raw = tr.spec32(sc, "last", raw=True)
    assert np.isposinf(raw["inv_z"][tr.ZERO_DEPTH]) and np.isnan(raw["u"][tr.ZERO_DEPTH])
    assert last["stage"][tr.ZERO_DEPTH] == tr.STAGES["last"].index("image") and kf["stage"][tr.ZERO_DEPTH] == tr.STAGES["kf"].index("image")
    assert last["stage"][tr.SKIPPED] == 0 and kf["stage"][tr.SKIPPED] == 0
    assert tr.spec32(sc, "last", skip=np.zeros(len(sc["pos"]), np.uint8))["valid"][tr.SKIPPED] == 1
    assert last["valid"].mean() > 0.1 and kf["valid"].mean() > 0.05


def test_every_mode_occurs_and_the_frames_are_well_formed():
    assert {tr.scene(s, n, K)["mode"] for s, n, K in LAST_SCENES if n >= 255} == {0, 1, 2}
    sc = tr.scene(*KF_SCENES[2])
    assert np.diff(sc["offsets"]).tolist() == [256, 1, 0, 255, 300]
    for f, stereo in ((sc["cur"], False), (sc["cur_stereo"], True)):
        assert len(f["x"]) == tr.CUR_POINTS and f["octave"].min() >= 0 and f["octave"].max() < tr.LEVELS
        assert (f["u_right"] is not None) == stereo
        assert (f["x"] >= tr.BOUNDS[0]).all() and (f["x"] < tr.BOUNDS[1]).all() and (f["y"] >= tr.BOUNDS[2]).all() and (f["y"] < tr.BOUNDS[3]).all()
    assert (sc["cur_stereo"]["u_right"] < 0).any() and (sc["cur_stereo"]["u_right"] >= 0).any()
