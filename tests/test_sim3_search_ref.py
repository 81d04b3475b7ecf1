"""CPU checks of tests/sim3_search_ref.py, the reference of the SearchBySim3 prologue the GPU tests compare against: its two
statements of the arithmetic agree away from the thresholds, and its scenes exercise what they claim to.

The guard-band caps are those of tests/test_track_ref.py: at most 0.2 % (CAP) of a scene's (leg, point) pairs may lie inside
the guard bands of ref64, not counting the three points that are PUT on a threshold (u == max_x, u == min_x, c2 == 0:
sim3_search_ref.on_threshold_by_design); with those counted the cap is 2 % (CAP_ALL)."""
import numpy as np
import pytest

import sim3_search_ref as sr
from test_track_ref import CAP, CAP_ALL

# the (seed, N1, (N2_k)) of every scene tests/test_gpu_sim3_search.py builds: sizes around the workgroup boundary, K = 1 / 3 / 5,
# unequal candidates, an empty one
GPU_SCENES = [(0, 300, (300,)), (1, 256, (257, 0, 255)), (2, 257, (300, 1, 0, 255, 256)), (3, 0, (300,)), (4, 1, (1,)),
              (5, 255, (256,)), (6, 300, (0,))]
IDS = [f"seed{s}-K{len(n2)}" for s, _, n2 in GPU_SCENES]
BIG = [s for s in GPU_SCENES if s[1] >= 255 and max(s[2]) >= 255]
BIG_IDS = [i for i, s in zip(IDS, GPU_SCENES) if s in BIG]


@pytest.mark.parametrize("seed,n1,n2s", GPU_SCENES, ids=IDS)
def test_spec32_and_ref64_agree_outside_the_guard_bands(seed, n1, n2s):
    sc = sr.scene(seed, n1, n2s)
    s32, r64 = sr.spec32(sc), sr.ref64(sc)
    N = len(s32["valid"])
    assert N == len(n2s) * n1 + sum(n2s)
    out = sr.excluded(r64)
    keep = ~out
    assert np.array_equal(s32["valid"][keep], r64["valid"][keep])
    assert np.array_equal(s32["stage"][keep], r64["stage"][keep])
    assert np.array_equal(s32["level"][keep], r64["level"][keep])
    ok = keep & (r64["valid"] != 0)
    for name in ("u", "v", "dist"):
        assert np.allclose(s32[name][ok], r64[name][ok], rtol=1e-5, atol=2e-3), name
    # a property of ref64 alone: the scenes keep out of the bands
    assert (out & ~sr.on_threshold_by_design(sc)).sum() <= CAP * N, (int(out.sum()), N)
    assert out.sum() <= max(CAP_ALL * N, 3 if n1 >= 16 else 0), (int(out.sum()), N)


@pytest.mark.parametrize("seed,n1,n2s", BIG, ids=BIG_IDS)
def test_scenes_exercise_every_stage_level_and_engineered_point(seed, n1, n2s):
    sc = sr.scene(seed, n1, n2s)
    s = sr.spec32(sc)
    raw = sr.spec32(sc, raw=True)
    st = sr.STAGES.index
    assert set(np.unique(s["stage"])) == set(range(-1, len(sr.STAGES)))
    assert set(np.unique(s["level"][s["valid"] != 0])) == set(range(sr.LEVELS))
    assert s["level"][:sr.LEVELS].tolist() == list(range(sr.LEVELS)) and s["valid"][:sr.LEVELS].all()
    # u == max_x exactly is rejected (the bound is strict), u == min_x exactly is accepted
    assert raw["u"][sr.ON_MAX] == np.float32(sr.BOUNDS[1]) and s["stage"][sr.ON_MAX] == st("image")
    assert raw["u"][sr.ON_MIN] == np.float32(sr.BOUNDS[0]) and s["valid"][sr.ON_MIN] == 1
    assert s["stage"][sr.BEHIND] == st("depth")
    b = sr.BOUNDS
    assert b[0] <= raw["u"][sr.BEHIND] < b[1] and b[2] <= raw["v"][sr.BEHIND] < b[3]
    # c2 == 0: the depth test passes (0 < 0 is false), invz = inf, u = NaN, rejected at the image test
    assert raw["dist"][sr.ZERO] == 0 and np.isnan(raw["u"][sr.ZERO]) and s["stage"][sr.ZERO] == st("image")
    assert s["stage"][sr.BAD] == st("bad") and s["stage"][sr.NOSLOT] == st("noslot") and s["stage"][sr.SKIPPED] == st("skip")
    assert sr.spec32(sc, skips=None)["valid"][sr.SKIPPED] == 1
    assert s["valid"].mean() > 0.1


def test_the_key_frames_are_well_formed_and_hold_mutual_pairs():
    sc = sr.scene(*GPU_SCENES[2])
    assert [len(f["x"]) for f in sc["kf2"]] == [300, 1, 0, 255, 256] and len(sc["kf1"]["x"]) == 257
    for f in [sc["kf1"]] + sc["kf2"]:
        assert len(f["x"]) == 0 or (f["octave"].min() >= 0 and f["octave"].max() < sr.LEVELS)
        b = sr.BOUNDS
        assert (f["x"] >= b[0]).all() and (f["x"] < b[1]).all() and (f["y"] >= b[2]).all() and (f["y"] < b[3]).all()
    assert (sc["slot1"] == -1).any() and all((s == -1).any() for s in sc["slot2"] if len(s) > 100)


def test_sim3_legs_composes_the_scene_legs_bit_for_bit():
    """loop_closing.sim3_legs (the documented float32 composition of sR12, sR21, t21) gives the 24 floats per candidate the scenes
    are built from, and puts each direction's source pose and transform in the right leg."""
    from orb_slam2_annotate_amd.loop_closing import sim3_legs
    sc = sr.scene(*GPU_SCENES[2])
    K4, names = (sr.FX, sr.FY, sr.CX, sr.CY), ("Rw", "tw", "sR", "t")
    for k, s in enumerate(sc["sim3"]):
        got = sim3_legs(s["R1w"], s["t1w"], s["R2w"], s["t2w"], s["s12"], s["R12"], s["t12"], K4, sr.BOUNDS, sr.SCALE, sr.LEVELS)
        for leg, want in zip(got, (sc["legs"][2 * k], sc["legs"][2 * k + 1])):
            for name in names:
                a = np.array(getattr(leg, name)[:], np.float32)
                assert np.array_equal(a.view(np.uint32), want[name].reshape(-1).view(np.uint32)), (k, name)
            assert (leg.fx, leg.cx, leg.max_x, leg.n_levels) == (np.float32(sr.FX), np.float32(sr.CX), np.float32(sr.BOUNDS[1]), sr.LEVELS)
        assert not np.array_equal(np.array(got[0].sR[:]), np.array(got[1].sR[:]))  # (the two directions differ)
    # a second camera for KF2 lands in the leg that projects INTO KF2
    l12, l21 = sim3_legs(s["R1w"], s["t1w"], s["R2w"], s["t2w"], s["s12"], s["R12"], s["t12"], K4, sr.BOUNDS, sr.SCALE, sr.LEVELS,
                         K4_2=(500.0, 501.0, 320.0, 240.0), bounds2=(0.0, 640.0, 0.0, 480.0), scale_factor2=1.25, n_levels2=6)
    assert (l12.fx, l12.fy, l12.max_x, l12.n_levels) == (500.0, 501.0, 640.0, 6) and (l21.fx, l21.n_levels) == (np.float32(sr.FX), sr.LEVELS)
