"""CPU tests of tests/triangulate_ref.py, the float64 restatement of CreateNewMapPoints' per-pair loop the GPU test compares
with: the guard bands of the GPU test's scenes, the statuses the scenes reach, and the reference's own noise the GPU
tolerance is built on (profiles/triangulate_tolerance.txt)."""
from pathlib import Path

import numpy as np
import pytest

import triangulate_ref as tr

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def scenes():
    return [(id_, sc, tr.run(sc)) for id_, sc in tr.gpu_scenes()]


def test_every_gpu_scene_keeps_out_of_the_guard_bands(scenes):
    for id_, sc, r in scenes:
        assert not tr.guard_violations(sc, r), id_


def test_pair_counts_are_the_wave_and_workgroup_edges(scenes):
    counts = {id_: int((sc["match12"] >= 0).sum()) for id_, sc, r in scenes}
    for id_, spec in tr.small_specs():
        assert counts[id_] == spec["n_pairs"], id_
    assert counts[tr.FULL_ID] == tr.FULL_SPEC["n_pairs"]


def test_every_reachable_status_occurs_and_both_unproject_branches_run(scenes):
    seen = set()
    unp1 = unp2 = dlt = 0
    for id_, sc, r in scenes:
        seen |= set(r["pair_status"].tolist())
        unp1 += int(r["unp1"].sum()); unp2 += int(r["unp2"].sum()); dlt += int(r["dlt"].sum())
        assert ((r["status"] == tr.NO_MATCH) == (sc["match12"] < 0)).all(), id_
    assert seen == set(tr.REACHABLE)
    assert unp1 > 0 and unp2 > 0 and dlt > 0
    # a keypoint of key frame 1 created against more than one neighbour: winner has something to decide
    id_, sc, r = [s for s in scenes if s[0] == tr.FULL_ID][0]
    assert ((r["status"] == tr.CREATED).sum(axis=0) > 1).any()


def test_known_answer_noise_free_points_come_back():
    sc = tr.scene(3, 50, 1, "mono", 0)
    sc["match12"][0, :] = -1
    # a noise-free monocular pair: project a known point into both key frames
    X = sc["cam1"]["Ow"].astype(np.float64) + sc["cam1"]["Tcw"][:, :3].astype(np.float64).T @ np.array([0.3, -0.2, 3.0])
    for cam, f in ((sc["cam1"], sc["kf1"]), (sc["cams2"][0], sc["kf2"][0])):
        u, v, _ = tr._project(cam, X)
        f["x"][0], f["y"][0] = np.float32(u), np.float32(v)
    sc["kf1"]["octave"][0] = sc["kf2"][0]["octave"][0] = 2
    sc["match12"][0, 0] = 0
    r = tr.run(sc)
    assert r["status"][0, 0] == tr.CREATED and r["n_created"][0] == 1 and r["winner"][0] == 0
    assert np.abs(r["x3d"][0, 0] - X).max() < 1e-3  # pixels rounded to float32 at ~500 px over f = 517 px, 3 m away


def test_reference_noise_is_measured_and_recorded(scenes):
    """s_tri: the largest relative difference of an accepted point between svd(A) and svd(A with its rows reversed)."""
    s = 0.0
    for id_, sc, r in scenes:
        rr = tr.run(sc, reverse=True)
        assert np.array_equal(r["status"], rr["status"]), id_
        ok = r["status"] == tr.CREATED
        if ok.any():
            d = np.linalg.norm(r["x3d"][ok] - rr["x3d"][ok], axis=-1) / np.linalg.norm(r["x3d"][ok], axis=-1)
            s = max(s, float(d.max()))
    rec = dict(line.split("=") for line in (ROOT / "profiles" / "triangulate_tolerance.txt").read_text().split() if "=" in line)
    assert s > 0 and float(rec["s_tri"]) == pytest.approx(s, rel=1e-6, abs=0)
