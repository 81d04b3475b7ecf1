#!/usr/bin/env python3
"""Latency of orbfe_fuse_mappoints (csrc/k_project.hip: k_project_fuse + the window search) -> profiles/fuse_latency.txt.

The scene of tests/fuse_ref.py: n map points against K resident key frames of 300 keypoints, chi-square gate on, the points'
mask given.  Shapes: (K = 1, n = 1500) and (K = 20, n = 1500), the first Fuse of LocalMapping::SearchInNeighbors, and
(K = 1, n = 8000), the second.  Each time is the median of the timed calls after warm-up, host clock around the complete
Python call (the call is complete on return).  Beside it the path a caller had before: the prologue of
src/ORBmatcher.cc:960-1006 in numpy on the host (vectorised float32 over all n points, per key frame, from host copies of the
points) and orbfe_fuse_search_multi on the same resident frames with the K * n records it uploads.

    python tools/fuse_latency.py [--reps 50] [--warmup 5] [--out profiles/fuse_latency.txt]
"""
import argparse
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import orb_slam2_annotate_amd as amd  # noqa: E402
import fuse_ref as fr  # noqa: E402
from orb_slam2_annotate_amd.map_points import MapPoints, camera_pose  # noqa: E402

f32 = np.float32


def host_prologue(sc, mask):
    """Fuse's prologue on the host for all K poses: numpy float32, one vectorised pass per key frame."""
    P, N = sc["pos"], sc["normal"]
    X, Y, Z = P[:, 0], P[:, 1], P[:, 2]
    lo, hi = f32(0.8) * sc["min_dist"], f32(1.2) * sc["max_dist"]
    logf = float(f32(np.log(f32(fr.SCALE))))
    bad = (sc["flags"] & 1) != 0
    out = {k: [] for k in ("valid", "u", "v", "ur", "level")}
    with np.errstate(all="ignore"):
        for k, p in enumerate(sc["poses"]):
            R, t, Ow = p["Rcw"], p["tcw"], p["Ow"]
            xc, yc, zc = [((R[r, 0] * X + R[r, 1] * Y) + R[r, 2] * Z) + t[r] for r in range(3)]
            invz = f32(1) / zc
            u = f32(fr.FX) * (xc * invz) + f32(fr.CX)
            v = f32(fr.FY) * (yc * invz) + f32(fr.CY)
            PO = (P - Ow).astype(np.float64)
            dist = np.sqrt((PO * PO).sum(axis=1)).astype(f32)
            dot = (PO * N).sum(axis=1)
            ok = ~bad & ~mask[k] & ~(zc < 0) & (u >= fr.BOUNDS[0]) & (u < fr.BOUNDS[1]) & (v >= fr.BOUNDS[2]) & (v < fr.BOUNDS[3]) & \
                ~((dist < lo) | (dist > hi)) & ~(dot < 0.5 * dist)
            lv = np.clip(np.nan_to_num(np.ceil(np.log((sc["max_dist"] / dist).astype(np.float64)) / logf)), 0, fr.LEVELS - 1).astype(np.int32)
            out["valid"].append(ok.astype(np.uint8)); out["u"].append(u); out["v"].append(v)
            out["ur"].append(u - f32(fr.MBF) * invz); out["level"].append(np.where(ok, lv, 0))
    return {k: np.stack(v) for k, v in out.items()}


def median_ms(call, reps, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "fuse_latency.txt"))
    a = ap.parse_args()
    try:
        commit = subprocess.run(["git", "-C", str(ROOT), "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip()
    except OSError:
        commit = ""
    lines = [f"ORBmatcher::Fuse on the resident map points (orbfe_fuse_mappoints: k_project_fuse + one window search); MI355X, median of "
             f"{a.reps} calls after {a.warmup} warm-up calls,",
             "Python call included (tools/fuse_latency.py).  K resident key frames of 300 keypoints, chi-square gate on, mask given.",
             "before: the prologue in numpy on the host (float32, vectorised per key frame) + orbfe_fuse_search_multi on the same frames.",
             f"taken on the tree that follows commit {commit or 'unknown'}", "",
             f"{'K':>3} {'n':>6} {'one call ms':>12} {'before ms':>10} {'(host prologue':>15} {'+ search)':>10} {'before / call':>14}"]
    m = amd.ORBmatcher(0.6)
    for K, n in ((1, 1500), (20, 1500), (1, 8000)):
        sc = fr.scene(100 + K, n, K)
        slot = np.random.default_rng(K).permutation(16384)[:n].astype(np.int32)
        mp = MapPoints(16384)
        mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
        poses = [camera_pose(p["Rcw"], p["tcw"], (fr.FX, fr.FY, fr.CX, fr.CY), fr.MBF, fr.BOUNDS, fr.SCALE, fr.LEVELS, Ow=p["Ow"])
                 for p in sc["poses"]]
        views = [amd.FrameView(f["x"], f["y"], f["octave"], f["desc"], fr.BOUNDS, angle=np.zeros(len(f["x"]), f32),
                               u_right=f["u_right"]).upload() for f in sc["frames"]]
        mask = (sc["skip"] != 0) | sc["in_kf"]

        def one():
            return mp.fuse(views, poses, slot, skip=mask, scale_factors=fr.SF, inv_level_sigma2=fr.INV_SIGMA2)

        def prologue():
            return host_prologue(sc, mask)

        def before():
            pr = prologue()
            return m.FuseSearchMulti(views, fr.SF, pr["valid"], pr["u"], pr["v"], pr["level"], sc["desc"], th=3.0,
                                     inv_level_sigma2=fr.INV_SIGMA2, ur=pr["ur"])

        assert np.array_equal(one(), before()), "the two paths disagree"
        t_one, t_before, t_pro = median_ms(one, a.reps, a.warmup), median_ms(before, a.reps, a.warmup), median_ms(prologue, a.reps, a.warmup)
        lines.append(f"{K:>3} {n:>6} {t_one:>12.3f} {t_before:>10.3f} {t_pro:>15.3f} {t_before - t_pro:>10.3f} {t_before / t_one:>14.2f}")
        mp.close()
    text = "\n".join(lines) + "\n"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
