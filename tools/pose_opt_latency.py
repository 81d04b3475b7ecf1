#!/usr/bin/env python3
"""Latency of orbfe_pose_optimization* (csrc/k_poseopt.hip) -> profiles/pose_opt_latency.txt.

Single calls at n = 200, 1000, 2000 (mixed mono / stereo edges, 20 % planted outliers) in the array and the table form, one
batch of 512 problems at n = 1000, and the TrackLocalMap pair -- SearchLocalPoints then the optimisation on its match[] -- as
two calls.  Each time is the median of the timed repetitions after warm-up, wall clock around the complete Python call
(every call is complete on return).  The Levenberg iterations and lambda trials the kernel executed stand next to each
time: latency is proportional to them.  No CPU g2o figure exists for this project (g2o needs Eigen, which the build machines
do not have), so none is quoted.

    python tools/pose_opt_latency.py [--reps 30] [--warmup 5] [--out profiles/pose_opt_latency.txt]
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import frustum_ref as fr  # noqa: E402
import orb_slam2_annotate_amd as amd  # noqa: E402
import pose_opt_ref as pr  # noqa: E402


def timed(fn, reps, warmup):
    for _ in range(warmup):
        out = fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * statistics.median(ts), out


def work(st):
    return f"rounds {st['rounds']}  iterations {sum(st['iterations']):3d}  trials {sum(st['trials']):3d}"


def table_of(sc):
    """The scene's edges as a map-point table, a resident-free frame view and the identity match."""
    n = len(sc["u"])
    mp = amd.MapPoints(n)
    slots = np.arange(n, dtype=np.int32)
    z = np.zeros(n, np.float32)
    mp.update(slots, sc["xw"], np.zeros((n, 3), np.float32), z, z + 1, np.zeros((n, 32), np.uint8), np.full(n, 2, np.uint8))
    F = amd.FrameView(sc["u"], sc["v"], sc["octave"], np.zeros((n, 32), np.uint8), fr.BOUNDS, u_right=sc["u_right"])
    return mp, F, slots, slots.copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pose_opt_latency.txt"))
    a = ap.parse_args()
    lines = [f"Optimizer::PoseOptimization on the device (k_pose_optimize, one launch per call); MI355X, median of {a.reps} calls after "
             f"{a.warmup} warm-up calls,", "Python call included (tools/pose_opt_latency.py).  Mixed mono / stereo edges, 20 % planted outliers "
             "(tests/pose_opt_ref.py scene).", "No CPU g2o figure exists for this project (g2o needs Eigen, which is not available): none is quoted.",
             ""]
    for n in (200, 1000, 2000):
        sc = pr.scene(0, n, 0.5, 0.2)
        ms, out = timed(lambda: amd.pose_optimization(sc["xw"], sc["u"], sc["v"], sc["u_right"], sc["inv_sigma2"], sc["K5"], sc["Tcw"]),
                        a.reps, a.warmup)
        lines.append(f"array form   n = {n:5d}                     {ms:8.3f} ms   {work(out[3])}   inliers {out[0]}")
        mp, F, slots, match = table_of(sc)
        ms, out = timed(lambda: mp.pose_optimization(F, slots, match, sc["Tcw"], sc["K5"], pr.INV_LEVEL_SIGMA2), a.reps, a.warmup)
        lines.append(f"table form   n = {n:5d}                     {ms:8.3f} ms   {work(out[3])}   inliers {out[0]}")
        mp.close()
    Q, n = 512, 1000
    scs = [pr.scene(s, n, 0.5, 0.2) for s in range(Q)]
    off = (np.arange(Q + 1) * n).astype(np.int32)
    cat = lambda k: np.concatenate([s[k] for s in scs])
    arrs = [cat(k) for k in ("xw", "u", "v", "u_right", "inv_sigma2")]
    K, T = np.stack([s["K5"] for s in scs]), np.stack([s["Tcw"] for s in scs])
    ms, out = timed(lambda: amd.pose_optimization_batch(off, *arrs, K, T), max(a.reps // 3, 5), 2)
    its = sum(sum(st["iterations"]) for st in out[3]) / Q
    trs = sum(sum(st["trials"]) for st in out[3]) / Q
    lines.append(f"batch        Q = {Q}, n = {n}              {ms:8.3f} ms   = {Q / ms * 1e3:9.0f} problems/s   mean iterations {its:.1f}  "
                 f"trials {trs:.1f} per problem")
    # TrackLocalMap: 2000 local map points (tests/frustum_ref.py scene 0), one keypoint on every visible point
    npts = 2000
    sc = fr.scene(0, npts)
    mp = amd.MapPoints(npts)
    slots = np.arange(npts, dtype=np.int32)
    mp.update(slots, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
    s32 = fr.spec32(sc)
    vis = np.flatnonzero(s32["in_view"])
    rng = np.random.default_rng(1)
    x = (s32["proj_x"][vis] + rng.normal(0, 0.5, len(vis))).astype(np.float32)
    y = (s32["proj_y"][vis] + rng.normal(0, 0.5, len(vis))).astype(np.float32)
    ur = np.where(rng.random(len(vis)) < 0.5, s32["proj_xr"][vis], -1).astype(np.float32)
    F = amd.FrameView(x, y, s32["level"][vis].astype(np.int32), sc["desc"][vis], fr.BOUNDS, u_right=ur)
    pose = amd.camera_pose(sc["Rcw"], sc["tcw"], (fr.FX, fr.FY, fr.CX, fr.CY), fr.MBF, fr.BOUNDS, fr.SCALE, fr.LEVELS, Ow=sc["Ow"])
    sf = np.array([fr.SCALE ** l for l in range(fr.LEVELS)], np.float32)
    Tcw = np.eye(4, dtype=np.float32)
    Tcw[:3, :3], Tcw[:3, 3] = sc["Rcw"], sc["tcw"]
    K5 = np.array(pr.K5, np.float32)
    ms_s, (nm, match, _) = timed(lambda: mp.SearchLocalPoints(F, slots, pose, sf, th=3.0), a.reps, a.warmup)
    ms_o, out = timed(lambda: mp.pose_optimization(F, slots, match, Tcw, K5, pr.INV_LEVEL_SIGMA2), a.reps, a.warmup)

    def pair():
        _, m, _ = mp.SearchLocalPoints(F, slots, pose, sf, th=3.0)
        return mp.pose_optimization(F, slots, m, Tcw, K5, pr.INV_LEVEL_SIGMA2)
    ms_p, _ = timed(pair, a.reps, a.warmup)
    lines += ["", f"TrackLocalMap pair: {npts} local map points in the table, a frame of {F.N} keypoints (one on every visible point), {nm} matches",
              f"  SearchLocalPoints                            {ms_s:8.3f} ms   (profiles/local_points_latency.txt: 0.056 ms on its 2000-keypoint resident frame)",
              f"  pose optimisation on its match[]             {ms_o:8.3f} ms   {work(out[3])}   inliers {out[0]}",
              f"  both, as two calls                           {ms_p:8.3f} ms"]
    mp.close()
    text = "\n".join(lines) + "\n"
    Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
