#!/usr/bin/env python3
"""Latency of the last-frame / key-frame searches on the resident map points (csrc/k_project.hip: k_project_track + the window
search and claim) -> profiles/track_latency.txt.

The scenes of tests/track_ref.py against one resident current frame of 2000 keypoints (stereo):
  last frame   n = 1000 points, th = 7, mode 0, rotation check on (Tracking::TrackWithMotionModel);
  key frames   K = 5 candidates of 500 points each, th = 10 / 3, ORBdist = 100 / 64 (Tracking::Relocalization).
"after" is the one resident call of this tree.  "before" is what a caller had: the prologue in numpy on the host (float32,
vectorised, the descriptors gathered from a host array of all map points) plus the host-array call
(orbfe_search_by_projection_last_frame / orbfe_search_by_projection_keyframe_multi) on the same resident frame -- timed with
the package of a checkout of the PARENT commit (--parent-root, built), in a process of its own on the same machine.  The two
sides alternate for --rounds rounds; each side's figure is the median of its rounds' medians (median of --reps calls after
--warmup calls, host clock around the complete Python call, which is complete on return).

    python tools/track_latency.py --parent-root <checkout of the parent commit> [--out profiles/track_latency.txt]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
CUR = 2000


def median_ms(call, reps, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def host_prologue(tr, sc, world_desc, order, kf):
    """The caller's prologue on the host for the concatenated list: numpy float32, one vectorised pass per pose."""
    out = {k: [] for k in ("valid", "u", "v", "inv_z", "level")}
    off = sc["offsets"]
    with np.errstate(all="ignore"):
        for k, p in enumerate(sc["poses"]):
            s = slice(off[k], off[k + 1])
            P = sc["pos"][s]
            R, t, Ow = p["Rcw"], p["tcw"], p["Ow"]
            xc, yc, zc = [((R[r, 0] * P[:, 0] + R[r, 1] * P[:, 1]) + R[r, 2] * P[:, 2]) + t[r] for r in range(3)]
            invz = f32(1) / zc
            u = f32(tr.FX) * xc * invz + f32(tr.CX)
            v = f32(tr.FY) * yc * invz + f32(tr.CY)
            ok = (sc["skip"][s] == 0) & (u >= tr.BOUNDS[0]) & (u <= tr.BOUNDS[1]) & (v >= tr.BOUNDS[2]) & (v <= tr.BOUNDS[3])
            lv = np.zeros(len(P), np.int32)
            if kf:
                PO = (P - Ow).astype(np.float64)
                dist = np.sqrt((PO * PO).sum(axis=1)).astype(f32)
                ok &= ((sc["flags"][s] & 1) == 0) & ~((dist < f32(0.8) * sc["min_dist"][s]) | (dist > f32(1.2) * sc["max_dist"][s]))
                logf = float(f32(np.log(f32(tr.SCALE))))
                lv = np.clip(np.nan_to_num(np.ceil(np.log((sc["max_dist"][s] / dist).astype(np.float64)) / logf)), 0, tr.LEVELS - 1).astype(np.int32)
            else:
                ok &= ~(invz < 0)
            for name, a in (("valid", ok.astype(np.uint8)), ("u", np.where(ok, u, 0).astype(f32)), ("v", np.where(ok, v, 0).astype(f32)),
                            ("inv_z", np.where(ok, invz, 0).astype(f32)), ("level", np.where(ok, lv, 0).astype(np.int32))):
                out[name].append(a)
    out["desc"] = world_desc[order]  # the gather of 32 bytes per point from the map points
    out["obs"] = (sc["flags"] >> 1) & 1
    return out


def side(which, reps, warmup):
    """One side's medians (ms) as a dict; run in a process that imports the package from sys.path[0]."""
    sys.path.insert(1, str(ROOT / "tests"))
    import track_ref as tr
    import orb_slam2_annotate_amd as amd
    from orb_slam2_annotate_amd.map_points import MapPoints, camera_pose
    m = amd.ORBmatcher(0.9, True)
    res = {}
    for name, (seed, n, K) in (("last", (200, 1000, 1)), ("kf", (201, 500, 5))):
        sc = tr.scene(seed, n, K)
        N = len(sc["pos"])
        frame = tr.current_frame(np.random.default_rng(seed), sc, stereo=True, m=CUR)
        Cur = amd.FrameView(frame["x"], frame["y"], frame["octave"], frame["desc"], tr.BOUNDS, angle=frame["angle"],
                            u_right=frame["u_right"]).upload()
        slot = np.random.default_rng(seed).permutation(16384)[:N].astype(np.int32)
        world_desc = np.zeros((16384, 32), np.uint8)
        world_desc[slot] = sc["desc"]
        mp = MapPoints(16384)
        mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
        poses = [camera_pose(p["Rcw"], p["tcw"], (tr.FX, tr.FY, tr.CX, tr.CY), tr.MBF, tr.BOUNDS, tr.SCALE, tr.LEVELS, Ow=p["Ow"])
                 for p in sc["poses"]]
        off = sc["offsets"]
        jobs = lambda a: [a[off[k]:off[k + 1]] for k in range(K)]  # noqa: E731

        def prologue():
            return host_prologue(tr, sc, world_desc, slot, name == "kf")

        if name == "last":
            def before():
                pr = prologue()
                return m.SearchByProjectionLastFrame(Cur, tr.SF, pr["valid"][0], pr["u"][0], pr["v"][0], sc["last_octave"], sc["angle"],
                                                     pr["desc"], 7.0, mode=0, mbf=tr.MBF, invzc=pr["inv_z"][0], obs_positive=pr["obs"])[1]

            def after():
                return mp.SearchByProjectionLastFrame(Cur, slot, sc["last_octave"], sc["angle"], poses[0], tr.SF, 7.0, mode=0, skip=sc["skip"])[1]
        else:
            def before():
                pr = prologue()
                cands = [dict(valid=pr["valid"][k], u=pr["u"][k], v=pr["v"][k], level=pr["level"][k], kf_angle=jobs(sc["angle"])[k],
                              mp_desc=jobs(pr["desc"])[k], th=float(sc["th"][k]), ORBdist=int(sc["orb_dist"][k])) for k in range(K)]
                return m.SearchByProjectionKeyFrameMulti(Cur, tr.SF, cands)[1]

            def after():
                return mp.SearchByProjectionKeyFrames(Cur, poses, jobs(slot), jobs(sc["angle"]), tr.SF, sc["th"], sc["orb_dist"],
                                                      skips=jobs(sc["skip"]))[1]
        if which == "after":
            res[name + "_agree"] = bool(np.array_equal(after(), before()))
            res[name] = median_ms(after, reps, warmup)
        else:
            res[name] = median_ms(before, reps, warmup)
            res[name + "_prologue"] = median_ms(prologue, reps, warmup)
        mp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: the 'before' side imports its package")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "track_latency.txt"))
    ap.add_argument("--side", choices=["after", "before"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.side:
        print("RESULT " + json.dumps(side(a.side, a.reps, a.warmup)))
        return
    if not a.parent_root:
        ap.error("--parent-root is needed: 'before' is timed with the parent commit's package")
    rounds = {"before": [], "after": []}
    for _ in range(a.rounds):
        for which, root in (("before", Path(a.parent_root).resolve()), ("after", ROOT)):
            code = (f"import sys; sys.path.insert(0, {str(root)!r}); sys.argv = ['track_latency', '--side', {which!r}, '--reps', '{a.reps}', "
                    f"'--warmup', '{a.warmup}']; import runpy; runpy.run_path({str(Path(__file__).resolve())!r}, run_name='__main__')")
            r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True)
            rounds[which].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
    agree = all(x["last_agree"] and x["kf_agree"] for x in rounds["after"])
    for x in rounds["after"]:
        del x["last_agree"], x["kf_agree"]
    med = {w: {k: statistics.median(x[k] for x in rounds[w]) for k in rounds[w][0]} for w in rounds}
    rng = {w: {k: (min(x[k] for x in rounds[w]), max(x[k] for x in rounds[w])) for k in rounds[w][0]} for w in rounds}
    lines = [f"The last-frame / key-frame SearchByProjection on the resident map points (k_project_track + window search + claim); MI355X, "
             f"median of {a.reps} calls after {a.warmup} warm-up calls,",
             f"Python call included (tools/track_latency.py); {a.rounds} alternating rounds a side, the median round, min .. max of the rounds in brackets.",
             f"One resident current frame of {CUR} keypoints (stereo), rotation check on, mask given.",
             "before: the prologue in numpy on the host (float32, vectorised, descriptors gathered) + the host-array call, with the PARENT commit's package",
             "in a process of its own on the same machine; after: the one resident call of this tree.", "",
             f"{'case':<28} {'one call ms':>22} {'before ms':>22} {'(host prologue)':>16} {'before / call':>14}"]
    for name, label in (("last", "last frame, n = 1000"), ("kf", "key frames, K = 5 x 500")):
        t1, t0, tp = med["after"][name], med["before"][name], med["before"][name + "_prologue"]
        b1, b0 = rng["after"][name], rng["before"][name]
        lines.append(f"{label:<28} {t1:>8.3f} [{b1[0]:.3f}..{b1[1]:.3f}] {t0:>8.3f} [{b0[0]:.3f}..{b0[1]:.3f}] {tp:>16.3f} {t0 / t1:>14.2f}")
    lines += ["", f"the match arrays of the two paths are equal: {'yes' if agree else 'NO'}"]
    text = "\n".join(lines) + "\n"
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(text)
    print(text)


if __name__ == "__main__":
    main()
