#!/usr/bin/env python3
"""Latency of orbfe_triangulate_matches_multi (csrc/k_triangulate.hip) -> profiles/triangulate_latency.txt.

One key frame of 2000 keypoints against K = 1, 10 and 20 resident neighbours (the mixed mono / stereo scene of
tests/triangulate_ref.py, 30 % of the slots matched).  Each time is the median of the timed calls after warm-up, host clock
around the complete Python call (the call is complete on return).  Beside it: the single-thread time of the same arithmetic
(csrc/triangulate_math.h) compiled for the CPU, tests/cpp/triangulate_cpu.cpp, on the same pairs (best of 20 runs of its pair
loop, pair list included, files excluded).

    python tools/triangulate_latency.py [--reps 50] [--warmup 5] [--out profiles/triangulate_latency.txt]
"""
import argparse
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import orb_slam2_annotate_amd as amd  # noqa: E402
import triangulate_ref as tr  # noqa: E402


def operands(sc):
    def view(f):
        return amd.FrameView(f["x"], f["y"], f["octave"], np.zeros((f["n"], 32), np.uint8), (0.0, 640.0, 0.0, 480.0),
                             angle=np.zeros(f["n"], np.float32), u_right=f["u_right"]).upload()

    def cam(c, f):
        return amd.KeyFrameCamera(c["Tcw"], c["Ow"], c["fx"], c["fy"], c["cx"], c["cy"], c["mb"], c["mbf"], depth=f["depth"],
                                  invfx=c["invfx"], invfy=c["invfy"])
    return (view(sc["kf1"]), cam(sc["cam1"], sc["kf1"]), [view(f) for f in sc["kf2"]],
            [cam(c, f) for c, f in zip(sc["cams2"], sc["kf2"])])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangulate_latency.txt"))
    a = ap.parse_args()
    tmp = Path(tempfile.mkdtemp())
    exe = tmp / "triangulate_cpu"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "include"), "-I", str(ROOT / "tests" / "cpp"), str(ROOT / "tests" / "cpp" / "triangulate_cpu.cpp"),
                    "-o", str(exe)], check=True)
    lines = [f"LocalMapping::CreateNewMapPoints' per-pair loop on the device (k_triangulate, one launch per call); MI355X, median of "
             f"{a.reps} calls after {a.warmup} warm-up calls,",
             "Python call included (tools/triangulate_latency.py).  n1 = 2000 keypoints, resident frames, mixed mono / stereo "
             "keypoints, 30 % of the K * n1 slots matched.",
             "CPU: the same arithmetic (csrc/triangulate_math.h) single-threaded, g++ -O2 -ffp-contract=off, best of 20 "
             "(tests/cpp/triangulate_cpu.cpp).", ""]
    for K in (1, 10, 20):
        sc = tr.scene(0, 2000, K, "mixed", int(0.3 * K * 2000), short=(1, 7, 13))
        v1, c1, v2, c2 = operands(sc)
        fn = lambda: amd.triangulate_matches_multi(v1, c1, v2, c2, sc["match12"], tr.SCALE_FACTORS, tr.LEVEL_SIGMA2, tr.RATIO_FACTOR)
        for _ in range(a.warmup):
            out = fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        tr.write_scene(tmp / "scene.txt", sc)
        cpu = subprocess.run([str(exe), str(tmp / "scene.txt"), str(tmp / "out.txt"), "20"], check=True, capture_output=True,
                             text=True).stdout
        kv = dict(t.split("=") for t in cpu.split())
        status, _, _ = tr.read_result(tmp / "out.txt", K, 2000)
        assert np.array_equal(status, out[1]), "device and CPU statuses differ"
        pairs = int((sc["match12"] >= 0).sum())
        lines.append(f"K = {K:2d}   pairs {pairs:5d}   created {int(out[2].sum()):5d}   device call {1e3 * statistics.median(ts):7.3f} ms"
                     f"   CPU single thread {float(kv['cpu_us']) / 1e3:7.3f} ms")
        for f in [v1] + v2:
            f.close()
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
