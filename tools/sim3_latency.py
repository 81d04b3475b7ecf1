#!/usr/bin/env python3
"""Latency of orbfe_sim3_ransac_multi (csrc/k_sim3.hip) -> profiles/sim3_latency.txt.

K = 1, 5 and 10 candidates of 300 hypotheses each over 100 and 500 matched pairs per candidate (the planted scene of
tests/sim3_ref.py, 30 % outliers).  Each time is the median of the timed calls after warm-up, host clock around the complete
Python call (the call is complete on return).  Beside it: the single-thread time of the same arithmetic (csrc/sim3_math.h)
compiled for the CPU, tests/cpp/sim3_cpu.cpp, on the same hypotheses (best of 20 runs of its hypothesis loop, layout
included, files excluded).

    python tools/sim3_latency.py [--reps 50] [--warmup 5] [--out profiles/sim3_latency.txt]
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
import sim3_ref as sr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sim3_latency.txt"))
    a = ap.parse_args()
    tmp = Path(tempfile.mkdtemp())
    exe = tmp / "sim3_cpu"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "tests" / "cpp"), str(ROOT / "tests" / "cpp" / "sim3_cpu.cpp"), "-o", str(exe)], check=True)
    import torch
    box = torch.cuda.get_device_name(0)  # the card the numbers are from, as the runtime names it
    lines = [f"Sim3Solver's RANSAC hypotheses on the device (k_sim3, one launch per call, one wave per hypothesis); {box}, median of "
             f"{a.reps} calls after {a.warmup} warm-up calls,",
             "Python call included (tools/sim3_latency.py).  300 hypotheses per candidate, 30 % outlier pairs, scale free.",
             "CPU: the same arithmetic (csrc/sim3_math.h) single-threaded, g++ -O2 -ffp-contract=off, best of 20 "
             "(tests/cpp/sim3_cpu.cpp).", ""]
    for n in (100, 500):
        for K in (1, 5, 10):
            sc = sr.scene(0, dict(fix_scale=0, cands=[dict(n=n, H=300, outliers=0.3)] * K))
            o = sr.operands(sc)
            fn = lambda: amd.sim3_ransac_multi(o["pair_off"], o["x1"], o["x2"], o["max1"], o["max2"], o["cam1"], o["cam2"],
                                               o["fix_scale"], o["hyp_off"], o["triples"])
            for _ in range(a.warmup):
                out = fn()
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                out = fn()
                ts.append(time.perf_counter() - t0)
            sr.write_scene(tmp / "scene.txt", sc)
            cpu = subprocess.run([str(exe), str(tmp / "scene.txt"), str(tmp / "out.txt"), "20"], check=True, capture_output=True,
                                 text=True).stdout
            kv = dict(t.split("=") for t in cpu.split())
            n_inl, status, _, _, _ = sr.read_result(tmp / "out.txt", 300 * K)
            assert np.array_equal(status, out[1]) and np.array_equal(n_inl, out[0]), "device and CPU results differ"
            lines.append(f"K = {K:2d}   pairs {n:3d}   hypotheses {300 * K:4d}   best count {int(out[0].max()):3d}   device call "
                         f"{1e3 * statistics.median(ts):7.3f} ms   CPU single thread {float(kv['cpu_us']) / 1e3:7.3f} ms")
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
