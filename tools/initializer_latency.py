#!/usr/bin/env python3
"""Latency of orbfe_initializer_ransac_multi (csrc/k_initializer.hip) -> profiles/initializer_latency.txt.

One problem of 200 sets (the reference's mMaxIterations; both models, so 400 hypotheses) over 100, 300 and 1000 matched pairs,
and K = 1 and 8 problems at 300 pairs (the general scene of tests/initializer_ref.py, 30 % outliers).  Each time is the median
of the timed calls after warm-up, host clock around the complete Python call (the call is complete on return).  Beside it: the
single-thread time of the same arithmetic (csrc/initializer_math.h) compiled for the CPU, tests/cpp/initializer_cpu.cpp, on the
same hypotheses (best of 10 runs of its hypothesis loop, layout included, files excluded).

    python tools/initializer_latency.py [--reps 50] [--warmup 5] [--out profiles/initializer_latency.txt]
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
import initializer_ref as ir  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "initializer_latency.txt"))
    a = ap.parse_args()
    tmp = Path(tempfile.mkdtemp())
    exe = tmp / "initializer_cpu"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "tests" / "cpp"), str(ROOT / "tests" / "cpp" / "initializer_cpu.cpp"), "-o", str(exe)], check=True)
    import torch
    box = torch.cuda.get_device_name(0)  # the card the numbers are from, as the runtime names it
    lines = [f"Initializer's H / F RANSAC hypotheses on the device (k_initializer, one launch per call, one wave per (set, model)); {box},",
             f"median of {a.reps} calls after {a.warmup} warm-up calls, Python call included (tools/initializer_latency.py).  200 sets per",
             "problem and both models (400 hypotheses), general 3-D scene, 30 % outlier pairs, sigma 1.",
             "CPU: the same arithmetic (csrc/initializer_math.h) single-threaded, g++ -O2 -ffp-contract=off, best of 10 "
             "(tests/cpp/initializer_cpu.cpp).", ""]
    for n, K in ((100, 1), (300, 1), (1000, 1), (300, 8)):
        sc = ir.build("latency", dict(probs=[dict(kind="general", n=n, S=200, sigma=1.0, outliers=0.3)] * K))
        o = ir.operands(sc)
        fn = lambda: amd.initializer_ransac_multi(o["pair_off"], o["pairs"], o["T1"], o["T2"], o["sigma"], o["hyp_off"], o["sets"])
        for _ in range(a.warmup):
            out = fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        ir.write_scene(tmp / "scene.txt", sc)
        cpu = subprocess.run([str(exe), str(tmp / "scene.txt"), str(tmp / "out.txt"), "10"], check=True, capture_output=True,
                             text=True).stdout
        kv = dict(t.split("=") for t in cpu.split())
        score, status, n_inl, _, _, _, _ = ir.read_result(tmp / "out.txt", 200 * K)
        assert np.array_equal(status, out[1]) and np.array_equal(n_inl, out[2]), "device and CPU results differ"
        lines.append(f"K = {K:2d}   pairs {n:4d}   hypotheses {400 * K:4d}   best F count {int(out[2][:, 1].max()):4d}   device call "
                     f"{1e3 * statistics.median(ts):7.3f} ms   CPU single thread {float(kv['cpu_us']) / 1e3:8.3f} ms")
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
