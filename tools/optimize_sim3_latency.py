#!/usr/bin/env python3
"""Latency of orbfe_optimize_sim3_multi (csrc/k_optsim3.hip) -> profiles/optimize_sim3_latency.txt.

K = 1, 5 and 10 loop candidates of 100 matched pairs each, and one problem of 2000 pairs (the scenes of
tests/optimize_sim3_ref.py, 20 % outliers, scale free).  Each time is the median of the timed calls after warm-up, host clock
around the complete Python call (the call is complete on return).  Beside it: the single-thread time of the same arithmetic
(csrc/optsim3_math.h) compiled for the CPU in the kernel's summation order, tests/cpp/optsim3_cpu.cpp, on the same problems
(best of 20 runs, packing included, files excluded).

    python tools/optimize_sim3_latency.py [--reps 50] [--warmup 5] [--out profiles/optimize_sim3_latency.txt]
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
import optimize_sim3_check as chk  # noqa: E402
import optimize_sim3_ref as osr  # noqa: E402

KEYS = ("x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2", "cam1", "cam2", "sim3_in", "th2", "fix_scale")


def batch(scs):
    cat = lambda k, shape: np.concatenate([np.asarray(sc[k], np.float32).reshape(shape) for sc in scs])
    return dict(pair_off=np.concatenate([[0], np.cumsum([len(sc["x3dc1"]) for sc in scs])]).astype(np.int32),
                x3dc1=cat("x3dc1", (-1, 3)), x3dc2=cat("x3dc2", (-1, 3)), obs1=cat("obs1", (-1, 2)), obs2=cat("obs2", (-1, 2)),
                inv_sigma2_1=cat("inv_sigma2_1", -1), inv_sigma2_2=cat("inv_sigma2_2", -1), cam1=cat("cam1", (1, 4)),
                cam2=cat("cam2", (1, 4)), sim3_in=cat("sim3_in", (1, 13)), th2=np.array([sc["th2"] for sc in scs], np.float32),
                fix_scale=np.array([sc["fix_scale"] for sc in scs], np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "optimize_sim3_latency.txt"))
    a = ap.parse_args()
    tmp = Path(tempfile.mkdtemp())
    exe = tmp / "optsim3_cpu"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    str(ROOT / "tests" / "cpp" / "optsim3_cpu.cpp"), "-o", str(exe)], check=True)
    import torch
    box = torch.cuda.get_device_name(0)  # the card the numbers are from, as the runtime names it
    lines = [f"Optimizer::OptimizeSim3 on the device (k_optimize_sim3, one launch per call, one wave per candidate); {box}, median of "
             f"{a.reps} calls after {a.warmup} warm-up calls,",
             "Python call included (tools/optimize_sim3_latency.py).  20 % outlier pairs, scale free, th2 = 10.",
             "CPU: the same arithmetic (csrc/optsim3_math.h) single-threaded in the kernel's summation order, g++ -O2 "
             "-ffp-contract=off, best of 20 (tests/cpp/optsim3_cpu.cpp).", ""]
    for K, n in ((1, 100), (5, 100), (10, 100), (1, 2000)):
        scs = [osr.scene(k, n, 0, 0.2) for k in range(K)]
        b = batch(scs)
        fn = lambda: amd.optimize_sim3_multi(b["pair_off"], *[b[k] for k in KEYS])
        for _ in range(a.warmup):
            out = fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        chk.write_scenes(tmp / "scenes.bin", scs)
        cpu = subprocess.run([str(exe), str(tmp / "scenes.bin"), str(tmp / "out.bin"), "20"], check=True, capture_output=True,
                             text=True).stdout
        kv = dict(t.split("=") for t in cpu.split())
        got = chk.read_results(tmp / "out.bin", scs)
        assert [g[0] for g in got] == [int(v) for v in out[0]], "device and CPU results differ"
        its = sum(sum(st["iterations"]) for st in out[3])
        lines.append(f"K = {K:2d}   pairs {n:4d}   kept {int(out[0].sum()):5d}   Levenberg iterations {its:3d}   device call "
                     f"{1e3 * statistics.median(ts):7.3f} ms   CPU single thread {float(kv['cpu_us']) / 1e3:7.3f} ms")
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
