#!/usr/bin/env python3
"""Latency of orbfe_initializer_reconstruct_multi (csrc/k_init_reconstruct.hip) -> profiles/initializer_reconstruct_latency.txt.

One H problem (planar scene, 8 hypotheses) and one F problem (general scene, 4 hypotheses) at 100, 300 and 1000 inlier pairs, and
K = 8 problems of 300 (4 H and 4 F).  Each time is the median of the timed calls after warm-up, host clock around the complete
Python call (the call is complete on return).  Beside it: the single-thread time of the same arithmetic
(csrc/initializer_reconstruct_math.h) compiled for the CPU, tests/cpp/initializer_reconstruct_cpu.cpp, on the same problems
(median of 10 passes over its hypothesis loop, files excluded).  Whatever comes out is written down, rows where the CPU is
ahead included.

    python tools/initializer_reconstruct_latency.py [--reps 50] [--warmup 5] [--out profiles/initializer_reconstruct_latency.txt]
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
import initializer_reconstruct_ref as rr  # noqa: E402


def problem(rng, kind, n):
    if kind == rr.MH:
        return rr.problem(rr.MH, ir.plant("planar")[2], ir.points(rng, "planar", n), np.ones(n, bool))
    return rr.problem(rr.MF, ir.fundamental(), ir.points(rng, "general", n), np.ones(n, bool))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "initializer_reconstruct_latency.txt"))
    a = ap.parse_args()
    tmp = Path(tempfile.mkdtemp())
    exe = tmp / "initializer_reconstruct_cpu"
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", str(ROOT / "orb_slam2_annotate_amd" / "csrc"),
                    "-I", str(ROOT / "tests" / "cpp"), str(ROOT / "tests" / "cpp" / "initializer_reconstruct_cpu.cpp"), "-o", str(exe)],
                   check=True)
    import torch
    box = torch.cuda.get_device_name(0)  # the card the numbers are from, as the runtime names it
    lines = [f"ReconstructH / ReconstructF hypotheses and CheckRT on the device (k_init_reconstruct, one launch per call, one workgroup",
             f"per (problem, hypothesis)); {box}, median of {a.reps} calls after {a.warmup} warm-up calls, Python call included",
             "(tools/initializer_reconstruct_latency.py).  Every pair an inlier, sigma 1.  CPU: the same arithmetic",
             "(csrc/initializer_reconstruct_math.h) single-threaded, g++ -O2 -ffp-contract=off, median of 10 passes",
             "(tests/cpp/initializer_reconstruct_cpu.cpp).", ""]
    rng = np.random.default_rng(0)
    cases = [(f"{name} x 1", [problem(rng, kind, n)]) for n in (100, 300, 1000) for kind, name in ((rr.MH, "H"), (rr.MF, "F"))]
    cases.append(("4 H + 4 F", [problem(rng, kind, 300) for kind in (rr.MH, rr.MF) * 4]))
    for name, probs in cases:
        sc = dict(probs=probs)
        o = rr.operands(sc)
        fn = lambda: amd.initializer_reconstruct_multi(o["pair_off"], o["pairs"], o["model_kind"], o["model"], o["K4"], o["sigma"],
                                                       o["inlier_words"], o["in_word_off"])
        for _ in range(a.warmup):
            out = fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        rr.write_scene(tmp / "scene.txt", sc)
        cpu = subprocess.run([str(exe), str(tmp / "scene.txt"), str(tmp / "out.txt"), "10"], check=True, capture_output=True,
                             text=True).stdout
        host, _ = rr.read_result(tmp / "out.txt", sc)
        same = all(out[k].tobytes() == host[k].reshape(out[k].shape).tobytes() for k in ("n_good", "pair_flags", "cos_sel", "x3d", "R", "t"))
        lines.append(("" if same else "(DEVICE AND CPU BYTES DIFFER) ") +f"{name:9s}   pairs per problem {len(probs[0]['pairs']):4d}   hypotheses {len(out['n_good']):3d}   most accepted "
                     f"{int(out['n_good'].max()):4d}   device call {1e3 * statistics.median(ts):7.3f} ms   CPU single thread "
                     f"{1e3 * statistics.median(float(v) for v in cpu.split()):8.3f} ms")
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
