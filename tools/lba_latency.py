#!/usr/bin/env python3
"""Latency of orbfe_local_bundle_adjustment (csrc/k_lba.hip, csrc/lba.hip) -> profiles/lba_latency.txt.

Two shapes of tests/lba_ref.py: scene(): (10 local, 10 fixed key frames, 1 000 points, about 5 000 edges) and (30, 30, 4 000,
about 20 000), 30 % stereo edges, 2 % gross outliers.  Each time is the median of the timed calls after warm-up, host clock
around the complete Python call (the call is complete on return; it holds iterations + trials + 1 host synchronisations).
Beside it: the single-thread time of the same arithmetic and schedule (csrc/lba_math.h, csrc/lba_host.h) compiled for the CPU
in the kernels' summation orders, tests/cpp/lba_cpu.cpp, on the same scene (best of 3 runs, packing included, files
excluded).  The two must agree in every erase flag and count.  No CPU g2o figure exists here.

    python tools/lba_latency.py [--reps 10] [--warmup 2] [--out profiles/lba_latency.txt]
"""
import argparse
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import orb_slam2_annotate_amd as amd  # noqa: E402
import lba_check as chk  # noqa: E402
import lba_ref as lr  # noqa: E402

ARGS = ("edge_pose", "edge_point", "u", "v", "u_right", "inv_sigma2")
SHAPES = ((10, 10, 1000, 5000), (30, 30, 4000, 20000))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "lba_latency.txt"))
    a = ap.parse_args()
    tmp = Path(tempfile.mkdtemp())
    exe = chk.build_cpu_program(tmp)
    import subprocess

    import torch
    box = torch.cuda.get_device_name(0)  # the card the numbers are from, as the runtime names it
    cpu_name = next((l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")), "unknown CPU")
    lines = [f"Optimizer::LocalBundleAdjustment on the device (k_lba_*: host-driven Levenberg, 3 launches per iteration, 5 per trial, "
             f"one record back each); {box}, median of {a.reps} calls after {a.warmup} warm-up calls,",
             "Python call included (tools/lba_latency.py).  30 % stereo edges, 2 % gross outliers.",
             f"CPU: the same arithmetic and schedule (csrc/lba_math.h, csrc/lba_host.h) single-threaded in the kernels' summation orders, "
             f"-O2 -ffp-contract=off, best of 3 (tests/cpp/lba_cpu.cpp); {cpu_name}.", ""]
    for n_local, n_fixed, n_points, n_edges in SHAPES:
        rng = np.random.default_rng(n_points)
        outl = tuple((int(rng.integers(n_local + n_fixed)), int(p), 80) for p in rng.choice(n_points, n_edges // 50, replace=False))
        sc = lr.scene(n_points, n_local, n_fixed, n_points, stereo_fraction=0.3, vis_prob=n_edges / ((n_local + n_fixed) * n_points),
                      outliers=outl)
        fn = lambda: amd.local_bundle_adjustment(sc["n_local"], sc["Tcw"], sc["cam"], sc["xw"], *[sc[k] for k in ARGS])
        for _ in range(a.warmup):
            out = fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        chk.write_scene(tmp / "scene.bin", sc)
        cpu = subprocess.run([str(exe), str(tmp / "scene.bin"), str(tmp / "out.bin"), "3"], check=True, capture_output=True, text=True).stdout
        kv = dict(t.split("=") for t in cpu.split())
        got = chk.read_result(tmp / "out.bin", sc)
        st = out[4]
        assert np.array_equal(got["erase"], out[2]) and got["iterations"] == st["iterations"] and got["trials"] == st["trials"], \
            "device and CPU results differ"
        lines.append(f"local {n_local:2d}  fixed {n_fixed:2d}  points {n_points:4d}  edges {len(sc['u']):5d}  erased {int((out[2] != 0).sum()):4d}  "
                     f"iterations {sum(st['iterations']):2d}  trials {sum(st['trials']):2d}  syncs {st['host_syncs']:2d}   device call "
                     f"{1e3 * statistics.median(ts):8.3f} ms   CPU single thread {float(kv['cpu_us']) / 1e3:8.3f} ms")
    Path(a.out).write_text("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
