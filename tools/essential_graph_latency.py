#!/usr/bin/env python
"""Latency of orbfe_optimize_essential_graph and the point correction (csrc/k_essgraph.hip, csrc/essgraph.hip) next to the CPU
program (tests/cpp/essgraph_cpu.cpp: the same arithmetic and schedule on one thread) -> profiles/essential_graph_latency.txt.
A chain with a covisibility band of 3 at 200, 1 000 and 3 000 key frames with one and three loop bundles, 5 iterations; the
correction at 10^4 and 10^5 points in the array and the table form.  Recorded, not gated."""
import math
import re
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import essgraph_check as ec  # noqa: E402
import essgraph_ref as er  # noqa: E402
import orb_slam2_annotate_amd as amd  # noqa: E402
from orb_slam2_annotate_amd import optimizer  # noqa: E402


def scene(n, loops, rng):
    M = er._trajectory(n, rng, 30.0)
    corr = (er.quat_from_R(er._rot([0.1, 1.0, -0.2], 6.0)), np.array([3.0, -1.0, 2.0]), 1.05)
    S = [er.sim3_mul(corr, M[k]) if k >= n - 10 else M[k] for k in range(n)]
    edges = [(k, k + d, 0) for k in range(n) for d in (1, 2, 3) if k + d < n]
    for b in range(loops):
        a = b * (n // 8)
        edges += [(n - 2 - 3 * b, a, 1), (n - 1 - 3 * b, a + 1, 1), (n - 2 - 3 * b, a + 1, 1), (n - 1 - 3 * b, a, 1)]
    return er._scene(S, M, [1] + [0] * (n - 1), edges, n_iterations=5)


def best(f, reps=3):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        t.append(time.perf_counter() - t0)
    return min(t) * 1e3, out


def main():
    rng = np.random.default_rng(5)
    lines = ["orbfe_optimize_essential_graph on an MI355X against tests/cpp/essgraph_cpu.cpp on one CPU thread (best of 3; 5 iterations).",
             "device_ms is the whole call (staging, symbolic factorisation on the host, every round trip); the CPU program's split is its own.",
             "A split of the device time by kernel has not been taken.", ""]
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        exe = ec.build_cpu_program(tmp)
        for n in (200, 1000, 3000):
            for loops in (1, 3):
                sc = scene(n, loops, rng)
                ms, got = best(lambda: ec.call_device(optimizer, sc))
                ec.write_scene(tmp / "s.bin", sc)
                r = subprocess.run([str(exe), "opt", str(tmp / "s.bin"), str(tmp / "o.bin"), "3"], capture_output=True, text=True, check=True)
                cpu = {k: float(v) for k, v in re.findall(r"(\w+_us)=([0-9.]+)", r.stdout)}
                lines.append(f"key_frames={n} loop_bundles={loops} edges={len(sc['edge_i'])} blocks_A={got['blocks_A']} blocks_L={got['blocks_L']} "
                             f"fill={got['blocks_L'] / got['blocks_A']:.2f} iterations={got['iterations']} trials={got['trials']} "
                             f"host_syncs={got['host_syncs']} device_ms={ms:.2f} cpu_ms={cpu['cpu_us'] / 1e3:.2f} "
                             f"(cpu tables {cpu['tables_us'] / 1e3:.2f}, linearise+assemble {cpu['linearise_us'] / 1e3:.2f}, "
                             f"factor+solve {cpu['solve_us'] / 1e3:.2f}, errors {cpu['errors_us'] / 1e3:.2f})")
        sc = scene(200, 1, rng)
        out = ec.call_device(optimizer, sc)["sim3_out"]
        for npts in (10 ** 4, 10 ** 5):
            xw = (rng.normal(size=(npts, 3)) * 20).astype(np.float32)
            ref = rng.integers(0, 200, npts).astype(np.int32)
            slot = np.arange(npts, dtype=np.int32)
            mp = amd.MapPoints(npts)
            mp.update(slot, xw, np.tile(np.array([0, 0, 1], np.float32), (npts, 1)), np.full(npts, 0.1, np.float32),
                      np.full(npts, 100.0, np.float32), np.zeros((npts, 32), np.uint8), np.zeros(npts, np.uint8))
            a_ms, _ = best(lambda: optimizer.essential_graph_correct_points(sc["sim3"], out, xw, ref))
            t_ms, _ = best(lambda: mp.essential_graph_correct(slot, sc["sim3"], out, ref))
            t0 = time.perf_counter()
            er.correct_points(sc["sim3"], out, xw[:2000], ref[:2000])
            lines.append(f"correct_points={npts} array_form_ms={a_ms:.3f} table_form_ms={t_ms:.3f} "
                         f"(numpy restatement, extrapolated from 2000 points: {(time.perf_counter() - t0) * 1e3 * npts / 2000:.0f} ms)")
            mp.close()
    text = "\n".join(lines) + "\n"
    (ROOT / "profiles" / "essential_graph_latency.txt").write_text(text)
    print(text)


if __name__ == "__main__":
    main()
