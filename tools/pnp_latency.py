"""Latency of orbfe_pnp_solve_multi (both launches and the record scan), host to host: K = 1 / 5 / 10 candidates x 300
hypotheses at 50 and 200 correspondences, median of 30 calls, next to the same arithmetic on one CPU thread
(tests/cpp/pnp_cpu.cpp, best of 5).  Writes profiles/pnp_latency.txt, or the file named as its argument."""
import os
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

import pnp_ref as pr  # noqa: E402

import orb_slam2_annotate_amd as amd  # noqa: E402


def main():
    tmp = Path(tempfile.mkdtemp())
    exe = tmp / "pnp_cpu"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++", "-std=c++17", "-O2", "-ffp-contract=off", "-I",
                    str(ROOT / "orb_slam2_annotate_amd" / "csrc"), str(ROOT / "tests" / "cpp" / "pnp_cpu.cpp"), "-o", str(exe)],
                   check=True)
    lines = ["# tools/pnp_latency.py on one MI355X: orbfe_pnp_solve_multi host to host (upload, k_pnp_ransac, download, record scan,",
             "# upload, k_pnp_refine, download), median of 30 calls after 3 warm-up calls; cpu = tests/cpp/pnp_cpu.cpp, the same",
             "# arithmetic on one CPU thread of the same machine, best of 5.  70 % inliers, 0.3 px noise, 300 hypotheses per candidate.",
             "# K  n    hypotheses  records  gpu_ms   cpu_ms"]
    for n in (50, 200):
        for K in (1, 5, 10):
            cands = [pr.make_candidate(900 + 10 * K + k, n, 300) for k in range(K)]
            off = np.concatenate([[0], np.cumsum([n] * K)]).astype(np.int32)
            ho = np.concatenate([[0], np.cumsum([300] * K)]).astype(np.int32)
            args = (off, np.concatenate([c["p3d"] for c in cands]), np.concatenate([c["p2d"] for c in cands]),
                    np.concatenate([c["max_err"] for c in cands]), np.stack([c["cam"] for c in cands]), ho,
                    np.concatenate([c["sets"] for c in cands]), [c["min_inliers"] for c in cands])
            ts = []
            for i in range(33):
                t0 = time.perf_counter()
                r = amd.pnp_solve_multi(*args)
                ts.append((time.perf_counter() - t0) * 1e3)
            pr.write_scene(tmp / "s.txt", cands)
            out = subprocess.run([str(exe), str(tmp / "s.txt"), str(tmp / "o.txt"), "5"], check=True, capture_output=True, text=True)
            cpu_ms = float(out.stdout.split("cpu_us=")[1]) / 1e3
            lines.append(f"{K:<3d} {n:<4d} {300 * K:<11d} {len(r['rec_hyp']):<8d} {statistics.median(ts[3:]):<8.3f} {cpu_ms:.3f}")
            print(lines[-1], flush=True)
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "pnp_latency.txt"
    out.write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
