#!/usr/bin/env python3
"""Latency of orbfe_mappoints_update (csrc/mappoints.hip): one update of n points, with and without descriptors, into a table
of n slots.  Median of the timed repetitions after warm-up, wall clock around the complete Python call (the call is
complete on return), as tools/pose_opt_latency.py measures.

    python tools/mappoints_update_latency.py [--n 2000] [--reps 30] [--warmup 5]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))
from pose_opt_latency import amd, fr, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    sc = fr.scene(0, a.n)
    mp = amd.MapPoints(a.n)
    slots = np.arange(a.n, dtype=np.int32)
    for label, desc in (("with descriptors", sc["desc"]), ("without descriptors", None)):
        ms, _ = timed(lambda: mp.update(slots, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], desc, sc["flags"]),
                      a.reps, a.warmup)
        print(f"mappoints_update n = {a.n:5d} {label:20s} {ms:8.3f} ms")
    mp.close()


if __name__ == "__main__":
    main()
