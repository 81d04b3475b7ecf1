#!/usr/bin/env python3
"""Latency of MapPoint::ComputeDistinctiveDescriptors for the points a new key frame touched, host to host, two ways on the
world of tools/obsgraph_latency.py (500 key frames, 20 000 points, mean row 6):

  (a) resident: orbfe_obsgraph_distinctive_descriptors_mappoints -- only the slot list travels, the winners land in the
      map-point table;
  (b) arrays:   what a caller had before it -- a compiled host gather of the descriptor lists from flat arrays
      (tools/distinctive_host_gather.cpp, -O2, one thread), orbfe_distinctive_descriptors, the winners picked and written
      through orbfe_mappoints_update.

Both leave the same descriptors in the table (checked).  Fails without a GPU.

  python tools/distinctive_latency.py [--out profiles/distinctive_latency.txt] [--reps 30]
"""
import argparse
import ctypes as C
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import orb_slam2_annotate_amd as amd  # noqa: E402
from obsgraph_latency import N_KF, N_PTS, build  # noqa: E402
from orb_slam2_annotate_amd import _lib  # noqa: E402
from orb_slam2_annotate_amd._lib import check, ptr  # noqa: E402


def timed(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    L = _lib.load()
    if L.orbfe_device_count() < 1:
        sys.exit("distinctive_latency: no GPU")
    rng = np.random.default_rng(1)
    g, rows, _, _, pos = build(rng)  # the rows hold idx 0: this tool gives every observation a descriptor row of its own
    g.clear()
    g.set_keyframes(np.arange(N_KF), np.arange(N_KF), np.zeros((N_KF, 3), np.float32))
    g.set_points(np.arange(N_PTS), np.zeros(N_PTS, np.uint8), [r[0] for r in rows])
    row_off = np.zeros(N_PTS + 1, np.int32)
    row_off[1:] = np.cumsum([len(r) for r in rows])
    row_kf = np.concatenate(rows).astype(np.int32)
    seen = np.zeros(N_KF, np.int64)
    row_idx = np.zeros(len(row_kf), np.uint16)
    for e, k in enumerate(row_kf):
        row_idx[e] = seen[k]
        seen[k] += 1
    width = int((seen.max() + 63) // 64 * 64)
    # an observation's descriptor: the point's own with a few bits flipped
    base = rng.integers(0, 256, (N_PTS, 32), dtype=np.uint8)
    kf_desc = np.zeros((N_KF, width, 32), np.uint8)
    owner = np.repeat(np.arange(N_PTS), np.diff(row_off))
    noise = np.packbits(rng.random((len(row_kf), 256)) < 0.03, axis=1)
    kf_desc[row_kf, row_idx] = base[owner] ^ noise
    g.add_observations(owner.astype(np.int32), row_kf, row_idx, np.zeros(len(row_kf), np.uint8), np.zeros(len(row_kf), np.uint8))
    g.enable_keyframe_descriptors(width)
    for k in range(N_KF):
        g.set_keyframe_descriptors(k, kf_desc[k, :seen[k]])
    kf_bad = np.zeros(N_KF, np.uint8)
    lens = np.diff(row_off)

    with tempfile.TemporaryDirectory() as tmp:
        so = Path(tmp) / "libdistinctive_host_gather.so"
        subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", str(ROOT / "tools" / "distinctive_host_gather.cpp"), "-o", str(so)],
                       check=True)
        H = C.CDLL(str(so))
        vp, ci = C.c_void_p, C.c_int
        H.distinctive_gather.argtypes = [ci, vp, vp, vp, vp, vp, vp, ci, vp, vp]
        H.distinctive_pick.argtypes = [ci, vp, vp, vp, vp]
        H.distinctive_pick.restype = None
        lines = [f"ComputeDistinctiveDescriptors on the resident graph: {N_KF} key frames, {N_PTS} points, rows mean {lens.mean():.1f} longest "
                 f"{lens.max()}, {len(row_kf)} descriptors in a store of {width} per key frame; median of {a.reps} calls, ms, host to host",
                 "(a) resident = orbfe_obsgraph_distinctive_descriptors_mappoints;  (b) arrays = compiled gather + "
                 "orbfe_distinctive_descriptors + pick + orbfe_mappoints_update (its three parts listed)"]
        for n in (1000, 4000):
            slots = rng.choice(N_PTS, n, replace=False).astype(np.int32)
            resident, arrays = amd.MapPoints(N_PTS), amd.MapPoints(N_PTS)
            p, one, flags = np.ascontiguousarray(pos[slots]), np.ones(n, np.float32), np.zeros(n, np.uint8)
            for mp in (resident, arrays):
                mp.update(slots, p, p, one, one, np.zeros((n, 32), np.uint8), flags)
            valid = np.zeros(n, np.uint8)
            run_a = lambda: check(L.orbfe_obsgraph_distinctive_descriptors_mappoints(g._h, resident._h, n, ptr(slots), None, None, ptr(valid)))  # noqa: E731
            total = int(lens[slots].sum())
            lists, off = np.zeros((total, 32), np.uint8), np.zeros(n + 1, np.int32)
            best, winners = np.zeros(n, np.int32), np.zeros((n, 32), np.uint8)
            gather = lambda: H.distinctive_gather(n, ptr(slots), ptr(row_off), ptr(row_kf), ptr(row_idx), ptr(kf_bad), ptr(kf_desc), width,  # noqa: E731
                                                  ptr(lists), ptr(off))
            device = lambda: check(L.orbfe_distinctive_descriptors(0, ptr(lists), ptr(off), n, ptr(best)))  # noqa: E731

            def update():
                H.distinctive_pick(n, ptr(best), ptr(lists), ptr(off), ptr(winners))
                check(L.orbfe_mappoints_update(arrays._h, n, ptr(slots), ptr(p), ptr(p), ptr(one), ptr(one), ptr(winners), ptr(flags)))

            def run_b():
                gather()
                device()
                update()

            ta, tb = timed(run_a, a.reps), timed(run_b, a.reps)
            parts = [timed(f, a.reps) for f in (gather, device, update)]
            assert valid.all() and np.array_equal(resident.descriptors(slots), arrays.descriptors(slots)), "the two paths disagree"
            lines.append(f"{n:5d} points ({total:6d} observations)   (a) resident {ta:8.3f}   (b) arrays {tb:8.3f}   "
                         f"[gather {parts[0]:.3f}  orbfe_distinctive_descriptors {parts[1]:.3f}  pick + update {parts[2]:.3f}]")
            resident.close()
            arrays.close()
    out_text = "\n".join(lines) + "\n"
    print(out_text, end="")
    if a.out:
        Path(a.out).write_text(out_text)


if __name__ == "__main__":
    main()
