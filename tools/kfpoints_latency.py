#!/usr/bin/env python3
"""Latency of the key-frame-row calls of the observation graph (orbfe_obsgraph_keyframe_points_union, _tracked_points), host
to host around the C call with its arrays prepared, next to the same loops compiled (tools/kfpoints_host_bench.cpp: the
reference's loops of csrc/obsgraph_host.h over the same flat arrays, one CPU thread, -O2, no sanitizer).  Map: 80 key frames
of 2048 entries over 60 000 point slots, every point in about 8 key frames -- the per-frame shape of
Tracking::UpdateLocalPoints.  Fails without a GPU.

  python tools/kfpoints_latency.py [--out profiles/kfpoints_latency.txt] [--reps 30]
"""
import argparse
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import orb_slam2_annotate_amd as amd  # noqa: E402
from orb_slam2_annotate_amd import _lib  # noqa: E402
from orb_slam2_annotate_amd._lib import check, ptr  # noqa: E402

K, W, P, POOL = 80, 2048, 60000, 20480  # 80 * 2048 entries over 20 480 points: 8-fold overlap


def build(rng):
    pool = rng.choice(P, POOL, replace=False).astype(np.int32)
    rows = pool[rng.integers(0, POOL, (K, W))]
    rows[rng.random((K, W)) < 0.1] = -1  # NULL
    bad = (rng.random(P) < 0.05).astype(np.uint8)
    g = amd.ObservationGraph(P, K, 8)
    g.set_keyframes(np.arange(K), np.arange(K), np.zeros((K, 3), np.float32))
    g.set_points(np.arange(P), bad, np.full(P, -1, np.int32))
    # nObs: one to three mono observations per pool point
    n_obs = np.zeros(P, np.int32)
    for k in range(3):
        seen = pool[rng.random(POOL) < 0.6]
        g.add_observations(seen, np.full(len(seen), k, np.int32), np.zeros(len(seen), np.uint16), np.zeros(len(seen), np.uint8),
                           np.zeros(len(seen), np.uint8))
        n_obs[seen] += 1
    g.enable_keyframe_points(W)
    for k in range(K):
        g.set_keyframe_points(k, rows[k])
    return g, rows, bad, n_obs


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
        sys.exit("kfpoints_latency: no GPU")
    rng = np.random.default_rng(1)
    g, rows, bad, n_obs = build(rng)
    cases = [  # (name, kind, queries, min_obs)
        ("union, 80 key frames x 2048 (UpdateLocalPoints per frame)", 0, [rng.permutation(K).tolist()], 0),
        ("union, 20 key frames x 2048", 0, [rng.permutation(K)[:20].tolist()], 0),
        ("union, 10 one-frame queries in one call", 0, [[int(k)] for k in rng.permutation(K)[:10]], 0),
        ("TrackedMapPoints(3), 1 key frame", 1, [[5]], 3),
        ("TrackedMapPoints(3), 30 key frames in one call", 1, [[int(k)] for k in rng.permutation(K)[:30]], 3),
    ]
    blob = [np.array([P, K, W, len(cases), a.reps], np.int32), rows.astype(np.int32).reshape(-1), np.full(K, W, np.int32),
            bad.astype(np.int32), n_obs]
    device, counts = [], []
    for name, kind, qs, min_obs in cases:
        off = np.zeros(len(qs) + 1, np.int32)
        off[1:] = np.cumsum([len(q) for q in qs])
        flat = np.concatenate([np.asarray(q, np.int32) for q in qs])
        blob += [np.array([kind, len(qs), min_obs], np.int32), off, flat]
        cnt = np.zeros(len(qs), np.int32)
        if kind == 0:
            cap = P
            out = np.zeros(len(qs) * cap, np.int32)
            call = lambda: check(L.orbfe_obsgraph_keyframe_points_union(g._h, len(qs), ptr(off), ptr(flat), cap, ptr(out), ptr(cnt)))  # noqa: E731
        else:
            call = lambda: check(L.orbfe_obsgraph_tracked_points(g._h, len(flat), ptr(flat), min_obs, ptr(cnt)))  # noqa: E731
        device.append(timed(call, a.reps))
        counts.append((int(cnt[0]), int(cnt.sum())))
    with tempfile.TemporaryDirectory() as tmp:
        exe, data = Path(tmp) / "kfpoints_host_bench", Path(tmp) / "arrays.bin"
        subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'orb_slam2_annotate_amd' / 'csrc'}", str(ROOT / "tools" / "kfpoints_host_bench.cpp"),
                        "-o", str(exe)], check=True)
        np.concatenate(blob).astype(np.int32).tofile(data)
        text = subprocess.run([str(exe), str(data)], check=True, capture_output=True, text=True).stdout
    cpu = [line.split() for line in text.splitlines()]
    lines = [f"key-frame rows: {K} key frames x {W} entries over {P} point slots ({POOL} of them in the rows, 10 % NULL entries, 5 % bad points); "
             f"median of {a.reps} calls, ms, host to host around the C call; cpu = the same loop compiled (-O2), one thread, same arrays"]
    for (name, _, qs, _), dev, c, (first, total) in zip(cases, device, cpu, counts):
        assert (int(c[3]), int(c[4])) == (first, total), (name, c, first, total)  # both sides did the same work
        lines.append(f"{name:<60s} device {dev:8.3f}   cpu {float(c[2]):8.4f}   count[0] {first:6d}  sum {total:6d}")
    out_text = "\n".join(lines) + "\n"
    print(out_text, end="")
    if a.out:
        Path(a.out).write_text(out_text)


if __name__ == "__main__":
    main()
