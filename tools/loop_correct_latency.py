#!/usr/bin/env python3
"""Latency of the loop correction on the resident map points (orbfe_correct_loop_mappoints, orbfe_gba_update_mappoints), host
to host around the C call with its arrays prepared, next to the path a caller had before them: orbfe_mappoints_positions ->
the host loop compiled (tools/loop_correct_host_bench.cpp: csrc/loopcorrect_host.h over flat arrays, one CPU thread, -O2, no
sanitizer) -> orbfe_mappoints_update -> orbfe_obsgraph_update_normal_depth_mappoints (the last only for CorrectLoop).  Map:
20 and 80 key frames of 2048 entries over 60 000 point slots, the shape of tools/kfpoints_latency.py; the GBA update at
60 000 points, 5 % of them not in the GBA.  A record, not a gate.  Fails without a GPU.

  python tools/loop_correct_latency.py [--out profiles/loop_correct_latency.txt] [--reps 30]
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

KMAX, W, P, POOL = 80, 2048, 60000, 20480
SF = (1.2 ** np.arange(8)).astype(np.float32)
f32 = np.float32


def build(rng):
    pool = rng.choice(P, POOL, replace=False).astype(np.int32)
    rows = pool[rng.integers(0, POOL, (KMAX, W))]
    rows[rng.random((KMAX, W)) < 0.1] = -1  # NULL
    bad = (rng.random(P) < 0.05).astype(np.uint8)
    ref = rng.integers(0, 3, P).astype(np.int32)
    g = amd.ObservationGraph(P, KMAX, 8)
    g.set_keyframes(np.arange(KMAX), np.arange(KMAX), rng.uniform(-2, 2, (KMAX, 3)).astype(f32))
    g.set_points(np.arange(P), bad, ref)
    for k in range(3):  # every point is seen by key frames 0, 1, 2: rows of three entries
        g.add_observations(np.arange(P), np.full(P, k, np.int32), np.zeros(P, np.uint16), rng.integers(0, 8, P).astype(np.uint8),
                           np.zeros(P, np.uint8))
    g.enable_keyframe_points(W)
    for k in range(KMAX):
        g.set_keyframe_points(k, rows[k])
    pos = rng.uniform(-5, 5, (P, 3)).astype(f32)
    mp = amd.MapPoints(P)
    mp.update(np.arange(P), pos, np.tile(f32([0, 0, 1]), (P, 1)), np.full(P, 0.1, f32), np.full(P, 100.0, f32), np.zeros((P, 32), np.uint8),
              np.zeros(P, np.uint8))
    return g, mp, rows, bad, ref, pos


def records(rng, K):
    q = rng.normal(size=(K, 4)) * 0.05 + [0, 0, 0, 1]
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    cor = np.concatenate([q, rng.uniform(-1, 1, (K, 3)), np.full((K, 1), 1.0)], axis=1)  # scale 1: repeated calls stay bounded
    non = np.concatenate([q, rng.uniform(-1, 1, (K, 3)), np.ones((K, 1))], axis=1)
    return np.ascontiguousarray(cor), np.ascontiguousarray(non)


def timed(f, reps):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def host_loop(exe, tmp, arrays):
    data, res = Path(tmp) / "arrays.bin", Path(tmp) / "result.bin"
    with open(data, "wb") as f:
        for a in arrays:
            f.write(np.ascontiguousarray(a).tobytes())
    ms = float(subprocess.run([str(exe), str(data), str(res)], check=True, capture_output=True, text=True).stdout)
    raw = np.fromfile(res, np.int32)
    n = int(raw[0])
    return ms, raw[1:1 + n], raw[1 + n:].view(f32).reshape(-1, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    L = _lib.load()
    if L.orbfe_device_count() < 1:
        sys.exit("loop_correct_latency: no GPU")
    rng = np.random.default_rng(1)
    g, mp, rows, bad, ref, pos = build(rng)
    everything = np.arange(P, dtype=np.int32)
    base_n, base_lo, base_hi = np.tile(f32([0, 0, 1]), (P, 1)), np.full(P, 0.1, f32), np.full(P, 100.0, f32)
    flags = np.zeros(P, np.uint8)
    lines = [f"loop correction: key frames x {W} entries over {P} point slots ({POOL} of them in the rows, 10 % NULL entries, 5 % bad points); "
             f"median of {a.reps} calls, ms, host to host around the C calls; four trips = positions + compiled host loop (-O2, one thread) "
             f"+ update + update_normal_depth_mappoints, each a median of its own"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = Path(tmp) / "loop_correct_host_bench"
        subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'orb_slam2_annotate_amd' / 'csrc'}", str(ROOT / "tools" / "loop_correct_host_bench.cpp"),
                        "-o", str(exe)], check=True)
        for K in (20, 80):
            kf = np.arange(K, dtype=np.int32)
            cor, non = records(rng, K)
            ow = rng.uniform(-2, 2, (K, 3)).astype(f32)
            slots, rf, valid, cnt = np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.uint8), np.zeros(1, np.int32)
            one = lambda: check(L.orbfe_correct_loop_mappoints(g._h, mp._h, K, ptr(kf), ptr(cor), ptr(non), ptr(ow), 0, None, ptr(SF), len(SF),  # noqa: E731
                                                               P, ptr(slots), ptr(rf), ptr(valid), ptr(cnt)))
            dev = timed(one, a.reps)
            n_dev = int(cnt[0])
            xw = np.zeros((P, 3), f32)
            t_pos = timed(lambda: check(L.orbfe_mappoints_positions(mp._h, P, ptr(everything), ptr(xw))), a.reps)
            cpu, claimed, out = host_loop(exe, tmp, [np.array([0, a.reps, K, W, P], np.int32), rows[:K].astype(np.int32), bad, cor, non, xw])
            assert len(claimed) == n_dev and np.array_equal(claimed, slots[:n_dev]), (len(claimed), n_dev)  # both sides did the same work
            sl = np.ascontiguousarray(claimed)
            args = [np.ascontiguousarray(x[sl]) for x in (out, base_n, base_lo, base_hi, flags)]
            t_upd = timed(lambda: check(L.orbfe_mappoints_update(mp._h, len(sl), ptr(sl), ptr(args[0]), ptr(args[1]), ptr(args[2]), ptr(args[3]),
                                                                 None, ptr(args[4]))), a.reps)
            v = np.zeros(len(sl), np.uint8)
            t_nd = timed(lambda: check(L.orbfe_obsgraph_update_normal_depth_mappoints(g._h, mp._h, len(sl), ptr(sl), ptr(SF), len(SF), ptr(v))), a.reps)
            lines.append(f"CorrectLoop, {K:2d} key frames x {W}: one call {dev:8.3f}   four trips {t_pos + cpu + t_upd + t_nd:8.3f} "
                         f"(positions {t_pos:.3f} + host loop {cpu:.4f} + update {t_upd:.3f} + normal/depth {t_nd:.3f})   claimed {n_dev}")
        in_gba = (rng.random(P) >= 0.05).astype(np.uint8)
        pos_gba = rng.uniform(-5, 5, (P, 3)).astype(f32)
        kf = np.arange(KMAX, dtype=np.int32)
        reached = np.ones(KMAX, np.uint8)
        T = np.tile(np.eye(4, dtype=f32).reshape(16), (KMAX, 1))
        Tb, Tn = T.copy(), T.copy()
        Tb[:, [3, 7, 11]] = rng.uniform(-1, 1, (KMAX, 3))
        Tn[:, [3, 7, 11]] = rng.uniform(-1, 1, (KMAX, 3))
        moved = np.zeros(P, np.uint8)
        dev = timed(lambda: check(L.orbfe_gba_update_mappoints(g._h, mp._h, P, ptr(everything), ptr(in_gba), ptr(pos_gba), KMAX, ptr(kf), ptr(reached),
                                                               ptr(Tb), ptr(Tn), ptr(moved))), a.reps)
        xw = np.zeros((P, 3), f32)
        t_pos = timed(lambda: check(L.orbfe_mappoints_positions(mp._h, P, ptr(everything), ptr(xw))), a.reps)
        cpu, cmoved, out = host_loop(exe, tmp, [np.array([1, a.reps, KMAX, 0, P], np.int32), bad, in_gba, xw, pos_gba, ref, reached, Tb, Tn])
        assert np.array_equal(cmoved.astype(np.uint8), moved)
        t_upd = timed(lambda: check(L.orbfe_mappoints_update(mp._h, P, ptr(everything), ptr(out), ptr(base_n), ptr(base_lo), ptr(base_hi), None,
                                                             ptr(flags))), a.reps)
        lines.append(f"GBA update, {P} points, 5 % not in the GBA: one call {dev:8.3f}   three trips {t_pos + cpu + t_upd:8.3f} "
                     f"(positions {t_pos:.3f} + host loop {cpu:.4f} + update {t_upd:.3f})   moved through a key frame {(moved == 2).sum()}")
    out_text = "\n".join(lines) + "\n"
    print(out_text, end="")
    if a.out:
        Path(a.out).write_text(out_text)


if __name__ == "__main__":
    main()
