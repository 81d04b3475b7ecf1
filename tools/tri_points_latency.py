#!/usr/bin/env python3
"""Latency of orbfe_create_triangulated_points, host to host around the C call with its arrays prepared, next to the path a
CreateNewMapPoints caller had before it: orbfe_triangulate_matches_multi, the host loop compiled
(tools/tri_points_host_bench.cpp: the winner replay and the gathers; one CPU thread, -O2, no sanitizer) and then the seven
trips orbfe_mappoints_update -> orbfe_obsgraph_set_points -> _add_observations (key frame 1) -> _add_observations (the
neighbours) -> _assign_keyframe_points -> _distinctive_descriptors_mappoints -> _update_normal_depth_mappoints.
Scene: a monocular key frame of 2000 keypoints and K = 1 / 10 / 20 neighbours a few decimetres aside, each matching a quarter
of the keypoints.  Every repetition takes fresh point slots, as every new key frame does.  The two paths alternate, five
rounds each; the spread over the rounds is reported.  A record, not a gate.  Fails without a GPU.

The one call leaves the new points' graph rows marked in the mirror; they travel with the graph's next reading call.  The
seven trips end with such calls, so their figure contains that upload; "one call + read" adds a reading call
(orbfe_obsgraph_tracked_points of key frame 1) to the one call for the same footing.

  python tools/tri_points_latency.py [--out profiles/tri_points_latency.txt] [--reps 20] [--rounds 5]
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
import orb_slam2_annotate_amd as amd  # noqa: E402
from orb_slam2_annotate_amd import _lib  # noqa: E402
from orb_slam2_annotate_amd._lib import FrameViewC, KeyFrameCameraC, check, ptr  # noqa: E402

N, L = 2000, 8
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0
SF = (1.2 ** np.arange(L)).astype(np.float32)
SG = (SF * SF).astype(np.float32)
RATIO = np.float32(1.5) * np.float32(1.2)
f32 = np.float32


def scene(K, rng):
    """points 3-8 m in front of key frame 1 (identity pose); neighbour k stands 0.3 + 0.05 k m aside, alternating sides"""
    z = rng.uniform(3.0, 8.0, N)
    X = np.stack([rng.uniform(-0.55, 0.55, N) * z, rng.uniform(-0.4, 0.4, N) * z, z], axis=1)
    octave = rng.integers(0, L, N).astype(np.int32)
    frames, cams, centres = [], [], []
    for j in range(K + 1):
        ow = np.zeros(3) if j == 0 else np.array([(0.3 + 0.05 * j) * (1 if j % 2 else -1), 0.02 * j, 0.01 * j])
        Xc = X - ow
        x = (FX * Xc[:, 0] / Xc[:, 2] + CX + rng.normal(0, 0.2, N)).astype(f32)
        y = (FY * Xc[:, 1] / Xc[:, 2] + CY + rng.normal(0, 0.2, N)).astype(f32)
        desc = rng.integers(0, 256, (N, 32)).astype(np.uint8)
        view = amd.FrameView(x, y, octave, desc, (-400.0, 1040.0, -300.0, 780.0), angle=np.zeros(N, f32))
        T = np.concatenate([np.eye(3), -ow[:, None]], axis=1).astype(f32)
        frames.append((view, view.upload(), desc))
        cams.append(amd.KeyFrameCamera(T, ow.astype(f32), FX, FY, CX, CY))
        centres.append(ow.astype(f32))
    match12 = np.full((K, N), -1, np.int32)
    for k in range(K):
        sel = rng.random(N) < 0.25
        match12[k, sel] = np.flatnonzero(sel)
    return frames, cams, np.stack(centres), octave, match12


def median_ms(f, reps):
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    Lb = _lib.load()
    if Lb.orbfe_device_count() < 1:
        sys.exit("tri_points_latency: no GPU")
    lines = [f"orbfe_create_triangulated_points at n1 = {N} keypoints, each neighbour matching about a quarter of them; median of {a.reps} calls "
             f"per round, ms, host to host around the C calls; {a.rounds} rounds, the two paths alternating; trips = "
             "orbfe_triangulate_matches_multi + compiled host loop (-O2, one thread) + the C calls of the seven-trip path timed as one sequence"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = Path(tmp) / "tri_points_host_bench"
        subprocess.run(["g++", "-O2", "-std=c++17", str(ROOT / "tools" / "tri_points_host_bench.cpp"), "-o", str(exe)], check=True)
        for K in (1, 10, 20):
            rng = np.random.default_rng(K)
            frames, cams, centres, octave, match12 = scene(K, rng)
            res = [f[1] for f in frames]
            x3d, status, _, winner = amd.triangulate_matches_multi(res[0], cams[0], res[1:], cams[1:], match12, SF, SG, RATIO)
            keep = (status == 1) & (winner[None, :] == np.arange(K)[:, None])
            ck, ci1 = np.nonzero(keep)
            ck, ci1 = ck.astype(np.int32), ci1.astype(np.int32)
            ci2 = match12[ck, ci1].astype(np.int32)
            m = len(ck)
            data = Path(tmp) / "arrays.bin"
            with open(data, "wb") as f:
                for arr in (np.array([N, K, a.reps], np.int32), match12, status, winner.astype(np.int32), x3d, octave, frames[0][2]):
                    f.write(np.ascontiguousarray(arr).tobytes())
            cpu_s, made = subprocess.run([str(exe), str(data)], check=True, capture_output=True, text=True).stdout.split()
            cpu = float(cpu_s)
            assert int(made) == m
            calls = a.rounds * (a.reps + 1) * 3 + 4
            P = m * calls + 8
            mp, g = amd.MapPoints(P), amd.ObservationGraph(P, K + 1, 8)
            kf_slots = np.arange(K + 1, dtype=np.int32)
            g.set_keyframes(kf_slots, 100 + ((np.arange(K + 1) * 5) % (K + 1)), centres)  # mnIds on both sides of key frame 1's
            g.enable_keyframe_points(2048)
            g.enable_keyframe_descriptors(2048)
            for s in kf_slots:
                g.set_keyframe_points(int(s), np.full(N, -1, np.int32))
                g.set_keyframe_descriptors(int(s), res[s])
            nxt = [0]

            def fresh():
                s = np.arange(nxt[0], nxt[0] + m, dtype=np.int32)
                nxt[0] += m
                return s

            # the operands of both paths, prepared once
            hv = (C.c_void_p * K)(*[r._h.value for r in res[1:]])
            views = (C.POINTER(FrameViewC) * K)(*[C.pointer(r.c) for r in res[1:]])
            cc = (KeyFrameCameraC * K)()
            for k in range(K):
                cams[1 + k].fill(cc[k])
            c1 = cams[0].c
            m12 = np.ascontiguousarray(match12)
            nb_slots = np.ascontiguousarray(kf_slots[1:])
            ok, oi1, oi2, oslot = (np.zeros(max(m, 1), np.int32) for _ in range(4))
            ostatus, per, nc = np.zeros((K, N), np.uint8), np.zeros(K, np.int32), C.c_int32(0)
            tx, ts, tn, tw = np.zeros((K, N, 3), f32), np.zeros((K, N), np.uint8), np.zeros(K, np.int32), np.zeros(N, np.int32)
            pos = np.ascontiguousarray(x3d[ck, ci1])
            zero3, zero1, d1 = np.zeros((m, 3), f32), np.zeros(m, f32), np.ascontiguousarray(frames[0][2][ci1])
            flags, zero8, valid = np.full(m, 2, np.uint8), np.zeros(m, np.uint8), np.zeros(m, np.uint8)
            kf1s, kf2s = np.zeros(m, np.int32), np.ascontiguousarray(nb_slots[ck])
            i1_16, i2_16, oct8 = ci1.astype(np.uint16), ci2.astype(np.uint16), octave[ci1].astype(np.uint8)
            oct2 = octave[ci2].astype(np.uint8)  # (every frame of the scene shares the octaves)
            both_kf, both_idx = np.concatenate([kf1s, kf2s]), np.concatenate([i1_16, i2_16])
            bkf, bidx = np.zeros(m, np.int32), np.zeros(m, np.int32)
            kf1, cnt = np.array([0], np.int32), np.zeros(1, np.int32)

            def one():
                s = fresh()
                check(Lb.orbfe_create_triangulated_points(mp._h, g._h, res[0]._h, 0, C.byref(c1), K, hv, ptr(nb_slots), cc, ptr(m12), ptr(SF),
                                                          ptr(SG), L, float(RATIO), ptr(s), m, ptr(ok), ptr(oi1), ptr(oi2), ptr(oslot),
                                                          ptr(ostatus), ptr(per), C.byref(nc)))

            def one_and_read():
                one()
                check(Lb.orbfe_obsgraph_tracked_points(g._h, 1, ptr(kf1), 0, ptr(cnt)))

            def trips():
                s = fresh()
                check(Lb.orbfe_triangulate_matches_multi(0, C.byref(res[0].c), C.byref(c1), K, views, cc, ptr(m12), ptr(SF), ptr(SG), L, float(RATIO),
                                                         ptr(tx), ptr(ts), ptr(tn), ptr(tw)))
                check(Lb.orbfe_mappoints_update(mp._h, m, ptr(s), ptr(pos), ptr(zero3), ptr(zero1), ptr(zero1), ptr(d1), ptr(flags)))
                check(Lb.orbfe_obsgraph_set_points(g._h, m, ptr(s), ptr(zero8), ptr(kf1s)))
                check(Lb.orbfe_obsgraph_add_observations(g._h, m, ptr(s), ptr(kf1s), ptr(i1_16), ptr(oct8), ptr(zero8)))
                check(Lb.orbfe_obsgraph_add_observations(g._h, m, ptr(s), ptr(kf2s), ptr(i2_16), ptr(oct2), ptr(zero8)))
                s2 = np.concatenate([s, s])
                check(Lb.orbfe_obsgraph_assign_keyframe_points(g._h, 2 * m, ptr(both_kf), ptr(both_idx), ptr(s2)))
                check(Lb.orbfe_obsgraph_distinctive_descriptors_mappoints(g._h, mp._h, m, ptr(s), ptr(bkf), ptr(bidx), ptr(valid)))
                check(Lb.orbfe_obsgraph_update_normal_depth_mappoints(g._h, mp._h, m, ptr(s), ptr(SF), L, ptr(valid)))

            one()
            assert nc.value == m and np.array_equal(ok[:m], ck) and np.array_equal(oi1[:m], ci1), (nc.value, m)  # both sides do the same work
            t1, t2, t7 = [], [], []
            for _ in range(a.rounds):
                t1.append(median_ms(one, a.reps))
                t2.append(median_ms(one_and_read, a.reps))
                t7.append(cpu + median_ms(trips, a.reps))

            def show(t):
                return f"{np.median(t):7.3f} (rounds {min(t):.3f} .. {max(t):.3f})"

            lines.append(f"K = {K:2d}, {int((match12 >= 0).sum())} pairs, {m} points created: one call {show(t1)}   one call + read {show(t2)}   "
                         f"trips {show(t7)}, of which host loop {cpu:.4f}")
            mp.close()
            g.close()
            for _, r, _ in frames:
                r.close()
    out_text = "\n".join(lines) + "\n"
    print(out_text, end="")
    if a.out:
        Path(a.out).write_text(out_text)


if __name__ == "__main__":
    main()
