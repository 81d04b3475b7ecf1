#!/usr/bin/env python3
"""Latency of orbfe_create_stereo_points, host to host around the C call with its arrays prepared, next to the path a stereo
caller had before it: the host loop compiled (tools/stereo_points_host_bench.cpp: csrc/stereopoints_host.h over flat arrays
-- depth sort, walk, UnprojectStereo, normal and range, descriptor gather; one CPU thread, -O2, no sanitizer) and then the
trips orbfe_mappoints_update -> orbfe_obsgraph_set_points -> _add_observations -> _assign_keyframe_points ->
_update_normal_depth_mappoints (mode KEYFRAME), or orbfe_mappoints_update alone (mode TEMPORAL, which names no graph).
Frame: 2000 keypoints, about 56 % with a depth, half of those occupied, th_depth above every depth (the whole list is
walked).  In mode KEYFRAME every repetition takes fresh point slots, as every new key frame does; in mode TEMPORAL both
paths write the same slots again each time, as a caller recycles its temporal slots.  The two paths alternate, five rounds
each; the spread over the rounds is reported.  A record, not a gate.  Fails without a GPU.

The one call leaves the new points' graph rows marked in the mirror; they travel with the graph's next reading call.  The
five trips end with such a call (update_normal_depth_mappoints), so their figure contains that upload; "one call + read"
adds a reading call (orbfe_obsgraph_tracked_points of the key frame) to the one call for the same footing.

  python tools/stereo_points_latency.py [--out profiles/stereo_points_latency.txt] [--reps 20] [--rounds 5]
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
from orb_slam2_annotate_amd._lib import check, ptr  # noqa: E402

N, L, KF, TH = 2000, 8, 1, 100.0
KEYFRAME, TEMPORAL = 1, 2
SF = (1.2 ** np.arange(L)).astype(np.float32)
f32 = np.float32


def frame(rng):
    x = rng.uniform(5, 1236, N).astype(f32)
    y = rng.uniform(5, 371, N).astype(f32)
    octave = rng.integers(0, L, N).astype(np.int32)
    desc = rng.integers(0, 256, (N, 32)).astype(np.uint8)
    depth = rng.uniform(0.5, 60.0, N).astype(f32)
    depth[rng.random(N) >= 0.56] = -1.0
    occupied = ((depth > 0) & (rng.random(N) < 0.5)).astype(np.uint8)
    u_right = np.where(depth > 0, x - f32(386.0) / np.where(depth > 0, depth, 1), -1).astype(f32)
    return x, y, octave, desc, depth, occupied, u_right


def host_loop(exe, tmp, arrays):
    data, res = Path(tmp) / "arrays.bin", Path(tmp) / "result.bin"
    with open(data, "wb") as f:
        for a in arrays:
            f.write(a if isinstance(a, bytes) else np.ascontiguousarray(a).tobytes())
    ms = float(subprocess.run([str(exe), str(data), str(res)], check=True, capture_output=True, text=True).stdout)
    raw = np.fromfile(res, np.uint8)
    m = int(raw[:4].view(np.int32)[0])
    at = [4]

    def cut(count, dtype):
        nbytes = count * np.dtype(dtype).itemsize
        out = raw[at[0]:at[0] + nbytes].view(dtype).copy()
        at[0] += nbytes
        return out

    return ms, cut(m, np.int32), cut(3 * m, f32).reshape(m, 3), cut(3 * m, f32).reshape(m, 3), cut(m, f32), cut(m, f32), cut(32 * m, np.uint8)


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
        sys.exit("stereo_points_latency: no GPU")
    rng = np.random.default_rng(1)
    x, y, octave, desc, depth, occupied, u_right = frame(rng)
    stale = np.zeros(N, np.uint8)
    R = np.eye(3, dtype=f32)
    pose = amd.camera_pose(R, f32([0.3, -0.2, 0.5]), (718.856, 718.856, 607.19, 185.22), 386.0, (0, 1241, 0, 376), 1.2, L)
    centre = np.array(list(pose.Ow), f32)
    view = amd.FrameView(x, y, octave, desc, (0.0, 1241.0, 0.0, 376.0), angle=np.zeros(N, f32), u_right=u_right)
    F = view.upload()
    lines = [f"orbfe_create_stereo_points at n = {N} keypoints, {int((depth > 0).sum())} with a depth, {int(occupied.sum())} of them occupied; "
             f"median of {a.reps} calls per round, ms, host to host around the C calls; {a.rounds} rounds, the two paths alternating; "
             "trips = compiled host loop (-O2, one thread) + the C calls of the five-trip path timed as one sequence"]
    with tempfile.TemporaryDirectory() as tmp:
        exe = Path(tmp) / "stereo_points_host_bench"
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", f"-I{ROOT / 'orb_slam2_annotate_amd' / 'csrc'}",
                        str(ROOT / "tools" / "stereo_points_host_bench.cpp"), "-o", str(exe)], check=True)
        for mode, name in ((KEYFRAME, "KEYFRAME"), (TEMPORAL, "TEMPORAL")):
            head = np.array([N, a.reps, mode, L], np.int32)
            rest = np.concatenate([f32([TH]), centre, SF]).astype(f32)
            cpu, idx, pos, normal, lo, hi, ndesc = host_loop(exe, tmp, [head, x, y, depth, octave, occupied, stale, desc, bytes(pose), rest])
            m = len(idx)
            calls = a.rounds * (a.reps + 1) * 3 + 4
            P = N + m * calls
            mp = amd.MapPoints(P)
            g = None
            if mode == KEYFRAME:
                g = amd.ObservationGraph(P, 4, 8)
                g.set_keyframes([0, KF], [3, 9], np.array([[9, 9, 9], centre], f32))
                g.enable_keyframe_points(2048)
                held = np.flatnonzero(occupied).astype(np.int32)
                g.set_points(held, np.zeros(len(held), np.uint8), np.zeros(len(held), np.int32))
                g.add_observations(held, np.zeros(len(held), np.int32), held, np.zeros(len(held), np.uint8), np.ones(len(held), np.uint8))
                row = np.full(N, -1, np.int32)
                row[held] = held
                g.set_keyframe_points(KF, row)
            gh = g._h if g is not None else None
            nxt = [N]

            def fresh():  # KEYFRAME: the next m free slots; TEMPORAL: the same m slots again (nothing makes them live)
                s = np.arange(nxt[0], nxt[0] + m, dtype=np.int32)
                if mode == KEYFRAME:
                    nxt[0] += m
                return s

            cidx, cslot, cleared = np.zeros(m, np.int32), np.zeros(m, np.int32), np.zeros(N, np.uint8)
            nc, nw = C.c_int32(0), C.c_int32(0)
            kfs, idx16 = np.full(m, KF, np.int32), idx.astype(np.uint16)
            oct8, st8 = octave[idx].astype(np.uint8), (u_right[idx] >= 0).astype(np.uint8)
            zero8, flags, valid = np.zeros(m, np.uint8), np.full(m, 0 if mode == TEMPORAL else 2, np.uint8), np.zeros(m, np.uint8)
            kf1, cnt = np.array([KF], np.int32), np.zeros(1, np.int32)

            def one():
                s = fresh()
                check(Lb.orbfe_create_stereo_points(mp._h, gh, F._h, KF, C.byref(pose), N, ptr(depth), ptr(occupied), None, TH, mode, ptr(SF), L,
                                                    ptr(s), m, ptr(cidx), ptr(cslot), ptr(cleared), C.byref(nc), C.byref(nw)))

            def one_and_read():
                one()
                check(Lb.orbfe_obsgraph_tracked_points(gh, 1, ptr(kf1), 0, ptr(cnt)))

            def trips():
                s = fresh()
                check(Lb.orbfe_mappoints_update(mp._h, m, ptr(s), ptr(pos), ptr(normal), ptr(lo), ptr(hi), ptr(ndesc), ptr(flags)))
                if mode == TEMPORAL:
                    return
                check(Lb.orbfe_obsgraph_set_points(gh, m, ptr(s), ptr(zero8), ptr(kfs)))
                check(Lb.orbfe_obsgraph_add_observations(gh, m, ptr(s), ptr(kfs), ptr(idx16), ptr(oct8), ptr(st8)))
                check(Lb.orbfe_obsgraph_assign_keyframe_points(gh, m, ptr(kfs), ptr(idx16), ptr(s)))
                check(Lb.orbfe_obsgraph_update_normal_depth_mappoints(gh, mp._h, m, ptr(s), ptr(SF), L, ptr(valid)))

            one()
            assert nc.value == m and np.array_equal(cidx, idx), (nc.value, m)  # both sides did the same work
            t1, t2, t5 = [], [], []
            for _ in range(a.rounds):
                t1.append(median_ms(one, a.reps))
                if mode == KEYFRAME:
                    t2.append(median_ms(one_and_read, a.reps))
                t5.append(cpu + median_ms(trips, a.reps))

            def show(t):
                return f"{np.median(t):7.3f} (rounds {min(t):.3f} .. {max(t):.3f})"

            line = f"{name}, {m} points created: one call {show(t1)}"
            if mode == KEYFRAME:
                line += f"   one call + read {show(t2)}"
            line += f"   trips {show(t5)}, of which host loop {cpu:.4f}"
            lines.append(line)
            mp.close()
            if g is not None:
                g.close()
    F.close()
    out_text = "\n".join(lines) + "\n"
    print(out_text, end="")
    if a.out:
        Path(a.out).write_text(out_text)


if __name__ == "__main__":
    main()
