#!/usr/bin/env python3
"""Latency of the observation-graph calls (orbfe_obsgraph) next to the same loops on one CPU thread over the same arrays:
numpy loops over the CSR of the rows, the project's usual yardstick.  Graph: 500 key frames, mean row 6 with a tail to 60.

  python tools/obsgraph_latency.py [--out profiles/obsgraph_latency.txt] [--reps 30]
"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import orb_slam2_annotate_amd as amd  # noqa: E402

N_KF, N_PTS, RW, N_LEVELS = 500, 20000, 64, 8


def build(rng):
    n_obs = np.minimum(60, np.maximum(2, rng.geometric(1.0 / 5.0, N_PTS) + 1))  # mean about 6, a tail to 60
    rows = [np.sort(rng.choice(N_KF, size=int(n), replace=False)).astype(np.int32) for n in n_obs]
    octs = [rng.integers(0, N_LEVELS, len(r)).astype(np.uint8) for r in rows]
    Ow = rng.uniform(-5, 5, (N_KF, 3)).astype(np.float32)
    pos = rng.uniform(-20, 20, (N_PTS, 3)).astype(np.float32)
    g = amd.ObservationGraph(N_PTS, N_KF, RW)
    g.set_keyframes(np.arange(N_KF), np.arange(N_KF), Ow)
    g.set_points(np.arange(N_PTS), np.zeros(N_PTS, np.uint8), [r[0] for r in rows])
    slot = np.concatenate([np.full(len(r), p, np.int32) for p, r in enumerate(rows)])
    kf = np.concatenate(rows)
    g.add_observations(slot, kf, np.zeros(len(kf), np.uint16), np.concatenate(octs), np.zeros(len(kf), np.uint8))
    return g, rows, octs, Ow, pos


def cpu_votes(rows, q, me):
    c = np.zeros(N_KF, np.int32)
    for p in q:
        for k in rows[p]:
            if k != me:
                c[k] += 1
    return c


def cpu_culling(rows, octs, kf, slots, levels):
    n_mps = n_red = 0
    for p, lv in zip(slots, levels):
        n_mps += 1
        r, o = rows[p], octs[p]
        if len(r) > 3:
            n = 0
            for k, oi in zip(r, o):
                if k != kf and oi <= lv + 1:
                    n += 1
                    if n >= 3:
                        break
            n_red += n >= 3
    return n_mps, n_red


def cpu_normals(rows, octs, Ow, pos, slots, sf):
    out = np.zeros((len(slots), 5), np.float32)
    for i, p in enumerate(slots):
        d = pos[p] - Ow[rows[p]]
        nrm = np.sqrt((d.astype(np.float64) ** 2).sum(1))
        out[i, :3] = (d * (1.0 / nrm).astype(np.float32)[:, None]).sum(0) / np.float32(len(d))
        out[i, 4] = np.float32(nrm[0]) * sf[octs[p][0]]
        out[i, 3] = out[i, 4] / sf[-1]
    return out


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
    rng = np.random.default_rng(1)
    g, rows, octs, Ow, pos = build(rng)
    sf = (np.float32(1.2) ** np.arange(N_LEVELS)).astype(np.float32)
    lines = [f"observation graph: {N_KF} key frames, {N_PTS} points, row_width {RW}, mean row {np.mean([len(r) for r in rows]):.2f}, "
             f"longest {max(len(r) for r in rows)}; median of {a.reps} calls, ms; CPU = the same loop in one Python thread over numpy arrays"]

    def row(name, dev, cpu):
        lines.append(f"{name:<58s} device {timed(dev, a.reps):8.3f}   cpu {timed(cpu, max(3, a.reps // 10)):9.3f}")

    q1000 = rng.integers(0, N_PTS, 1000).tolist()
    row("UpdateConnections votes, 1 key frame x 1000 points", lambda: g.votes([q1000], [3]), lambda: cpu_votes(rows, q1000, 3))
    q20 = [rng.integers(0, N_PTS, 1000).tolist() for _ in range(20)]
    row("UpdateConnections votes, 20 key frames x 1000 points", lambda: g.votes(q20, list(range(20))),
        lambda: [cpu_votes(rows, q, i) for i, q in enumerate(q20)])
    q300 = rng.integers(0, N_PTS, 300).tolist()
    row("UpdateLocalKeyFrames votes, 300 matches", lambda: g.votes([q300]), lambda: cpu_votes(rows, q300, -1))
    feats = [(rng.integers(0, N_PTS, 500).astype(np.int32), rng.integers(0, N_LEVELS, 500).astype(np.uint8)) for _ in range(30)]
    row("KeyFrameCulling counts, 30 candidates x 500 points", lambda: g.culling_counts(np.arange(30), feats),
        lambda: [cpu_culling(rows, octs, c, f[0], f[1]) for c, f in enumerate(feats)])
    s4000 = rng.choice(N_PTS, 4000, replace=False).astype(np.int32)
    row("UpdateNormalAndDepth, 4000 points, array form", lambda: g.update_normal_depth(s4000, sf, pos[s4000]),
        lambda: cpu_normals(rows, octs, Ow, pos, s4000, sf))
    mp = amd.MapPoints(N_PTS)
    z = np.zeros(N_PTS, np.float32)
    mp.update(np.arange(N_PTS), pos, np.zeros((N_PTS, 3), np.float32), z, z, np.zeros((N_PTS, 32), np.uint8), np.zeros(N_PTS, np.uint8))

    def round_trip():  # what the table form saves: positions down, the loop, the three fields up again
        p = mp.positions(s4000)
        g.update_normal_depth(s4000, sf, p)

    row("UpdateNormalAndDepth, 4000 points, table form", lambda: g.update_normal_depth(s4000, sf, mp=mp), round_trip)
    lines.append("(last row: 'cpu' is the array form with the positions read back from the table first, the round trip the table form saves)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        Path(a.out).write_text(text)


if __name__ == "__main__":
    main()
