#!/usr/bin/env python3
"""Latency of orbfe_kfdb_query (the scored set of KeyFrameDatabase::DetectRelocalizationCandidates,
src/KeyFrameDatabase.cc:228-291): one query and a 64-query batch against 1 000 and 5 000 stored key frames.  The
BowVectors are those of synth frames (640x480, 1200 features) on the k = 10, L = 6 synthetic vocabulary; the queries are
views between stored ones.  Each row gives ms per query (host clock around the call, which ends in a stream
synchronise; median of --reps calls after a warm-up) and, beside it, the bytes-touched bound: the stored word ids
(4 bytes each -- what the counting kernel must read once per call) over the HBM rate measured here with a large
device-to-device copy.  No threshold: this tool reports.

  python tools/kfdb_latency.py [--out profiles/kfdb_latency.txt] [--commit ID]"""
import argparse
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import orb_slam2_annotate_amd as amd  # noqa: E402
from orb_slam2_annotate_amd import synth  # noqa: E402
from orb_slam2_annotate_amd.vocabulary import synthetic_vocabulary_arrays  # noqa: E402

W, H, NFEAT = 640, 480, 1200
PER_SCENE = 250  # frames per scene, 4 pixels apart; every fifth one is a query, the others are key frames


def med(fn, reps):
    fn()
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(t))


def hbm_rate():
    """bytes / s of a 1 GiB device-to-device copy (read + write counted), best of 10, by device events"""
    n = 1 << 30
    a = torch.empty(n, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    a.zero_()
    b.copy_(a)
    best = None
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        best = ms if best is None or ms < best else best
    del a, b
    return 2 * n / (best * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default="unknown")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 5000])
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    voc = amd.ORBVocabulary()
    assert voc.createFromArrays(synthetic_vocabulary_arrays(10, 6, 1))
    e = amd.ORBextractor(NFEAT, 1.2, 8, 20, 7)
    need = max(a.sizes) + 64
    stored, queries = [], []
    scene = 0
    while len(stored) < need or len(queries) < 64:
        frames = synth.render_sequence(500 + scene, PER_SCENE, W, H, step=4.0)
        for i in range(0, PER_SCENE, 50):
            for j, (_, d) in enumerate(e.extract_batch(np.stack(frames[i:i + 50]))):
                (queries if (i + j) % 5 == 2 else stored).append(voc.transform_bow(d, 4))
        scene += 1
    queries = queries[:64]
    rate = hbm_rate()
    say(f"# orbfe_kfdb_query, commit {a.commit}; {torch.cuda.get_device_name(0)}")
    say(f"# key frames: synth {W}x{H}, nFeatures={NFEAT}, {scene} scenes x {PER_SCENE} frames, k=10 L=6 vocabulary; "
        f"mean {np.mean([len(b[0]) for b in stored]):.0f} words per BowVector")
    say(f"# HBM rate (1 GiB device-to-device copy, read + write): {rate / 1e9:.0f} GB/s; median of {a.reps} calls")
    say("# stored  Q  ms/call  ms/query  survivors/query  stored_word_bytes  bound_ms(bytes/rate)")
    for n in a.sizes:
        db = amd.KeyFrameDatabase(voc)
        t0 = time.perf_counter()
        for k in range(n):
            db.add(k, stored[k])
        add_us = 1e6 * (time.perf_counter() - t0) / n
        word_bytes = 4 * sum(len(stored[k][0]) for k in range(n))
        for Q in (1, 64):
            packed = db.pack_queries(queries[:Q])  # the operands as arrays: the call is timed, not their packing
            res = db.query_packed(packed)
            surv = np.mean([len(r[0]) for r in res])
            cap = max(max(len(r[0]) for r in res), 1)
            ms = med(lambda: db.query_packed(packed, cap), a.reps)
            say(f"{n:7d} {Q:3d} {ms:8.3f} {ms / Q:9.4f} {surv:12.1f} {word_bytes:16d} {1e3 * word_bytes / rate:12.5f}")
        say(f"# {n} key frames: orbfe_kfdb_add {add_us:.1f} us per key frame")
        del db
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
