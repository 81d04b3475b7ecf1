#!/usr/bin/env python3
"""Byte-for-byte record of what the observation graph, the loop correction and the key-frame database return, for comparing
two builds of the library ($ORBFE_LIB selects one; each build runs in a process of its own).

  record OUT.json   runs the GPU tests of the graph, its key-frame rows and descriptors, the loop correction and the database
                    with every public method of ObservationGraph, MapPoints and KeyFrameDatabase wrapped: each call's
                    result (or the code, counts and partial results of its OrbfeError) is reduced to dtype, shape and
                    sha256 of the bytes of every array in it, keyed by test, method and the call's place in the test
  compare A B       per method: calls, output arrays, and whether all of them are identical; exit status 1 on a difference

The worlds are the ones the tests construct, so every entry point runs on them, the table forms included (what a call
left in a map-point table is read back by the tests through MapPoints.positions / ProjectInFrustum, which are recorded too).
"""
import collections
import hashlib
import inspect
import json
import os
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
TESTS = ["test_gpu_obsgraph.py", "test_gpu_kfpoints.py", "test_gpu_obsdesc.py", "test_gpu_loop_correct.py", "test_gpu_kfdb.py"]


def digest(x, out):
    """Appends one (dtype, shape, sha256) per array found in x, walking containers in order; scalars by repr."""
    import numpy as np
    if isinstance(x, np.ndarray):
        out.append([str(x.dtype), list(x.shape), hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()])
    elif isinstance(x, dict):
        for k in sorted(x, key=repr):
            digest(x[k], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            digest(v, out)
    elif isinstance(x, (bool, int, float, str, bytes, type(None), np.generic)):
        out.append(["scalar", [], repr(x)])
    # anything else (a handle, a frame) is not an output


def record(path):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import pytest

    import orb_slam2_annotate_amd as amd
    calls, seen = {}, collections.Counter()

    def wrap(cls, name):
        orig = getattr(cls, name)

        def method(self, *a, **k):
            test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
            seen[(test, name)] += 1
            key = f"{test}|{cls.__name__}.{name}|{seen[(test, name)]}"
            got = []
            try:
                r = orig(self, *a, **k)
            except amd.OrbfeError as e:
                digest([e.code, getattr(e, "count", None), getattr(e, "partial", None)], got)
                calls[key] = got
                raise
            digest(r, got)
            calls[key] = got
            return r

        setattr(cls, name, method)

    for cls in (amd.ObservationGraph, amd.MapPoints, amd.KeyFrameDatabase):
        for name, v in list(vars(cls).items()):
            if inspect.isfunction(v) and not name.startswith("_") and name != "close":
                wrap(cls, name)
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider"] + [str(ROOT / "tests" / t) for t in TESTS])
    Path(path).write_text(json.dumps({"lib": os.environ.get("ORBFE_LIB", "in-tree"), "pytest": int(rc), "calls": calls}, indent=0))
    return int(rc)


def compare(a_path, b_path):
    a, b = json.loads(Path(a_path).read_text()), json.loads(Path(b_path).read_text())
    print(f"A: {a['lib']} (pytest exit {a['pytest']})\nB: {b['lib']} (pytest exit {b['pytest']})\n")
    per = collections.defaultdict(lambda: [0, 0, 0])  # calls, arrays, differing calls
    keys = sorted(set(a["calls"]) | set(b["calls"]))
    for k in keys:
        m = per[k.split("|")[1]]
        m[0] += 1
        m[1] += len(a["calls"].get(k, []))
        if a["calls"].get(k) != b["calls"].get(k):
            m[2] += 1
            print("DIFFERENT", k)
    for name in sorted(per):
        c, n, d = per[name]
        print(f"  {name:58s}{c:6d} calls {n:7d} outputs   {'identical' if not d else f'{d} calls differ'}")
    bad = sum(m[2] for m in per.values())
    print(f"\n{len(keys)} calls, {sum(m[1] for m in per.values())} outputs, {bad} calls differ")
    return 1 if bad or a["pytest"] or b["pytest"] else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        sys.exit(record(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
