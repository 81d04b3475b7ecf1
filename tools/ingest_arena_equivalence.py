#!/usr/bin/env python3
"""Byte-for-byte record of what the ingest calls and the vocabulary's transform / FeatureVector calls return, for comparing
two builds of the library ($ORBFE_LIB selects one; each build runs in a process of its own).

  record OUT.json   runs the GPU tests of tests/test_gpu_ingest.py, tests/test_vocabulary.py and tests/test_rectify_map_oracle.py
                    with every public function of ingest.py, Rectifier.__call__ / batch_device and ORBVocabulary.transform /
                    transform_features / transform_bow / featvec_batch_device wrapped: each call's result (or the code of its
                    OrbfeError) is reduced to dtype, shape and sha256 of the bytes of every array in it.  The two
                    device-pointer wrappers return nothing, so what they wrote is copied back from the device and recorded.
                    A call is keyed by test, function, the sha256 of its array arguments and how often that test made the
                    same call before -- not by its place in the test, which two threads of one test do not fix.
  compare A B       per function: calls, output arrays, and whether all of them are identical; exit status 1 on a difference
"""
import collections
import hashlib
import inspect
import json
import os
import sys
import threading
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
TESTS = ["test_gpu_ingest.py", "test_vocabulary.py", "test_rectify_map_oracle.py"]
# two threads on one handle: a build whose handle keeps the transform scratch mixes their descriptors up, so the test fails
# there by design and there is nothing to compare; the test itself holds each threaded result against the sequential one
NOT_COMPARED = "test_vocabulary.py::test_gpu_two_threads_transform_on_one_handle"


def digest(x, out):
    """Appends one (dtype, shape, sha256) per array found in x, walking containers in order; scalars by repr."""
    import numpy as np
    if isinstance(x, np.ndarray):
        out.append([str(x.dtype), list(x.shape), hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()])
    elif isinstance(x, dict):
        for k in sorted(x, key=repr):
            digest([k, x[k]], out)
    elif isinstance(x, (list, tuple)):
        for v in x:
            digest(v, out)
    elif isinstance(x, (bool, int, float, str, bytes, type(None), np.generic)):
        out.append(["scalar", [], repr(x)])
    elif hasattr(x, "node_ids") and hasattr(x, "offsets") and hasattr(x, "indices"):  # a FeatureVector
        digest([x.node_ids, x.offsets, x.indices], out)
    # anything else (a handle) is not an output


def record(path):
    sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
    import ctypes as C

    import numpy as np
    import pytest

    import orb_slam2_annotate_amd as amd
    from orb_slam2_annotate_amd import ingest
    calls, seen, lock = {}, collections.Counter(), threading.Lock()
    L = amd._lib.load()

    def from_device(address, dtype, count):
        out = np.zeros(count, dtype)
        assert L.hipMemcpy(amd._lib.ptr(out), C.c_void_p(address), C.c_size_t(out.nbytes), 2) == 0  # hipMemcpyDeviceToHost
        return out

    def no_addresses(x):
        if isinstance(x, (list, tuple)):
            return [no_addresses(v) for v in x]
        if isinstance(x, dict):
            return {k: no_addresses(v) for k, v in x.items()}
        return "address" if isinstance(x, int) and not isinstance(x, bool) and x >= 1 << 32 else x

    def written(name, self, a, k):
        """What a device-pointer wrapper wrote (it returns None)."""
        if name == "featvec_batch_device":
            (_, _, F, cap, d_nodes, d_off, d_idx, d_cnt) = a[:8]
            out = [from_device(d_nodes, np.uint32, F * cap), from_device(d_off, np.int32, F * (cap + 1)),
                   from_device(d_idx, np.uint32, F * cap), from_device(d_cnt, np.int32, F)]
            if k.get("d_word"):
                out += [from_device(k["d_word"], np.uint32, F * cap), from_device(k["d_weight"], np.float64, F * cap)]
            return out
        if name == "batch_device":  # up to the last pixel of the last frame
            (_, F, _, _, _, _, d_dst, dst_stride, dst_frame_stride) = a
            return from_device(d_dst, np.uint8, (F - 1) * dst_frame_stride + (self.height - 1) * dst_stride + self.width)
        return None

    def wrap(owner, name, label, holders):
        orig = getattr(owner, name)
        is_method = inspect.isclass(owner)

        def call(*a, **k):
            test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
            args = []  # (device addresses differ from run to run: not part of the key)
            digest(no_addresses([a[1:] if is_method else a, k]), args)
            akey = hashlib.sha256(json.dumps(args).encode()).hexdigest()[:16]
            with lock:
                seen[(test, label, akey)] += 1
                key = f"{test}|{label}|{akey}|{seen[(test, label, akey)]}"
            got = []
            try:
                r = orig(*a, **k)
            except amd.OrbfeError as e:
                digest([e.code], got)
                with lock:
                    calls[key] = got
                raise
            digest(r if r is not None else written(name, a[0] if is_method else None, a[1:] if is_method else a, k), got)
            with lock:
                calls[key] = got
            return r

        for h in holders:
            setattr(h, name, call)

    for name, v in list(vars(ingest).items()):
        if inspect.isfunction(v) and not name.startswith("_") and v.__module__ == ingest.__name__:
            wrap(ingest, name, name, [ingest] + ([amd] if getattr(amd, name, None) is v else []))
    for name in ("__call__", "batch_device"):
        wrap(ingest.Rectifier, name, f"Rectifier.{name}", [ingest.Rectifier])
    for name in ("transform_features", "transform", "transform_bow", "featvec_batch_device"):
        wrap(amd.ORBVocabulary, name, f"ORBVocabulary.{name}", [amd.ORBVocabulary])
    rc = pytest.main(["-q", "-m", "gpu", "-p", "no:cacheprovider", "--rootdir", str(ROOT), "--deselect", "tests/" + NOT_COMPARED]
                     + [str(ROOT / "tests" / t) for t in TESTS])
    Path(path).write_text(json.dumps({"lib": Path(os.environ.get("ORBFE_LIB", "in-tree")).name, "pytest": int(rc), "calls": calls}, indent=0))
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
        print(f"  {name:44s}{c:6d} calls {n:7d} outputs   {'identical' if not d else f'{d} calls differ'}")
    bad = sum(m[2] for m in per.values())
    print(f"\n{len(keys)} calls, {sum(m[1] for m in per.values())} outputs, {bad} calls differ")
    return 1 if bad or a["pytest"] or b["pytest"] else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "record":
        sys.exit(record(sys.argv[2]))
    if len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(__doc__)
