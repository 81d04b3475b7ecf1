"""The REFERENCE's own DBoW2 FeatureVector / BowVector (Thirdparty/DBoW2/DBoW2/{FeatureVector,BowVector}.cpp) as
recorded results: tests/golden/dbow2_ref.npz holds what the reference's two containers return for every input the
tests hand them, keyed by the input's bytes.  tools/gen_ref_golden.py records it by calling oracle/_ref/libdbow2_ref.so
(`make -C oracle ref REF=<reference tree>`: the two sources compiled in place, nothing copied).  Test infrastructure only."""
from __future__ import annotations

import ctypes as C
import hashlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
SO = ROOT / "oracle" / "_ref" / "libdbow2_ref.so"
GOLDEN = ROOT / "tests" / "golden" / "dbow2_ref.npz"
_lib = None
_golden = None
recording = None  # {name: array} while tools/gen_ref_golden.py records: calls go to the library and are kept here


def lib():
    global _lib
    if _lib is None:
        _lib = C.CDLL(str(SO))
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _recorded(kind, inputs, compute):
    """compute() through the library while recording, else the recorded result for these exact inputs."""
    global _golden
    h = hashlib.sha1(kind.encode())
    for a in inputs:
        h.update(repr((a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    key = f"{kind}_{h.hexdigest()[:24]}"
    if recording is not None:
        out = compute()
        for i, a in enumerate(out):
            recording[f"{key}_{i}"] = a
        return out
    if _golden is None:
        with np.load(GOLDEN) as z:
            _golden = dict(z)
    if f"{key}_0" not in _golden:
        raise KeyError(f"{GOLDEN.name} has no reference result for this input ({key}); regenerate it with tools/gen_ref_golden.py")
    n = sum(1 for k in _golden if k.startswith(key + "_"))
    return tuple(_golden[f"{key}_{i}"] for i in range(n))


def featvec(node_of_feature):
    """(node_ids, offsets, indices) of the reference's FeatureVector after addFeature(node[i], i), i = 0..n-1."""
    nof = np.ascontiguousarray(node_of_feature, dtype=np.uint32)

    def compute():
        n = len(nof)
        nodes = np.zeros(max(n, 1), np.uint32)
        offs = np.zeros(n + 1, np.int32)
        idx = np.zeros(max(n, 1), np.uint32)
        k = lib().ref_featvec_build(_p(nof), n, _p(nodes), _p(offs), _p(idx))
        return nodes[:k].copy(), offs[:k + 1].copy(), idx[:n].copy()

    return _recorded("featvec", [nof], compute)


def bowvec(word, weight, l1_normalize=True):
    word = np.ascontiguousarray(word, dtype=np.uint32)
    weight = np.ascontiguousarray(weight, dtype=np.float64)

    def compute():
        n = len(word)
        ids = np.zeros(max(n, 1), np.uint32)
        val = np.zeros(max(n, 1), np.float64)
        k = lib().ref_bowvec_build(_p(word), _p(weight), n, int(bool(l1_normalize)), _p(ids), _p(val))
        return ids[:k].copy(), val[:k].copy()

    return _recorded("bowvec", [word, weight, np.array([bool(l1_normalize)])], compute)
