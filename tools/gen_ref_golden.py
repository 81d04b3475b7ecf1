#!/usr/bin/env python3
"""Records the reference-derived fixtures of the tests from a reference source tree:

  tests/golden/dbow2_ref.npz              what the reference's DBoW2 FeatureVector / BowVector return for every input
                                          tests/test_dbow2_ref.py hands them (tests/ref_lib.py looks results up by input)
  tests/golden/orbextractor_ref.npz       what the reference's src/ORBextractor.cc (built untouched against the OpenCV
                                          double oracle/ref_cv/) returns for ref_lib.CASES and ref_lib.octree_sets():
                                          records and descriptors up to ~300 keypoints, else per-level counts and
                                          SHA-256 digests; digests of the pyramid levels and of every input; the tables
  tests/golden/orbmatcher_ref_methods.json the public methods of the reference's include/ORBmatcher.h, as
                                          tests/test_dropin_headers.py normalises them

    python tools/gen_ref_golden.py <reference tree>

The DBoW2 sources and the extractor are compiled in place into oracle/_ref/ (`make -C oracle ref`); nothing of the
tree is copied, and the recordings hold results only.  The GPU test's inputs are the oracle's (bit-identical to the device extractor and vocabulary)."""
import json
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import oracle_lib as orc  # noqa: E402
import ref_lib  # noqa: E402
import test_dbow2_ref as t  # noqa: E402
import test_dropin_headers  # noqa: E402
from orb_slam2_annotate_amd import synth  # noqa: E402
from orb_slam2_annotate_amd.vocabulary import write_synthetic_vocabulary  # noqa: E402


def gpu_test_inputs(tmp):
    """The featvec / bowvec calls of test_gpu_featvec_and_bow_equal_reference_container, on the oracle's outputs."""
    path = tmp / "voc6.txt"
    write_synthetic_vocabulary(path, k=10, L=3, seed=6)
    vo = orc.Vocabulary(path)
    o = orc.Oracle(700, 1.2, 8, 20, 7)
    for frame in synth.render_sequence(31, 3, 480, 360, step=2.0):
        _, desc = o.extract(frame)
        for levelsup in (0, 1):
            _, word, weight, node = vo.transform(desc, levelsup)
            ref_lib.featvec(node[weight > 0])
            ref_lib.bowvec(word, weight, True)
        ref_lib.featvec(vo.transform(desc, 1)[3])


def record_extractor():
    """The reference build on every case (ref_lib refuses a case outside the reference's domain) and candidate set."""
    rec = {}
    for name in ref_lib.CASE_NAMES:
        kps, desc, levels, _ = ref_lib.ref_extract(name)
        rec.update(ref_lib.case_record(name, kps, desc, levels, ref_lib.ref_tables(ref_lib.case(name)[5])))
    rec.update(ref_lib.octree_record([ref_lib.ref_octree(*s[1:]) for s in ref_lib.octree_sets()]))
    rec.update(ref_lib.octree_edges_record([ref_lib.ref_octree(*s[1:]) for s in ref_lib.octree_edge_sets_in_domain()]))
    if ref_lib.GOLDEN_X.is_file():  # a recording that is already there keeps every record it holds, byte for byte
        with np.load(ref_lib.GOLDEN_X) as z:
            for k in z.files:
                assert k in rec and rec[k].dtype == z[k].dtype and rec[k].shape == z[k].shape and \
                    rec[k].tobytes() == z[k].tobytes(), f"record {k} changed"
            print(len(z.files), "earlier records unchanged")
    np.savez_compressed(ref_lib.GOLDEN_X, **rec)
    print(ref_lib.GOLDEN_X, len(rec), "arrays", ref_lib.GOLDEN_X.stat().st_size, "bytes")


def main():
    ref = Path(sys.argv[1]).resolve()
    ref_lib.REF_TREE = ref
    subprocess.run(["make", "-C", str(ROOT / "oracle"), "ref", f"REF={ref}"], check=True)
    ref_lib.recording = {}
    with tempfile.TemporaryDirectory() as d:
        tmp = Path(d)
        t.test_featvec_csr_equals_reference_container()
        t.test_oracle_vocabulary_transform_grouping_equals_reference(tmp)
        t.test_bowvector_accumulation_order_equals_reference()
        gpu_test_inputs(tmp)
    np.savez_compressed(ref_lib.GOLDEN, **ref_lib.recording)
    print(ref_lib.GOLDEN, len(ref_lib.recording), "arrays")
    record_extractor()
    methods = sorted(test_dropin_headers._methods((ref / "include" / "ORBmatcher.h").read_text(errors="replace")))
    test_dropin_headers.REF_METHODS.write_text(json.dumps(methods, indent=1) + "\n")
    print(test_dropin_headers.REF_METHODS, len(methods), "methods")


if __name__ == "__main__":
    main()
