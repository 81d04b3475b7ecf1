"""The descriptor methods of orbfe_cpp::ObservationGraph and orbfe_cpp::MapPointTable (include/orbfe_classes.hpp) compiled
with g++ against liborbfe.so (tests/cpp/test_obsdesc.cpp) on a world made by a formula both sides repeat: the classes equal
the Python binding and the restatement (tests/distinctive_ref.py); refused operands throw."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import distinctive_ref as dr
import orb_slam2_annotate_amd as amd

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K, P, W = 24, 60, 64


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("obsdesccpp") / "test_obsdesc"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_obsdesc.cpp"), "-o", str(exe),
                    f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return dict(t.split("=") for t in text.split())


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


def world():
    """-> (graph, what the restatement reads, the slot list)"""
    g = amd.ObservationGraph(P, K, 128)
    g.enable_keyframe_descriptors(W)
    kf_id = [500 - 7 * k for k in range(K)]
    g.set_keyframes(list(range(K)), kf_id, np.zeros((K, 3), np.float32))
    kf_desc = []
    for k in range(K):
        d = np.array([[((i + k) % 3) * 85 + int(b == (i * 7 + k) % 32) for b in range(32)] for i in range(10 + k)], np.uint8)
        kf_desc.append(d)
        g.set_keyframe_descriptors(k, d)
    pts = list(range(P - 10))
    point_bad = [p % 11 == 4 for p in pts] + [True] * 10
    g.set_points(pts, [int(b) for b in point_bad[:P - 10]], [-1] * len(pts))
    obs = [[] for _ in range(P)]
    for p in pts:
        if p == 7:
            continue
        obs[p] = [((p + 5 * j) % K, (p + j) % 10) for j in range(1 + p % 9)]
        g.add_observations([p] * len(obs[p]), [k for k, _ in obs[p]], [i for _, i in obs[p]], [0] * len(obs[p]), [0] * len(obs[p]))
    kf_bad = [k in (3, 12) for k in range(K)]
    g.set_keyframes([3, 12], [kf_id[3], kf_id[12]], np.zeros((2, 3), np.float32), [1, 1])
    slots = [(p * 7) % P for p in range(P)]
    want = [dr.distinctive(point_bad[s], obs[s], kf_id, kf_bad, kf_desc) for s in slots]
    return g, kf_desc, slots, want


def test_cpp_descriptor_methods_equal_the_binding_and_the_restatement(out):
    g, kf_desc, slots, want = world()
    assert ints(out["kf5_desc"]) == kf_desc[5].reshape(-1).tolist() == g.get_keyframe_descriptors(5).reshape(-1).tolist()
    valid = [int(r is not None) for r in want]
    kf = [-1 if r is None else r[0] for r in want]
    idx = [-1 if r is None else r[1] for r in want]
    desc = [b for r in want for b in (bytes(32) if r is None else r[2])]
    assert 0 < sum(valid) < len(valid) and len(set(kf)) > 5
    b_kf, b_idx, b_desc, b_valid = g.distinctive_descriptors(slots)
    assert ints(out["valid"]) == valid == b_valid.tolist()
    assert ints(out["kf"]) == kf == b_kf.tolist() and ints(out["idx"]) == idx == b_idx.tolist()
    assert ints(out["desc"]) == desc == b_desc.reshape(-1).tolist()
    # the table form: the winners in valid slots, the slot's own bytes elsewhere
    assert ints(out["table_valid"]) == valid and ints(out["table_kf"]) == kf and ints(out["table_idx"]) == idx
    table = np.array([[200 + p % 50] * 32 for p in range(P)], np.uint8)
    for s, r in zip(slots, want):
        if r is not None:
            table[s] = np.frombuffer(r[2], np.uint8)
    assert ints(out["table_desc"]) == table.reshape(-1).tolist()
    assert int(out["positions_kept"]) == 1
    assert ints(out["table_valid_no_winners"]) == [valid[slots.index(s)] for s in (0, 1, 2)]
    assert int(out["threw"]) == 5
    g.close()
