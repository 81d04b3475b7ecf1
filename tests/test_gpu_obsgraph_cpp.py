"""orbfe_cpp::ObservationGraph and MapPointTable::UpdateNormalAndDepth (include/orbfe_classes.hpp) compiled with g++ against
liborbfe.so (tests/cpp/test_obsgraph.cpp) on a world made by a formula both sides repeat: the class equals the Python
binding and the restatement (tests/obsgraph_ref.py), floats bit for bit; the table form equals the array form written by
hand; refused operands throw."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import obsgraph_ref as orf
import orb_slam2_annotate_amd as amd

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
K, P = 6, 40


@pytest.fixture(scope="module")
def out(tmp_path_factory):
    exe = tmp_path_factory.mktemp("obsgraphcpp") / "test_obsgraph"
    lib = ROOT / "orb_slam2_annotate_amd"
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", f"-I{ROOT / 'include'}", str(ROOT / "tests/cpp/test_obsgraph.cpp"), "-o", str(exe),
                    f"-L{lib}", "-lorbfe", f"-Wl,-rpath,{lib}"], check=True)
    text = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    return dict(t.split("=") for t in text.split())


def ints(s):
    return [int(x) for x in s.split(",")] if s else []


def floats(s):
    return np.array([int(x, 16) for x in s.split(",")], np.uint32).view(np.float32) if s else np.zeros(0, np.float32)


def world():
    w = orf.World()
    ident = {10 + (5 - k) * 2: k for k in range(K)}
    slot_id = {k: i for i, k in ident.items()}
    for k in range(K):
        w.add_keyframe(slot_id[k], np.float32([0.25 * k, -0.5 * k, 0.125 * k]))
    pos = np.zeros((P, 3), np.float32)
    for p in range(P):
        seen = [k for k in range(K) if (p * 7 + k * 3) % 5 < 2]
        w.add_point(p, ref=slot_id[seen[0]] if seen else -1, bad=(p % 11 == 10))
        for k in seen:
            w.add_observation(p, slot_id[k], p, (p + k) % 4, (p + 2 * k) % 3 == 0)
        pos[p] = [np.float32(0.125) * p - np.float32(2), 0.25 * (p % 5), 5 + 0.5 * (p % 7)]
    sf = np.ones(8, np.float32)
    for i in range(1, 8):
        sf[i] = sf[i - 1] * np.float32(1.2)
    return w, ident, slot_id, pos, sf


def test_cpp_observation_graph_equals_the_binding_and_the_restatement(out):
    w, ident, slot_id, pos, sf = world()
    g = amd.ObservationGraph(P, 70, 8)
    orf.load(w, g, ident, {p: p for p in range(P)})
    q = list(range(P))
    (kf, wt), = g.votes([q], [2])
    assert ints(out["votes_kf"]) == kf.tolist() and ints(out["votes_w"]) == wt.tolist()
    assert {slot_id[k]: v for k, v in zip(kf.tolist(), wt.tolist())} == w.votes(q, slot_id[2])
    uc = orf.update_connections(w.votes(q, slot_id[2]))
    assert ints(out["ordered_id"]) == uc["ordered_id"] and ints(out["ordered_w"]) == uc["ordered_weight"] and int(out["parent"]) == uc["parent_id"]
    feats = [[(p, w.pts[p]["obs"][slot_id[k]][1]) for p in range(P) if slot_id[k] in w.pts[p]["obs"]] for k in (1, 3)]
    want = [w.culling_counts(slot_id[k], f) for k, f in zip((1, 3), feats)]
    assert list(zip(ints(out["n_mps"]), ints(out["n_redundant"]))) == want
    normal, lo, hi, valid = g.update_normal_depth(q, sf, pos)
    assert ints(out["valid"]) == valid.tolist() and 0 < valid.sum() < P
    for key, arr in (("normal", normal.reshape(-1)), ("min", lo), ("max", hi)):
        assert np.array_equal(floats(out[key]).view(np.uint32), arr.view(np.uint32)), key
    for p in range(P):
        r = w.normal_depth(p, pos[p], sf)
        assert (r is not None) == bool(valid[p])
        if r is not None:
            assert np.array_equal(r[0].view(np.uint32), normal[p].view(np.uint32)) and r[1] == lo[p] and r[2] == hi[p]
    assert int(out["table_equal"]) == 1 and int(out["in_view"]) > 0
    became = [int(w.erase_observation(p, slot_id[0])) for p in (0, 1, 2)]
    assert ints(out["became_bad"]) == became
    assert ints(out["erased_kf_bad"]) == w.erase_keyframe(slot_id[4])
    v2 = w.votes(q)
    assert {slot_id[k]: v for k, v in zip(ints(out["votes2_kf"]), ints(out["votes2_w"]))} == v2
    assert int(out["threw"]) == 3
