"""orbfe_triangulated_points_select (host code, no device) against the sequential restatement tests/tri_points_ref.py: every
output exactly equal, the floats by their bits, on inputs engineered so that one rule decides each outcome; the capacity
rule; every argument error."""
import ctypes as C

import numpy as np
import pytest

import orb_slam2_annotate_amd as amd
import tri_points_ref as ref
from orb_slam2_annotate_amd import OrbfeError, _lib

CASES = ref.cases()
BY_NAME = {c["name"]: c for c in CASES}
LISTS = ("created_k", "created_i1", "created_i2", "desc_from")
FLOATS = ("pos", "normal", "min_dist", "max_dist")


def run_both(c, capacity=None):
    want = ref.select(c["match12"], c["status"], c["x3d"], c["kf1_id"], c["kf2_ids"], c["centre1"], c["centre2"], c["octave1"], ref.SCALE)
    got = amd.triangulated_points_select(c["match12"], c["status"], c["x3d"], c["kf1_id"], c["kf2_ids"], c["centre1"], c["centre2"],
                                         c["octave1"], ref.SCALE, capacity=capacity)
    return want, got


def same(want, got):
    assert got["n_created"] == want["n_created"]
    for k in LISTS:
        assert np.array_equal(got[k], want[k]), k
    for k in FLOATS:
        assert ref.same_bits(got[k], want[k]), k


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_select_equals_the_restatement(c):
    same(*run_both(c))


def test_the_cases_show_what_they_are_named_for():
    w = {name: run_both(c)[0] for name, c in BY_NAME.items()}
    assert w["no_neighbour"]["n_created"] == 0 and w["none_created"]["n_created"] == 0 and w["one_pair"]["n_created"] == 1
    c = w["contested"]  # ascending (k, i1); i1 = 3 goes to neighbour 0, so keypoint 8 of neighbour 2 gets nothing
    assert list(zip(c["created_k"], c["created_i1"], c["created_i2"])) == [(0, 0, 0), (0, 3, 7), (2, 5, 2)]
    assert list(zip(w["later_neighbour_wins"]["created_k"], w["later_neighbour_wins"]["created_i1"])) == [(1, 0), (1, 2)]
    assert sorted(set(w["empty_middle"]["created_k"].tolist())) == [0, 2]
    assert w["ids_both_sides"]["desc_from"].tolist() == [1, 1, 0, 0]
    d = w["dense"]
    assert d["n_created"] > 40 and len(set(d["created_i1"].tolist())) == d["n_created"] and set(d["desc_from"].tolist()) == {0, 1}
    key = d["created_k"].astype(np.int64) * 1000 + d["created_i1"]
    assert (np.diff(key) > 0).all()


def test_rounding_far_from_the_origin_is_part_of_the_definition():
    """1e3 from the origin P - C loses bits and (float)(1.0 / nrm) is not 1.0f / (float)nrm: a float32-only formula differs"""
    c = BY_NAME["far_from_origin"]
    want, got = run_both(c)
    same(want, got)
    naive = []
    for j in range(want["n_created"]):
        k, P = want["created_k"][j], want["pos"][j]
        d1, d2 = P - c["centre1"], P - c["centre2"][k]
        t1, t2 = d1 / np.linalg.norm(d1), d2 / np.linalg.norm(d2)
        a, b = (t2, t1) if want["desc_from"][j] else (t1, t2)
        naive.append(((a + b) / np.float32(2)).astype(np.float32))
    assert not ref.same_bits(np.asarray(naive), want["normal"])
    assert np.allclose(np.asarray(naive), want["normal"], rtol=0, atol=1e-6)


def test_octave_ends_use_the_first_and_last_level():
    c = BY_NAME["octave_ends"]
    want, got = run_both(c)
    same(want, got)
    ratio = got["max_dist"] / got["min_dist"]
    assert np.allclose(ratio, ref.SCALE[-1], rtol=1e-6)
    d1 = np.linalg.norm(got["pos"].astype(np.float64) - c["centre1"].astype(np.float64), axis=1)
    assert np.allclose(got["max_dist"] / d1, ref.SCALE[c["octave1"][got["created_i1"]]], rtol=1e-6)


def test_capacity_equal_below_and_above():
    c = BY_NAME["dense"]
    want, _ = run_both(c)
    m = want["n_created"]
    same(want, run_both(c, capacity=m)[1])
    same(want, run_both(c, capacity=m + 1)[1])
    with pytest.raises(OrbfeError) as ei:
        run_both(c, capacity=m - 1)
    assert ei.value.code == _lib.ERR_CAPACITY and ei.value.n_created == m


def test_capacity_error_writes_no_array():
    c = BY_NAME["contested"]
    L = _lib.load()
    cap = 2
    outs = [np.full(cap, 77, np.int32) for _ in range(3)] + [np.full((cap, 3), 7.0, np.float32) for _ in range(2)] + \
           [np.full(cap, 7.0, np.float32) for _ in range(2)] + [np.full(cap, 77, np.uint8)]
    before = [o.copy() for o in outs]
    n = C.c_int32(-5)
    p = _lib.ptr
    rc = L.orbfe_triangulated_points_select(c["n1"], c["K"], p(c["match12"]), p(c["status"]), p(c["x3d"]), c["kf1_id"], p(c["kf2_ids"]),
                                            p(c["centre1"]), p(c["centre2"]), p(c["octave1"]), p(ref.SCALE), ref.N_LEVELS, cap,
                                            *[p(o) for o in outs], C.byref(n))
    assert rc == _lib.ERR_CAPACITY and n.value == 3
    assert all(np.array_equal(a, b) for a, b in zip(before, outs))


def test_argument_errors():
    c = BY_NAME["contested"]
    L = _lib.load()
    p = _lib.ptr
    cap = c["n1"]
    outs = [np.zeros(cap, np.int32) for _ in range(3)] + [np.zeros((cap, 3), np.float32) for _ in range(2)] + \
           [np.zeros(cap, np.float32) for _ in range(2)] + [np.zeros(cap, np.uint8)]
    n = C.c_int32(0)

    def call(**kw):
        a = dict(n1=c["n1"], K=c["K"], match12=c["match12"], status=c["status"], x3d=c["x3d"], kf1_id=c["kf1_id"], kf2_ids=c["kf2_ids"],
                 centre1=c["centre1"], centre2=c["centre2"], octave1=c["octave1"], scale=ref.SCALE, n_levels=ref.N_LEVELS, capacity=cap,
                 outs=outs, n=C.byref(n))
        a.update(kw)
        return L.orbfe_triangulated_points_select(a["n1"], a["K"], p(a["match12"]), p(a["status"]), p(a["x3d"]), a["kf1_id"], p(a["kf2_ids"]),
                                                  p(a["centre1"]), p(a["centre2"]), p(a["octave1"]), p(a["scale"]), a["n_levels"],
                                                  a["capacity"], *[p(o) for o in a["outs"]], a["n"])

    assert call() == 0 and n.value == 3
    bad = lambda **kw: call(**kw) == _lib.ERR_INVALID
    assert bad(n1=-1) and bad(n1=16385) and bad(K=-1) and bad(K=65) and bad(capacity=-1)
    assert bad(n_levels=0) and bad(n_levels=257)
    for key in ("match12", "status", "x3d", "kf2_ids", "centre1", "centre2", "octave1", "scale"):
        assert bad(**{key: None}), key
    assert bad(n=None)
    for j in range(len(outs)):
        o = list(outs)
        o[j] = None
        assert bad(outs=o), j
    assert bad(kf1_id=-1) and bad(kf2_ids=np.array([11, -1, 13], np.int64))
    assert bad(kf2_ids=np.array([11, 10, 13], np.int64))  # a neighbour with key frame 1's mnId
    assert bad(kf2_ids=np.array([11, 13, 13], np.int64))  # two neighbours with one mnId
    for v in (np.inf, np.nan):
        x = c["centre1"].copy()
        x[1] = v
        assert bad(centre1=x)
        x = c["centre2"].copy()
        x[2, 0] = v
        assert bad(centre2=x)
    m = c["match12"].copy()
    m[0, 3] = -2
    assert bad(match12=m)
    m[0, 3] = 16384
    assert bad(match12=m)
    m = c["match12"].copy()
    m[2, 5] = 8  # keypoint 8 of neighbour 2 named by i1 = 3 and by i1 = 5
    assert bad(match12=m)
    s = c["status"].copy()
    s[0, 3] = 10  # above ORBFE_TRI_SCALE
    assert bad(status=s)
    s = c["status"].copy()
    s[0, 1] = ref.CREATED  # a status where match12 holds no match
    assert bad(status=s)
    s = c["status"].copy()
    s[0, 3] = 0  # NO_MATCH where match12 holds one
    assert bad(status=s)
    o = c["octave1"].copy()
    o[3] = ref.N_LEVELS  # a created keypoint's octave
    assert bad(octave1=o)
    o[3] = -1
    assert bad(octave1=o)
    o = c["octave1"].copy()
    o[1] = ref.N_LEVELS  # (1 is matched but not created: its octave is not read)
    assert call(octave1=o) == 0
    assert call() == 0 and n.value == 3
