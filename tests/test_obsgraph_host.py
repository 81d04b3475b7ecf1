"""CPU, through the library: the two host replays of the observation graph against tests/obsgraph_ref.py, the host mirror
alone (creating a graph and changing it never touches the device), and the argument checks -- every invalid argument fails
before a device call, and without a device the compute entries fail with ORBFE_ERR_HIP."""
import ctypes as C

import numpy as np
import pytest

import obsgraph_ref as orf
import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd import _lib
from orb_slam2_annotate_amd import observation_graph as og
from orb_slam2_annotate_amd._lib import ptr


def _uc(counter):
    ids = list(counter)
    got = og.update_connections(ids, [counter[i] for i in ids])
    want = orf.update_connections(counter)
    for k in ("ordered_id", "ordered_weight", "connect_id", "connect_weight"):
        assert got[k].tolist() == want[k], (k, counter)
    assert got["parent_id"] == want["parent_id"] and got["counter"] == counter
    return got


def test_update_connections_threshold_and_ties():
    got = _uc({5: 14, 2: 15, 9: 40})  # exactly 14 stays out, exactly 15 is in
    assert got["ordered_id"].tolist() == [9, 2]
    got = _uc({8: 3, 4: 7, 6: 7, 1: 2})  # nobody at 15; two tie for the maximum: the lower id
    assert got["ordered_id"].tolist() == [4] and got["ordered_weight"].tolist() == [7] and got["parent_id"] == 4
    got = _uc({3: 20, 11: 20, 7: 20, 5: 16})  # equal weights: descending id
    assert got["ordered_id"].tolist() == [11, 7, 3, 5]
    assert _uc({})["parent_id"] == -1
    rng = np.random.default_rng(3)
    for _ in range(20):
        ids = rng.choice(1000, size=int(rng.integers(1, 40)), replace=False).tolist()
        _uc({i: int(rng.integers(1, 30)) for i in ids})
    for bad in (([1, 1], [3, 3]), ([1, 2], [3, 0])):  # an id twice, a weight of 0
        with pytest.raises(amd.OrbfeError) as ei:
            og.update_connections(*bad)
        assert ei.value.code == _lib.ERR_INVALID


def _lk(counter, bad, neigh, child, parent):
    ids = list(counter)
    nb = [neigh.get(i, []) for i in ids]
    ch = [sorted(child.get(i, [])) for i in ids]
    got, ref = og.local_keyframes(ids, [counter[i] for i in ids], [i in bad for i in ids], nb, [[j in bad for j in x] for x in nb],
                                  ch, [[j in bad for j in x] for x in ch], [parent.get(i, -1) for i in ids])
    want, wref = orf.local_keyframes(counter, bad, neigh, child, parent)
    assert got.tolist() == want and ref == wref, (counter, got.tolist(), want)
    return got.tolist(), ref


def test_local_keyframes_walk():
    # the only eligible neighbour is in place 11: not read
    bad = set(range(100, 110))
    assert _lk({1: 1}, bad, {1: list(range(100, 111))}, {}, {}) == ([1], 1)
    assert _lk({1: 1}, bad - {109}, {1: list(range(100, 111))}, {}, {}) == ([1, 109], 1)
    # a bad child is passed over; a bad voted key frame is neither local nor the reference
    assert _lk({1: 1, 2: 9}, {2, 11}, {1: [2, 10]}, {1: [13, 11]}, {}) == ([1, 10, 13], 1)
    # the parent's break leaves the whole loop: key frame 3 is never visited
    got, ref = _lk({3: 3, 1: 1, 2: 3}, set(), {1: [2, 10], 2: [10, 12], 3: [30]}, {1: [11], 3: [31]}, {1: 2, 2: 20, 3: 1})
    assert got == [1, 2, 3, 10, 11, 12, 20] and ref == 2
    # the stop at 81
    neigh = {k: [1000 + k] for k in range(81)}
    child = {k: [2000 + k] for k in range(81)}
    assert len(_lk({k: 1 for k in range(81)}, set(), neigh, child, {})[0]) == 81
    assert _lk({k: 1 for k in range(79)}, set(), neigh, child, {})[0][79:] == [1000, 2000]
    assert _lk({k: 1 for k in range(80)}, set(), neigh, child, {})[0][80:] == [1000, 2000]
    assert _lk({}, set(), {}, {}, {}) == ([], -1)
    rng = np.random.default_rng(5)
    for _ in range(20):
        ids = rng.choice(60, size=int(rng.integers(1, 30)), replace=False).tolist()
        bad = set(rng.choice(80, size=10, replace=False).tolist())
        neigh = {i: rng.choice(80, size=int(rng.integers(0, 14)), replace=False).tolist() for i in ids}
        child = {i: rng.choice(80, size=int(rng.integers(0, 4)), replace=False).tolist() for i in ids}
        parent = {i: int(rng.integers(-1, 80)) for i in ids}
        _lk({i: int(rng.integers(1, 9)) for i in ids}, bad, neigh, child, parent)


def _graph(rw=8):
    g = amd.ObservationGraph(point_capacity=32, kf_capacity=20, row_width=rw)
    g.set_keyframes(list(range(12)), [100 - 3 * k for k in range(12)], np.zeros((12, 3), np.float32))  # ids DESCEND with the slot
    g.set_points(list(range(32)), [0] * 32, [0] * 32)
    return g


def _row(g, slot):
    r = g.get_row(slot)
    return [tuple(int(v) for v in e) for e in r["entries"]], r["n_obs"], r["bad"], r["ref_kf_slot"]


def test_mirror_rows_are_in_ascending_id_and_a_present_pair_is_ignored():
    g = _graph()
    g.add_observations([3, 3, 3], [0, 5, 2], [7, 8, 9], [1, 2, 3], [0, 1, 0])
    # ids 100, 85, 94 -> ascending id: slot 5, slot 2, slot 0
    assert _row(g, 3) == ([(5, 8, 2, 1), (2, 9, 3, 0), (0, 7, 1, 0)], 4, 0, 0)
    g.add_observations([3], [5], [99], [6], [0])  # present: no-op, the entry keeps idx 8 and its stereo weight
    assert _row(g, 3) == ([(5, 8, 2, 1), (2, 9, 3, 0), (0, 7, 1, 0)], 4, 0, 0)
    g.clear()
    assert _row(g, 3) == ([], 0, 1, -1)


def test_a_full_row_refuses_the_whole_call():
    g = _graph()
    g.add_observations([4] * 8, list(range(8)), [0] * 8, [0] * 8, [0] * 8)
    before = [_row(g, s) for s in (4, 5)]
    with pytest.raises(amd.OrbfeError) as ei:
        g.add_observations([5, 4], [1, 9], [0, 0], [0, 0], [0, 0])  # slot 5 has room, slot 4 has none
    assert ei.value.code == _lib.ERR_CAPACITY
    assert [_row(g, s) for s in (4, 5)] == before and before[1][0] == []
    g.add_observations([5], [1], [0], [0], [0])
    assert _row(g, 5)[1] == 1


def test_erase_with_stereo_weight_makes_the_point_bad_and_moves_the_reference():
    g = _graph()
    g.add_observations([6, 6], [1, 2], [0, 0], [0, 0], [1, 1])  # nObs = 4
    g.set_points([6], [0], [2])
    assert g.erase_observations([6, 6], [7, 2]).tolist() == [0, 1]  # absent: ignored; 4 - 2 = 2: bad, row cleared
    assert _row(g, 6) == ([], 2, 1, 1)
    # the reference key frame moves to the lowest remaining id: slots 0 1 2 3 hold ids 100 97 94 91
    g.add_observations([7] * 4, [0, 1, 2, 3], [0] * 4, [0] * 4, [0] * 4)
    g.set_points([7], [0], [1])
    assert g.erase_observations([7], [1]).tolist() == [0]
    assert _row(g, 7) == ([(3, 0, 0, 0), (2, 0, 0, 0), (0, 0, 0, 0)], 3, 0, 3)
    # erase_keyframe: point 7 drops to 2 and becomes bad, point 8 stays
    g.add_observations([8] * 4, [0, 3, 4, 5], [0] * 4, [0] * 4, [0] * 4)
    assert g.erase_keyframe(3).tolist() == [7]
    assert _row(g, 7)[:3] == ([], 2, 1) and _row(g, 8)[1] == 3 and len(_row(g, 8)[0]) == 3


def test_invalid_arguments_fail_before_any_device_call():
    L = _lib.load()
    h = C.c_void_p()
    for args in ((0, 0, 4, 8), (0, 4, 0, 8), (0, 4, 4, 12), (0, 4, 4, 4), (0, 4, 4, 512), (-1, 4, 4, 8), (0, 1 << 24, 4, 256)):
        assert L.orbfe_obsgraph_create(*args, C.byref(h)) == _lib.ERR_INVALID, args
    assert L.orbfe_obsgraph_create(0, 4, 4, 8, None) == _lib.ERR_INVALID
    g = _graph()
    inv = lambda f, *a: pytest.raises(amd.OrbfeError, f, *a).value.code == _lib.ERR_INVALID  # noqa: E731
    assert inv(g.set_keyframes, [20], [1], np.zeros((1, 3)))
    assert inv(g.set_keyframes, [15], [100], np.zeros((1, 3)))  # id 100 is slot 0's
    assert inv(g.set_points, [32], [0], [0])
    assert inv(g.set_points, [0], [0], [20])
    assert inv(g.add_observations, [-1], [0], [0], [0], [0])
    assert inv(g.add_observations, [0], [20], [0], [0], [0])
    assert inv(g.add_observations, [0], [15], [0], [0], [0])  # a kf slot that was never set
    g.add_observations([0], [1], [0], [0], [0])
    assert inv(g.set_keyframes, [1], [555], np.zeros((1, 3)))  # rows name it: its id is fixed
    assert inv(g.erase_observations, [32], [0])
    assert inv(g.erase_keyframe, 20)
    assert inv(g.get_row, 32)
    assert inv(g.votes, [[32]])
    assert inv(g.votes, [[0]], [20])
    assert inv(g.culling_counts, [20], [([0], [0])])
    assert inv(g.culling_counts, [0], [([32], [0])])
    sf = np.ones(8, np.float32)
    assert inv(g.update_normal_depth, [32], sf, np.zeros((1, 3)))
    assert inv(g.update_normal_depth, [0], np.ones(0, np.float32), np.zeros((1, 3)))
    g.add_observations([1], [1], [0], [9], [0])
    g.set_points([1], [0], [1])
    assert inv(g.update_normal_depth, [1], sf, np.zeros((1, 3)))  # the reference entry's octave 9 is no level of 8
    mp = amd.MapPoints(16)  # fewer slots than the graph's 32
    assert inv(lambda: g.update_normal_depth([0], sf, mp=mp))
    mp32 = amd.MapPoints(32)
    assert inv(lambda: g.update_normal_depth([0, 0], sf, mp=mp32))
    z = np.zeros(4, np.int32)
    assert L.orbfe_obsgraph_votes(g._h, -1, ptr(z), ptr(z), ptr(z), 4, ptr(z), ptr(z), ptr(z)) == _lib.ERR_INVALID
    assert L.orbfe_obsgraph_votes(g._h, 1, None, ptr(z), ptr(z), 4, ptr(z), ptr(z), ptr(z)) == _lib.ERR_INVALID
    assert L.orbfe_obsgraph_votes(g._h, 65536, ptr(z), ptr(z), ptr(z), 4, ptr(z), ptr(z), ptr(z)) == _lib.ERR_INVALID
    assert L.orbfe_obsgraph_set_points(g._h, 1, ptr(z), None, ptr(z)) == _lib.ERR_INVALID
    assert L.orbfe_obsgraph_add_observations(g._h, -1, ptr(z), ptr(z), ptr(z), ptr(z), ptr(z)) == _lib.ERR_INVALID


def test_compute_entries_fail_with_err_hip_without_a_device():
    if _lib.load().orbfe_device_count() > 0:
        pytest.skip("a GPU is present")
    g = _graph()
    g.add_observations([0, 0], [1, 2], [0, 0], [0, 0], [0, 0])
    sf = np.ones(8, np.float32)
    mp = amd.MapPoints(32)
    for call in (lambda: g.votes([[0]]), lambda: g.culling_counts([1], [([0], [0])]),
                 lambda: g.update_normal_depth([0], sf, np.zeros((1, 3))), lambda: g.update_normal_depth([0], sf, mp=mp),
                 lambda: g.get_row(0, from_device=True), lambda: g.update_connections(1, [0])):
        with pytest.raises(amd.OrbfeError) as ei:
            call()
        assert ei.value.code == _lib.ERR_HIP
    assert _row(g, 0)[1] == 2  # the mirror is untouched by the failures
