"""CPU, through the library: the key-frame rows (KeyFrame::mvpMapPoints) of the observation graph's host mirror -- set,
assign, get and clear need no device; an assign applies as a whole or not at all; every refused operand answers
ORBFE_ERR_INVALID before a device call; the device calls answer ORBFE_ERR_HIP on a device that does not exist; and a handle
that never enables the rows answers the existing calls as before."""
import ctypes as C

import numpy as np
import pytest

import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd import _lib
from orb_slam2_annotate_amd._lib import ptr

INV = _lib.ERR_INVALID


def _graph(width=64, device=0, enable=True):
    g = amd.ObservationGraph(point_capacity=32, kf_capacity=20, row_width=8, device=device)
    g.set_keyframes(list(range(12)), [100 - 3 * k for k in range(12)], np.zeros((12, 3), np.float32))
    g.set_points(list(range(30)), [0] * 30, [0] * 30)  # slots 30, 31 are never set
    if enable:
        g.enable_keyframe_points(width)
    return g


def _code(f, *a):
    with pytest.raises(amd.OrbfeError) as ei:
        f(*a)
    return ei.value.code


def test_set_assign_get_clear_on_the_mirror():
    g = _graph()
    assert g.get_keyframe_points(3).tolist() == []
    g.set_keyframe_points(3, [4, -1, 9, 4, 31])
    assert g.get_keyframe_points(3).tolist() == [4, -1, 9, 4, 31]
    g.assign_keyframe_points([3, 3, 3], [1, 0, 2], [7, -1, 8])  # AddMapPoint, EraseMapPointMatch, ReplaceMapPointMatch
    assert g.get_keyframe_points(3).tolist() == [-1, 7, 8, 4, 31]
    g.assign_keyframe_points([3, 3], [0, 0], [5, 6])  # in order: the later entry stands
    assert g.get_keyframe_points(3).tolist() == [6, 7, 8, 4, 31]
    g.set_keyframe_points(3, [1, 2])  # the row's length becomes n
    assert g.get_keyframe_points(3).tolist() == [1, 2]
    g.set_keyframe_points(4, list(range(30)) + [-1] * 34)  # n = kf_row_width
    assert len(g.get_keyframe_points(4)) == 64
    g.set_keyframe_points(3, [])
    assert g.get_keyframe_points(3).tolist() == []
    # erase_keyframe leaves the row of the erased key frame (SetBadFlag does not clear mvpMapPoints)
    g.set_keyframe_points(5, [1, 2, 3])
    g.erase_keyframe(5)
    assert g.get_keyframe_points(5).tolist() == [1, 2, 3]
    g.clear()  # empties the rows, keeps the width
    assert g.get_keyframe_points(4).tolist() == [] and g.get_keyframe_points(5).tolist() == []
    assert _code(g.set_keyframe_points, 4, [1]) == INV  # the kf slots are gone too
    g.set_keyframes([4], [7], np.zeros((1, 3), np.float32))
    g.set_keyframe_points(4, [-1] * 64)
    assert _code(g.set_keyframe_points, 4, [-1] * 65) == INV  # the width stayed 64
    g.enable_keyframe_points(64)  # the same width again: a no-op
    assert len(g.get_keyframe_points(4)) == 64


def test_an_assign_applies_as_a_whole_or_not_at_all():
    g = _graph()
    g.set_keyframe_points(1, [1, 2, 3])
    g.set_keyframe_points(2, [4, 5])
    for bad in (([1, 2, 1], [0, 2, 1], [9, 9, 9]),     # idx 2 is not below row 2's length
                ([1, 2], [0, 0], [9, 32]),            # a slot past point_capacity
                ([1, 2], [0, 0], [9, -2]),
                ([1, 20], [0, 0], [9, 9]),            # a kf slot out of range
                ([1, 6], [0, 0], [9, 9])):            # a row that was never set has length 0
        assert _code(g.assign_keyframe_points, *bad) == INV, bad
        assert g.get_keyframe_points(1).tolist() == [1, 2, 3] and g.get_keyframe_points(2).tolist() == [4, 5]
    g.assign_keyframe_points([1, 2, 1], [0, 1, 1], [9, 9, 9])
    assert g.get_keyframe_points(1).tolist() == [9, 9, 3] and g.get_keyframe_points(2).tolist() == [4, 9]


def test_every_refused_operand_is_invalid():
    L = _lib.load()
    g = _graph(enable=False)
    for w in (0, 32, 63, 96 + 1, 100, 16384 + 64, -64):
        assert _code(g.enable_keyframe_points, w) == INV, w
    # every other function on a handle that is not enabled
    z = np.zeros(4, np.int32)
    assert _code(g.set_keyframe_points, 1, [1]) == INV
    assert _code(g.assign_keyframe_points, [1], [0], [1]) == INV
    assert _code(g.get_keyframe_points, 1) == INV
    assert _code(g.keyframe_points_union, [[1]]) == INV
    assert _code(g.keyframe_points_union, []) == INV
    assert _code(g.tracked_points, [1]) == INV
    assert _code(g.tracked_points, []) == INV
    g.enable_keyframe_points(128)
    assert _code(g.enable_keyframe_points, 64) == INV  # another width
    g.enable_keyframe_points(128)
    big = amd.ObservationGraph(point_capacity=8, kf_capacity=(1 << 14) + 1, row_width=8)
    assert _code(big.enable_keyframe_points, 16384) == INV  # kf_capacity * kf_row_width > 2^28
    big.enable_keyframe_points(8192)
    # set
    assert _code(g.set_keyframe_points, 20, [1]) == INV and _code(g.set_keyframe_points, -1, [1]) == INV
    assert _code(g.set_keyframe_points, 15, [1]) == INV  # never given to set_keyframes
    assert _code(g.set_keyframe_points, 1, [32]) == INV and _code(g.set_keyframe_points, 1, [-2]) == INV
    assert _code(g.set_keyframe_points, 1, [0] * 129) == INV
    assert L.orbfe_obsgraph_set_keyframe_points(g._h, 1, -1, ptr(z)) == INV
    assert L.orbfe_obsgraph_set_keyframe_points(g._h, 1, 2, None) == INV
    # assign, get
    assert L.orbfe_obsgraph_assign_keyframe_points(g._h, -1, ptr(z), ptr(z), ptr(z)) == INV
    assert L.orbfe_obsgraph_assign_keyframe_points(g._h, 1, ptr(z), None, ptr(z)) == INV
    assert _code(g.get_keyframe_points, 20) == INV
    n = C.c_int32(0)
    assert L.orbfe_obsgraph_get_keyframe_points(g._h, 0, 1, None, C.byref(n)) == INV
    # the union: all of these fail before the device is looked for
    g.set_keyframe_points(1, [1, 2])
    assert _code(g.keyframe_points_union, [[20]]) == INV
    assert _code(g.keyframe_points_union, [[1], [-1]]) == INV
    assert _code(g.keyframe_points_union, [[1, 15]]) == INV  # a kf slot that was never set
    out, cnt = np.zeros(8, np.int32), np.zeros(4, np.int32)
    one = np.array([1], np.int32)
    union = L.orbfe_obsgraph_keyframe_points_union
    assert union(g._h, 1, ptr(np.array([0, 1], np.int32)), ptr(one), -1, ptr(out), ptr(cnt)) == INV
    assert union(g._h, -1, ptr(np.array([0, 1], np.int32)), ptr(one), 4, ptr(out), ptr(cnt)) == INV
    assert union(g._h, 65536, ptr(np.zeros(65537, np.int32)), ptr(one), 4, ptr(out), ptr(cnt)) == INV
    assert union(g._h, 2, ptr(np.array([0, 1, 0], np.int32)), ptr(one), 4, ptr(out), ptr(cnt)) == INV  # descending offsets
    assert union(g._h, 1, ptr(np.array([1, 1], np.int32)), ptr(one), 4, ptr(out), ptr(cnt)) == INV
    assert union(g._h, 1, None, ptr(one), 4, ptr(out), ptr(cnt)) == INV
    assert union(g._h, 1, ptr(np.array([0, 1], np.int32)), None, 4, ptr(out), ptr(cnt)) == INV
    assert union(g._h, 1, ptr(np.array([0, 1], np.int32)), ptr(one), 4, None, ptr(cnt)) == INV
    assert union(g._h, 1, ptr(np.array([0, 1], np.int32)), ptr(one), 4, ptr(out), None) == INV
    # key frames * kf_row_width must stay below 2^31
    wide = amd.ObservationGraph(point_capacity=8, kf_capacity=4, row_width=8)
    wide.set_keyframes([0], [1], np.zeros((1, 3), np.float32))
    wide.enable_keyframe_points(16384)
    many = np.zeros(1 << 17, np.int32)
    assert union(wide._h, 1, ptr(np.array([0, 1 << 17], np.int32)), ptr(many), 4, ptr(out), ptr(cnt)) == INV
    # tracked_points
    assert _code(g.tracked_points, [20]) == INV and _code(g.tracked_points, [15]) == INV
    assert L.orbfe_obsgraph_tracked_points(g._h, -1, ptr(one), 0, ptr(cnt)) == INV
    assert L.orbfe_obsgraph_tracked_points(g._h, 1, None, 0, ptr(cnt)) == INV
    assert L.orbfe_obsgraph_tracked_points(g._h, 1, ptr(one), 0, None) == INV
    # nothing to do needs no device
    assert g.keyframe_points_union([]) == [] and g.tracked_points([]).tolist() == []


def test_device_calls_answer_err_hip_on_a_device_that_is_not_there():
    absent = _lib.load().orbfe_device_count()  # 0 without a GPU; one past the last with one
    g = _graph(device=absent)
    g.set_keyframe_points(1, [1, 2, 3])
    for call in (lambda: g.keyframe_points_union([[1]]), lambda: g.local_points([1]), lambda: g.tracked_points([1], 1),
                 lambda: g.get_keyframe_points(1, from_device=True)):
        assert _code(call) == _lib.ERR_HIP
    assert g.get_keyframe_points(1).tolist() == [1, 2, 3]  # the mirror is untouched by the failures


def test_a_handle_that_never_enables_the_rows_answers_as_before():
    g = _graph(enable=False)
    g.add_observations([3, 3, 3], [0, 5, 2], [7, 8, 9], [1, 2, 3], [0, 1, 0])
    r = g.get_row(3)
    assert [tuple(int(v) for v in e) for e in r["entries"]] == [(5, 8, 2, 1), (2, 9, 3, 0), (0, 7, 1, 0)] and r["n_obs"] == 4
    assert g.erase_observations([3], [5]).tolist() == [1]  # 4 - 2 = 2: bad
    assert g.erase_keyframe(2).tolist() == []
    g.clear()
    assert g.get_row(3)["bad"] == 1 and len(g.get_row(3)["entries"]) == 0
