"""CPU, through the library: the key-frame descriptor store of the observation graph and the distinctive-descriptor calls
as far as they go without a device -- enable and its limits; every refused operand answers ORBFE_ERR_INVALID before a device
call; the two set calls and both loops answer ORBFE_ERR_HIP on a device that does not exist (the store has no host copy of
the bytes, so a set must reach the device); and a handle that never enables the store answers the existing calls as
before."""
import ctypes as C

import numpy as np
import pytest

import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd import _lib
from orb_slam2_annotate_amd._lib import ptr

INV, HIP = _lib.ERR_INVALID, _lib.ERR_HIP


def _absent():
    return _lib.load().orbfe_device_count()  # 0 without a GPU; one past the last with one


def _graph(width=64, device=None, enable=True):
    g = amd.ObservationGraph(point_capacity=32, kf_capacity=20, row_width=8, device=_absent() if device is None else device)
    g.set_keyframes(list(range(12)), [100 - 3 * k for k in range(12)], np.zeros((12, 3), np.float32))
    g.set_points(list(range(30)), [0] * 30, [0] * 30)  # slots 30, 31 are never set
    if enable:
        g.enable_keyframe_descriptors(width)
    return g


def _code(f, *a, **kw):
    with pytest.raises(amd.OrbfeError) as ei:
        f(*a, **kw)
    return ei.value.code


def test_enable_once_and_its_limits():
    g = _graph(enable=False)
    for w in (0, 32, 63, 96 + 1, 100, 16384 + 64, -64):
        assert _code(g.enable_keyframe_descriptors, w) == INV, w
    g.enable_keyframe_descriptors(128)
    g.enable_keyframe_descriptors(128)  # the same width again: a no-op
    assert _code(g.enable_keyframe_descriptors, 64) == INV  # another width
    big = amd.ObservationGraph(point_capacity=8, kf_capacity=(1 << 12) + 1, row_width=8, device=_absent())
    assert _code(big.enable_keyframe_descriptors, 16384) == INV  # kf_capacity * kf_desc_width > 2^26
    big.enable_keyframe_descriptors(8192)
    # independent of the key-frame rows, in either order
    g.enable_keyframe_points(64)
    h = _graph(enable=False)
    h.enable_keyframe_points(64)
    h.enable_keyframe_descriptors(64)


def test_everything_refuses_on_a_handle_that_is_not_enabled():
    L = _lib.load()
    g = _graph(enable=False)
    mp = amd.MapPoints(32, device=_absent())
    d = np.zeros((2, 32), np.uint8)
    assert _code(g.set_keyframe_descriptors, 1, d) == INV
    assert _code(g.get_keyframe_descriptors, 1) == INV
    assert _code(g.distinctive_descriptors, [1]) == INV
    assert _code(g.distinctive_descriptors, []) == INV
    assert _code(g.distinctive_descriptors, [1], mp=mp) == INV
    assert _code(mp.compute_distinctive_descriptors, g, []) == INV
    assert L.orbfe_obsgraph_set_keyframe_descriptors_frame(g._h, 1, None) == INV


def test_every_refused_operand_is_invalid_before_the_device_is_looked_for():
    L = _lib.load()
    g = _graph()
    d = np.zeros((65, 32), np.uint8)
    # set: the kf slot, the count, the array
    assert _code(g.set_keyframe_descriptors, 20, d[:1]) == INV and _code(g.set_keyframe_descriptors, -1, d[:1]) == INV
    assert _code(g.set_keyframe_descriptors, 15, d[:1]) == INV  # never given to set_keyframes
    assert _code(g.set_keyframe_descriptors, 1, d) == INV       # 65 rows in a store of 64
    assert L.orbfe_obsgraph_set_keyframe_descriptors(g._h, 1, -1, ptr(d)) == INV
    assert L.orbfe_obsgraph_set_keyframe_descriptors(g._h, 1, 2, None) == INV
    assert L.orbfe_obsgraph_set_keyframe_descriptors(None, 1, 2, ptr(d)) == INV
    assert L.orbfe_obsgraph_set_keyframe_descriptors_frame(g._h, 1, None) == INV
    # get
    n = C.c_int32(0)
    assert _code(g.get_keyframe_descriptors, 20) == INV
    assert L.orbfe_obsgraph_get_keyframe_descriptors(g._h, 1, None, C.byref(n)) == INV
    assert L.orbfe_obsgraph_get_keyframe_descriptors(g._h, 1, ptr(d), None) == INV
    assert len(g.get_keyframe_descriptors(1)) == 0  # nothing set: nothing to read, no device needed
    # the array form
    kf, idx, valid = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.uint8)
    one = np.array([3], np.int32)
    run = L.orbfe_obsgraph_distinctive_descriptors
    assert run(g._h, -1, ptr(one), ptr(kf), ptr(idx), None, ptr(valid)) == INV
    assert run(g._h, 1, None, ptr(kf), ptr(idx), None, ptr(valid)) == INV
    assert run(g._h, 1, ptr(one), None, ptr(idx), None, ptr(valid)) == INV
    assert run(g._h, 1, ptr(one), ptr(kf), None, None, ptr(valid)) == INV
    assert run(g._h, 1, ptr(one), ptr(kf), ptr(idx), None, None) == INV
    assert run(None, 1, ptr(one), ptr(kf), ptr(idx), None, ptr(valid)) == INV
    assert _code(g.distinctive_descriptors, [32]) == INV and _code(g.distinctive_descriptors, [3, -1]) == INV
    # a live entry whose key frame received no descriptors -- whether or not that key frame is bad
    g.add_observations([3, 3], [0, 5], [7, 8], [1, 2], [0, 0])
    assert _code(g.distinctive_descriptors, [3]) == INV
    g.set_keyframes([5], [100 - 15], np.zeros((1, 3), np.float32), [1])
    assert _code(g.distinctive_descriptors, [4, 3]) == INV
    kf_v, idx_v, desc_v, valid_v = g.distinctive_descriptors([])  # nothing to do needs no device
    assert len(kf_v) == len(idx_v) == len(desc_v) == len(valid_v) == 0
    # the table form: the same, and the two handles
    mp = amd.MapPoints(32, device=_absent())
    tab = L.orbfe_obsgraph_distinctive_descriptors_mappoints
    assert tab(g._h, None, 1, ptr(one), None, None, ptr(valid)) == INV
    assert tab(g._h, mp._h, -1, ptr(one), None, None, ptr(valid)) == INV
    assert tab(g._h, mp._h, 1, None, None, None, ptr(valid)) == INV
    assert tab(g._h, mp._h, 1, ptr(one), None, None, None) == INV
    assert _code(g.distinctive_descriptors, [32], mp=mp) == INV
    assert _code(g.distinctive_descriptors, [3], mp=mp) == INV       # the key frames' descriptors were never set
    assert _code(g.distinctive_descriptors, [4, 6, 4], mp=mp) == INV  # a slot named twice
    assert _code(g.distinctive_descriptors, [4], mp=amd.MapPoints(31, device=_absent())) == INV  # fewer slots than the graph
    assert _code(g.distinctive_descriptors, [4], mp=amd.MapPoints(32, device=_absent() + 1)) == INV  # another device
    assert len(g.distinctive_descriptors([], mp=mp)[2]) == 0
    # orbfe_mappoints_descriptors
    out = np.zeros((2, 32), np.uint8)
    assert _code(mp.descriptors, [32]) == INV and _code(mp.descriptors, [-1]) == INV
    assert L.orbfe_mappoints_descriptors(None, 1, ptr(one), ptr(out)) == INV
    assert L.orbfe_mappoints_descriptors(mp._h, 1, None, ptr(out)) == INV
    assert L.orbfe_mappoints_descriptors(mp._h, 1, ptr(one), None) == INV
    assert L.orbfe_mappoints_descriptors(mp._h, -1, ptr(one), ptr(out)) == INV
    assert len(mp.descriptors([])) == 0


def test_set_and_both_loops_answer_err_hip_on_a_device_that_is_not_there():
    g = _graph()
    d = np.arange(3 * 32, dtype=np.uint8).reshape(3, 32)
    assert _code(g.set_keyframe_descriptors, 1, d) == HIP
    assert _code(g.set_keyframe_descriptors, 1, d[:0]) == HIP  # even with nothing to copy: a set is a device call
    assert len(g.get_keyframe_descriptors(1)) == 0             # ... and the failed set left no count behind
    # slot 4 has an empty row and slot 31 was never set: the checks pass, the device is looked for
    assert _code(g.distinctive_descriptors, [4, 31]) == HIP
    mp = amd.MapPoints(32, device=_absent())
    assert _code(g.distinctive_descriptors, [4, 31], mp=mp) == HIP
    assert _code(mp.compute_distinctive_descriptors, g, [4]) == HIP
    assert _code(mp.descriptors, [1, 2]) == HIP


def test_clear_and_erase_keyframe_keep_the_store_enabled():
    g = _graph()
    g.add_observations([3, 3, 3], [0, 5, 2], [7, 8, 9], [1, 2, 3], [0, 1, 0])
    assert g.erase_keyframe(2).tolist() == []
    g.clear()
    assert _code(g.enable_keyframe_descriptors, 128) == INV  # the width stayed 64
    g.enable_keyframe_descriptors(64)
    assert _code(g.set_keyframe_descriptors, 1, np.zeros((1, 32), np.uint8)) == INV  # the kf slots are gone


def test_a_handle_that_never_enables_the_store_answers_as_before():
    g = _graph(enable=False)
    g.add_observations([3, 3, 3], [0, 5, 2], [7, 8, 9], [1, 2, 3], [0, 1, 0])
    r = g.get_row(3)
    assert [tuple(int(v) for v in e) for e in r["entries"]] == [(5, 8, 2, 1), (2, 9, 3, 0), (0, 7, 1, 0)] and r["n_obs"] == 4
    assert g.erase_observations([3], [5]).tolist() == [1]  # 4 - 2 = 2: bad
    assert g.erase_keyframe(2).tolist() == []
    g.clear()
    assert g.get_row(3)["bad"] == 1 and len(g.get_row(3)["entries"]) == 0
    g.enable_keyframe_points(64)
    g.set_keyframes([4], [7], np.zeros((1, 3), np.float32))
    g.set_keyframe_points(4, [1, 2, -1])
    assert g.get_keyframe_points(4).tolist() == [1, 2, -1]
