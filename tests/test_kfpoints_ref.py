"""CPU: the restatement of the reference's loops over KeyFrame::mvpMapPoints (tests/kfpoints_ref.py) pinned with answers
worked out by hand from src/Tracking.cc:1315-1333 and src/KeyFrame.cc:264-289."""
import kfpoints_ref as kr


def _world():
    w = kr.KeyFramePoints()
    N = None
    w.set_row(0, [5, N, 7, 5, 9])   # 5 twice in one row
    w.set_row(1, [7, 3, N, 8])      # 7 is also in key frame 0; 8 is bad everywhere it appears
    w.set_row(2, [])                # an empty row
    w.set_row(3, [8, 2, 3, N, 5])
    w.bad = {8}
    w.n_obs = {5: 4, 7: 1, 9: 2, 3: 3, 2: 0, 8: 9}
    return w


def test_the_union_keeps_first_occurrences_in_visiting_order():
    w = _world()
    assert w.local_points([0]) == [5, 7, 9]                  # a point twice in one row: once
    assert w.local_points([0, 1]) == [5, 7, 9, 3]            # a point in two key frames: at its first place; bad 8 never
    assert w.local_points([1, 0]) == [7, 3, 5, 9]            # the order is the visiting order
    assert w.local_points([3, 2, 1, 0]) == [2, 3, 5, 7, 9]   # an empty row adds nothing
    assert w.local_points([1, 1]) == [7, 3]                  # a key frame named twice: nothing the second time
    assert w.local_points([0, 1, 0, 3, 1]) == [5, 7, 9, 3, 2]
    assert w.local_points([2]) == [] and w.local_points([]) == []
    w.bad = {8, 5}
    assert w.local_points([0, 3]) == [7, 9, 2, 3]            # a bad point that is good nowhere is in no list
    w.set_row(4, [8, 8, None])
    assert w.local_points([4]) == []


def test_the_four_loops_are_one_loop():
    w = _world()
    for kfs in ([0, 1, 3], [3, 1], [2, 0]):
        want = w.local_points(kfs)
        assert w.fuse_candidates(kfs) == want and w.loop_points(kfs) == want and w.local_ba_points(kfs) == want


def test_assignments_change_the_lists():
    w = _world()
    w.assign(0, 1, 4)    # AddMapPoint into the NULL place
    w.assign(0, 0, -1)   # EraseMapPointMatch(0): 5 now first appears at idx 3
    w.assign(1, 0, 9)    # ReplaceMapPointMatch
    assert w.rows[0] == [None, 4, 7, 5, 9] and w.rows[1] == [9, 3, None, 8]
    assert w.local_points([0, 1]) == [4, 7, 5, 9, 3]
    assert w.local_points([1, 0]) == [9, 3, 4, 7, 5]


def test_tracked_map_points():
    w = _world()
    # row 0 = [5, NULL, 7, 5, 9]: four non-NULL, none bad; nObs 4, 1, 4, 2
    assert [w.tracked_points(0, m) for m in (0, 1, 2, 3, 5)] == [4, 4, 3, 2, 0]
    # row 3 = [8, 2, 3, NULL, 5]: 8 is bad (its nObs of 9 does not count); nObs 0, 3, 4
    assert [w.tracked_points(3, m) for m in (0, 1, 3, 4)] == [3, 2, 2, 1]
    assert w.tracked_points(2, 0) == 0 and w.tracked_points(2, 1) == 0
    assert w.tracked_points(0, -1) == 4   # minObs <= 0: no check (:269)
