"""CPU: hand-computed known answers of tests/obsgraph_ref.py, so that the restatement the device is compared against is
not checked only against the code under test."""
import numpy as np

import obsgraph_ref as orf


def five_keyframe_world():
    """Key frames 1..5, points:   p0 seen by 1 2 3     p1 by 1 2     p2 by 1 3 4     p3 by 2 5     p4 (bad) by 1 2 3 4 5.
    Key frame 1 holds p0 p1 p2 p4.  Its votes, itself excluded and p4 skipped: p0 -> 2, 3; p1 -> 2; p2 -> 3, 4, that is
    {2: 2, 3: 2, 4: 1}.  A frame with the same points excludes nobody: {1: 3, 2: 2, 3: 2, 4: 1}."""
    w = orf.World()
    for k in range(1, 6):
        w.add_keyframe(k, (float(k), 0.0, 0.0))
    seen = {0: [1, 2, 3], 1: [1, 2], 2: [1, 3, 4], 3: [2, 5], 4: [1, 2, 3, 4, 5]}
    for p, kfs in seen.items():
        w.add_point(p, ref=kfs[0])
        for k in kfs:
            w.add_observation(p, k, idx=10 * p + k, octave=0, stereo=False)
    w.pts[4]["bad"] = True
    return w


def test_votes_of_the_five_keyframe_world():
    w = five_keyframe_world()
    assert w.votes([0, 1, 2, 4], self_id=1) == {2: 2, 3: 2, 4: 1}
    assert w.votes([0, 1, 2, 4]) == {1: 3, 2: 2, 3: 2, 4: 1}
    assert w.votes([4]) == {} and w.votes([]) == {}
    assert w.votes([3, 3]) == {2: 2, 5: 2}  # a point named twice votes twice


def test_update_connections_known_answers():
    # nobody reaches 15: the maximum alone, and of two equal maxima the lower id (strict >)
    r = orf.update_connections({2: 2, 3: 2, 4: 1})
    assert r["ordered_id"] == [2] and r["ordered_weight"] == [2] and r["connect_id"] == [2] and r["parent_id"] == 2
    # 14 stays out, 15 is in; equal weights come out in descending id (sort ascending by (weight, id), then push_front)
    r = orf.update_connections({7: 15, 3: 14, 9: 15, 4: 20})
    assert r["ordered_id"] == [4, 9, 7] and r["ordered_weight"] == [20, 15, 15]
    assert r["connect_id"] == [4, 7, 9] and r["connect_weight"] == [20, 15, 15] and r["parent_id"] == 4
    assert orf.update_connections({})["parent_id"] == -1


def test_observation_weights_and_the_bad_flag():
    w = orf.World()
    for k in (1, 2, 3):
        w.add_keyframe(k, (0, 0, 0))
    w.add_point(0, ref=2)
    w.add_observation(0, 1, 5, 0, True)
    w.add_observation(0, 2, 6, 0, True)
    w.add_observation(0, 2, 9, 3, False)  # present: ignored
    assert w.pts[0]["nObs"] == 4 and w.pts[0]["obs"][2] == (6, 0, True)
    assert w.erase_observation(0, 3) is False and w.pts[0]["nObs"] == 4
    assert w.erase_observation(0, 2) is True  # 4 - 2 = 2 <= 2
    assert w.pts[0]["bad"] and w.pts[0]["obs"] == {} and w.pts[0]["nObs"] == 2 and w.pts[0]["ref"] == 1


def culling_world(last_point_observers):
    """Candidate 0 sees ten points at octave 0.  Points 0..8 are seen by 0 1 2 3 (nObs 4 > 3, three others at the same
    scale: redundant).  Point 9 is seen by `last_point_observers`."""
    w = orf.World()
    for k in range(5):
        w.add_keyframe(k, (0, 0, 0))
    for p in range(10):
        w.add_point(p, ref=0)
        for k in ([0, 1, 2, 3] if p < 9 else last_point_observers):
            w.add_observation(p, k, p, 0, False)
    return w, [(p, 0) for p in range(10)]


def test_culling_at_nine_and_ten_of_ten():
    w, feats = culling_world([0, 1, 2])  # nObs = 3: not > 3
    assert w.culling_counts(0, feats) == (10, 9)
    assert not orf.should_cull(10, 9)  # 9 > 0.9 * 10 is false
    assert w.keyframe_culling([(0, feats)]) == ([], [])
    w, feats = culling_world([0, 1, 2, 3])
    assert w.culling_counts(0, feats) == (10, 10) and orf.should_cull(10, 10)
    culled, bad = w.keyframe_culling([(0, feats)])
    assert culled == [0] and bad == [] and w.kfs[0]["bad"] and all(0 not in w.pts[p]["obs"] for p in range(10))


def test_culling_scale_and_own_entry():
    w = orf.World()
    for k in range(5):
        w.add_keyframe(k, (0, 0, 0))
    w.add_point(0, ref=0)
    for k, octv in ((0, 2), (1, 3), (2, 3), (3, 4)):  # the candidate sees it at 2; 3 = 2 + 1 counts, 4 does not
        w.add_observation(0, k, 0, octv, False)
    assert w.culling_counts(0, [(0, 2)]) == (1, 0)  # two qualifying observers
    w.add_observation(0, 4, 0, 0, False)
    assert w.culling_counts(0, [(0, 2)]) == (1, 1)  # three
    assert w.culling_counts(1, [(0, 3)]) == (1, 1)  # from 1 at octave 3: 0, 2, 3 (4 <= 4), 4 qualify, 1 itself is skipped


def test_normal_of_two_observers_on_the_axes():
    """P at the origin, observers at (-2, 0, 0) and (0, -4, 0): unit vectors (1, 0, 0) and (0, 1, 0), mean (0.5, 0.5, 0).
    The reference key frame is the first, at octave 1 of 1.2-spaced levels: dist = 2, max = 2 * 1.2f = 2.4f,
    min = 2.4f / 1.44f."""
    w = orf.World()
    w.add_keyframe(1, (-2, 0, 0))
    w.add_keyframe(2, (0, -4, 0))
    w.add_point(0, ref=1)
    w.add_observation(0, 1, 0, 1, False)
    w.add_observation(0, 2, 0, 0, False)
    sf = np.array([1.0, 1.2, 1.44], np.float32)
    normal, lo, hi = w.normal_depth(0, (0, 0, 0), sf)
    assert normal.dtype == np.float32 and normal.tolist() == [0.5, 0.5, 0.0]
    assert hi == np.float32(2.4) and lo == np.float32(np.float32(2.4) / np.float32(1.44)) and abs(float(lo) - 5.0 / 3.0) < 1e-6
    w.pts[0]["ref"] = 7  # a reference key frame that is not among the observers
    assert w.normal_depth(0, (0, 0, 0), sf) is None
    w.pts[0]["ref"], w.pts[0]["bad"] = 1, True
    assert w.normal_depth(0, (0, 0, 0), sf) is None


def test_local_keyframes_known_answers():
    # K1 = 1 2 3 (ascending id), reference = 2 (3 votes; 3 also has 3 but strict > keeps the first)
    counter = {3: 3, 1: 1, 2: 3}
    # 1: neighbours 2 (local), 10 -> 10; child 11; parent 2 is local.  2: neighbour 10 is local now, 12 -> 12; no child;
    # parent 20 -> appended and the loop ends: 3 is never visited
    neigh = {1: [2, 10], 2: [10, 12], 3: [30]}
    child = {1: [11], 3: [31]}
    parent = {1: 2, 2: 20, 3: 1}
    local, ref = orf.local_keyframes(counter, set(), neigh, child, parent)
    assert local == [1, 2, 3, 10, 11, 12, 20] and ref == 2
    # a bad voted key frame is no K1 member and cannot be the reference; a bad child is passed over
    local, ref = orf.local_keyframes({1: 1, 2: 9}, {2, 11}, {1: [2, 10]}, {1: [11, 13]}, {})
    assert local == [1, 10, 13] and ref == 1
    # only the best ten covisibles are read
    local, _ = orf.local_keyframes({1: 1}, set(range(100, 110)), {1: list(range(100, 111))}, {}, {})
    assert local == [1]
    # 81 voted key frames: nothing is appended; 79: the first visit makes 81 and the walk stops
    neigh = {k: [1000 + k] for k in range(81)}
    child = {k: [2000 + k] for k in range(81)}
    assert len(orf.local_keyframes({k: 1 for k in range(81)}, set(), neigh, child, {})[0]) == 81
    local, _ = orf.local_keyframes({k: 1 for k in range(79)}, set(), neigh, child, {})
    assert local[79:] == [1000, 2000] and len(local) == 81
    assert orf.local_keyframes({}, set(), {}, {}, {}) == ([], -1)
