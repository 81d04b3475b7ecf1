"""GPU: the key-frame rows of the device observation graph -- orbfe_obsgraph_keyframe_points_union (the ordered union of
Tracking::UpdateLocalPoints and its three siblings) and orbfe_obsgraph_tracked_points (KeyFrame::TrackedMapPoints) -- compared
for equality with the restatement in tests/kfpoints_ref.py.  Position p = k * kf_row_width + idx; the union's grid works in
blocks of 1024 positions and waves of 64, which is what the engineered rows straddle."""
import numpy as np
import pytest

import kfpoints_ref as kr
import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd import _lib

pytestmark = pytest.mark.gpu


def build(P, K, W, rows, bad=(), unset=(), row_width=8):
    """-> (graph, restatement) holding rows = {kf slot: [point slot or -1, ...]}; every point slot outside `unset` is given to
    set_points, the ones in `bad` as bad.  The restatement counts a slot that was never set as bad, as the graph does."""
    g = amd.ObservationGraph(P, K, row_width)
    kfs = sorted(rows)
    g.set_keyframes(kfs, [1000 + 7 * k for k in kfs], np.zeros((len(kfs), 3), np.float32))
    used = sorted({s for r in rows.values() for s in r if s >= 0} - set(unset))
    if used:
        g.set_points(used, [int(s in bad) for s in used], [-1] * len(used))
    g.enable_keyframe_points(W)
    w = kr.KeyFramePoints()
    w.bad = set(bad) | set(unset)
    for k in kfs:
        g.set_keyframe_points(k, rows[k])
        w.set_row(k, rows[k])
    return g, w


def lists(arrays):
    return [a.tolist() for a in arrays]


A, B, C, TWICE, BAD, UNSET = 100, 101, 102, 103, 104, 105


@pytest.fixture(scope="module")
def engineered():
    rng = np.random.default_rng(1)
    rows = {k: rng.integers(200, 512, 48).tolist() for k in range(20)}
    rows[0] = rows[0] + [-1] * 15 + [B]      # p = 63: the last lane of a wave ...
    rows[1] = [B] + rows[1]                   # ... and p = 64, the first lane of the next
    rows[3] = rows[3] + [-1] * 15 + [C]      # p = 255 | 256: the last chunk of one wave, the first of the next
    rows[4] = [C] + rows[4]
    rows[5] = [-1] * 40                       # all NULL
    rows[6] = []                              # n = 0
    rows[7] = rng.integers(200, 512, 64).tolist()  # n = kf_row_width
    rows[8][3] = rows[8][9] = TWICE           # one slot at two idx of one row
    rows[9][0], rows[9][1] = BAD, UNSET
    rows[10][5], rows[11][2] = BAD, UNSET
    rows[15] = rows[15] + [-1] * 15 + [A]    # p = 1023: the last entry of the first 1024-entry block ...
    rows[16] = [A] + rows[16]                 # ... and p = 1024, the first entry of the next
    g, w = build(512, 20, 64, rows, bad={BAD}, unset={UNSET})
    return g, w


def test_engineered_rows_one_query(engineered):
    g, w = engineered
    q = list(range(20))
    want = w.local_points(q)
    got = g.local_points(q).tolist()
    assert got == want
    for s in (A, B, C, TWICE):
        assert got.count(s) == 1
    assert BAD not in got and UNSET not in got
    twice = q + [2, 16, 15]  # kf slots named twice add nothing
    assert g.local_points(twice).tolist() == want
    back = q[::-1]  # the repeats now come first: A, B, C are taken from rows 16, 1, 4
    assert g.local_points(back).tolist() == w.local_points(back)
    for single in ([5], [6], [7], [8], [16, 15], [5, 6]):
        assert g.local_points(single).tolist() == w.local_points(single), single
    assert g.local_points([5]).tolist() == [] and g.local_points([6]).tolist() == []


def test_empty_queries_and_no_queries(engineered):
    g, w = engineered
    assert g.keyframe_points_union([]) == []
    assert lists(g.keyframe_points_union([[]])) == [[]]
    qs = [[], [15, 16], [], [6], list(range(20)), []]
    assert lists(g.keyframe_points_union(qs)) == [w.local_points(q) for q in qs]


def test_capacity_exact_and_one_short(engineered):
    g, w = engineered
    qs = [[15, 16], list(range(20)), [7]]
    want = [w.local_points(q) for q in qs]
    n = max(len(x) for x in want)
    assert len(want[1]) == n
    assert lists(g.keyframe_points_union(qs, capacity=n)) == want
    with pytest.raises(amd.OrbfeError) as ei:
        g.keyframe_points_union(qs, capacity=n - 1)
    assert ei.value.code == _lib.ERR_CAPACITY
    assert ei.value.count.tolist() == [len(x) for x in want]  # every count is set
    assert lists(ei.value.partial) == [x[:n - 1] for x in want]  # the first `capacity` entries: the reference's prefix
    assert lists(g.keyframe_points_union(qs, capacity=n)) == want  # and the handle works on


def test_queries_that_share_key_frames_and_points_do_not_interfere(engineered):
    g, w = engineered
    qs = [list(range(20)), list(range(19, -1, -1)), [15, 16], [16, 15], [0, 1, 3, 4, 8], [8, 4, 3, 1, 0, 8], [1], [1]]
    together = lists(g.keyframe_points_union(qs))
    assert together == [w.local_points(q) for q in qs]
    assert together == [g.local_points(q).tolist() for q in qs]


def test_the_workspace_bound_splits_the_queries_into_groups():
    # point_capacity 2^20 int32 per query against a bound of 2^26: 64 queries per group, so 80 need two
    P, K = 1 << 20, 80
    rng = np.random.default_rng(2)
    pool = np.concatenate([rng.choice(P, 300, replace=False), [0, P - 1]]).astype(np.int64)
    rows = {k: rng.choice(pool, 64).tolist() for k in range(K)}
    rows[70][10] = rows[70][20] = P - 1
    bad = set(pool[:40].tolist())
    g, w = build(P, K, 64, rows, bad=bad)
    qs = [[k] for k in range(K)]
    got = lists(g.keyframe_points_union(qs))
    assert got == [w.local_points(q) for q in qs]
    assert got[70].count(P - 1) == 1
    # 64 lists of 1024 entries are more than come back in one copy: the counts first, then the filled part
    assert lists(g.keyframe_points_union(qs, capacity=1024)) == got
    g.close()


@pytest.mark.parametrize("seed", range(20))
def test_randomised_unions_equal_the_restatement(seed):
    rng = np.random.default_rng(100 + seed)
    K, W, P = 40, 128, 3000
    pool = rng.choice(P, 400, replace=False)  # 40 rows of up to 128 over 400 slots: every point is in many key frames
    rows = {}
    for k in range(K):
        n = int(rng.integers(int(0.3 * W), W + 1))
        r = rng.choice(pool, n)
        r[rng.random(n) < 0.1] = -1
        rows[k] = r.tolist()
    flags = rng.random(P)
    bad = set(np.flatnonzero(flags < 0.15).tolist())
    unset = set(np.flatnonzero((flags >= 0.15) & (flags < 0.30)).tolist())
    g, w = build(P, K, W, rows, bad=bad, unset=unset)
    qs = [rng.permutation(K)[:int(rng.integers(1, K + 1))].tolist() for _ in range(6)] + [rng.permutation(K).tolist(), [int(rng.integers(K))]]
    got = g.keyframe_points_union(qs)
    want = [w.local_points(q) for q in qs]
    assert lists(got) == want
    assert sum(len(x) for x in want) > 200 and not (set(want[6]) & (bad | unset))
    again = g.keyframe_points_union(qs)
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    g.close()


def test_mutations_between_calls():
    rng = np.random.default_rng(3)
    K, W, P = 6, 64, 200
    rows = {k: rng.integers(0, 120, 50).tolist() for k in range(K)}
    g, w = build(P, K, W, rows)
    g.set_points(list(range(120)), [0] * 120, [-1] * 120)  # every slot the rows may come to name; 150 and 151 stay unset
    q = [3, 0, 5, 1, 4, 2]

    def same():
        for k in range(K):
            on_device = g.get_keyframe_points(k, from_device=True).tolist()
            assert on_device == g.get_keyframe_points(k).tolist() == [-1 if s is None else s for s in w.rows[k]]
        assert g.local_points(q).tolist() == w.local_points(q)
        assert g.local_points(q[::-1]).tolist() == w.local_points(q[::-1])

    same()
    # assign: AddMapPoint into an erased place, ReplaceMapPointMatch, EraseMapPointMatch(idx)
    first = w.local_points(q)[0]
    w.bad |= {150, 151}  # never given to set_points
    for kf, idx, slot in ((3, 0, -1), (3, 0, 150), (0, 7, 151), (5, 49, first), (1, 20, -1), (1, 21, -1)):
        g.assign_keyframe_points([kf], [idx], [slot])
        w.assign(kf, idx, slot)
    same()  # 150 and 151 were never given to set_points: they are in no list
    assert 150 not in g.local_points(q).tolist()
    g.set_points([150, 151], [0, 0], [-1, -1])
    w.bad -= {150, 151}
    same()
    assert g.local_points(q).tolist()[0] == 150
    # set_points flips the bad flag
    victims = w.local_points(q)[1:4]
    g.set_points(victims, [1] * 3, [-1] * 3)
    w.bad |= set(victims)
    same()
    g.set_points(victims[:1], [0], [-1])
    w.bad -= set(victims[:1])
    same()
    # erase_observations makes a point bad: three mono observations, one erased -> nObs 2
    p = w.local_points(q)[5]
    g.add_observations([p] * 3, [0, 1, 2], [0, 0, 0], [0, 0, 0], [0, 0, 0])
    same()
    assert g.erase_observations([p], [1]).tolist() == [1]
    w.bad.add(p)
    same()
    # a whole row again, shorter and longer
    for kf, n in ((2, 5), (4, 64), (0, 0)):
        r = rng.integers(-1, 120, n).tolist()
        g.set_keyframe_points(kf, r)
        w.set_row(kf, r)
    same()
    g.clear()
    assert g.get_keyframe_points(2, from_device=True).tolist() == []
    g.close()


def test_tracked_points():
    K, W, P = 5, 64, 40
    g = amd.ObservationGraph(P, K, 8)
    g.set_keyframes(list(range(K)), [10 + k for k in range(K)], np.zeros((K, 3), np.float32))
    pts = list(range(30))  # 30 .. 39 are never set
    bad = {4, 11, 17}
    g.set_points(pts, [int(p in bad) for p in pts], [-1] * 30)
    w = kr.KeyFramePoints()
    w.bad = bad | set(range(30, 40))
    for p in pts:  # point p is seen by p % 4 key frames, the first of them in stereo when p % 8 >= 4: nObs 0 .. 4
        seen = list(range(p % 4))
        stereo = [int(p % 8 >= 4 and k == 0) for k in seen]
        if seen:
            g.add_observations([p] * len(seen), seen, [p] * len(seen), [0] * len(seen), stereo)
        w.n_obs[p] = len(seen) + sum(stereo)
    assert sorted(set(w.n_obs.values())) == [0, 1, 2, 3, 4]
    g.enable_keyframe_points(W)
    rng = np.random.default_rng(4)
    rows = {0: rng.integers(-1, 40, 64).tolist(), 1: rng.integers(-1, 40, 37).tolist(), 2: [], 3: [-1] * 10, 4: [4, 11, 17, 35, 3, 3, 7]}
    for k, r in rows.items():
        g.set_keyframe_points(k, r)
        w.set_row(k, r)
    for min_obs in (0, 1, 3):
        want = [w.tracked_points(k, min_obs) for k in range(K)]
        assert g.tracked_points(list(range(K)), min_obs).tolist() == want, min_obs
        assert g.tracked_points([4, 1, 4], min_obs).tolist() == [want[4], want[1], want[4]]
    assert [w.tracked_points(4, m) for m in (0, 1, 3)] == [3, 3, 3] and w.n_obs[3] == 3 and w.n_obs[7] == 4
    assert g.tracked_points([0], 0)[0] > g.tracked_points([0], 3)[0] > 0
    g.close()


def test_local_points_feed_search_local_points():
    """The chain of Tracking::TrackLocalMap: the union's list is, unchanged, the slot list of SearchLocalPoints."""
    import frustum_ref as fr
    from test_gpu_frustum import SF, _frame_for, _pose, _slots, _table
    sc = fr.scene(2, 2000)
    slot = _slots(2000, 3)
    mp = _table(sc, slot)
    rng = np.random.default_rng(5)
    K, W = 12, 512
    rows = {}
    for k in range(K):  # each key frame sees a window of the map, overlapping its neighbours
        r = slot[(np.arange(400) * 3 + 151 * k) % 2000].astype(np.int64)
        r[rng.random(400) < 0.1] = -1
        rows[k] = r.tolist()
    flags_bad = set(slot[(sc["flags"] & 1) != 0].tolist())
    g, w = build(4096, K, W, rows, bad=flags_bad)
    kfs = rng.permutation(K).tolist()
    got, want = g.local_points(kfs), np.array(w.local_points(kfs), np.int32)
    assert np.array_equal(got, want) and len(want) > 500
    F, _ = _frame_for(sc, fr.spec32(sc, np.zeros(2000, np.uint8)), True, seed=12)
    pose = _pose(sc)
    n_got, m_got, iv_got = mp.SearchLocalPoints(F, got, pose, SF, th=3.0, nnratio=0.8, viewing_cos_limit=fr.LIMIT)
    n_want, m_want, iv_want = mp.SearchLocalPoints(F, want, pose, SF, th=3.0, nnratio=0.8, viewing_cos_limit=fr.LIMIT)
    assert n_got == n_want and n_got > 100
    assert np.array_equal(m_got, m_want) and np.array_equal(iv_got, iv_want)
    mp.close()
    g.close()


def test_a_larger_call_between_two_equal_small_ones_on_one_handle():
    """The handle's workspace and pinned block grow with the largest call: a small union, then one far larger than anything
    the handle has staged (64 lists of 3000 entries come back in two copies), then the small one again."""
    rng = np.random.default_rng(6)
    K, W, P = 40, 128, 3000
    pool = rng.choice(P, 400, replace=False)
    rows = {k: rng.choice(pool, int(rng.integers(40, W + 1))).tolist() for k in range(K)}
    g, w = build(P, K, W, rows, bad=set(pool[:30].tolist()))
    small = [[3, 1, 2]]
    first = lists(g.keyframe_points_union(small, capacity=400))
    assert first == [w.local_points(small[0])] and len(first[0]) > 50
    large = [rng.permutation(K)[:int(rng.integers(1, K + 1))].tolist() for _ in range(64)]
    assert lists(g.keyframe_points_union(large, capacity=P)) == [w.local_points(q) for q in large]
    assert g.tracked_points(list(range(K)), 0).tolist() == [w.tracked_points(k, 0) for k in range(K)]
    assert lists(g.keyframe_points_union(small, capacity=400)) == first
    g.close()


def test_a_flush_of_more_key_frame_rows_than_one_chunk_holds():
    """kf_row_width 2048: a marked non-empty row is staged as 8 KiB and 12 bytes, so one 8 MiB chunk holds 1022 of them
    and 1100 need two stagings.  The rows on both sides of the chunk boundary and the last one must have arrived."""
    K, W, P = 1100, 2048, 600
    rng = np.random.default_rng(7)
    rows = {k: rng.integers(-1, P, int(rng.integers(1, 6))).tolist() for k in range(K)}
    g, w = build(P, K, W, rows, bad=set(range(0, P, 11)))
    per_chunk = (8 << 20) // (12 + W * 4)
    assert per_chunk < K <= 2 * per_chunk
    q = [K - 1, per_chunk, per_chunk - 1, 0, 500]
    assert g.local_points(q).tolist() == w.local_points(q)  # the first call that reads the rows: the flush
    for k in [0, 1, per_chunk - 2, per_chunk - 1, per_chunk, per_chunk + 1, K - 1] + list(range(5, K, 83)):
        assert g.get_keyframe_points(k, from_device=True).tolist() == rows[k], k
    everything = list(range(K))
    assert g.local_points(everything).tolist() == w.local_points(everything)
    g.close()
