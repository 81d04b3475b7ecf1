"""GPU: MapPoint::ComputeDistinctiveDescriptors over the device observation graph and the key frames' descriptors it holds
-- orbfe_obsgraph_distinctive_descriptors (array form) and orbfe_obsgraph_distinctive_descriptors_mappoints (table form) --
compared for EQUALITY with the restatement in tests/distinctive_ref.py: the results are integers and bytes, there is no
tolerance.  The kernel takes a wave per point, four points per workgroup, rows of up to 64 entries with one descriptor per
lane and longer rows with four: the engineered rows sit on both sides of each of these."""
import numpy as np
import pytest

import distinctive_ref as dr
import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd import _lib

pytestmark = pytest.mark.gpu
INV = _lib.ERR_INVALID


def bits(v):
    """The descriptor with the first v bits set: the distance of two of them is |v - w|."""
    return np.packbits(np.arange(256) < v).astype(np.uint8)


def near_prototypes(rng, n, flips=2):
    """n descriptors drawn from 4 prototypes with at most `flips` flipped bits each: median ties are the rule."""
    proto = rng.integers(0, 256, (4, 32), dtype=np.uint8)
    d = proto[rng.integers(0, 4, n)].copy()
    for r in range(n):
        for b in rng.integers(0, 256, int(rng.integers(0, flips + 1))):
            d[r, b // 8] ^= np.uint8(0x80 >> (b % 8))
    return d


class World:
    """A graph and, next to it, what the restatement reads: mnIds that do not ascend with the kf slot, bad flags, the key
    frames' descriptors, the points' observations."""

    def __init__(self, P, K, row_width, desc_width=64):
        self.P, self.K = P, K
        self.g = amd.ObservationGraph(P, K, row_width)
        self.g.enable_keyframe_descriptors(desc_width)
        self.kf_id = [(k * 37) % 1009 + 1 for k in range(K)]
        self.kf_bad = [False] * K
        self.kf_desc = [np.zeros((0, 32), np.uint8)] * K
        self.g.set_keyframes(list(range(K)), self.kf_id, np.zeros((K, 3), np.float32))
        self.point_bad = [True] * P  # a slot that was never set counts as bad
        self.obs = [[] for _ in range(P)]

    def descriptors(self, k, d):
        self.kf_desc[k] = np.ascontiguousarray(d, dtype=np.uint8).reshape(-1, 32)
        self.g.set_keyframe_descriptors(k, self.kf_desc[k])

    def points(self, slots, bad=None):
        slots = list(slots)
        bad = [0] * len(slots) if bad is None else bad
        self.g.set_points(slots, bad, [-1] * len(slots))
        for s, b in zip(slots, bad):
            self.point_bad[s] = bool(b)

    def observe(self, p, kfs, idx):
        kfs, idx = [int(k) for k in kfs], [int(i) for i in idx]
        self.g.add_observations([p] * len(kfs), kfs, idx, [0] * len(kfs), [0] * len(kfs))
        self.obs[p] += list(zip(kfs, idx))

    def erase(self, p, k):
        self.g.erase_observations([p], [k])
        self.obs[p] = [o for o in self.obs[p] if o[0] != k]

    def mark_bad(self, k):
        self.g.set_keyframes([k], [self.kf_id[k]], np.zeros((1, 3), np.float32), [1])
        self.kf_bad[k] = True

    def want(self, slots):
        """-> (kf, idx, desc, valid) with -1 / -1 / zeros where the reference returns early."""
        n = len(slots)
        kf, idx = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        desc, valid = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
        for i, s in enumerate(slots):
            r = dr.distinctive(self.point_bad[s], self.obs[s], self.kf_id, self.kf_bad, self.kf_desc)
            if r is not None:
                kf[i], idx[i], valid[i] = r[0], r[1], 1
                desc[i] = np.frombuffer(r[2], np.uint8)
        return kf, idx, desc, valid

    def table(self, seed=3):
        """A map-point table of the graph's size whose every slot holds something of its own."""
        rng = np.random.default_rng(seed)
        mp = amd.MapPoints(self.P)
        held = {"pos": rng.normal(0, 3, (self.P, 3)).astype(np.float32), "normal": rng.normal(0, 1, (self.P, 3)).astype(np.float32),
                "lo": rng.uniform(0.1, 1, self.P).astype(np.float32), "hi": rng.uniform(5, 9, self.P).astype(np.float32),
                "desc": rng.integers(0, 256, (self.P, 32), dtype=np.uint8), "flags": (np.arange(self.P) % 3 == 0).astype(np.uint8) * 2}
        mp.update(np.arange(self.P), held["pos"], held["normal"], held["lo"], held["hi"], held["desc"], held["flags"])
        return mp, held

    def check(self, slots, expect_valid=None):
        """Both forms on slots[] against the restatement; returns the restatement's (kf, idx, desc, valid)."""
        slots = [int(s) for s in slots]
        kf, idx, desc, valid = self.want(slots)
        if expect_valid is not None:
            assert valid.tolist() == list(expect_valid)
        got = self.g.distinctive_descriptors(slots)
        # the wrapper's outputs start as -1 / -1 / zeros: an entry with valid = 0 was not written
        for name, g_, w_ in zip(("kf", "idx", "desc", "valid"), got, (kf, idx, desc, valid)):
            assert np.array_equal(g_, w_), (name, slots)
        if len(set(slots)) == len(slots):
            mp, held = self.table()
            tkf, tidx, tvalid = mp.compute_distinctive_descriptors(self.g, slots)
            assert np.array_equal(tkf, kf) and np.array_equal(tidx, idx) and np.array_equal(tvalid, valid)
            after = held["desc"].copy()
            after[np.array(slots, np.int64)[valid == 1]] = desc[valid == 1]  # winners in valid slots, the previous bytes elsewhere
            assert np.array_equal(mp.descriptors(np.arange(self.P)), after)
            assert np.array_equal(mp.descriptors(slots), after[slots])
            assert np.array_equal(mp.positions(np.arange(self.P)), held["pos"])
            mp.close()
        return kf, idx, desc, valid

    def close(self):
        self.g.close()


def filled(P, K, row_width, lengths, seed, n_desc=None, make=near_prototypes):
    """A world whose point p has a row of lengths[p] entries: random key frames, random idx below each key frame's count."""
    rng = np.random.default_rng(seed)
    w = World(P, K, row_width)
    n_desc = [int(rng.integers(1, 65)) for _ in range(K)] if n_desc is None else n_desc
    every = make(rng, sum(n_desc))  # one set of prototypes for the whole world
    at = np.concatenate([[0], np.cumsum(n_desc)])
    for k in range(K):
        w.descriptors(k, every[at[k]:at[k + 1]])
    w.points(range(len(lengths)))
    for p, n in enumerate(lengths):
        kfs = rng.permutation(K)[:n]
        w.observe(p, kfs, [rng.integers(0, n_desc[k]) for k in kfs])
    return w


def test_row_lengths_on_both_sides_of_the_wave():
    lengths = [1, 2, 3, 4, 63, 64, 65, 100, 128, 5, 64, 65]
    w = filled(40, 130, 128, lengths, seed=1)
    kf, idx, desc, valid = w.check(range(len(lengths)), expect_valid=[1] * len(lengths))
    assert len({bytes(d) for d in desc}) > 1
    w.check([6, 0, 5, 8, 3, 7, 4])  # another order: each kernel form skips the other's points at other places
    w.check([4, 5, 10])             # no long row in the list: the one-chunk form alone
    w.check([7])
    w.close()


def test_row_width_256_full_and_one_short():
    w = filled(8, 260, 256, [255, 256, 3, 256], seed=2)
    w.check([0, 1, 2, 3], expect_valid=[1, 1, 1, 1])
    w.close()


def test_row_width_8_full():
    w = filled(12, 30, 8, [8, 8, 1, 8, 7, 8, 8, 2, 8], seed=3)
    w.check(range(9), expect_valid=[1] * 9)
    w.close()


def test_identical_and_complementary_descriptors():
    rng = np.random.default_rng(4)
    w = World(16, 12, 8)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    for k in range(12):
        w.descriptors(k, np.stack([a, ~a, bits(k), a]))
    w.points(range(8))
    w.observe(0, [3, 1, 7, 5, 9], [0, 3, 0, 3, 0])       # five times the same bytes: every median 0, the lowest mnId wins
    w.observe(1, [4, 2], [0, 1])                          # a complementary pair: distance 256, both medians 0
    w.observe(2, [4, 2, 6], [0, 1, 1])                    # a, ~a, ~a: medians 256, 0, 0
    w.observe(3, [0, 1, 2, 3, 4, 5, 6, 7], [2] * 8)       # bits(0 .. 7): a line
    kf, idx, desc, valid = w.check(range(4), expect_valid=[1, 1, 1, 1])
    first = lambda ks: min(ks, key=lambda k: w.kf_id[k])  # noqa: E731
    assert kf[0] == first([3, 1, 7, 5, 9]) and bytes(desc[0]) == bytes(a)
    assert kf[1] == first([4, 2])
    assert kf[2] == first([2, 6]) and bytes(desc[2]) == bytes(~a)
    w.close()


@pytest.mark.parametrize("seed", range(20))
def test_prototype_descriptors_twice_with_equal_bytes(seed):
    rng = np.random.default_rng(100 + seed)
    lengths = [int(n) for n in rng.integers(1, 65, 30)] + [int(rng.integers(65, 129))]
    w = filled(40, 130, 128, lengths, seed=200 + seed)
    slots = rng.permutation(len(lengths)).tolist()
    first = w.g.distinctive_descriptors(slots)
    again = w.g.distinctive_descriptors(slots)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    w.check(slots, expect_valid=[1] * len(slots))
    w.close()


def test_last_descriptor_of_a_full_store():
    """kf_desc_width = 64 with n = 64, and idx = desc_n - 1 of shorter key frames."""
    n_desc = [64, 64, 1, 17, 64, 33]
    w = filled(8, 6, 8, [], seed=6, n_desc=n_desc)
    w.points(range(3))
    w.observe(0, range(6), [n - 1 for n in n_desc])
    w.observe(1, [0, 1, 4], [63, 0, 63])
    w.observe(2, [2], [0])
    w.check([0, 1, 2], expect_valid=[1, 1, 1])
    # one past the last: refused on the host, from the mirror
    w.g.add_observations([3], [3], [17], [0], [0])
    w.g.set_points([3], [0], [-1])
    with pytest.raises(amd.OrbfeError) as ei:
        w.g.distinctive_descriptors([0, 3])
    assert ei.value.code == INV
    w.close()


def test_bad_key_frames_empty_rows_and_bad_points_in_one_list():
    w = World(24, 80, 8)
    values = [0, 1, 8, 9, 20]
    for k in range(80):
        w.descriptors(k, np.stack([bits(values[k % 5]), bits(200)]))
    w.points(range(16), bad=[int(p == 9) for p in range(16)])  # 9 is bad; 16 .. 23 are never set
    by_id = sorted(range(80), key=lambda k: w.kf_id[k])

    used = set()

    def row(p):
        """five key frames of its own, ascending in mnId, that hold 0, 1, 8, 9, 20 in that order"""
        ks = []
        for k in by_id:
            if k not in used and k % 5 == len(ks):
                ks.append(k)
                if len(ks) == 5:
                    break
        assert len(ks) == 5
        used.update(ks)
        w.observe(p, ks, [0] * 5)
        return ks

    rows = {p: row(p) for p in (0, 1, 2, 3, 5, 9)}
    w.mark_bad(rows[1][0])   # the first place of row 1
    w.mark_bad(rows[2][2])   # a middle place of row 2
    w.mark_bad(rows[3][4])   # the last place of row 3
    for k in rows[5]:
        w.mark_bad(k)        # every key frame of row 5
    # live, bad-kf rows, an empty row (4), all bad (5), a bad point with a row (9), a never-set point (20): nine entries, so the
    # dead ones fall on both sides of the four-point workgroup boundary
    slots = [0, 4, 1, 20, 2, 5, 9, 3, 6]
    kf, idx, desc, valid = w.check(slots, expect_valid=[1, 0, 1, 0, 1, 0, 0, 1, 0])
    live = {s: [k for k in rows[s] if not w.kf_bad[k]] for s in (0, 1, 2, 3)}
    # by hand: [0 1 8 9 20] -> medians 8 7 7 8 12: the 1;  [1 8 9 20] -> 7 1 1 11: the 8;  [0 1 9 20] -> 1 1 8 11: the 0;
    # [0 1 8 9] -> 1 1 1 1: the 0
    assert [int(k) for k in kf[valid == 1]] == [rows[0][1], rows[1][2], rows[2][0], rows[3][0]]
    assert all(len(v) == n for v, n in zip(live.values(), (5, 4, 4, 4)))
    w.check([5, 4, 9, 20, 6], expect_valid=[0] * 5)  # nothing valid at all
    w.close()


def test_mutations_between_calls_change_the_winner():
    w = World(8, 8, 8)
    by_id = sorted(range(8), key=lambda k: w.kf_id[k])
    A, B, C, D = by_id[:4]
    for k, v in ((A, 0), (B, 10), (C, 6), (D, 1)):
        w.descriptors(k, bits(v)[None])
    w.points([2])
    w.observe(2, [C, A, B], [0, 0, 0])
    assert w.check([2])[0][0] == B       # [0, 10, 6]: medians 6, 4, 4
    w.observe(2, [D], [0])
    assert w.check([2])[0][0] == A       # [0, 10, 6, 1]: medians 1, 4, 4, 1
    w.erase(2, A)
    assert w.check([2])[0][0] == B       # [10, 6, 1]: medians 4, 4, 5
    w.mark_bad(B)
    assert w.check([2])[0][0] == C       # [6, 1]: the first
    w.close()


def test_descriptors_from_a_resident_frame_equal_the_ones_from_the_host():
    rng = np.random.default_rng(7)
    n = 50
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    view = amd.FrameView(rng.uniform(0, 600, n).astype(np.float32), rng.uniform(0, 400, n).astype(np.float32), np.zeros(n, np.int32), desc,
                         (0.0, 640.0, 0.0, 480.0))
    w = World(8, 4, 8)
    frame = amd.ResidentFrame(view)
    w.g.set_keyframe_descriptors(1, frame)
    frame.close()  # released before anything reads the store
    w.kf_desc[1] = desc
    w.descriptors(2, desc)
    w.descriptors(3, desc[::-1])
    assert np.array_equal(w.g.get_keyframe_descriptors(1), desc) and np.array_equal(w.g.get_keyframe_descriptors(2), desc)
    assert np.array_equal(w.g.get_keyframe_descriptors(3), desc[::-1]) and len(w.g.get_keyframe_descriptors(0)) == 0
    w.points([0, 1])
    w.observe(0, [1, 2, 3], [49, 49, 0])
    w.observe(1, [1, 3], [7, 20])
    kf, idx, got, valid = w.check([0, 1], expect_valid=[1, 1])
    assert bytes(got[0]) == bytes(desc[49])
    # a frame with more features than the store is wide is refused
    big = amd.ResidentFrame(amd.FrameView(np.zeros(65, np.float32), np.zeros(65, np.float32), np.zeros(65, np.int32),
                                          np.zeros((65, 32), np.uint8), (0.0, 640.0, 0.0, 480.0)))
    with pytest.raises(amd.OrbfeError) as ei:
        w.g.set_keyframe_descriptors(0, big)
    assert ei.value.code == INV
    big.close()
    w.g.clear()  # every count back to 0, the slab stays
    assert len(w.g.get_keyframe_descriptors(1)) == 0
    w.close()


def test_the_table_is_unchanged_after_a_refused_call_and_keeps_everything_but_the_descriptor():
    import frustum_ref as fr
    from orb_slam2_annotate_amd.map_points import camera_pose
    w = filled(40, 30, 8, [3, 4, 5, 1, 8, 2], seed=8)
    mp, held = w.table()
    everything = np.arange(w.P)
    pose = camera_pose(np.eye(3), np.zeros(3), (fr.FX, fr.FY, fr.CX, fr.CY), fr.MBF, fr.BOUNDS, fr.SCALE, fr.LEVELS)
    before = mp.ProjectInFrustum(everything, pose, -2.0)
    # a slot named twice; an idx that is not below its key frame's count
    with pytest.raises(amd.OrbfeError) as ei:
        mp.compute_distinctive_descriptors(w.g, [0, 1, 0])
    assert ei.value.code == INV
    w.g.set_points([6], [0], [-1])
    w.g.add_observations([6], [0], [64], [0], [0])
    with pytest.raises(amd.OrbfeError) as ei:
        mp.compute_distinctive_descriptors(w.g, [0, 1, 6])
    assert ei.value.code == INV
    assert np.array_equal(mp.descriptors(everything), held["desc"]) and np.array_equal(mp.positions(everything), held["pos"])
    kf, idx, valid = mp.compute_distinctive_descriptors(w.g, [0, 1, 2, 3, 4, 5, 7])
    assert valid.tolist() == [1] * 6 + [0]
    assert not np.array_equal(mp.descriptors(everything), held["desc"])
    after = mp.ProjectInFrustum(everything, pose, -2.0)
    for name in before:  # position, normal, distance range and flags are what isInFrustum reads
        assert np.array_equal(before[name], after[name]), name
    assert np.array_equal(mp.positions(everything), held["pos"])
    # a graph larger than the table, and a table on its own
    small = amd.MapPoints(w.P - 1)
    with pytest.raises(amd.OrbfeError) as ei:
        small.compute_distinctive_descriptors(w.g, [0])
    assert ei.value.code == INV
    small.close()
    mp.close()
    w.close()


def test_search_local_points_after_the_resident_call_equals_the_array_path():
    """The descriptor in the table is what SearchLocalPoints matches against: the resident call and the path a caller had
    before it (gathered lists, orbfe_distinctive_descriptors, orbfe_mappoints_update) leave tables that match alike."""
    import frustum_ref as fr
    from test_gpu_frustum import SF, _frame_for, _pose
    n, P, K = 250, 300, 40
    sc = fr.scene(3, n)
    rng = np.random.default_rng(9)
    slot = rng.permutation(P)[:n].astype(np.int32)
    w = World(P, K, 8, desc_width=128)
    seen = [[] for _ in range(K)]  # per key frame: (point, descriptor)
    rows = []
    for p in range(n):
        kfs = rng.permutation(K)[:int(rng.integers(1, 8))]
        for k in kfs:
            noise = np.packbits(rng.random(256) < 0.04)
            seen[k].append(sc["desc"][p] ^ noise)
        rows.append([(int(k), len(seen[k]) - 1) for k in kfs])
    for k in range(K):
        w.descriptors(k, np.stack(seen[k]))
    w.points(slot.tolist())
    for p in range(n):
        w.observe(int(slot[p]), [k for k, _ in rows[p]], [i for _, i in rows[p]])
    zeros = np.zeros((n, 32), np.uint8)
    resident, arrays = amd.MapPoints(P), amd.MapPoints(P)
    for mp in (resident, arrays):
        mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], zeros, sc["flags"])
    kf, idx, valid = resident.compute_distinctive_descriptors(w.g, slot)
    assert valid.all()
    # the array path: the lists in the graph's order, the winners written through update()
    lists, order = [], []
    for p in range(n):
        o = sorted(rows[p], key=lambda e: w.kf_id[e[0]])
        order.append(o)
        lists.append(np.stack([w.kf_desc[k][i] for k, i in o]))
    best = amd.ComputeDistinctiveDescriptors(lists)
    winners = np.stack([lists[p][int(best[p])] for p in range(n)])
    assert [order[p][int(best[p])] for p in range(n)] == list(zip(kf.tolist(), idx.tolist()))
    arrays.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], winners, sc["flags"])
    assert np.array_equal(resident.descriptors(slot), winners) and np.array_equal(arrays.descriptors(slot), winners)
    F, _ = _frame_for(sc, fr.spec32(sc, np.zeros(n, np.uint8)), True, seed=12)
    pose = _pose(sc)
    n_r, m_r, iv_r = resident.SearchLocalPoints(F, slot, pose, SF, th=3.0, nnratio=0.8, viewing_cos_limit=fr.LIMIT)
    n_a, m_a, iv_a = arrays.SearchLocalPoints(F, slot, pose, SF, th=3.0, nnratio=0.8, viewing_cos_limit=fr.LIMIT)
    assert n_r == n_a and n_r >= 5
    assert np.array_equal(m_r, m_a) and np.array_equal(iv_r, iv_a)
    resident.close()
    arrays.close()
    w.close()
