"""GPU: the device observation graph (orbfe_obsgraph) against tests/obsgraph_ref.py on a row_width = 8 graph with 12 key
frames in a kf_capacity of 70 (no multiple of 64; one key frame in slot 69) and 300 point slots.  Votes and culling counts are
integers and must be exactly the restatement's; normal / min / max are bit-equal (sqrt, / and * are correctly rounded on
both sides); the table form must leave an orbfe_mappoints table as the array form's results written by hand would."""
import numpy as np
import pytest

import obsgraph_ref as orf
import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd import _lib

pytestmark = pytest.mark.gpu

N_PTS, KF_CAP, RW, N_LEVELS = 300, 70, 8, 8
KF_SLOTS = list(range(11)) + [69]
SF = (np.float32(1.2) ** np.arange(N_LEVELS)).astype(np.float32)


def make_world(seed=11):
    rng = np.random.default_rng(seed)
    ids = rng.permutation(np.arange(40, 52)).tolist()  # slot order is not id order
    kf_slot_of = dict(zip(ids, KF_SLOTS))
    w = orf.World()
    for k in ids:
        w.add_keyframe(k, rng.uniform(-1, 1, 3).astype(np.float32))
    for p in range(N_PTS):
        n = [1, 2, 8][p] if p < 3 else int(rng.integers(1, 9))
        obs = rng.choice(ids, size=n, replace=False).tolist()
        w.add_point(p, ref=obs[int(rng.integers(n))], bad=(p % 10 == 9))
        for k in obs:
            w.add_observation(p, k, int(rng.integers(0, 2000)), int(rng.integers(0, N_LEVELS)), bool(rng.integers(2)))
    # engineered: reference at level 0 / at the top level / absent from the row; an empty row
    k3, k4 = sorted(w.pts[3]["obs"])[0], sorted(w.pts[4]["obs"])[0]
    w.pts[3]["ref"], w.pts[3]["obs"][k3] = k3, (1, 0, w.pts[3]["obs"][k3][2])
    w.pts[4]["ref"], w.pts[4]["obs"][k4] = k4, (1, N_LEVELS - 1, w.pts[4]["obs"][k4][2])
    w.pts[5]["ref"] = next(k for k in ids if k not in w.pts[5]["obs"])  # (a row holds 8 of the 12 at the most)
    w.pts[6]["obs"], w.pts[6]["nObs"] = {}, 0
    pos = np.stack([rng.uniform(-1, 1, N_PTS), rng.uniform(-1, 1, N_PTS), rng.uniform(4, 10, N_PTS)], 1).astype(np.float32)
    return w, kf_slot_of, pos


@pytest.fixture(scope="module")
def env():
    w, kf_slot_of, pos = make_world()
    g = amd.ObservationGraph(N_PTS, KF_CAP, RW)
    orf.load(w, g, kf_slot_of, {p: p for p in range(N_PTS)})
    return w, kf_slot_of, pos, g


def as_counter(kf_slots, weights, kf_slot_of):
    id_of = {s: k for k, s in kf_slot_of.items()}
    assert np.all(np.diff(kf_slots) > 0), "kf slots must ascend"
    return {id_of[s]: int(v) for s, v in zip(kf_slots.tolist(), weights.tolist())}


def test_votes_equal_the_restatement(env):
    w, kf_slot_of, _, g = env
    rng = np.random.default_rng(2)
    bad = [p for p in range(N_PTS) if w.pts[p]["bad"]]
    full = next(p for p in range(N_PTS) if len(w.pts[p]["obs"]) == RW and not w.pts[p]["bad"])
    in69 = next(k for k, s in kf_slot_of.items() if s == 69)
    sees69 = [p for p in range(N_PTS) if in69 in w.pts[p]["obs"] and not w.pts[p]["bad"]]
    assert sees69
    queries = [[], bad, [7], [full], sees69, [8, 8, 12, 8]] + [rng.integers(0, N_PTS, n).tolist() for n in (1, 63, 64, 65, 257)]
    for q in queries:
        for me in (None, in69, next(iter(kf_slot_of))):
            (kf, wt), = g.votes([q], [-1 if me is None else kf_slot_of[me]])
            assert as_counter(kf, wt, kf_slot_of) == w.votes(q, me), (len(q), me)
    assert len(g.votes([bad])[0][0]) == 0 and len(g.votes([[]])[0][0]) == 0
    assert in69 in as_counter(*g.votes([sees69])[0], kf_slot_of)
    # three queries of different lengths in one call against the same three alone
    me = [kf_slot_of[in69], -1, 3]
    together = g.votes([queries[-1], queries[2], queries[-3]], me)
    for (kf, wt), q, m in zip(together, [queries[-1], queries[2], queries[-3]], me):
        (kf1, wt1), = g.votes([q], [m])
        assert np.array_equal(kf, kf1) and np.array_equal(wt, wt1)
    # capacity one short of the count: ORBFE_ERR_CAPACITY, the counts right, `capacity` entries filled
    (kf, wt), = g.votes([queries[-1]])
    with pytest.raises(amd.OrbfeError) as ei:
        g.votes([queries[-1], [7]], capacity=len(kf) - 1)
    assert ei.value.code == _lib.ERR_CAPACITY and ei.value.count.tolist() == [len(kf), len(g.votes([[7]])[0][0])]
    assert np.array_equal(ei.value.partial[0][0], kf[:-1]) and np.array_equal(ei.value.partial[0][1], wt[:-1])


@pytest.mark.parametrize("kf_capacity", [8192, 8193])
def test_votes_on_both_sides_of_the_lds_bound(kf_capacity):
    """kf_capacity 8192 keeps the counters in LDS, 8193 in the workspace slice: the same world, a key frame in the last
    slot, two queries in one call (each its own slice)."""
    w, kf_slot_of, _ = make_world(seed=31)
    last = next(k for k, s in kf_slot_of.items() if s == 69)
    kf_slot_of[last] = kf_capacity - 1
    g = amd.ObservationGraph(N_PTS, kf_capacity, RW)
    orf.load(w, g, kf_slot_of, {p: p for p in range(N_PTS)})
    qa, qb = list(range(N_PTS)), list(range(0, N_PTS, 7))
    (ka, wa), (kb, wb) = g.votes([qa, qb], [-1, kf_slot_of[last]])
    assert as_counter(ka, wa, kf_slot_of) == w.votes(qa) and ka[-1] == kf_capacity - 1
    assert as_counter(kb, wb, kf_slot_of) == w.votes(qb, last)
    again = g.votes([qa, qb], [-1, kf_slot_of[last]])
    assert np.array_equal(again[0][0], ka) and np.array_equal(again[0][1], wa) and np.array_equal(again[1][1], wb)


def test_update_connections_and_local_keyframes_on_device_votes(env):
    w, kf_slot_of, _, g = env
    q = list(range(0, 200))
    me = next(iter(kf_slot_of))
    got = g.update_connections(kf_slot_of[me], q)
    want = orf.update_connections(w.votes(q, me))
    assert got["ordered_id"].tolist() == want["ordered_id"] and got["ordered_weight"].tolist() == want["ordered_weight"]
    assert got["parent_id"] == want["parent_id"] and got["counter"] == w.votes(q, me)
    ids = sorted(kf_slot_of)
    neigh = {k: [j for j in ids if j != k][:3] + [900 + k] for k in ids}
    local, ref = g.local_keyframes([0, 1, 2], neigh, {ids[0]: [800]}, {k: 700 for k in ids}, bad={ids[1]})
    assert (local.tolist(), ref) == orf.local_keyframes(w.votes([0, 1, 2]), {ids[1]}, neigh, {ids[0]: [800]}, {k: 700 for k in ids})


def culling_world():
    """Candidate 0 (and 1) with engineered points; every key frame at the origin.  kf ids = slots."""
    w = orf.World()
    for k in range(12):
        w.add_keyframe(k, (0, 0, 0))
    cases = {  # point: [(kf, octave, stereo)]; the candidate 0 sees each at octave 2
        0: [(0, 2, 0), (1, 0, 0), (2, 0, 0)],                          # nObs = 3 by mono weight: not > 3
        1: [(0, 2, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)],               # nObs = 4, three others
        2: [(0, 2, 1), (1, 0, 0)],                                     # nObs = 3 by stereo weight
        3: [(0, 2, 1), (1, 0, 1)],                                     # nObs = 4 by stereo weight, one other
        4: [(0, 2, 0), (1, 3, 0), (2, 3, 0), (3, 3, 0)],               # three at octave + 1
        5: [(0, 2, 0), (1, 3, 0), (2, 3, 0), (3, 4, 0)],               # one at octave + 2: two qualify
        6: [(0, 2, 0), (1, 1, 0), (2, 1, 0), (3, 7, 0), (4, 1, 0)],    # exactly three of four
        7: [(0, 0, 0), (1, 0, 0), (2, 0, 0)] + [(k, 9, 0) for k in (3, 4, 5, 6, 7)],  # a full row; own entry would be the third
        8: [(0, 2, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)],               # bad
        9: [(1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0)],               # not seen by the candidate at all
    }
    for p, obs in cases.items():
        w.add_point(p, ref=obs[0][0], bad=(p == 8))
        for k, o, s in obs:
            w.add_observation(p, k, p, o, bool(s))
    return w


def test_culling_counts_equal_the_restatement():
    w = culling_world()
    g = amd.ObservationGraph(64, KF_CAP, RW)
    ident = {k: k for k in range(12)}
    orf.load(w, g, ident, {p: p for p in w.pts})
    feats0 = [(p, 2) for p in range(10)]
    feats1 = [(p, 0) for p in (1, 4, 6, 7, 9, 9)]
    nm, nr = g.culling_counts([0, 1, 5], [tuple(zip(*feats0)), tuple(zip(*feats1)), ([], [])])
    want = [w.culling_counts(0, feats0), w.culling_counts(1, feats1), (0, 0)]
    assert list(zip(nm.tolist(), nr.tolist())) == want
    assert want[0] == (9, 4)  # points 1, 4, 6 and 9 are redundant for candidate 0; 7 is not (its own entry does not count)
    for p, level in feats0:  # and each alone
        nm, nr = g.culling_counts([0], [([p], [level])])
        assert (int(nm[0]), int(nr[0])) == w.culling_counts(0, [(p, level)]), p


def test_keyframe_culling_replays_the_order_dependence():
    """Candidates A = 1 and B = 2.  X (point 0) is seen by A, B and 3 (nObs 3).  A also sees ten points that 3 4 5 see too:
    11 points, 10 redundant, 10 > 9.9: culled.  That takes X to nObs 2: bad.  B also sees nine points that 3 4 5 see:
    with X 10 points, 9 redundant, 9 > 9.0 is false; without X 9 of 9: culled -- only because A went first."""
    w = orf.World()
    for k in range(6):
        w.add_keyframe(k, (0, 0, 0))
    w.add_point(0, ref=1)
    for k in (1, 2, 3):
        w.add_observation(0, k, 0, 0, False)
    for p in range(1, 20):
        w.add_point(p, ref=3)
        for k in ([1] if p <= 10 else [2]) + [3, 4, 5]:
            w.add_observation(p, k, p, 0, False)
    fa = [(p, 0) for p in range(0, 11)]
    fb = [(0, 0)] + [(p, 0) for p in range(11, 20)]
    assert w.culling_counts(1, fa) == (11, 10) and w.culling_counts(2, fb) == (10, 9)
    g = amd.ObservationGraph(64, KF_CAP, RW)
    orf.load(w, g, {k: k for k in range(6)}, {p: p for p in w.pts})
    culled, bad = g.keyframe_culling([4, 1, 2], [([], []), tuple(zip(*fa)), tuple(zip(*fb))])
    assert (culled, bad) == w.keyframe_culling([(4, []), (1, fa), (2, fb)]) == ([1, 2], [0])
    for p in w.pts:  # the device table is the mirror is the restatement
        for dev in (False, True):
            r = g.get_row(p, from_device=dev)
            ent, nobs, isbad, ref = orf.mirror_row(w, p, {k: k for k in range(6)})
            assert [tuple(int(v) for v in e) for e in r["entries"]] == ent and (r["n_obs"], r["bad"]) == (nobs, isbad), (p, dev)


def test_normal_and_depth_are_bit_equal_to_the_restatement(env):
    w, _, pos, g = env
    slots = np.arange(N_PTS)
    normal, lo, hi, valid = g.update_normal_depth(slots, SF, pos)
    want = [w.normal_depth(p, pos[p], SF) for p in range(N_PTS)]
    assert valid.tolist() == [int(x is not None) for x in want]
    assert not valid[5] and not valid[6] and not valid[9] and valid[0] and valid[1] and valid[2] and valid[3] and valid[4]
    for p in range(N_PTS):
        if want[p] is None:  # outputs untouched
            assert not normal[p].any() and lo[p] == 0 and hi[p] == 0
            continue
        assert np.array_equal(normal[p].view(np.uint32), want[p][0].view(np.uint32)), p
        assert lo[p].view(np.uint32) == want[p][1].view(np.uint32) and hi[p].view(np.uint32) == want[p][2].view(np.uint32), p


def test_the_table_form_leaves_the_table_as_the_array_form_would(env):
    w, _, pos, g = env
    n = N_PTS
    base = dict(normal=np.tile(np.float32([0, 0, 1]), (n, 1)), min_dist=np.full(n, 0.1, np.float32), max_dist=np.full(n, 100, np.float32))
    desc, flags = np.zeros((n, 32), np.uint8), np.zeros(n, np.uint8)
    touched = np.arange(0, n, 2, dtype=np.int32)  # the odd slots stay as they are
    normal, lo, hi, valid = g.update_normal_depth(touched, SF, pos[touched])
    mp, mp_want = amd.MapPoints(n + 20), amd.MapPoints(n + 20)
    for t in (mp, mp_want):
        t.update(np.arange(n), pos, base["normal"], base["min_dist"], base["max_dist"], desc, flags)
    v = g.update_normal_depth(touched, SF, mp=mp)
    assert np.array_equal(v, valid) and valid.any() and not valid.all()
    ok = valid.astype(bool)
    mp_want.update(touched[ok], pos[touched[ok]], normal[ok], lo[ok], hi[ok], None, flags[touched[ok]])
    pose = amd.camera_pose(np.eye(3), np.zeros(3), (500, 500, 320, 240), 40.0, (0, 640, 0, 480), 1.2, N_LEVELS)
    a, b = mp.ProjectInFrustum(np.arange(n), pose, 0.5), mp_want.ProjectInFrustum(np.arange(n), pose, 0.5)
    assert a["in_view"].sum() > n // 2
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert np.array_equal(mp.positions(np.arange(n)), pos)


def test_mutation_between_two_vote_calls():
    w, kf_slot_of, _ = make_world(seed=23)
    g = amd.ObservationGraph(N_PTS, KF_CAP, RW)
    orf.load(w, g, kf_slot_of, {p: p for p in range(N_PTS)})
    ids = sorted(kf_slot_of)
    q = list(range(N_PTS))

    def check():
        (kf, wt), = g.votes([q])
        assert as_counter(kf, wt, kf_slot_of) == w.votes(q)
        for p in range(0, N_PTS, 3):
            ent, nobs, isbad, ref = orf.mirror_row(w, p, kf_slot_of)
            for dev in (False, True):
                r = g.get_row(p, from_device=dev)
                assert [tuple(int(v) for v in e) for e in r["entries"]] == ent, (p, dev)
                assert (r["n_obs"], r["bad"], r["ref_kf_slot"]) == (nobs, isbad, ref), (p, dev)

    check()
    rng = np.random.default_rng(4)
    adds = [(p, ids[int(rng.integers(12))]) for p in range(0, N_PTS, 3) if len(w.pts[p]["obs"]) < RW and not w.pts[p]["bad"]]
    for p, k in adds:
        w.add_observation(p, k, 5, 1, True)
    g.add_observations([p for p, _ in adds], [kf_slot_of[k] for _, k in adds], [5] * len(adds), [1] * len(adds), [1] * len(adds))
    check()
    erases = [(p, sorted(w.pts[p]["obs"])[0]) for p in range(0, N_PTS, 6) if w.pts[p]["obs"]]
    want_bad = [int(w.erase_observation(p, k)) for p, k in erases]
    assert g.erase_observations([p for p, _ in erases], [kf_slot_of[k] for _, k in erases]).tolist() == want_bad and any(want_bad)
    check()
    assert g.erase_keyframe(kf_slot_of[ids[4]]).tolist() == w.erase_keyframe(ids[4])
    check()


def test_a_flush_of_more_rows_than_one_chunk_holds():
    """row_width 256 (the widest): a marked non-empty row is staged as 2 KiB and 24 bytes, so one 8 MiB chunk holds 4048 of
    them and 4100 need two stagings.  Every row must have arrived, the ones on both sides of the chunk boundary and the last
    one among them."""
    rw, n_pts = 256, 4100
    rng = np.random.default_rng(41)
    ids = list(range(40, 52))
    kf_slot_of = dict(zip(ids, KF_SLOTS))
    w = orf.World()
    for k in ids:
        w.add_keyframe(k, rng.uniform(-1, 1, 3).astype(np.float32))
    for p in range(n_pts):
        obs = rng.choice(ids, size=int(rng.integers(1, 4)), replace=False).tolist()
        w.add_point(p, ref=obs[0], bad=False)
        for k in obs:
            w.add_observation(p, k, int(rng.integers(0, 2000)), int(rng.integers(0, N_LEVELS)), bool(rng.integers(2)))
    g = amd.ObservationGraph(n_pts, KF_CAP, rw)
    orf.load(w, g, kf_slot_of, {p: p for p in range(n_pts)})
    per_chunk = (8 << 20) // (4 + 16 + 4 + rw * 8)
    assert per_chunk < n_pts <= 2 * per_chunk
    q = list(range(n_pts))
    (kf, wt), = g.votes([q])  # the first call that reads the table: the flush
    assert as_counter(kf, wt, kf_slot_of) == w.votes(q)
    for p in [0, 1, per_chunk - 2, per_chunk - 1, per_chunk, per_chunk + 1, n_pts - 1] + list(range(7, n_pts, 97)):
        ent, nobs, isbad, ref = orf.mirror_row(w, p, kf_slot_of)
        r = g.get_row(p, from_device=True)
        assert [tuple(int(v) for v in e) for e in r["entries"]] == ent, p
        assert (r["n_obs"], r["bad"], r["ref_kf_slot"]) == (nobs, isbad, ref), p
    g.close()
