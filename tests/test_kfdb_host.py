"""CPU tests of the key-frame database's host side: orbfe_kfdb_group_candidates (the covisibility stage of
KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates, src/KeyFrameDatabase.cc:165-218, :293-346)
against the plain-Python restatement tests/kfdb_ref.py, and the argument checks of orbfe_kfdb_add that must fail before
any device call."""
import ctypes as C

import numpy as np
import pytest

import kfdb_ref as ref

F32 = np.float32


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


def _both(amd, mode, min_score, ids, scores, neigh):
    """(library, restatement) candidate lists of one scored set; neigh: {kf_id: ids}."""
    asked = []

    def get(k):
        asked.append(k)
        return neigh.get(k, ())
    got = amd.group_candidates(mode, min_score, ids, np.zeros(len(ids), np.int32), np.asarray(scores, F32), get)
    assert sorted(asked) == sorted(ids), "neighbours are asked for exactly the scored key frames"
    want = ref.group_candidates(mode, min_score, list(ids), [F32(s) for s in scores], lambda k: neigh.get(k, ()))
    return [int(x) for x in got], [int(x) for x in want]


@pytest.mark.parametrize("mode", [ref.RELOC, ref.LOOP])
def test_empty_set(amd, mode):
    got, want = _both(amd, mode, 0.1, [], [], {})
    assert got == want == []


def test_neighbours_inside_and_outside_the_set(amd):
    ids = [10, 11, 12, 13]
    scores = [0.20, 0.30, 0.05, 0.25]
    neigh = {10: [11, 99, 12], 11: [98], 12: [97, 96], 13: [10, 95]}  # 95..99 were never scored
    for mode in (ref.RELOC, ref.LOOP):
        got, want = _both(amd, mode, 0.04, ids, scores, neigh)
        assert got == want and len(want) >= 2
    # the neighbours outside the set change nothing
    inside = {k: [x for x in v if x in ids] for k, v in neigh.items()}
    assert _both(amd, ref.RELOC, 0.0, ids, scores, inside)[0] == _both(amd, ref.RELOC, 0.0, ids, scores, neigh)[0]


def test_duplicate_best_key_frame_is_listed_once_at_its_first_place(amd):
    ids = [1, 2, 3, 4]
    scores = [0.30, 0.10, 0.12, 0.35]
    # the groups of 2 and 3 both elect key frame 1 (its own group, 0.30, falls below 0.75f * 0.42): listed once, where
    # group 2 stands, before group 4's
    neigh = {2: [1], 3: [1], 4: []}
    for mode in (ref.RELOC, ref.LOOP):
        got, want = _both(amd, mode, 0.05, ids, scores, neigh)
        assert got == want == [1, 4]
    got, want = _both(amd, ref.RELOC, 0.0, [4, 2, 3, 1], [0.35, 0.10, 0.12, 0.30], neigh)
    assert got == want == [4, 1]


def test_ties_at_the_retain_threshold(amd):
    """acc > 0.75f * bestAccScore is strict: a group exactly at the threshold goes, one ulp above stays."""
    at = F32(0.75) * F32(1.0)
    above = np.nextafter(at, F32(2.0))
    below = np.nextafter(at, F32(0.0))
    ids, scores = [1, 2, 3, 4], [F32(1.0), at, above, below]
    for mode in (ref.RELOC, ref.LOOP):
        got, want = _both(amd, mode, 0.5, ids, scores, {})
        assert got == want == [1, 3]
    # loop mode: bestAccScore starts at min_score, so with every group below it the threshold is 0.75f * min_score
    ms = F32(0.8)
    ids, scores = [1, 2], [F32(0.75) * ms, np.nextafter(F32(0.75) * ms, F32(1.0))]
    got, want = _both(amd, ref.LOOP, ms, ids, scores, {})
    assert got == want == []  # neither seeds a group: both are below min_score
    # a strictly-greater replacement of the best key frame: an equal neighbour does not take over
    got, want = _both(amd, ref.RELOC, 0.0, [5, 6], [F32(0.5), F32(0.5)], {5: [6], 6: [5]})
    assert got == want == [5, 6]


def test_loop_entries_below_min_score_still_contribute_as_neighbours(amd):
    ids = [1, 2, 3]
    scores = [0.30, 0.04, 0.31]  # 2 is scored (it passed the word filter) but below min_score = 0.05
    neigh = {1: [2], 3: []}
    got, want = _both_loop_only(amd, 0.05, ids, scores, neigh)
    assert got == want == [1, 3]
    # without 2's contribution group 1 is not the best one: the order of the groups' scores differs
    acc1 = F32(F32(0.30) + F32(0.04))
    assert acc1 > F32(0.31) > F32(0.30)
    # ... and at a higher threshold it decides: 0.75f * 0.46 = 0.345 cuts group 3 and keeps group 1 only with 2 counted
    ids, scores = [1, 2, 3], [0.30, 0.04, 0.46]
    got, want = _both_loop_only(amd, 0.05, ids, scores, {1: [2], 3: []})
    assert got == want == [3]
    ids, scores = [1, 2, 3], [0.30, 0.049, 0.46]
    got, want = _both_loop_only(amd, 0.05, ids, scores, {1: [2], 3: []})
    assert got == want == [1, 3]
    assert _both_loop_only(amd, 0.05, ids, scores, {3: []})[0] == [3]


def _both_loop_only(amd, min_score, ids, scores, neigh):
    return _both(amd, ref.LOOP, min_score, ids, scores, neigh)


@pytest.mark.parametrize("seed", range(8))
def test_seeded_scored_sets(amd, seed):
    """Random scored sets with up-to-10 neighbours drawn from inside and outside the set; coarse scores make equal
    scores, duplicate elections and threshold ties frequent."""
    rng = np.random.default_rng([0x6B66, seed])
    seen_some = seen_cut = 0
    for _ in range(60):
        n = int(rng.integers(1, 40))
        pool = rng.permutation(200)[:n + 30]
        ids = [int(x) for x in pool[:n]]
        scores = (rng.integers(1, 33, size=n) / 64.0).astype(F32) if rng.random() < 0.5 else rng.random(n).astype(F32) * F32(0.4)
        neigh = {k: [int(x) for x in rng.choice(pool, size=int(rng.integers(0, 11)), replace=False)] for k in ids}
        min_score = float(rng.choice([0.0, 0.1, 0.25, 0.6]))
        for mode in (ref.RELOC, ref.LOOP):
            got = amd.group_candidates(mode, min_score, ids, np.zeros(n, np.int32), scores, neigh)
            want = ref.group_candidates(mode, min_score, ids, list(scores), lambda k: neigh.get(k, ()))
            assert [int(x) for x in got] == want, (seed, mode, ids)
            seen_some += len(want) >= 2
            seen_cut += len(want) < n
    assert seen_some and seen_cut


def test_group_candidates_capacity_and_arguments(amd):
    from orb_slam2_annotate_amd import _lib
    L = _lib.load()
    ids = np.array([1, 2, 3], np.int64)
    sc = np.array([0.5, 0.5, 0.5], F32)
    off = np.zeros(4, np.int32)
    out = np.zeros(3, np.int64)
    n = C.c_int(-1)
    p = _lib.ptr
    assert L.orbfe_kfdb_group_candidates(0, 0.0, 3, p(ids), None, p(sc), p(off), None, p(out), 3, C.byref(n)) == 0 and n.value == 3
    assert L.orbfe_kfdb_group_candidates(0, 0.0, 3, p(ids), None, p(sc), p(off), None, p(out), 2, C.byref(n)) == _lib.ERR_CAPACITY
    assert n.value == 3
    assert L.orbfe_kfdb_group_candidates(2, 0.0, 3, p(ids), None, p(sc), p(off), None, p(out), 3, C.byref(n)) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_group_candidates(0, 0.0, 3, p(ids), None, p(sc), None, None, p(out), 3, C.byref(n)) == _lib.ERR_INVALID
    bad = np.array([0, 2, 1, 1], np.int32)
    assert L.orbfe_kfdb_group_candidates(0, 0.0, 3, p(ids), None, p(sc), p(bad), p(ids), p(out), 3, C.byref(n)) == _lib.ERR_INVALID


def test_add_checks_its_operands_before_any_device_call(amd):
    """Creating a database touches no device, and a bad BowVector is refused by the host checks alone: the same status with
    and without a GPU.  Without one a well-formed add fails loudly (no CPU fallback) and leaves the database empty."""
    from orb_slam2_annotate_amd import _lib
    L = _lib.load()
    db = amd.KeyFrameDatabase(n_words=1000)
    assert len(db) == 0
    vals = np.full(4, 0.25)

    def code(ids, values=vals):
        with pytest.raises(amd.OrbfeError) as ei:
            db.add(7, (np.asarray(ids, np.uint32), values[:len(ids)]))
        return ei.value.code
    assert code([5, 3, 8, 9]) == _lib.ERR_INVALID       # descending
    assert code([3, 3, 8, 9]) == _lib.ERR_INVALID       # repeated
    assert code([3, 5, 8, 1000]) == _lib.ERR_INVALID    # == n_words
    assert code([3, 5, 8, 0xFFFFFFFF]) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_add(db._h, 7, None, None, 4) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_add(db._h, 7, None, None, -1) == _lib.ERR_INVALID
    assert L.orbfe_kfdb_add(None, 7, None, None, 0) == _lib.ERR_INVALID
    h = C.c_void_p()
    assert L.orbfe_kfdb_create(0, 0, C.byref(h)) == _lib.ERR_INVALID and not h.value
    # more queries than one launch takes are refused by the host, like every malformed query
    off, cnt = np.zeros(70001, np.int32), np.zeros(70000, np.int32)
    assert L.orbfe_kfdb_query(db._h, 70000, _lib.ptr(off), None, None, None, None, 0, None, None, None, _lib.ptr(cnt)) == _lib.ERR_INVALID
    assert len(db) == 0 and not db.erase(7)
    if L.orbfe_device_count() == 0:
        assert code([3, 5, 8, 9]) == _lib.ERR_HIP
        assert len(db) == 0
        with pytest.raises(amd.OrbfeError) as ei:
            db.query([{3: 1.0}])
        assert ei.value.code == _lib.ERR_HIP
    else:
        db.add(7, ([3, 5, 8, 9], vals))
        assert len(db) == 1 and code([1, 2]) == _lib.ERR_INVALID  # the id is in the database already
    db.clear()
    assert len(db) == 0
