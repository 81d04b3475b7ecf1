"""GPU tests of the device KeyFrameDatabase (include/orbfe.h orbfe_kfdb, orb_slam2_annotate_amd/keyframe_database.py)
against the plain-Python restatement tests/kfdb_ref.py.  Every comparison is exact: ids, word counts, order, and the
scores as bit patterns (float32 for the scored sets, float64 for orbfe_kfdb_score)."""
import numpy as np
import pytest

import kfdb_ref as ref
import kfdb_world as kw
import oracle_lib as orc
from orb_slam2_annotate_amd.vocabulary import synthetic_vocabulary_arrays, write_vocabulary_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


@pytest.fixture(scope="module")
def voc6(amd):
    voc = amd.ORBVocabulary()
    assert voc.createFromArrays(synthetic_vocabulary_arrays(*kw.VOC))
    return voc


@pytest.fixture(scope="module")
def world(amd, voc6):
    e = amd.ORBextractor(kw.NFEAT, 1.2, 8, 20, 7)

    def extract(imgs):
        out = []
        for i in range(0, len(imgs), 64):
            out += e.extract_batch(np.stack(imgs[i:i + 64]))
        return out
    return kw.World(extract, lambda d: voc6.transform_bow(d, 4))


def _fill(amd, n_words, ids, bows):
    db, rdb = amd.KeyFrameDatabase(n_words=n_words), ref.Database()
    for k, b in zip(ids, bows):
        db.add(k, b)
        rdb.add(k, b)
    return db, rdb


def _bits32(x):
    return np.asarray(x, np.float32).view(np.uint32).tolist()


def _same(got, want):
    """One query's scored set from the library against the restatement's."""
    ids, common, scores = want
    assert got[0].tolist() == list(ids)
    assert got[1].tolist() == list(common)
    assert _bits32(got[2]) == _bits32(scores)


def _check(db, rdb, bows, excluded=None):
    """One batched call and one call per query agree with each other and with the restatement.  -> per query
    ((ids, common, scores), number of key frames sharing a word)."""
    ex = excluded if excluded is not None else [()] * len(bows)
    want = [rdb.scored(b, x) for b, x in zip(bows, ex)]
    got = db.query(bows, excluded=excluded)
    for g, (w, _) in zip(got, want):
        _same(g, w)
    for i in range(len(bows)):
        g1 = db.query([bows[i]], excluded=None if excluded is None else [ex[i]])[0]
        _same(g1, want[i][0])
    return want


def _tie_on_first_word(rdb, bow, ids):
    """True when two survivors share their smallest common word with the query."""
    q = set(w for w, _ in ref.as_pairs(bow))
    first = [min(w for w, _ in rdb.kfs[k].bow if w in q) for k in ids]
    return len(set(first)) < len(first)


# ---------------------------------------------------------------------------------------------- transform_bow

def _bow_inputs(amd):
    from orb_slam2_annotate_amd import synth
    e = amd.ORBextractor(800, 1.2, 8, 20, 7)
    (_, d1), (_, d2) = e.extract_batch(np.stack(synth.render_sequence(3, 2, 640, 480, step=2.0)))
    rep = np.concatenate([d1[:200], d1[:200], d2[:50]])  # every word of the first 200 features at least twice
    return [d1, rep, d1[:1], d1[:0]]


@pytest.mark.parametrize("shape", ["text_k10_L2", "arrays_k10_L6"])
def test_transform_bow_equals_the_python_transform(amd, tmp_path, shape):
    """orbfe_vocabulary_transform_bow == the dict ORBVocabulary.transform builds (pinned to the reference's container by
    tests/test_dbow2_ref.py): same words, same doubles.  Repeated words (addWeight's += in feature order) and
    zero-weight words (skipped) included."""
    k, L = (10, 2) if shape.startswith("text") else (10, 6)
    arrays = list(synthetic_vocabulary_arrays(k, L, 4))
    rng = np.random.default_rng(9)
    weight = arrays[5].copy()
    weight[(rng.random(len(weight)) < 0.2) & (arrays[3] != 0)] = 0.0  # stop words
    arrays[5] = weight
    voc = amd.ORBVocabulary()
    if shape.startswith("text"):
        path = tmp_path / "voc.txt"
        write_vocabulary_text(path, arrays)
        assert voc.loadFromTextFile(path)
    else:
        assert voc.createFromArrays(tuple(arrays))
    levelsup = 0 if L == 2 else 4
    seen_repeat = seen_zero = 0
    for d in _bow_inputs(amd):
        bow, _ = voc.transform(d, levelsup)
        ids, values = voc.transform_bow(d, levelsup)
        assert ids.dtype == np.uint32 and values.dtype == np.float64
        assert ids.tolist() == sorted(bow)
        assert values.view(np.uint64).tolist() == np.array([bow[w] for w in sorted(bow)], np.float64).view(np.uint64).tolist()
        word, wt, _ = voc.transform_features(d, levelsup)
        seen_repeat += len(ids) < int((wt > 0).sum())
        seen_zero += int((wt == 0).sum()) > 0
    assert seen_repeat and seen_zero


def test_transform_bow_refuses_other_scorings_and_small_buffers(amd):
    import ctypes as C
    from orb_slam2_annotate_amd import _lib
    L = _lib.load()
    k, lv, parent, leaf, desc, weight = synthetic_vocabulary_arrays(10, 2, 4)
    h = C.c_void_p()
    p = _lib.ptr
    par, lf, ds, wt = (np.ascontiguousarray(parent, np.int32), np.ascontiguousarray(leaf, np.uint8),
                       np.ascontiguousarray(desc, np.uint8), np.ascontiguousarray(weight, np.float64))
    d = np.random.default_rng(1).integers(0, 256, size=(300, 32), dtype=np.uint8)
    ids, vals, n = np.zeros(300, np.uint32), np.zeros(300), C.c_int(0)
    for scoring, weighting in ((1, 0), (0, 1)):  # L2_NORM / TF_IDF, L1_NORM / TF
        _lib.check(L.orbfe_vocabulary_create(k, lv, scoring, weighting, len(par), p(par), p(lf), p(ds), p(wt), 0, C.byref(h)))
        assert L.orbfe_vocabulary_transform_bow(h, p(d), 300, 0, p(ids), p(vals), 300, C.byref(n)) == _lib.ERR_INVALID
        L.orbfe_vocabulary_destroy(h)
    _lib.check(L.orbfe_vocabulary_create(k, lv, 0, 0, len(par), p(par), p(lf), p(ds), p(wt), 0, C.byref(h)))
    assert L.orbfe_vocabulary_transform_bow(h, p(d), 300, 0, p(ids), p(vals), 300, C.byref(n)) == 0 and 50 < n.value <= 100
    full = n.value
    assert L.orbfe_vocabulary_transform_bow(h, p(d), 300, 0, p(ids), p(vals), 10, C.byref(n)) == _lib.ERR_CAPACITY
    assert n.value == full
    L.orbfe_vocabulary_destroy(h)


# ---------------------------------------------------------------------------------------------- score

def test_score_equals_the_restatement(amd, world):
    """orbfe_kfdb_score == L1Scoring::score as restated, as float64 bit patterns: real BowVectors against their
    neighbours, against themselves, against a disjoint vector, and empty vectors on either side."""
    ids, bows = list(world.ids[:40]), list(world.bows[:40])
    ids += [1, 2]
    bows += [world.no_share, world.empty]
    db, rdb = _fill(amd, 10 ** 6, ids, bows)
    nonzero = 0
    for q in (bows[3], bows[20], world.q_bows[0], world.no_share, world.empty):
        got = db.score(q, ids)
        want = np.array(rdb.score(q, ids), np.float64)
        assert got.view(np.uint64).tolist() == want.view(np.uint64).tolist()
        nonzero += int((want > 0).sum())
    assert nonzero > 30
    same = db.score(bows[3], [ids[3]])[0]
    assert abs(same - 1.0) < 1e-9  # an L1-normalised vector against itself
    assert db.score(bows[3], [1])[0] == 0.0 and db.score(world.empty, [ids[3]])[0] == 0.0
    with pytest.raises(amd.OrbfeError):
        db.score(bows[3], [999999])


# ---------------------------------------------------------------------------------------------- queries

def test_queries_on_synth_key_frames(amd, world):
    """Relocalisation and loop queries over 312 key frames of six scenes: noisy re-observations of stored views, views
    between two stored ones, a frame of a scene that was never stored, a query sharing no word, an empty query -- Q = 15 / 12 in one call, one query per call,
    and the restatement all agree; then the same after erasing a third of the key frames and adding some of them again
    (they move to the end of every word's list), and after clear()."""
    assert len(world.ids) >= 300
    db, rdb = _fill(amd, 10 ** 6, world.ids, world.bows)
    assert len(db) == len(world.ids)
    nq = len(world.q_near)

    def run(db, rdb):
        bows = world.q_bows + [world.no_share, world.empty]
        reloc = _check(db, rdb, bows)
        assert reloc[-2][0][0] == [] and reloc[-1][0][0] == []  # no shared word / no word: an empty result
        loop_bows = world.q_bows[:nq]
        ex = [world.connected(qi) for qi in range(nq)]
        loop = _check(db, rdb, loop_bows, ex)
        return reloc, loop, ex

    # the inputs are what they are meant to be: neighbouring key frames genuinely share words (more than twice what
    # frames 20 apart share), frames of different scenes share few (less than a quarter)
    S = [set(int(w) for w in b[0]) for b in world.bows]
    n, F = len(S), kw.FRAMES
    adj = np.mean([len(S[i] & S[i + 1]) for i in range(n - 1) if i // F == (i + 1) // F])
    far = np.mean([len(S[i] & S[i + 20]) for i in range(n - 20) if i // F == (i + 20) // F])
    other = np.mean([len(S[i] & S[(i + F) % n]) for i in range(n)])
    assert adj > 2 * far and adj > 4 * other and adj >= 20, (adj, far, other)

    reloc, loop, ex = run(db, rdb)
    # what keeps the comparison from passing vacuously, asserted on the restatement's own output
    assert sum(len(w[0][0]) >= 2 for w in reloc) >= 1 and sum(len(w[0][0]) >= 2 for w in loop) >= 1
    assert any(n and len(w[0]) * 2 <= n for w, n in reloc), "the word-count filter removes at least half somewhere"
    assert any(set(reloc[qi][0][0]) & set(ex[qi]) for qi in range(nq)), "a would-be survivor is lost to the exclusion list"
    assert any(_tie_on_first_word(rdb, b, w[0][0]) for b, w in zip(world.q_bows, reloc + loop)), "a tie on the first word"
    unseen = reloc[nq]
    assert unseen[1] > 0, "the unseen scene still shares some words with stored key frames"
    # own key frames: the re-observed view leads the word counts of its query
    for qi in range(len(world.q_index)):
        (ids, common, _), _ = reloc[qi]
        assert ids[int(np.argmax(common))] == world.q_near[qi]

    # mutation: erase every third key frame, add every second of those again
    gone = world.ids[::3]
    for k in gone:
        assert db.erase(k)
        rdb.erase(k)
    assert not db.erase(gone[0])
    back = gone[::2]
    where = {k: i for i, k in enumerate(world.ids)}
    for k in back:
        db.add(k, world.bows[where[k]])
        rdb.add(k, world.bows[where[k]])
    assert len(db) == len(world.ids) - len(gone) + len(back)
    reloc2, loop2, _ = run(db, rdb)
    assert any(r2[0][0] != r1[0][0] for r1, r2 in zip(reloc, reloc2)), "the mutation changes some result"
    assert any(set(w[0][0]) & set(back) for w in reloc2), "a re-added key frame is among the survivors"
    with pytest.raises(amd.OrbfeError):
        db.add(back[0], world.bows[where[back[0]]])  # present again: adding it twice is refused

    db.clear()
    rdb.clear()
    assert len(db) == 0
    assert [len(g[0]) for g in db.query(world.q_bows)] == [0] * len(world.q_bows)
    for k, b in zip(world.ids[:60], world.bows[:60]):  # the handle is as good as new
        db.add(k, b)
        rdb.add(k, b)
    _check(db, rdb, world.q_bows)


def test_capacity_is_reported(amd, world):
    import ctypes as C
    from orb_slam2_annotate_amd import _lib
    from orb_slam2_annotate_amd.keyframe_database import bow_arrays
    db, rdb = _fill(amd, 10 ** 6, world.ids[:104], world.bows[:104])
    qb = world.q_bows[7]  # a view between two stored ones: its neighbours on both sides survive the word filter
    (ids, common, scores), _ = rdb.scored(qb)
    assert len(ids) >= 2
    w, v = bow_arrays(qb)
    off = np.array([0, len(w)], np.int32)
    cap = len(ids) - 1
    kf, nc, sc, cnt = np.zeros(cap, np.int64), np.zeros(cap, np.int32), np.zeros(cap, np.float32), np.zeros(1, np.int32)
    p = _lib.ptr
    rc = _lib.load().orbfe_kfdb_query(db._h, 1, p(off), p(w), p(v), None, None, cap, p(kf), p(nc), p(sc), p(cnt))
    assert rc == _lib.ERR_CAPACITY and cnt[0] == len(ids)
    assert kf.tolist() == ids[:cap] and nc.tolist() == common[:cap] and _bits32(sc) == _bits32(scores[:cap])
    # the wrapper retries with the reported count
    _same(db.query([qb], capacity=1)[0], (ids, common, scores))
    bad = np.array([5, 4], np.uint32)
    off2 = np.array([0, 2], np.int32)
    assert _lib.load().orbfe_kfdb_query(db._h, 1, p(off2), p(bad), p(v), None, None, cap, p(kf), p(nc), p(sc), p(cnt)) == _lib.ERR_INVALID


def test_seeded_random_bow_vectors(amd):
    """2 000 key frames of 0..3000 words over 10^6 words; most vectors start with one of four words, so the survivors tie
    on the smallest shared word again and again and the insertion-order half of the order key decides.  Q = 32 in one
    call against one call per query and the restatement; then erase / re-add and query again."""
    bows = kw.random_bows(1, 2000)
    ids = [int(x) for x in np.random.default_rng(2).permutation(10 ** 5)[:2000]]  # ids carry no order
    db, rdb = _fill(amd, 10 ** 6, ids, bows)
    queries = kw.random_bows(3, 30) + [bows[7], (np.zeros(0, np.uint32), np.zeros(0))]
    assert len(queries) == 32
    ex = [[ids[j] for j in range(i, 2000, 41)] for i in range(32)]
    want = [rdb.scored(b) for b in queries]
    got = db.query(queries)
    ties = 0
    for g, (w, _), b in zip(got, want, queries):
        _same(g, w)
        ties += _tie_on_first_word(rdb, b, w[0])
    assert ties >= 10 and max(len(w[0]) for w, _ in want) >= 20
    for i in (0, 5, 30, 31):
        _same(db.query([queries[i]])[0], want[i][0])
    wantx = [rdb.scored(b, x) for b, x in zip(queries, ex)]
    for g, (w, _) in zip(db.query(queries, excluded=ex), wantx):
        _same(g, w)
    assert any(set(w[0][0]) & set(x) for w, x in zip(want, ex))
    for k in ids[::3]:
        db.erase(k)
        rdb.erase(k)
    for k in ids[:900:6]:
        db.add(k, bows[ids.index(k)])
        rdb.add(k, bows[ids.index(k)])
    for g, b in zip(db.query(queries[:12]), queries[:12]):
        _same(g, rdb.scored(b)[0])


def test_slabs_grow_across_a_doubling(amd):
    """9 000 small key frames: the slot array outgrows its first slab (8 192 slots) and the word arrays theirs, the
    earlier contents are carried over, and a second database takes the released slabs from the pool."""
    rng = np.random.default_rng(5)
    bows = []
    for _ in range(9000):
        ids = np.unique(rng.integers(0, 120, size=int(rng.integers(1, 9)))).astype(np.uint32)
        v = rng.random(len(ids)) + 0.1
        bows.append((ids, v / v.sum()))
    ids = list(range(9000))
    db, rdb = _fill(amd, 120, ids, bows)
    one = (np.array([5], np.uint32), np.array([1.0]))  # every key frame holding word 5 survives: max = 1, min = 0
    queries = [bows[0], bows[8999], bows[4000], one]
    want = _check(db, rdb, queries)
    assert max(len(w[0]) for w, _ in want) > 256  # beyond the wrapper's first capacity
    del db
    db2, rdb2 = _fill(amd, 120, ids[:500], bows[:500])
    _check(db2, rdb2, queries)


def test_rejected_operands_leave_the_database_usable(amd, world):
    """Adversarial BowVectors are refused by orbfe_kfdb_add on the host (descending, repeated, out-of-range and wrapped
    ids, an id already present): nothing of them reaches the device arrays, and the database answers as before."""
    from orb_slam2_annotate_amd import _lib
    ids, bows = world.ids[:120], world.bows[:120]
    db, rdb = _fill(amd, 10 ** 6, ids, bows)
    before = _check(db, rdb, world.q_bows[:3])
    good_w, good_v = bows[0]
    evil = [(good_w[::-1].copy(), good_v), (np.repeat(good_w[:5], 2), good_v[:10]),
            (np.array([1, 2, 10 ** 6], np.uint32), good_v[:3]), (np.array([1, 2, 0xFFFFFFFF], np.uint32), good_v[:3]),
            (np.array([0x80000000, 0x80000001], np.uint32), good_v[:2])]
    for w, v in evil:
        with pytest.raises(amd.OrbfeError) as ei:
            db.add(5, (w, v))
        assert ei.value.code == _lib.ERR_INVALID
    with pytest.raises(amd.OrbfeError):
        db.add(ids[3], bows[3])
    with pytest.raises(amd.OrbfeError):
        db.query([(np.array([7, 10 ** 6], np.uint32), np.array([0.5, 0.5]))])
    assert len(db) == len(ids)
    after = _check(db, rdb, world.q_bows[:3])
    assert [a[0] for a in after] == [b[0] for b in before]
    db.add(5, bows[0])  # the id is still free
    rdb.add(5, bows[0])
    _check(db, rdb, world.q_bows[:3])


# ---------------------------------------------------------------------------------------------- end to end

def test_relocalisation_end_to_end(amd, voc6, world):
    """extract -> transform_bow -> DetectRelocalizationCandidates -> orbfe_search_by_bow_multi on the candidates: the
    re-observed key frame is a candidate, the candidates equal the restatement's, and every
    candidate's matches equal the oracle's SearchByBoW."""
    db, rdb = _fill(amd, 10 ** 6, world.ids, world.bows)
    neigh = kw.neighbours_of(world.ids)
    where = {k: i for i, k in enumerate(world.ids)}
    m = amd.ORBmatcher(0.75, True)
    total = 0
    for qi in (0, 3):
        kq, dq = world.q_features[qi]
        bow = voc6.transform_bow(dq, 4)
        assert bow[0].tolist() == world.q_bows[qi][0].tolist()
        cands = [int(c) for c in db.DetectRelocalizationCandidates(bow, neigh)]
        (ids, _, scores), _ = rdb.scored(bow)
        assert cands == ref.group_candidates(ref.RELOC, 0.0, ids, scores, neigh) and cands
        true_id = world.q_near[qi]
        assert true_id in cands, (true_id, cands)
        _, fvq = voc6.transform(dq, 4)
        RF = amd.FrameView(kq["x"], kq["y"], kq["octave"], dq, (0.0, float(kw.W), 0.0, float(kw.H)), angle=kq["angle"]).upload(fvq)
        res, masks, refs = [], [], []
        wq, _, nq_ = voc6.transform_features(dq, 4)
        for c in cands:
            kc, dc = world.features[where[c]]
            _, fvc = voc6.transform(dc, 4)
            res.append(amd.FrameView(kc["x"], kc["y"], kc["octave"], dc, (0.0, float(kw.W), 0.0, float(kw.H)), angle=kc["angle"]).upload(fvc))
            has = np.ones(len(kc), np.uint8)
            masks.append(has)
            _, wtc, nc_ = voc6.transform_features(dc, 4)
            _, wtq, _ = voc6.transform_features(dq, 4)
            refs.append(orc.search_by_bow(dc, has, kc["angle"], orc.FeatVec(nc_, wtc > 0), dq, kq["angle"], orc.FeatVec(nq_, wtq > 0), 0.75, True))
        cnt, got = m.SearchByBoWMulti(res, masks, RF)
        for i in range(len(cands)):
            assert (int(cnt[i]), got[i].tolist()) == (int(refs[i][0]), refs[i][1].tolist()), cands[i]
            total += int(cnt[i])
        for r in res + [RF]:
            r.close()
    assert total > 40


def test_loop_candidates_through_the_wrapper(amd, world):
    """DetectLoopCandidates == the restatement's two stages, with minScore taken the way LoopClosing::DetectLoop takes it
    (the lowest score against the connected key frames, via orbfe_kfdb_score)."""
    db, rdb = _fill(amd, 10 ** 6, world.ids, world.bows)
    neigh = kw.neighbours_of(world.ids)
    some = 0
    for qi in range(len(world.q_near)):
        bow = world.q_bows[qi]
        con = world.connected(qi, radius=2)
        s = db.score(bow, con)
        assert s.view(np.uint64).tolist() == np.array(rdb.score(bow, con)).view(np.uint64).tolist()
        min_score = float(np.float32(min([1.0] + [float(x) for x in s])))
        got = [int(c) for c in db.DetectLoopCandidates(-1, bow, con, min_score, neigh)]
        (ids, _, scores), _ = rdb.scored(bow, con)
        assert got == ref.group_candidates(ref.LOOP, min_score, ids, scores, neigh)
        assert not set(got) & set(con)
        some += len(got) > 0
    assert some


def test_a_slab_that_changes_owner_carries_nothing_with_it(amd):
    """The database's arrays and the resident frames' slabs come from ONE pool: a destroyed database's slabs (doubled past
    64 KiB: 100 key frames x ~200 words) go to the next frame uploads, the released frames' slabs to the next database, and
    neither sees what the other left in them."""
    bows = [b for b in kw.random_bows(5, 200, max_words=400) if len(b[0]) >= 100][:100]
    assert len(bows) == 100 and sum(len(w) for w, _ in bows) * 8 > 2 * 65536
    ids = [7 * i + 3 for i in range(len(bows))]
    queries = [b for b in kw.random_bows(6, 16, max_words=400) if len(b[0])]

    def build_and_query():
        db, rdb = _fill(amd, 10 ** 6, ids, bows)
        got = db.query(queries)
        for g, q in zip(got, queries):
            _same(g, rdb.scored(q, ())[0])
        del db  # orbfe_kfdb_destroy: its slabs go back to the pool
        return got

    A = build_and_query()
    assert max(len(g[0]) for g in A) > 10
    rng = np.random.default_rng(21)
    base = rng.integers(0, 256, size=(500, 32), dtype=np.uint8)
    views, fvs, frames = [], [], []
    for f in range(8):
        n = 500 - 7 * f
        desc = (base ^ (rng.integers(0, 256, base.shape, dtype=np.uint8) & rng.integers(0, 256, base.shape, dtype=np.uint8)
                        & rng.integers(0, 256, base.shape, dtype=np.uint8) & rng.integers(0, 256, base.shape, dtype=np.uint8)))[:n]
        x, y = rng.uniform(1, 639, n).astype(np.float32), rng.uniform(1, 479, n).astype(np.float32)
        angle = (np.linspace(5, 355, 500)[:n] + rng.uniform(-2, 2, n)).astype(np.float32)
        views.append((desc, angle, amd.FrameView(x, y, rng.integers(0, 8, n).astype(np.int32), desc, (0.0, 640.0, 0.0, 480.0), angle=angle)))
        fvs.append(amd.FeatureVector.from_node_of_feature((base[:n, 0].astype(np.uint32) % 40) * 5 + 1))
        frames.append(views[-1][2].upload(fvs[-1]))
    m = amd.ORBmatcher(0.7, True)
    for f in range(8):
        g = (f + 1) % 8
        has = np.ones(len(views[f][0]), np.uint8)
        rn, r = m.SearchByBoW(views[f][0], has, views[f][1], fvs[f], views[g][0], views[g][1], fvs[g])
        gn, got = m.SearchByBoWResident(frames[f], has, frames[g])
        assert gn == rn and np.array_equal(got, r), f
        assert rn > 50
    for fr in frames:
        fr.close()
    B = build_and_query()
    for a, b in zip(A, B):
        assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and _bits32(a[2]) == _bits32(b[2])
