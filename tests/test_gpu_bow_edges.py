"""The engineered and seeded FeatureVector-search cases of tests/bow_edges.py through the kernels of csrc/k_match.hip
(k_search_by_bow<1|2|4>, k_search_by_bow_multi, k_search_by_bow_batch, k_search_triangulation, k_search_triangulation_multi,
k_rot_prune) by every route that reaches them, array_equal with the CPU oracle.  tests/test_bow_edges.py pins the oracle
itself to an independent restatement on the same cases, shows that every named case takes the branch it names and that every
wrong reading of bow_edges.VARIANTS changes the answer of some named case."""
import dataclasses

import numpy as np
import pytest

import bow_edges as be
import oracle_lib as orc

pytestmark = pytest.mark.gpu
ROUTES = ("host", "resident", "multi")


@pytest.fixture(scope="module")
def amd():
    import orb_slam2_annotate_amd as m
    return m


@pytest.fixture(scope="module")
def named():
    """every named case with the oracle's answer, computed once"""
    return [(c, be.run_oracle(c)[0]) for c in be.named_cases()]


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("kind", be.KINDS)
def test_named_cases(amd, named, kind, route):
    n = 0
    for c, ref in named:
        if c.kind != kind:
            continue
        if route == "multi":         # the case between two other problems of ONE call: all three are compared
            probs = be.multi_problems(c)
            got = be.run_gpu_multi(amd, probs)
            assert got[1] == ref, c.name
            assert got[0] == [0, [-1] * len(ref[1])], c.name
            assert got[2] == be.run_oracle(probs[2])[0], c.name
        else:
            assert be.run_gpu(amd, c, route) == ref, c.name
        n += 1
    assert n > 50


@pytest.mark.parametrize("route", ["host", "resident"])
@pytest.mark.parametrize("kind", be.KINDS)
def test_seeded_cases(amd, kind, route):
    for seed in range(200):
        c = be.seeded_case(kind, seed)
        assert be.run_gpu(amd, c, route) == be.run_oracle(c)[0], c.name


def _by_name(named, *names):
    d = {c.name: c for c, _ in named}
    return [d[n] for n in names]


def _empty_like(c, key):
    """the case with side `key` sharing no node with the other side"""
    s = getattr(c, key)
    return dataclasses.replace(c, **{key: dict(s, nodes=s["nodes"] + 9000001)})


def _no_query(c):
    """the case with no active query on side 1 (every (KF, Frame) / (KF, KF) feature without a map point)"""
    return dataclasses.replace(c, s1=dict(c.s1, has=np.zeros_like(c.s1["has"])))


@pytest.mark.parametrize("kind", ["bow_frame", "bow_kf"])
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("empty_at", ["first", "middle", "last"])
def test_bow_multi_empty_problems_and_mixed_node_sizes(amd, named, kind, K, empty_at):
    """k_search_by_bow_multi: the binary search on pairStart[] with problems that contribute no node pair in first, middle
    or last place, and problems whose largest nodes hold 40 / 300 / 100 candidates in one <4> launch"""
    key = "s1" if kind == "bow_frame" else "s2"      # the side that varies over the K problems
    base = _by_name(named, f"{kind}_nodes_10_100_200_300")[0]
    vary = getattr(base, key)

    def cut(limit, roll):
        """the varied side with the nodes of more than `limit` features moved out of reach, descriptors rolled"""
        ids, cnt = np.unique(base.s2["nodes"], return_counts=True)      # (a node's size is its candidate count, on side 2)
        big = np.isin(vary["nodes"], ids[cnt > limit])
        s = dict(vary, nodes=np.where(big, vary["nodes"] + 5000011, vary["nodes"]), desc=np.roll(vary["desc"], roll, axis=0))
        return dataclasses.replace(base, **{key: s})
    live = [cut(40, 0), cut(300, 1), cut(100, 2), cut(300, 3)]
    empty = _empty_like(base, key)
    k_empty = dict(first=0, middle=K // 2, last=K - 1)[empty_at]
    probs, it = [], iter(live)
    for k in range(K):
        probs.append(empty if k == k_empty else next(it))
    if kind == "bow_frame" and K == 5:
        probs[(k_empty + 1) % K] = _no_query(probs[(k_empty + 1) % K])    # a problem with node pairs but no query
    got = be.run_gpu_multi(amd, probs)
    refs = [be.run_oracle(p)[0] for p in probs]
    assert got == refs
    assert refs[k_empty] == [0, [-1] * len(refs[k_empty][1])]
    assert sum(r[0] for r in refs) > 0


@pytest.mark.parametrize("empty_at", ["first", "middle", "last"])
def test_triangulation_multi_query_counts_f12_and_epipole_per_problem(amd, empty_at):
    """k_search_triangulation_multi: the binary search on blockStart[] with problems of 1, 4 and 5 live queries (1, 1 and 2
    workgroups) and one that shares no node in first, middle or last place; every problem has its own F12 and epipole, and problems
    0 and 1 are the SAME pair of frames under two F12 that give different answers"""
    def prob(n_live, F, e):
        # key frame 1: 9 queries, query i alone in node 10 + i (the map-point mask of key frame 1 is one per call, so a
        # problem's query count is the number of nodes its neighbour shares).  Neighbour: query i is 3 bits from candidates
        # 2 i (on the line y = 0) and 2 i + 1 (on the line y = 7), both in node 10 + i for i < n_live and out of reach
        # otherwise; the rest of the 40 candidates are far and in a node of their own
        P = [be.bits(24, 28 * i) for i in range(9)]
        c = [be.bits(200)] * 40
        y = np.zeros(40, np.float32)
        nodes = np.full(40, 5, np.int64)
        for i in range(9):
            c[2 * i], c[2 * i + 1] = P[i] ^ be.bits(3, 252), P[i] ^ be.bits(3, 253)
            y[2 * i + 1] = 7.0
            nodes[2 * i:2 * i + 2] = 10 + i + (1000 if i >= n_live else 0)
        x = np.full(40, 30.0, np.float32)
        return be.mk("tri_multi", "tri", None, None, s1=be.side(P, nodes=10 + np.arange(9), has=np.zeros(9, np.uint8)),
                     s2=be.side(c, nodes=nodes, has=np.zeros(40, np.uint8), x=x, y=y), F12=F, ex=e[0], ey=e[1], check_ori=True)
    line0 = np.array([0, 0, 0, 0, 0, 0, 0, 1, 0], np.float32)        # y = 0
    line7 = np.array([0, 0, 0, 0, 0, 0, 0, 1, -7], np.float32)       # y = 7
    probs = [prob(9, line0, (900.0, 900.0)), prob(9, line7, (900.0, 900.0)), prob(1, line0, (30.0, 60.0)), prob(4, line7, (30.0, 60.0)),
             prob(5, line0, (30.0, 7.0))]
    probs.insert(dict(first=0, middle=3, last=5)[empty_at], prob(0, line0, (900.0, 900.0)))
    got = be.run_gpu_multi(amd, probs)
    refs = [be.run_oracle(p)[0] for p in probs]
    assert got == refs
    live = [r for r in refs if r[0]]
    assert live[0][1] == [2 * i for i in range(9)] and live[1][1] == [2 * i + 1 for i in range(9)]    # same frames, two F12
    assert [r[0] for r in live] == [9, 9, 1, 4]
    assert sum(r[0] == 0 for r in refs) == 2         # the one without a shared node, and the last: its epipole (30, 7) is within 10 px of every candidate


@pytest.fixture(scope="module")
def batch_world(amd):
    arrays, cent = be.batch_vocabulary_arrays()
    voc = amd.ORBVocabulary()
    assert voc.createFromArrays(arrays)
    return voc, orc.Vocabulary.from_arrays(arrays), cent


@pytest.mark.parametrize("nnratio", [0.6, 0.75, 0.8, 1.5])
def test_batch_kernel_on_named_cases(amd, named, batch_world, nnratio):
    """k_search_by_bow_batch (the shuffle reduction of bow_top2<false> for nodes of up to 64 candidates, the LDS-claim path
    beyond) through bow_match_consecutive_batch_device on tensors written here: the (KF, Frame) named cases that fit the
    form as consecutive frame pairs of one batch of capacity 320, with a frame of no key points, a pair sharing no node and
    a node present only in the second frame.  Every consecutive pair -- the cases and the pairs between them -- is compared"""
    voc, vo, cent = batch_world
    fit = [c for c, _ in named if be.fits_batch(c) and c.nnratio == nnratio]
    assert len(fit) >= (20 if nnratio in (0.75, 1.5) else 5), len(fit)
    frames, case_pair = [], {}
    for c in fit:
        case_pair[len(frames)] = c
        frames += be.batch_frames(c, cent)
    a0 = np.zeros(1, np.float32)
    node = lambda j, pat: (cent[j:j + 1] ^ pat[None], a0, np.array([j + 1], np.uint32))  # noqa: E731
    two = (np.stack([cent[2] ^ be.Z, cent[6] ^ be.bits(4)]), np.zeros(2, np.float32), np.array([3, 7], np.uint32))
    frames += [(np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), np.zeros(0, np.uint32)),      # n = 0, on both sides of a pair
               node(2, be.Z), node(5, be.bits(3)),                                                # a pair sharing no node
               node(2, be.bits(2)), two]                                                          # node 7 only in the second frame
    cap = 320
    match, nm, (d_nodes, d_off, d_idx, d_cnt) = be.run_gpu_batch(voc, frames, cap, nnratio)
    fvs = []
    for t, (desc, ang, want_node) in enumerate(frames):
        used, _, weight, got_node = vo.transform(desc, 1)
        assert used == len(desc) and np.array_equal(got_node, want_node), t       # every descriptor lands in its intended node
        fv = orc.FeatVec(got_node, weight > 0)
        k = int(d_cnt[t])
        assert k == len(fv.node_ids) and np.array_equal(d_nodes[t, :k].astype(np.uint32), fv.node_ids), t
        assert np.array_equal(d_off[t, :k + 1], fv.offsets) and np.array_equal(d_idx[t, :used].astype(np.uint32), fv.indices), t
        fvs.append(fv)
    total = lds = 0
    for t in range(1, len(frames)):
        (d1, a1, _), (d2, a2, _) = frames[t - 1], frames[t]
        rn, rm = orc.search_by_bow(d1, np.ones(len(d1), np.uint8), a1, fvs[t - 1], d2, a2, fvs[t], nnratio, True)
        assert int(nm[t - 1]) == rn and np.array_equal(match[t - 1, :len(d2)], rm), (t, getattr(case_pair.get(t - 1), "name", None))
        assert (match[t - 1, len(d2):] == -1).all(), t
        c = case_pair.get(t - 1)
        if c is not None and not c.check_ori:        # the case's own answer, as tests/test_bow_edges.py pins it (no pruning: <= 3 bins)
            assert [rn, rm.tolist()] == be.run_oracle(dataclasses.replace(c, check_ori=True))[0], c.name
        total += rn
        lds += int(len(d2) > 64)
    assert total > (10 if nnratio in (0.75, 1.5) else 3)
    if nnratio in (0.75, 1.5):
        assert lds >= 10
