"""GPU tests of LoopClosing::ComputeSim3's two searches on the resident map points (include/orbfe.h: orbfe_project_sim3,
orbfe_search_by_sim3_mappoints_multi, orbfe_search_by_projection_sim3_mappoints): the prologue pinned to
tests/sim3_search_ref.py bit for bit, the one call against the two-step form through the existing host-array searches and the
oracle, vbAlreadyMatched2 from the observation graph, engineered search cases, table updates and re-entrancy.

A key frame holds as many keypoints as its slot list has entries (GetMapPointMatches() is per keypoint), so the key frames
have the sizes of the scene (0 .. 300 keypoints)."""
import threading

import numpy as np
import pytest

import fuse_ref as fr
import sim3_search_ref as sr
from test_sim3_search_ref import BIG, BIG_IDS, GPU_SCENES, IDS
from test_track_ref import CAP, CAP_ALL

pytestmark = pytest.mark.gpu

TABLE = 4096
TH = 7.5  # LoopClosing::ComputeSim3 (src/LoopClosing.cc:361)
K4 = (sr.FX, sr.FY, sr.CX, sr.CY)
FIELDS = ("valid", "u", "v", "level", "dist")
SEARCH = [s for s in GPU_SCENES if s[1] > 1]
SEARCH_IDS = [i for i, s in zip(IDS, GPU_SCENES) if s[1] > 1]


def _table(sc):
    from orb_slam2_annotate_amd.map_points import MapPoints
    mp = MapPoints(TABLE)
    n = len(sc["pos"])
    if n:
        mp.update(np.arange(n, dtype=np.int32), sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
    return mp


def _leg(d):
    from orb_slam2_annotate_amd.map_points import sim3_leg
    return sim3_leg(d["Rw"], d["tw"], d["sR"], d["t"], K4, sr.BOUNDS, sr.SCALE, sr.LEVELS)


def _view(f, resident=False):
    from orb_slam2_annotate_amd import FrameView
    V = FrameView(f["x"], f["y"], f["octave"], f["desc"], sr.BOUNDS)
    return V.upload() if resident else V


def _same_bits(got, want, fields=FIELDS):
    for name in fields:
        a, b = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name]).astype(got[name].dtype)
        assert a.shape == b.shape, name
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (name, np.flatnonzero(a.reshape(-1) != b.reshape(-1))[:8])


def _cat(dicts):
    return {name: np.concatenate([d[name] for d in dicts] + [np.zeros(0, np.float32 if name in ("u", "v", "dist") else
                                                                     (np.uint8 if name == "valid" else np.int32))])
            for name in FIELDS}


def _project(mp, sc, skips=True):
    slots, sk = sr.leg_lists(sc)
    return _cat(mp.project_sim3([_leg(d) for d in sc["legs"]], slots, skips=sk if skips else None))


@pytest.mark.parametrize("seed,n1,n2s", GPU_SCENES, ids=IDS)
def test_project_sim3_equals_spec32_bit_for_bit(seed, n1, n2s):
    sc = sr.scene(seed, n1, n2s)
    mp = _table(sc)
    _same_bits(_project(mp, sc), sr.spec32(sc))
    _same_bits(_project(mp, sc, skips=False), sr.spec32(sc, skips=None))


@pytest.mark.parametrize("seed,n1,n2s", BIG, ids=BIG_IDS)
def test_project_sim3_agrees_with_ref64_outside_the_guard_bands(seed, n1, n2s):
    sc = sr.scene(seed, n1, n2s)
    g = _project(_table(sc), sc)
    r64 = sr.ref64(sc)
    N = len(g["valid"])
    out = sr.excluded(r64)
    print(f"{int(out.sum())} of {N} pairs inside the guard bands")
    assert (out & ~sr.on_threshold_by_design(sc)).sum() <= CAP * N and out.sum() <= CAP_ALL * N  # (tests/test_track_ref.py)
    keep = ~out
    assert np.array_equal(g["valid"][keep], r64["valid"][keep])
    assert np.array_equal(g["level"][keep], r64["level"][keep])
    ok = keep & (r64["valid"] != 0)
    assert ok.sum() > 20
    for name in ("u", "v"):
        # float32 projection of a KITTI-sized image: |u| < 1241 -> half an ulp is 6e-5, a handful of operations deep
        assert np.abs(g[name][ok] - r64[name][ok]).max() < 2e-3, name
    assert np.allclose(g["dist"][ok], r64["dist"][ok], rtol=1e-6)


def _matched_in(sc, seed):
    """vpMatches12 at entry per candidate, in slot space: the points skip1 marks hold some slot of the candidate's list"""
    K, n1 = len(sc["n2s"]), sc["n1"]
    m = np.full((K, n1), -1, np.int32)
    rng = np.random.default_rng(50 + seed)
    for k in range(K):
        pool = sc["slot2"][k][sc["slot2"][k] >= 0]
        on = np.flatnonzero(sc["skip1"][k])
        m[k, on] = rng.choice(pool, len(on)) if len(pool) else 0
    return m


def _multi(mp, sc, KF1, KF2s, matched, **kw):
    legs = [_leg(d) for d in sc["legs"]]
    return mp.SearchBySim3(KF1, sc["slot1"], KF2s, sc["slot2"], legs[0::2], legs[1::2], sr.SF, sr.SF, TH, matched12=matched, **kw)


def _desc_of(mp, slots):
    d = np.zeros((len(slots), 32), np.uint8)
    has = slots >= 0
    if has.any():
        d[has] = mp.descriptors(slots[has])
    return d


def _two_step(mp, sc, k, KF1, KF2, skip1, skip2):
    """candidate k through orbfe_project_sim3 and the existing orbfe_search_by_sim3"""
    import orb_slam2_annotate_amd as amd
    p1, p2 = mp.project_sim3([_leg(sc["legs"][2 * k]), _leg(sc["legs"][2 * k + 1])], [sc["slot1"], sc["slot2"][k]], skips=[skip1, skip2])
    d1, d2 = _desc_of(mp, sc["slot1"]), _desc_of(mp, sc["slot2"][k])
    return amd.ORBmatcher(0.9, True).SearchBySim3(KF1, KF2, sr.SF, sr.SF, p1["valid"], p1["u"], p1["v"], p1["level"], d1,
                                                  p2["valid"], p2["u"], p2["v"], p2["level"], d2, TH)


def _oracle(sc, k, skip1, skip2):
    """the oracle's SearchBySim3 fed with spec32's projections"""
    import oracle_lib as orc
    p1 = sr.spec32_leg(sc, sc["legs"][2 * k], sc["slot1"], skip1)
    p2 = sr.spec32_leg(sc, sc["legs"][2 * k + 1], sc["slot2"][k], skip2)
    d1 = sc["desc"][np.where(sc["slot1"] >= 0, sc["slot1"], 0)]
    d2 = sc["desc"][np.where(sc["slot2"][k] >= 0, sc["slot2"][k], 0)] if len(sc["slot2"][k]) else np.zeros((0, 32), np.uint8)
    F1 = orc.Frame(sc["kf1"]["x"], sc["kf1"]["y"], sc["kf1"]["octave"], sc["kf1"]["desc"], sr.BOUNDS)
    F2 = orc.Frame(sc["kf2"][k]["x"], sc["kf2"][k]["y"], sc["kf2"][k]["octave"], sc["kf2"][k]["desc"], sr.BOUNDS)
    return orc.search_by_sim3(F1, F2, sr.SF, sr.SF, p1["valid"], p1["u"], p1["v"], p1["level"], d1, p2["valid"], p2["u"], p2["v"],
                              p2["level"], d2, TH)


@pytest.mark.parametrize("resident", [False, True], ids=["views", "resident"])
@pytest.mark.parametrize("seed,n1,n2s", SEARCH, ids=SEARCH_IDS)
def test_multi_search_equals_the_two_step_calls_and_the_oracle(seed, n1, n2s, resident):
    sc = sr.scene(seed, n1, n2s)
    mp = _table(sc)
    KF1, KF2s = _view(sc["kf1"], resident), [_view(f, resident) for f in sc["kf2"]]
    matched = _matched_in(sc, seed)
    cnt, match = _multi(mp, sc, KF1, KF2s, matched, already2=sc["skip2"])
    assert match.shape == (len(n2s), n1)
    total = 0
    for k in range(len(n2s)):
        n, m = _two_step(mp, sc, k, KF1, KF2s[k], sc["skip1"][k], sc["skip2"][k])
        assert cnt[k] == n and np.array_equal(match[k], m), k
        if not resident:
            no, mo = _oracle(sc, k, sc["skip1"][k], sc["skip2"][k])
            assert cnt[k] == no and np.array_equal(match[k], mo), k
        assert not (match[k][sc["skip1"][k] != 0] >= 0).any() and not (match[k][sc["slot1"] < 0] >= 0).any()
        total += int(n)
    if min(n1, max(n2s)) >= 255:
        assert total >= 5  # the scenes hold mutual pairs
    if len(n2s) == 1:  # K = 1 without any mask
        cnt0, match0 = _multi(mp, sc, KF1, KF2s, None)
        n, m = _two_step(mp, sc, 0, KF1, KF2s[0], None, None)
        assert cnt0[0] == n and np.array_equal(match0[0], m)


def graph_rows(sc, seed=77, point_cap=600):
    """The rows of test 3, built on the CPU from the oracle's unmasked result so that every row kind MATTERS: (matched [K, N1],
    want (K masks = the correct vbAlreadyMatched2), observations [(slot, kf, idx)], kf2_slot, other kf, broken / kept: per
    candidate the i1 of the pairs the correct masks break / must leave alone).  Matched keypoints of KF1 are taken among those that
    are in no pair, so vbAlreadyMatched1 breaks nothing.  Per matched slot, in turn:
      (a) it observes KF2_k at the i2 of a mutual pair -> that keypoint is marked and the pair breaks;
      (b) it observes KF2_k at idx >= N2_k, placed so that a scatter without the bound would land on a kept pair's i2 of the NEXT
          non-empty candidate -> ignored;
      (c) it observes another key frame, and ANOTHER candidate's key frame, both at a kept pair's i2 of candidate k -> ignored;
      (d) it observes nothing;
      (e) it lies at or past the graph's point_capacity -> it has no row."""
    K, n1, n2s = len(sc["n2s"]), sc["n1"], sc["n2s"]
    assert len(sc["pos"]) > point_cap
    rng = np.random.default_rng(seed)
    kf2_slot, other = np.array([7, 3, 11, 5, 9][:K], np.int32), 20
    free = [_oracle(sc, k, None, None)[1] for k in range(K)]
    in_pair = np.zeros(n1, bool)
    for m in free:
        in_pair |= m >= 0
    cand_i1 = np.flatnonzero(~in_pair)[::3]
    matched = np.full((K, n1), -1, np.int32)
    want = [np.zeros(n, np.uint8) for n in n2s]
    obs, broken, kept = [], [[] for _ in range(K)], [[] for _ in range(K)]
    slots = list(rng.permutation(np.arange(sr.ENGINEERED + 1, point_cap)))
    off2 = np.concatenate([[0], np.cumsum(n2s)])
    pairs = [[(int(i1), int(m[i1])) for i1 in np.flatnonzero(m >= 0)] for m in free]
    for k in range(K):
        for j, (i1, i2) in enumerate(pairs[k]):  # every second pair is to break, the others are to survive
            (broken if j % 2 == 0 else kept)[k].append((i1, i2))
    kinds = set()
    for k in range(K):
        nxt = next((q for q in range(k + 1, K) if kept[q]), None)
        for j, i1 in enumerate(cand_i1):
            kind = "abcde"[j % 5]
            if kind == "e":
                matched[k, i1] = point_cap + (j % (len(sc["pos"]) - point_cap))
                kinds.add(kind)
                continue
            s = int(slots.pop())
            matched[k, i1] = s
            if kind == "a" and broken[k]:
                i2 = broken[k][(j // 5) % len(broken[k])][1]
                obs += [(s, kf2_slot[k], i2), (s, other, 5)]
                want[k][i2] = 1
            elif kind == "b":
                idx = n2s[k] + 5 if nxt is None else int(off2[nxt] - off2[k]) + kept[nxt][(j // 5) % len(kept[nxt])][1]
                assert idx >= n2s[k]
                obs.append((s, kf2_slot[k], idx))
            elif kind == "c" and kept[k]:
                i2 = kept[k][(j // 5) % len(kept[k])][1]
                obs += [(s, other, i2), (s, kf2_slot[(k + 1) % K], i2)]
            if kind != "a" or broken[k]:
                kinds.add(kind)
    assert kinds == set("abcde")
    return matched, want, np.array(obs, np.int64), kf2_slot, other, broken, kept


def test_already_matched2_from_the_graph_equals_the_mask_route():
    from orb_slam2_annotate_amd.observation_graph import ObservationGraph
    seed, n1, n2s = GPU_SCENES[1]
    sc = sr.scene(seed, n1, n2s)
    K = len(n2s)
    POINT_CAP = 600  # below the largest slot of the scene: some matched slots have no row
    matched, want, o, kf2_slot, other, broken, kept = graph_rows(sc, point_cap=POINT_CAP)
    mp = _table(sc)
    KF1, KF2s = _view(sc["kf1"]), [_view(f) for f in sc["kf2"]]
    g = ObservationGraph(POINT_CAP, 32, 8)
    allkf = np.concatenate([kf2_slot, [other]]).astype(np.int32)
    g.set_keyframes(allkf, np.arange(len(allkf), dtype=np.int64), np.zeros((len(allkf), 3), np.float32))
    g.set_points(np.arange(POINT_CAP, dtype=np.int32), np.zeros(POINT_CAP, np.uint8), np.full(POINT_CAP, -1, np.int32))
    g.add_observations(o[:, 0], o[:, 1], o[:, 2], np.zeros(len(o), np.uint8), np.zeros(len(o), np.uint8))
    by_graph = _multi(mp, sc, KF1, KF2s, matched, graph=g, kf2_slot=kf2_slot)
    by_mask = _multi(mp, sc, KF1, KF2s, matched, already2=want)
    none = _multi(mp, sc, KF1, KF2s, matched)
    assert np.array_equal(by_graph[0], by_mask[0]) and np.array_equal(by_graph[1], by_mask[1])
    # the masks matter: every pair put under a mark is found without the masks and lost with them; every pair that a wrongly
    # placed mark (no idx bound, no kf compare) would hit survives
    assert not np.array_equal(none[1], by_mask[1])
    assert sum(len(b) for b in broken) >= 8 and sum(len(b) for b in kept) >= 8
    for k in range(K):
        for i1, i2 in broken[k]:
            assert none[1][k, i1] == i2 and by_graph[1][k, i1] == -1, (k, i1, i2)
        for i1, i2 in kept[k]:
            assert none[1][k, i1] == i2 and by_graph[1][k, i1] == i2, (k, i1, i2)
        n, m = _two_step(mp, sc, k, KF1, KF2s[k], (matched[k] >= 0).astype(np.uint8), want[k])
        assert by_graph[0][k] == n and np.array_equal(by_graph[1][k], m)
    # both sources together are their union: half of the marks from the caller, all of them from the graph
    half = [w * (np.arange(len(w)) % 2 == 0).astype(np.uint8) for w in want]
    both = _multi(mp, sc, KF1, KF2s, matched, graph=g, kf2_slot=kf2_slot, already2=half)
    assert np.array_equal(both[1], by_mask[1])
    # and a caller's mark the graph does not have is kept: one more pair breaks
    k0 = next(k for k in range(K) if kept[k])
    extra = [w.copy() for w in want]
    extra[k0][kept[k0][0][1]] = 1
    more = _multi(mp, sc, KF1, KF2s, matched, graph=g, kf2_slot=kf2_slot, already2=[e * (1 - w) for e, w in zip(extra, want)])
    assert more[1][k0, kept[k0][0][0]] == -1 and more[0].sum() == by_graph[0].sum() - 1


def _flip(desc, nbits):
    d = np.unpackbits(np.asarray(desc, np.uint8))
    d[:nbits] ^= 1
    return np.packbits(d)


def _world_of(u, v, z):
    return np.array([(u - float(np.float32(sr.CX))) / float(np.float32(sr.FX)) * z, (v - float(np.float32(sr.CY))) / float(np.float32(sr.FY)) * z, z])


def _engineered(pairs):
    """Two key frames on ONE camera (identity poses, s12 = 1): pair j = (u, octave2, octave1, flips12, flips21, holds2) puts a
    point at level 3 in front of pixel (u, 150), KF1's keypoint j and KF2's keypoint j on its projection with the given
    octaves; KF2's keypoint carries the descriptor of KF1's point with flips12 bits flipped and KF1's keypoint that of KF2's
    point with flips21; holds2 = False leaves KF2's keypoint without a map point."""
    rng = np.random.default_rng(4)
    n = len(pairs)
    pos = np.zeros((2 * n, 3), np.float32)
    desc = rng.integers(0, 256, (2 * n, 32), dtype=np.uint8)
    kf1 = dict(x=np.zeros(n, np.float32), y=np.full(n, 150, np.float32), octave=np.zeros(n, np.int32), desc=np.zeros((n, 32), np.uint8))
    kf2 = dict(x=np.zeros(n, np.float32), y=np.full(n, 150, np.float32), octave=np.zeros(n, np.int32), desc=np.zeros((n, 32), np.uint8))
    slot2 = np.arange(n, 2 * n, dtype=np.int32)
    for j, (u, o2, o1, f12, f21, holds2) in enumerate(pairs):
        pos[j] = pos[n + j] = _world_of(u, 150.0, 10.0).astype(np.float32)
        kf1["x"][j] = kf2["x"][j] = u
        kf1["octave"][j], kf2["octave"][j] = o1, o2
        kf2["desc"][j] = _flip(desc[j], f12)
        kf1["desc"][j] = _flip(desc[n + j], f21)
        if not holds2:
            slot2[j] = -1
    dist = np.linalg.norm(pos.astype(np.float64), axis=1)
    max_dist = (dist * 1.2 ** 2.5).astype(np.float32)  # level 3
    sc = dict(pos=pos, normal=(pos / dist[:, None]).astype(np.float32), min_dist=(max_dist / np.float32(1.2 ** 7)).astype(np.float32),
              max_dist=max_dist, flags=np.full(2 * n, 2, np.uint8), desc=desc, slot1=np.arange(n, dtype=np.int32), slot2=[slot2],
              skip1=np.zeros((1, n), np.uint8), skip2=[np.zeros(n, np.uint8)], n1=n, n2s=[n], kf1=kf1, kf2=[kf2])
    eye, zero = np.eye(3, dtype=np.float32), np.zeros(3, np.float32)
    sc["legs"] = [sr.make_leg(eye, zero, eye, zero), sr.make_leg(eye, zero, eye, zero)]
    return sc


def test_engineered_search_cases():
    pairs = [
        (100.0, 3, 3, 0, 0, True),     # 0: a plain mutual pair
        (250.0, 3, 3, 0, 0, False),    # 1: only KF1 -> KF2 finds it (KF2's keypoint holds no point): no match
        (400.0, 3, 3, 100, 0, True),   # 2: best distance 100 = TH_HIGH: kept
        (550.0, 3, 3, 101, 0, True),   # 3: best distance 101: dropped
        (700.0, 4, 3, 0, 0, True),     # 4: KF2's keypoint at level + 1: refused
        (850.0, 2, 3, 0, 0, True),     # 5: KF2's keypoint at level - 1: taken
    ]
    sc = _engineered(pairs)
    # 6 / 7: two keypoints of KF2 at equal distance from KF1's point 6 -- the first in scan order wins
    for f in (sc["kf1"], sc["kf2"][0]):
        for name in ("x", "y", "octave"):
            f[name] = np.concatenate([f[name], f[name][:2]])
        f["desc"] = np.concatenate([f["desc"], f["desc"][:2]])
    n = len(pairs)
    P = _world_of(1000.0, 150.0, 10.0).astype(np.float32)
    extra = dict(pos=np.stack([P, P, P]), desc=np.random.default_rng(9).integers(0, 256, (3, 32), dtype=np.uint8))
    base = len(sc["pos"])
    for name in ("pos", "desc"):
        sc[name] = np.concatenate([sc[name], extra[name]])
    d = float(np.linalg.norm(P.astype(np.float64)))
    sc["normal"] = np.concatenate([sc["normal"], np.tile((P / d).astype(np.float32), (3, 1))])
    sc["max_dist"] = np.concatenate([sc["max_dist"], np.full(3, d * 1.2 ** 2.5, np.float32)])
    sc["min_dist"] = np.concatenate([sc["min_dist"], np.full(3, d * 1.2 ** 2.5 / 1.2 ** 7, np.float32)])
    sc["flags"] = np.concatenate([sc["flags"], np.full(3, 2, np.uint8)])
    sc["slot1"] = np.concatenate([sc["slot1"], [base, -1]]).astype(np.int32)
    sc["slot2"] = [np.concatenate([sc["slot2"][0], [base + 1, base + 2]]).astype(np.int32)]
    sc["skip1"], sc["skip2"], sc["n1"], sc["n2s"] = np.zeros((1, n + 2), np.uint8), [np.zeros(n + 2, np.uint8)], n + 2, [n + 2]
    k1, k2 = sc["kf1"], sc["kf2"][0]
    k1["x"][n:], k1["octave"][n:] = [1000.0, 30.0], [3, 0]
    k2["x"][n:], k2["octave"][n:] = [1000.0, 1000.0], [3, 3]
    k2["desc"][n] = k2["desc"][n + 1] = _flip(sc["desc"][base], 7)  # both 7 bits from KF1's point
    k1["desc"][n] = sc["desc"][base + 1]                            # and KF1's keypoint is the best of both of KF2's points
    mp = _table(sc)
    KF1, KF2 = _view(k1), _view(k2)
    cnt, match = _multi(mp, sc, KF1, [KF2], None)
    assert match[0].tolist() == [0, -1, 2, -1, -1, 5, n, -1], match[0]
    assert cnt[0] == 4
    n2, m2 = _two_step(mp, sc, 0, KF1, KF2, None, None)
    no, mo = _oracle(sc, 0, None, None)
    assert (n2, m2.tolist()) == (4, match[0].tolist()) and (no, mo.tolist()) == (4, match[0].tolist())
    # the one-directional result of pair 1 exists: with a map point on KF2's keypoint the pair is found
    sc["slot2"][0][1] = n + 1
    assert _multi(mp, sc, KF1, [KF2], None)[1][0][1] == 1

    # the projection form: TH_LOW = 50 kept, 51 dropped, level + 1 refused; match indexes slot[]
    from orb_slam2_annotate_amd.map_points import camera_pose
    pose = camera_pose(np.eye(3), np.zeros(3), K4, 0.0, sr.BOUNDS, sr.SCALE, sr.LEVELS)
    kp = dict(x=np.float32([100, 400, 550, 700]), y=np.full(4, 150, np.float32), octave=np.int32([3, 3, 3, 4]),
              desc=np.stack([sc["desc"][0], _flip(sc["desc"][2], 50), _flip(sc["desc"][3], 51), sc["desc"][4]]))
    slots = np.array([4, 3, 2, 0], np.int32)
    nm, m = mp.SearchByProjectionSim3(_view(kp), slots, pose, sr.SF, 10)
    assert (nm, m.tolist()) == (2, [3, 2, -1, -1])


def _projection_scene(seed, n):
    sc = fr.scene(seed, n, 1)
    slot = np.random.default_rng(900 + seed).permutation(TABLE)[:n].astype(np.int32)
    from orb_slam2_annotate_amd.map_points import MapPoints, camera_pose
    mp = MapPoints(TABLE)
    if n:
        mp.update(slot, sc["pos"], sc["normal"], sc["min_dist"], sc["max_dist"], sc["desc"], sc["flags"])
    p = fr.sim3_poses(sc, 1.07)[0]
    pose = camera_pose(p["Rcw"], p["tcw"], K4, fr.MBF, fr.BOUNDS, fr.SCALE, fr.LEVELS, Ow=p["Ow"])
    f = sc["frames"][0]
    return sc, slot, mp, pose, dict(x=f["x"], y=f["y"], octave=f["octave"], desc=f["desc"])


def _two_step_projection(mp, slot, pose, KF, th, matched, skip):
    import orb_slam2_annotate_amd as amd
    pr = mp.project_fuse([pose], slot, skip=skip)
    desc = mp.descriptors(slot) if len(slot) else np.zeros((0, 32), np.uint8)
    return amd.ORBmatcher(0.9, True).SearchByProjectionSim3(KF, sr.SF, pr["valid"][0], pr["u"][0], pr["v"][0], pr["level"][0], desc,
                                                           th, matched=matched), pr["valid"][0]


@pytest.mark.parametrize("resident", [False, True], ids=["view", "resident"])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 300])
def test_projection_sim3_equals_the_two_step_form(n, resident):
    sc, slot, mp, pose, f = _projection_scene(20 + n, n)
    KF = _view(f, resident)
    rng = np.random.default_rng(n)
    matched = (rng.random(len(f["x"])) < 0.15).astype(np.uint8)
    skip = (rng.random(n) < 0.1).astype(np.uint8)
    for mt, sk in ((None, None), (matched, skip), (matched, None)):
        (nw, mw), valid = _two_step_projection(mp, slot, pose, KF, 10, mt, sk)
        ng, mg, proj = mp.SearchByProjectionSim3(KF, slot, pose, sr.SF, 10, matched=mt, skip=sk, return_projected=True)
        assert ng == nw and np.array_equal(mg, mw) and np.array_equal(proj, valid)
        assert ng == (mg >= 0).sum() and (mg < n).all()
        if mt is not None:
            assert not (mg[mt != 0] >= 0).any()
        if sk is not None and n:
            assert not np.isin(np.flatnonzero(sk), mg).any()
    if n >= 255:
        assert nw > 10


def test_projection_sim3_grows_its_lists():
    """40 keypoints inside the window of one map point, more than the 32 entries the search's lists start with: the one call
    (k_project_fuse at K = 1 writes the queries on the device) searches a second time with longer lists, behind a producer
    whose staging starts anew, and still equals the two-step form.  The scene is the smallest of this file that holds a
    searched point (the size-1 scene's only point is rejected)."""
    import oracle_lib as O
    n, n_crowd, th = 255, 40, 10
    sc, slot, mp, pose, f = _projection_scene(20 + n, n)
    s32 = fr.spec32(sc, poses=fr.sim3_poses(sc, 1.07), skip=np.zeros(n, np.uint8), in_kf=np.zeros(n, bool))
    valid, u, v, level = s32["valid"][0], s32["u"][0], s32["v"][0], s32["level"][0]
    p = int(np.flatnonzero((valid != 0) & (u > 40) & (u < 1200) & (v > 40) & (v < 330) & (level >= 1))[0])
    lv = int(level[p])
    rng = np.random.default_rng(43)
    f = {k: a.copy() for k, a in f.items()}
    kp = rng.choice(len(f["x"]), n_crowd, replace=False)
    f["x"][kp] = (u[p] + rng.uniform(-3, 3, n_crowd)).astype(np.float32)
    f["y"][kp] = (v[p] + rng.uniform(-3, 3, n_crowd)).astype(np.float32)
    f["octave"][kp] = lv - rng.integers(0, 2, n_crowd)
    f["desc"][kp] = sc["desc"][p] ^ (rng.integers(0, 256, (n_crowd, 32), dtype=np.uint8) & rng.integers(0, 256, (n_crowd, 32), dtype=np.uint8) &
                                    rng.integers(0, 256, (n_crowd, 32), dtype=np.uint8))
    # the oracle's own window of that point (radius th * scale[level], octaves [level - 1, level]) holds the crowd
    Fo = O.Frame(f["x"], f["y"], f["octave"], f["desc"], fr.BOUNDS)
    assert Fo.features_in_area(u[p], v[p], th * sr.SF[lv], lv - 1, lv).size >= n_crowd > 32
    for resident in (True, False):
        KF = _view(f, resident)
        (nw, mw), proj_w = _two_step_projection(mp, slot, pose, KF, th, None, None)
        ng, mg, proj = mp.SearchByProjectionSim3(KF, slot, pose, sr.SF, th, return_projected=True)
        assert ng == nw and np.array_equal(mg, mw) and np.array_equal(proj, proj_w) and np.array_equal(proj, valid)
        assert ng == (mg >= 0).sum() and ng > 10 and (mg == p).sum() == 1


def test_projection_sim3_chain_of_points_that_claim_one_keypoint():
    sc, slot, mp, pose, f = _projection_scene(31, 300)
    KF = _view(f)
    n0, m0 = mp.SearchByProjectionSim3(KF, slot, pose, sr.SF, 10)
    first = int(m0[m0 >= 0][0])
    # the same map point five times in front of the list: all five want one keypoint, the first takes it, and the others fall
    # back on what is left in the window -- each claim depends on the one before
    chain = np.concatenate([np.full(5, slot[first], np.int32), slot]).astype(np.int32)
    (nw, mw), _ = _two_step_projection(mp, chain, pose, KF, 10, None, None)
    ng, mg = mp.SearchByProjectionSim3(KF, chain, pose, sr.SF, 10)
    assert ng == nw and np.array_equal(mg, mw)
    kp = int(np.flatnonzero(m0 == first)[0])
    assert mg[kp] == 0  # the position in slot[] of the first of the five
    assert (mg[mg >= 0] < len(chain)).all()


def test_a_table_update_between_two_calls_is_seen():
    seed, n1, n2s = GPU_SCENES[0]
    sc = sr.scene(seed, n1, n2s)
    mp = _table(sc)
    KF1, KF2s = _view(sc["kf1"]), [_view(f) for f in sc["kf2"]]
    cnt, match = _multi(mp, sc, KF1, KF2s, None)
    found = np.flatnonzero(match[0] >= 0)
    assert len(found) >= 5
    s = sc["slot1"][found[:3]]
    mp.update(s, sc["pos"][s], sc["normal"][s], sc["min_dist"][s], sc["max_dist"][s], None, np.full(3, 1, np.uint8))  # now bad
    cnt2, match2 = _multi(mp, sc, KF1, KF2s, None)
    assert (match2[0][found[:3]] == -1).all() and np.array_equal(match2[0][found[3:]], match[0][found[3:]])
    sc["flags"][s] = 1
    _same_bits(_project(mp, sc), sr.spec32(sc))
    # and the projection form
    scp, slot, mpp, pose, f = _projection_scene(33, 257)
    KF = _view(f)
    n0, m0 = mpp.SearchByProjectionSim3(KF, slot, pose, sr.SF, 10)
    hit = m0[m0 >= 0][:4]
    mpp.update(slot[hit], scp["pos"][hit], scp["normal"][hit], scp["min_dist"][hit], scp["max_dist"][hit], None, np.full(4, 1, np.uint8))
    n1_, m1 = mpp.SearchByProjectionSim3(KF, slot, pose, sr.SF, 10)
    assert not np.isin(hit, m1).any() and n1_ < n0 + 4


def test_two_threads_on_two_tables_give_the_single_thread_results():
    scenes = [sr.scene(*GPU_SCENES[1]), sr.scene(*GPU_SCENES[2])]
    tables = [_table(sc) for sc in scenes]
    views = [(_view(sc["kf1"]), [_view(f) for f in sc["kf2"]]) for sc in scenes]
    proj = [_projection_scene(40 + i, 300) for i in range(2)]

    def run(i):
        sc = scenes[i]
        out = [_multi(tables[i], sc, views[i][0], views[i][1], _matched_in(sc, i), already2=sc["skip2"]), _project(tables[i], sc)]
        _, slot, mp, pose, f = proj[i]
        out.append(mp.SearchByProjectionSim3(_view(f), slot, pose, sr.SF, 10))
        return out

    want = [run(0), run(1)]
    got, errors = [None, None], []

    def worker(i):
        try:
            for _ in range(3):
                got[i] = run(i)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert np.array_equal(got[i][0][0], want[i][0][0]) and np.array_equal(got[i][0][1], want[i][0][1])
        _same_bits(got[i][1], want[i][1])
        assert got[i][2][0] == want[i][2][0] and np.array_equal(got[i][2][1], want[i][2][1])
