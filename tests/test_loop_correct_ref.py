"""CPU: the restatement tests/loop_correct_ref.py on hand-computed cases, and the host calls of the loop correction
(orbfe_correct_loop_sim3s, orbfe_correct_loop_points, orbfe_gba_propagate_keyframes, orbfe_gba_update_points) against it.
Integer and flag outputs and the float matrices must be equal; the binary64 records are held to RECORD_BOUND (see there)."""
import numpy as np
import pytest

import essgraph_ref as er
import loop_correct_ref as lr
import obsgraph_ref as orf
from orb_slam2_annotate_amd import OrbfeError, loop_closing as lc

f32 = np.float32
SF = (1.2 ** np.arange(8)).astype(f32)
# The records are products of binary64 quaternions (g2o's Sim3 product).  The library evaluates Eigen's _transformVector in
# the association g2o_math.h spells out, (X + w uv) + (q x uv); numpy's restatement adds the same three terms as
# X + w uv + q x uv, left to right, which is the same association -- and every other step is one IEEE operation on both
# sides (the library is compiled without contraction).  The largest deviation measured over the poses below is 0: equality.
RECORD_BOUND = 0.0


def pose(rng, angle=0.4, dist=3.0):
    """a float32 4 x 4 rigid pose whose rotation is orthonormal to float32 rounding"""
    a = rng.normal(size=3)
    a = a / np.linalg.norm(a) * rng.uniform(0.05, angle)
    th = np.linalg.norm(a)
    K = er.skew(a / th)
    R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T = np.eye(4, dtype=f32)
    T[:3, :3] = R.astype(f32)
    T[:3, 3] = rng.uniform(-dist, dist, 3).astype(f32)
    return T


def inverse(T):
    out = np.eye(4, dtype=f32)
    out[:3, :3] = T[:3, :3].T
    out[:3, 3] = -(T[:3, :3].T.astype(np.float64) @ T[:3, 3].astype(np.float64)).astype(f32)
    return out


def scw_of(rng, T, s=1.07):
    S = er.sim3_from_Rts(T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64) * s + rng.normal(size=3) * 0.2, s)
    return er.to_record(S)


# ---- the restatement itself ----
def test_identity_sim3s_leave_everything_fixed():
    I8 = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    w = orf.World()
    w.add_keyframe(0, (0, 0, 0))
    w.add_keyframe(1, (1, 0, 0))
    w.add_point(0, ref=0)
    w.add_observation(0, 0, 0, 1, False)
    w.add_observation(0, 1, 0, 2, False)
    pos = {0: np.array([0.5, 0.25, 4.0], f32)}
    before = w.normal_depth(0, pos[0], SF)
    ids, refs, valid, nd = lr.correct_loop(w, [1, 0], {0: [0], 1: [-1, 0]}, [I8, I8], [I8, I8], [(1, 0, 0), (0, 0, 0)], pos, (), SF)
    assert (ids, refs, valid) == ([0], [0], [1])
    assert np.array_equal(pos[0], np.array([0.5, 0.25, 4.0], f32))
    assert all(np.array_equal(a, b) for a, b in zip(nd[0], before))
    cor, non, T = lr.correct_loop_sim3s(np.eye(4, dtype=f32)[None], np.eye(4, dtype=f32), 0, I8)
    assert np.array_equal(cor[0], I8) and np.array_equal(non[0], I8) and np.array_equal(T[0], np.eye(4, dtype=f32))


def test_a_pure_scale_about_the_current_camera():
    """Tcw = I for the current key frame, Scw = (I, 0, 2): CorrectedSwi.map(Siw.map(P)) = P / 2, and a neighbour at
    Tiw = [I | (-1, 0, 0)] (centre (1, 0, 0)) gets Siw_corrected = (I, (-1, 0, 0), 2): its centre moves to (0.5, 0, 0)."""
    S = np.array([0, 0, 0, 1, 0, 0, 0, 2.0])
    Ti = np.eye(4, dtype=f32)
    Ti[0, 3] = -1
    cor, non, T = lr.correct_loop_sim3s(np.array([Ti, np.eye(4, dtype=f32)]), np.eye(4, dtype=f32), 1, S)
    assert np.array_equal(cor[0], [0, 0, 0, 1, -1, 0, 0, 2]) and np.array_equal(non[0], [0, 0, 0, 1, -1, 0, 0, 1])
    assert np.array_equal(T[0][:3, 3], f32([-0.5, 0, 0])) and np.array_equal(T[1], np.eye(4, dtype=f32))
    assert np.array_equal(lr.correct_point(cor[1], non[1], f32([2, 4, 8])), f32([1, 2, 4]))
    assert np.array_equal(lr.correct_point(cor[0], non[0], f32([2, 4, 8])), f32([1, 2, 4]))


# ---- A1 ----
@pytest.fixture(scope="module")
def loop_case():
    rng = np.random.default_rng(5)
    K, cur = 7, 4
    Tiw = np.array([pose(rng) for _ in range(K)])
    return Tiw, inverse(Tiw[cur]), cur, scw_of(rng, Tiw[cur])


def test_correct_loop_sim3s_equals_the_restatement(loop_case):
    Tiw, Twc, cur, Scw = loop_case
    cor, non, T = lc.correct_loop_sim3s(Tiw, Twc, cur, Scw)
    wc, wn, wT = lr.correct_loop_sim3s(Tiw, Twc, cur, Scw)
    dev = max(np.abs(cor - wc).max(), np.abs(non - wn).max())
    print(f"largest deviation of the binary64 records from the restatement: {dev:.3e}")
    assert dev <= RECORD_BOUND
    assert np.array_equal(T.view(np.uint32), wT.view(np.uint32))
    assert np.array_equal(cor[cur].view(np.uint64), np.asarray(Scw).view(np.uint64))
    assert (non[:, 7] == 1.0).all()


def test_correct_loop_sim3s_refusals(loop_case):
    Tiw, Twc, cur, Scw = loop_case
    bad_T = Tiw.copy()
    bad_T[2, 1, 1] = np.nan
    for args, text in (((bad_T, Twc, cur, Scw), "not finite"), ((Tiw, Twc, -1, Scw), r"cur outside"), ((Tiw, Twc, 7, Scw), "cur outside"),
                       ((Tiw, Twc, cur, np.r_[Scw[:7], 0.0]), "scale"), ((Tiw, Twc, cur, np.r_[Scw[:7], -1.0]), "scale"),
                       ((Tiw, Twc, cur, np.r_[np.inf, Scw[1:]]), "not finite")):
        with pytest.raises(OrbfeError, match=text):
            lc.correct_loop_sim3s(*args)


# ---- A2 ----
def test_correct_loop_points_equals_the_restatement(loop_case):
    Tiw, Twc, cur, Scw = loop_case
    cor, non, _ = lc.correct_loop_sim3s(Tiw, Twc, cur, Scw)
    rng = np.random.default_rng(6)
    n = 90
    xw = rng.uniform(-5, 5, (n, 3)).astype(f32)
    lists = [rng.integers(-1, n, 30).tolist() for _ in range(len(cor))]
    lists[2] = []
    lists[3][4] = lists[3][9] = 17  # twice in one list
    skip = np.zeros(n, np.uint8)
    skip[[3, 17, 40]] = 1
    for sk in (None, skip):
        out, ref = lc.correct_loop_points(cor, non, lists, xw, sk)
        want, wref = lr.correct_loop_points(cor, non, lists, xw, sk)
        assert np.array_equal(ref, wref) and (ref >= 0).sum() > 40 and (ref < 0).any()
        bound = 4 * 2.0 ** -23 * max(1.0, np.abs(want).max())
        assert np.abs(out - want).max() <= bound
        assert np.array_equal(out[ref < 0].view(np.uint32), xw[ref < 0].view(np.uint32))
    assert ref[17] == -1 and ref[3] == -1
    with pytest.raises(OrbfeError, match="point index outside"):
        lc.correct_loop_points(cor, non, [[n]] + lists[1:], xw)
    worse = cor.copy()
    worse[1, 7] = 0
    with pytest.raises(OrbfeError, match="scale"):
        lc.correct_loop_points(worse, non, lists, xw)


# ---- B1 ----
def gba_world(rng, n):
    Tcw = np.array([pose(rng) for _ in range(n)])
    Twc = np.array([inverse(t) for t in Tcw])
    Tg = np.array([pose(rng) for _ in range(n)])
    return Tcw, Twc, Tg


def test_gba_propagate_keyframes_edge_cases():
    rng = np.random.default_rng(7)
    # 0: origin (GBA) -> 1 (GBA) -> 2, 3, 4 a chain of three new key frames; 0 -> 5 (new) -> 6 (GBA child of a new one);
    # 7: under no origin, in the GBA; 8: under no origin, new
    n = 9
    children = [[1, 5], [2], [3], [4], [], [6], [], [], []]
    in_gba = np.array([1, 1, 0, 0, 0, 0, 1, 1, 0], np.uint8)
    Tcw, Twc, Tg = gba_world(rng, n)
    new, reached, visited = lc.gba_propagate_keyframes([0], children, Tcw, Twc, in_gba, Tg)
    wn, wr, wv = lr.gba_propagate_keyframes([0], children, Tcw, Twc, in_gba, Tg)
    assert np.array_equal(reached, wr) and np.array_equal(visited, wv)
    assert reached.tolist() == [1, 1, 1, 1, 1, 1, 1, 1, 0] and visited.tolist() == [1, 1, 1, 1, 1, 1, 1, 0, 0]
    assert np.array_equal(new.view(np.uint32), wn.view(np.uint32))
    assert np.array_equal(new[6], Tg[6]) and np.array_equal(new[8], Tcw[8]) and not np.array_equal(new[4], Tg[4])
    assert np.array_equal(new[2], lr.mul44(lr.mul44(Tcw[2], Twc[1]), Tg[1]))
    # the order of the children is immaterial
    again = lc.gba_propagate_keyframes([0], [[5, 1]] + children[1:], Tcw, Twc, in_gba, Tg)
    assert all(np.array_equal(a, b) for a, b in zip(again, (new, reached, visited)))
    for ch, text in (([[1, 5], [2], [3], [1], [], [6], [], [], []], "visited twice"),     # a cycle
                     ([[1, 5], [2], [3], [4], [], [6, 2], [], [], []], "visited twice"),  # two parents
                     ([[1, 9], [2], [3], [4], [], [6], [], [], []], "child index outside")):
        with pytest.raises(OrbfeError, match=text):
            lc.gba_propagate_keyframes([0], ch, Tcw, Twc, in_gba, Tg)
        if "twice" in text:
            with pytest.raises(ValueError):
                lr.gba_propagate_keyframes([0], ch, Tcw, Twc, in_gba, Tg)
    with pytest.raises(OrbfeError, match="origin index outside"):
        lc.gba_propagate_keyframes([9], children, Tcw, Twc, in_gba, Tg)
    # an origin that was not in the GBA: as in the reference it receives whatever mTcwGBA holds and keeps its flag
    new, reached, visited = lc.gba_propagate_keyframes([8, 0], children, Tcw, Twc, in_gba, Tg)
    wn, wr, wv = lr.gba_propagate_keyframes([8, 0], children, Tcw, Twc, in_gba, Tg)
    assert np.array_equal(new.view(np.uint32), wn.view(np.uint32)) and np.array_equal(reached, wr) and np.array_equal(visited, wv)
    assert (reached[8], visited[8]) == (0, 1) and np.array_equal(new[8], Tg[8])


# ---- B2 ----
def test_gba_update_points_equals_the_restatement():
    rng = np.random.default_rng(8)
    p, m = 64, 5
    xw, pg = rng.uniform(-5, 5, (p, 3)).astype(f32), rng.uniform(-5, 5, (p, 3)).astype(f32)
    bad, ing = (rng.random(p) < 0.1).astype(np.uint8), (rng.random(p) < 0.5).astype(np.uint8)
    ref = rng.integers(-1, m, p).astype(np.int32)
    reached = np.array([1, 0, 1, 1, 0], np.uint8)
    Tb, _, Tn = gba_world(rng, m)
    out, moved = lc.gba_update_points(xw, bad, ing, pg, ref, reached, Tb, Tn)
    want, wm = lr.gba_update_points(xw, bad, ing, pg, ref, reached, Tb, Tn)
    assert np.array_equal(moved, wm) and set(moved.tolist()) == {0, 1, 2}
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(out[moved == 0], xw[moved == 0]) and np.array_equal(out[moved == 1], pg[moved == 1])
    with pytest.raises(OrbfeError, match="ref_kf outside"):
        lc.gba_update_points(xw, bad, ing, pg, np.full(p, m, np.int32), reached, Tb, Tn)
