"""GPU: the loop correction on the resident map points -- orbfe_correct_loop_mappoints (the point loop at the head of
LoopClosing::CorrectLoop with UpdateNormalAndDepth) and orbfe_gba_update_mappoints (the map-point loop at the tail of
RunGlobalBundleAdjustment) -- against the sequential restatement in tests/loop_correct_ref.py and the array forms.

The engineered world: 6 listed key frames and 3 outside, kf_row_width 128, row_width 8, about 320 live points (more than one
256-lane workgroup of the correction pass).  The list order [30, 60, 10, 50, 20, 40] (mnIds) is neither slot order nor id
order.  Row 60 is empty, row 10 is full (128 entries), row 30 has NULL holes.  Normal and range cannot be read from the
table directly; they are compared through Frame::isInFrustum (ProjectInFrustum) on a second table filled with the
restatement's values, whose view_cos / level / in_view outputs depend on the normal and the range.  view_cos along three
axes pins the normal's components; the range reaches the comparison only through the predicted level and the in/out test,
so this check of min_dist / max_dist is coarse: a last-place error in them would pass."""
import copy

import numpy as np
import pytest

import loop_correct_ref as lr
import obsgraph_ref as orf
import orb_slam2_annotate_amd as amd
from orb_slam2_annotate_amd import OrbfeError, loop_closing as lc
from test_loop_correct_ref import SF, gba_world, inverse, pose, scw_of

pytestmark = pytest.mark.gpu

f32 = np.float32
IDS = [10, 20, 30, 40, 50, 60, 70, 80, 90]
SLOT_OF = {10: 5, 20: 2, 30: 7, 40: 0, 50: 8, 60: 3, 70: 1, 80: 6, 90: 4}
ORDER = [30, 60, 10, 50, 20, 40]  # ranks 0 .. 5
P_CAP, KF_CAP, KW, RW, N = 400, 12, 128, 8, 340
THREE, TWICE, BAD, UNSET, SKIP, MIXED, REFLOW, NOREF, PROBE = 0, 1, 2, 3, 4, 5, 6, 7, 8


def make_world():
    rng = np.random.default_rng(11)
    w = orf.World()
    for k in IDS:
        w.add_keyframe(k, rng.uniform(-2, 2, 3).astype(f32))
    rows = {k: [] for k in IDS[:6]}

    def point(pid, obs, ref, listed, bad=False):
        w.add_point(pid, ref=ref, bad=bad)
        for k in obs:
            w.add_observation(pid, k, int(rng.integers(0, 500)), int(rng.integers(0, 8)), bool(rng.integers(0, 2)))
        for k in listed:
            rows[k].append(pid)

    point(THREE, [50, 20, 40], 20, [50, 20, 40])  # rank 3 claims: id 50 is neither the lowest id (20) nor the lowest slot (40 -> 0)
    point(TWICE, [10, 70], 10, [10, 10])
    point(BAD, [10, 20], 10, [10, 20], bad=True)
    rows[20].append(UNSET)  # never given to set_points
    point(SKIP, [30, 10], 30, [30, 10])
    point(MIXED, [30, 50, 40, 70], 50, [50, 40])  # observers before (30), at (50), after (40) the claimant and outside (70)
    point(REFLOW, [30, 20], 30, [20])             # the reference key frame 30 (rank 0) is below the claimant 20 (rank 4)
    point(NOREF, [10, 20], 90, [10])              # the reference key frame is not in the row
    point(PROBE, [30, 60, 40, 80], 60, [])        # listed by nobody: stays as it is
    for pid in range(20, N):
        obs = rng.choice(IDS, int(rng.integers(2, 6)), replace=False).tolist()
        listed = [k for k in obs if k in rows and k != 60 and len(rows[k]) < 100 and rng.random() < 0.8]
        point(pid, obs, obs[int(rng.integers(0, len(obs)))], listed, bad=rng.random() < 0.03)
    for at in (3, 9, 10, 40):
        rows[30].insert(at, -1)
    while len(rows[10]) < KW:
        rows[10].append(int(rng.integers(20, N)))
    assert rows[60] == [] and len(rows[10]) == KW and all(len(r) <= KW for r in rows.values())
    pos = {pid: rng.uniform(-5, 5, 3).astype(f32) for pid in range(N)}
    Tiw = np.array([pose(rng) for _ in ORDER])
    cur = 3
    cor, non, _ = lc.correct_loop_sim3s(Tiw, inverse(Tiw[cur]), cur, scw_of(rng, Tiw[cur]))
    ow_new = rng.uniform(-2, 2, (len(ORDER), 3)).astype(f32)
    return dict(w=w, rows=rows, pos=pos, cor=cor, non=non, ow_new=ow_new)


def load(sc):
    """-> (graph, table) holding the world as it stands"""
    w = sc["w"]
    g = amd.ObservationGraph(P_CAP, KF_CAP, RW)
    orf.load(w, g, SLOT_OF, {p: p for p in w.pts})
    g.enable_keyframe_points(KW)
    for k, r in sc["rows"].items():
        g.set_keyframe_points(SLOT_OF[k], r)
    mp = amd.MapPoints(P_CAP)
    fill(mp, np.array([sc["pos"][p] for p in range(N)]), *base())
    return g, mp


def base():
    return np.tile(f32([0, 0, 1]), (N, 1)), np.full(N, 0.1, f32), np.full(N, 100.0, f32)


def fill(mp, pos, normal, lo, hi):
    mp.update(np.arange(N), pos, normal, lo, hi, np.zeros((N, 32), np.uint8), np.zeros(N, np.uint8))


def call(sc, g, mp, order=ORDER, skip=(SKIP,), sel=None, **kw):
    sel = list(range(len(order))) if sel is None else sel
    return mp.correct_loop(g, [SLOT_OF[k] for k in order], sc["cor"][sel], sc["non"][sel], sc["ow_new"][sel], SF, skip=skip, **kw)


def centres_at(sc, w0, order, sel, rank):
    """the world with the corrected centres of the key frames at a place below `rank`"""
    w = copy.deepcopy(w0)
    seen = set()
    for r, k in enumerate(order):
        if r < rank and k not in seen:
            w.kfs[k]["Ow"] = sc["ow_new"][sel[r]]
        seen.add(k)
    return w


def want_table(sc, w0, order, sel, ids, refs, got_pos, start):
    """normal / min / max per slot after the call: World.normal_depth at the positions read back, with the mixed centres"""
    normal, lo, hi = (a.copy() for a in start)
    valid = []
    for pid, r in zip(ids, refs):
        nd = centres_at(sc, w0, order, sel, r).normal_depth(pid, got_pos[pid], SF)
        valid.append(int(nd is not None))
        if nd is not None:
            normal[pid], lo[pid], hi[pid] = nd
    return normal, lo, hi, valid


VIEWS = [np.eye(3), np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0.0]]), np.array([[0, 0, 1], [1, 0, 0], [0, 1, 0.0]])]  # z = world z, x, y


def frustum(mp, slots, R, centre):
    p = amd.camera_pose(R, -(R @ np.asarray(centre, np.float64)), (500, 500, 320, 240), 40.0, (0, 640, 0, 480), 1.2, len(SF))
    return mp.ProjectInFrustum(slots, p, -2.0)


def same_tables(a, b):
    for R in VIEWS:
        x, y = frustum(a, np.arange(N), R, -14 * R[2]), frustum(b, np.arange(N), R, -14 * R[2])
        for k in x:
            assert np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)), k


def probe(mp, pid, P, d):
    """view_cos of one point seen from distance d along the three axes: the three components of its normal"""
    return [frustum(mp, [pid], R, np.asarray(P, np.float64) - d * R[2]) for R in VIEWS]


@pytest.fixture(scope="module")
def run():
    sc = make_world()
    w0 = copy.deepcopy(sc["w"])
    g, mp = load(sc)
    before = mp.positions(np.arange(N))
    got = call(sc, g, mp)
    w, pos = copy.deepcopy(w0), dict(sc["pos"])
    want = lr.correct_loop(w, ORDER, sc["rows"], sc["cor"], sc["non"], sc["ow_new"], pos, (SKIP,), SF)
    return dict(sc=sc, w0=w0, g=g, mp=mp, before=before, got=got, want=want, want_pos=pos, w_after=w)


def test_the_claim_equals_the_sequential_loop(run):
    slots, ref, valid = run["got"]
    ids, refs, wvalid, _ = run["want"]
    assert slots.tolist() == ids and ref.tolist() == refs and valid.tolist() == wvalid
    assert len(ids) > 256 and 0 in wvalid
    at = {p: r for p, r in zip(ids, refs)}
    assert at[THREE] == 3 and at[MIXED] == 3 and at[REFLOW] == 4 and at[TWICE] == 2 and ids.count(TWICE) == 1
    assert not {BAD, UNSET, SKIP, PROBE} & set(ids)
    assert valid[ids.index(NOREF)] == 0 and valid[ids.index(MIXED)] == 1 and valid[ids.index(REFLOW)] == 1


def test_positions(run):
    sc, ids = run["sc"], run["want"][0]
    got = run["mp"].positions(np.arange(N))
    want = np.array([run["want_pos"][p] for p in range(N)])
    assert np.abs(got - want).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(want).max())
    skip = np.array([int(p in (SKIP, UNSET) or p not in sc["w"].pts or sc["w"].pts[p]["bad"]) for p in range(N)], np.uint8)
    arr, aref = lc.correct_loop_points(sc["cor"], sc["non"], [sc["rows"][k] for k in ORDER], run["before"], skip)
    assert np.array_equal(got.view(np.uint32), arr.view(np.uint32))  # bit-equal to the array form on the same floats
    assert sorted(np.flatnonzero(aref >= 0).tolist()) == sorted(ids) and all(aref[p] == r for p, r in zip(ids, run["want"][1]))
    untouched = np.setdiff1d(np.arange(N), ids)
    assert np.array_equal(got[untouched].view(np.uint32), run["before"][untouched].view(np.uint32))
    assert not np.array_equal(got[NOREF], run["before"][NOREF])  # valid = 0, the position is still corrected


def test_normal_and_range_follow_the_mixed_centre_rule(run):
    sc, (ids, refs, wvalid, _) = run["sc"], run["want"]
    sel = list(range(len(ORDER)))
    got = run["mp"].positions(np.arange(N))
    normal, lo, hi, valid = want_table(sc, run["w0"], ORDER, sel, ids, refs, got, base())
    assert valid == wvalid
    mw = amd.MapPoints(P_CAP)
    fill(mw, got, normal, lo, hi)
    same_tables(run["mp"], mw)  # unclaimed slots and valid = 0 slots keep the base normal and range
    # the mixed rule is observable: all-old and all-new centres give other normals for MIXED, another range for REFLOW
    old, new = run["w0"].normal_depth(MIXED, got[MIXED], SF), run["w_after"].normal_depth(MIXED, got[MIXED], SF)
    assert not np.array_equal(normal[MIXED], old[0]) and not np.array_equal(normal[MIXED], new[0])
    assert hi[REFLOW] != run["w0"].normal_depth(REFLOW, got[REFLOW], SF)[2]
    assert hi[REFLOW] == run["w_after"].normal_depth(REFLOW, got[REFLOW], SF)[2]
    for pid, others in ((MIXED, (old, new)), (REFLOW, (run["w0"].normal_depth(REFLOW, got[REFLOW], SF),))):
        d = float(lo[pid] + hi[pid]) / 2
        a, b = probe(run["mp"], pid, got[pid], d), probe(mw, pid, got[pid], d)
        assert all(x["in_view"][0] == 1 for x in a)
        for x, y in zip(a, b):
            assert all(np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)) for k in x)
        for o in others:  # a table that holds the other rule's values answers differently
            alt = (normal.copy(), lo.copy(), hi.copy())
            alt[0][pid], alt[1][pid], alt[2][pid] = o
            fill(mw, got, *alt)
            c = probe(mw, pid, got[pid], d)
            assert any(not np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)) for x, y in zip(a, c) for k in x)
        fill(mw, got, normal, lo, hi)


def test_the_graph_holds_the_corrected_centres(run):
    P = f32([0.3, -0.7, 4.0])
    normal, lo, hi, valid = run["g"].update_normal_depth([PROBE], SF, P[None])
    want = run["w_after"].normal_depth(PROBE, P, SF)
    assert valid[0] == 1 and np.array_equal(normal[0].view(np.uint32), want[0].view(np.uint32))
    assert lo[0] == want[1] and hi[0] == want[2]
    assert not np.array_equal(normal[0], run["w0"].normal_depth(PROBE, P, SF)[0])


def test_two_calls_on_equal_state_give_equal_bits(run):
    sc = run["sc"]
    g, mp = load(sc)
    again = call(sc, g, mp)
    assert all(np.array_equal(a, b) for a, b in zip(again, run["got"]))
    assert np.array_equal(mp.positions(np.arange(N)).view(np.uint32), run["mp"].positions(np.arange(N)).view(np.uint32))
    same_tables(mp, run["mp"])


def test_one_key_frame_then_another_list(run):
    """K = 1 (the current key frame alone), then a list in another order with the first call's points skipped and a kf slot
    named twice: the second call must not see the first one's ranks, and the current key frame is not first in its list."""
    sc = run["sc"]
    g, mp = load(sc)
    w, pos = copy.deepcopy(run["w0"]), dict(sc["pos"])
    first = call(sc, g, mp, order=[50], skip=(), sel=[3])
    want1 = lr.correct_loop(w, [50], sc["rows"], sc["cor"][[3]], sc["non"][[3]], sc["ow_new"][[3]], pos, (), SF)
    assert first[0].tolist() == want1[0] and first[1].tolist() == want1[1] == [0] * len(want1[0]) and first[2].tolist() == want1[2]
    order, sel = [40, 20, 10, 20, 30, 60], [5, 4, 2, 4, 0, 1]
    w1 = copy.deepcopy(w)
    second = call(sc, g, mp, order=order, skip=first[0], sel=sel)
    want2 = lr.correct_loop(w, order, sc["rows"], sc["cor"][sel], sc["non"][sel], sc["ow_new"][sel], pos, set(want1[0]), SF)
    assert second[0].tolist() == want2[0] and second[1].tolist() == want2[1] and second[2].tolist() == want2[2]
    assert len(want2[0]) > 100 and 3 not in want2[1]  # place 3 is key frame 20 again
    got = mp.positions(np.arange(N))
    wpos = np.array([pos[p] for p in range(N)])
    assert np.abs(got - wpos).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(wpos).max())
    start = want_table(sc, run["w0"], [50], [3], want1[0], want1[1], got, base())[:3]
    normal, lo, hi, valid = want_table(sc, w1, order, sel, want2[0], want2[1], got, start)
    assert valid == want2[2]
    mw = amd.MapPoints(P_CAP)
    fill(mw, got, normal, lo, hi)
    same_tables(mp, mw)


def test_a_short_capacity_leaves_everything_untouched(run):
    sc = run["sc"]
    g, mp = load(sc)
    with pytest.raises(OrbfeError, match="capacity") as e:
        call(sc, g, mp, capacity=len(run["want"][0]) - 1)
    assert e.value.code == -2
    assert np.array_equal(mp.positions(np.arange(N)).view(np.uint32), run["before"].view(np.uint32))
    P = f32([0.3, -0.7, 4.0])
    assert np.array_equal(g.update_normal_depth([PROBE], SF, P[None])[0][0], run["w0"].normal_depth(PROBE, P, SF)[0])
    again = call(sc, g, mp)  # and the rank table is idle again
    assert all(np.array_equal(a, b) for a, b in zip(again, run["got"]))


def test_refusals(run):
    sc = run["sc"]
    g, mp = load(sc)
    with pytest.raises(OrbfeError, match="kf slot outside"):
        mp.correct_loop(g, [KF_CAP], sc["cor"][:1], sc["non"][:1], sc["ow_new"][:1], SF)
    with pytest.raises(OrbfeError, match="never set"):
        mp.correct_loop(g, [9], sc["cor"][:1], sc["non"][:1], sc["ow_new"][:1], SF)
    bad = sc["cor"].copy()
    bad[2, 7] = 0
    with pytest.raises(OrbfeError, match="scale"):
        mp.correct_loop(g, [SLOT_OF[k] for k in ORDER], bad, sc["non"], sc["ow_new"], SF)
    bad[2, 7] = np.nan
    with pytest.raises(OrbfeError, match="not finite"):
        mp.correct_loop(g, [SLOT_OF[k] for k in ORDER], bad, sc["non"], sc["ow_new"], SF)
    with pytest.raises(OrbfeError, match="octave is not below n_levels"):
        mp.correct_loop(g, [SLOT_OF[k] for k in ORDER], sc["cor"], sc["non"], sc["ow_new"], SF[:3])
    with pytest.raises(OrbfeError, match="skip slot outside"):
        call(sc, g, mp, skip=(P_CAP,))
    plain = amd.ObservationGraph(P_CAP, KF_CAP, RW)
    with pytest.raises(OrbfeError, match="not enabled"):
        mp.correct_loop(plain, [], sc["cor"][:0], sc["non"][:0], sc["ow_new"][:0], SF)
    assert np.array_equal(mp.positions(np.arange(N)).view(np.uint32), run["before"].view(np.uint32))


def test_the_chain_correct_loop_essential_graph_correct_fuse(run):
    """slot_out / ref_out feed orbfe_essential_graph_correct_mappoints (ref_vertex = ref_out), and ORBmatcher::Fuse on the table
    the chain leaves equals Fuse on a table filled through update() with the restatement's positions, normals and ranges,
    given the same graph."""
    import essgraph_ref as er
    sc = run["sc"]
    g, mp = load(sc)
    rng = np.random.default_rng(13)
    desc = rng.integers(0, 256, (N, 32), dtype=np.uint8)
    flags = np.zeros(N, np.uint8)
    mp.update(np.arange(N), np.array([sc["pos"][p] for p in range(N)]), *base(), desc, flags)  # as load(), with descriptors
    slots, ref, valid = call(sc, g, mp)
    out = sc["cor"].copy()
    out[:, 4:7] += rng.normal(size=(len(out), 3)) * 0.05  # the optimised Sim3s of the essential graph
    mp.essential_graph_correct(slots, sc["cor"], out, ref)
    # the restatement's table
    w, pos = copy.deepcopy(run["w0"]), dict(sc["pos"])
    ids, refs, wvalid, nd = lr.correct_loop(w, ORDER, sc["rows"], sc["cor"], sc["non"], sc["ow_new"], pos, (SKIP,), SF)
    assert slots.tolist() == ids and ref.tolist() == refs
    wpos = np.array([pos[p] for p in range(N)])
    wpos[ids] = er.correct_points(sc["cor"], out, wpos[ids], refs)
    normal, lo, hi = base()
    for p, r in nd.items():
        normal[p], lo[p], hi[p] = r
    got = mp.positions(np.arange(N))
    assert np.abs(got - wpos).max() <= 4 * 2.0 ** -23 * max(1.0, np.abs(wpos).max())
    mw = amd.MapPoints(P_CAP)
    mw.update(np.arange(N), wpos, normal, lo, hi, desc, flags)
    # two key frames outside the list look at the cloud; every chosen point has a keypoint on its projection at every octave
    K4, bounds = (500.0, 500.0, 320.0, 240.0), (0, 640, 0, 480)
    frames, poses = [], []
    for R in VIEWS[:2]:
        t = 14 * R @ R[2]
        poses.append(amd.camera_pose(R, t, K4, 40.0, bounds, 1.2, len(SF)))
        Xc = (R @ wpos.T.astype(np.float64)).T + t
        pick = np.arange(0, N, 3)
        u, v = 500 * Xc[pick, 0] / Xc[pick, 2] + 320, 500 * Xc[pick, 1] / Xc[pick, 2] + 240
        x, y = np.repeat(u, 8).astype(f32), np.repeat(v, 8).astype(f32)
        octave = np.tile(np.arange(8), len(pick)).astype(np.int32)
        frames.append(amd.FrameView(x, y, octave, np.repeat(desc[pick], 8, axis=0), bounds, angle=np.zeros(len(x), f32),
                                    u_right=np.full(len(x), -1, f32)))
    kw = dict(graph=g, kf_slot=[SLOT_OF[70], SLOT_OF[80]], scale_factors=SF, inv_level_sigma2=(1 / SF.astype(np.float64) ** 2).astype(f32))
    a, b = mp.fuse(frames, poses, np.arange(N), **kw), mw.fuse(frames, poses, np.arange(N), **kw)
    assert np.array_equal(a, b) and (a >= 0).sum() > 20 and (a[:, ids] >= 0).sum() > 5


# ---- the map update of the global bundle adjustment ----
def test_gba_update_equals_the_array_form_and_the_restatement(run):
    sc, w = run["sc"], copy.deepcopy(run["w0"])
    g, mp = load(sc)
    rng = np.random.default_rng(12)
    slots = np.array(sorted(w.pts) + [UNSET], np.int32)  # distinct; more than 300
    rng.shuffle(slots)
    n = len(slots)
    in_gba = (rng.random(n) < 0.6).astype(np.uint8)
    pos_gba = rng.uniform(-5, 5, (n, 3)).astype(f32)
    compact = [30, 10, 70, 50, 20]  # 40, 60, 80, 90 are outside the compact list
    reached = np.array([1, 1, 0, 1, 1], np.uint8)
    Tb, _, Tn = gba_world(rng, len(compact))
    for pid, flag in ((THREE, 1), (REFLOW, 0), (TWICE, 0), (NOREF, 0), (BAD, 0), (UNSET, 1)):
        in_gba[np.flatnonzero(slots == pid)[0]] = flag
    w.pts[TWICE]["ref"] = 70   # not reached
    g.set_points([TWICE], [0], [SLOT_OF[70]])
    w.pts[MIXED]["ref"] = -1   # no reference key frame
    g.set_points([MIXED], [0], [-1])
    in_gba[np.flatnonzero(slots == MIXED)[0]] = 0
    before = mp.positions(slots)
    moved = mp.gba_update(g, slots, in_gba, pos_gba, [SLOT_OF[k] for k in compact], reached, Tb, Tn)
    bad = np.array([int(p not in w.pts or w.pts[p]["bad"]) for p in slots], np.uint8)
    ref = np.array([compact.index(w.pts[p]["ref"]) if p in w.pts and w.pts[p]["ref"] in compact else -1 for p in slots], np.int32)
    arr, amoved = lc.gba_update_points(before, bad, in_gba, pos_gba, ref, reached, Tb, Tn)
    want, wmoved = lr.gba_update_points(before, bad, in_gba, pos_gba, ref, reached, Tb, Tn)
    assert np.array_equal(moved, amoved) and np.array_equal(amoved, wmoved) and n > 300
    at = {int(p): int(m) for p, m in zip(slots, moved)}
    assert (at[THREE], at[REFLOW], at[TWICE], at[NOREF], at[BAD], at[UNSET], at[MIXED]) == (1, 2, 0, 0, 0, 0, 0)
    assert (moved == 2).sum() > 20 and (moved == 0).sum() > 20
    got = mp.positions(slots)
    assert np.array_equal(got.view(np.uint32), arr.view(np.uint32)) and np.array_equal(arr.view(np.uint32), want.view(np.uint32))
    with pytest.raises(OrbfeError, match="named twice"):
        mp.gba_update(g, np.r_[slots, slots[:1]], np.r_[in_gba, 0].astype(np.uint8), np.r_[pos_gba, pos_gba[:1]],
                      [SLOT_OF[k] for k in compact], reached, Tb, Tn)
    assert np.array_equal(mp.positions(slots).view(np.uint32), got.view(np.uint32))
    # the index table is idle again: a loop correction behind it gives what a fresh pair gives on the same state
    g2, mp2 = load(sc)
    g2.set_points([TWICE, MIXED], [0, 0], [SLOT_OF[70], -1])
    fill(mp2, mp.positions(np.arange(N)), *base())
    assert all(np.array_equal(a, b) for a, b in zip(call(sc, g, mp), call(sc, g2, mp2)))
