"""Every device form of DistributeOctTree (csrc/k_octree.hip) on the candidate sets of tests/octree_edges.py, through
orbfe_debug_octree_device: form 0 (what launch_octree picks), 1 k_octree, 2 k_octree_reg (register branch up to 4096
candidates, global-memory branch above), 3 k_octree_reg1024 (register branch up to 8192), 4 k_octree_global.

Count and ordered (x, y, response) are np.array_equal with the oracle's answer, and with the reference's recorded index
list for the sets inside its domain: no tolerance, no set excused.  The one permitted non-comparison: forms 1-3 must
REFUSE the node-list set whose list exceeds the LDS limit (ORBFE_ERR_INVALID).

What the kernels document about their output array is asserted on every run (_ordered): the first `count` slots are in
spatial order (128-pixel column strip, row, column of the level coordinate), `rank` is a permutation of the reference's
list positions, and the slots from `count` to kpCap are never written -- they keep the entry's 0xFF fill.

tests/test_octree_edges.py (CPU) shows that every set reaches the branch it was built for."""
import numpy as np
import pytest

import octree_edges as oe
import oracle_lib as orc
import ref_lib

pytestmark = pytest.mark.gpu

FORMS = (0, 1, 2, 3, 4)
BASE = oe.base_sets()
BASE_ENGINEERED = [s[0] for s in BASE if not s[0].startswith("random")]


@pytest.fixture(scope="module")
def dev():
    from orb_slam2_annotate_amd import extractor
    return extractor


@pytest.fixture(scope="module")
def world():
    """{name: (set, oracle index list)}: the reference answers, computed once and never written to"""
    out = {}
    for s in BASE + ref_lib.octree_edge_sets():
        idx = orc.distribute_octtree(*s[1:])
        idx.setflags(write=False)
        out[s[0]] = (s, idx)
    return out


def _ordered(res, kp_min_x, kp_min_y):
    """(x, y, response) of one frame's result in the reference's list order, after the checks of the output array"""
    n = res["count"]
    assert 0 <= n <= len(res["x"])
    x, y, r, rank = (res[k][:n].astype(np.int64) for k in ("x", "y", "resp", "rank"))
    assert np.array_equal(np.sort(rank), np.arange(n)), "rank is not a permutation of the list positions"
    lx, ly = x - kp_min_x + 16, y - kp_min_y + 16  # level coordinates of the kernel (kMinBorder = 16)
    key = ((lx >> 7) << 23) | (ly << 7) | (lx & 127)
    assert np.all(np.diff(key) > 0), "slots are not in spatial order"
    for k in ("x", "y", "resp", "rank"):
        assert np.all(res[k][n:] == 0xFFFF), f"{k}: a slot past the count was written"
    o = np.argsort(rank)
    return x[o], y[o], r[o]


def _assert_equals(res, s, idx):
    _, xs, ys, rs, minX, _, minY, _, _ = s
    x, y, r = _ordered(res, minX, minY)
    assert len(x) == len(idx), f"{s[0]}: {len(x)} keypoints, oracle {len(idx)}"
    assert np.array_equal(x, xs[idx] + minX) and np.array_equal(y, ys[idx] + minY) and np.array_equal(r, rs[idx]), s[0]


def _run_alone(dev, s, form):
    return dev.debug_octree_device([s[1:4]], *s[4:9], form=form)[0]


def _admits(dev, s, form):
    """forms 1-3 keep the node list in LDS; form 0 and 4 take every set"""
    d = dev.debug_octree_limits(*s[4:9], 1, len(s[1]))
    return form in (0, 4) or d["lds_bytes"] <= d["lds_limit"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", oe.EDGE_NAMES)
def test_edge_set_on_form(dev, world, name, form):
    from orb_slam2_annotate_amd import _lib
    s, idx = world[name]
    if not _admits(dev, s, form):
        assert name == oe.NODELIST_SETS[1]  # the only set a form may refuse
        with pytest.raises(_lib.OrbfeError) as ei:
            _run_alone(dev, s, form)
        assert ei.value.code == _lib.ERR_INVALID
        return
    _assert_equals(_run_alone(dev, s, form), s, idx)
    if name not in oe.OUT_OF_DOMAIN:
        assert np.array_equal(ref_lib.recorded_octree_edges()[name], idx)


def test_form_0_moves_to_the_global_form_at_the_node_list_seam(dev, world):
    last, first = (world[n][0] for n in oe.NODELIST_SETS)
    assert dev.debug_octree_limits(*last[4:9], 1, len(last[1]))["form"] == 3
    assert dev.debug_octree_limits(*first[4:9], 1, len(first[1]))["form"] == 4
    assert dev.debug_octree_limits(*last[4:9], 9, len(last[1]))["form"] == 1
    for form in (1, 2, 3):
        assert _admits(dev, last, form) and not _admits(dev, first, form)


@pytest.mark.parametrize("form", FORMS)
def test_earlier_engineered_sets_on_form(dev, world, form):
    recorded = dict(zip([s[0] for s in BASE], ref_lib.recorded_octree()))
    for name in BASE_ENGINEERED:
        s, idx = world[name]
        assert np.array_equal(recorded[name], idx), name
        _assert_equals(_run_alone(dev, s, form), s, idx)


@pytest.mark.parametrize("form", FORMS)
def test_seeded_sets_on_form(dev, world, form):
    """the 200 seeded sets of ref_lib.octree_sets(), one launch each (every set has its own area and quota)"""
    recorded = dict(zip([s[0] for s in BASE], ref_lib.recorded_octree()))
    names = [s[0] for s in BASE if s[0].startswith("random")]
    assert len(names) == 200
    for name in names:
        s, idx = world[name]
        assert np.array_equal(recorded[name], idx), name
        _assert_equals(_run_alone(dev, s, form), s, idx)


@pytest.mark.parametrize("F", (8, 9))
@pytest.mark.parametrize("form", (0, 1, 2, 3, 4))
def test_neighbours_in_one_launch(dev, form, F):
    """an empty, a one-point, a 4097-point and the equal-sized-nodes set as frames of one launch: each frame's result is
    the result of the same set run alone, and the oracle's.  F = 8 is the last latency size of form 0, F = 9 its first
    throughput size."""
    assert dev.debug_octree_limits(*oe.AREA, oe.NEIGHBOUR_N, F)["form"] == (3 if F <= 8 else 1)
    frames = oe.neighbour_frames(F)
    together = dev.debug_octree_device(frames, *oe.AREA, oe.NEIGHBOUR_N, form=form)
    alone = {}
    for f, (fr, res) in enumerate(zip(frames, together)):
        s = (f"frame{f}", *fr, *oe.AREA, oe.NEIGHBOUR_N)
        if len(fr[0]) not in alone:
            alone[len(fr[0])] = (_run_alone(dev, s, form), orc.distribute_octtree(*s[1:]))
        single, idx = alone[len(fr[0])]
        assert res["count"] == single["count"]
        for k in ("x", "y", "resp", "rank"):
            assert np.array_equal(res[k], single[k]), (f, k)
        _assert_equals(res, s, idx)


@pytest.mark.parametrize("form", FORMS)
def test_two_calls_give_the_same_bytes(dev, world, form):
    name = {0: "equal_sized_nodes", 1: "lattice_N17", 2: "n4097", 3: "n8193", 4: "equal_responses"}[form]
    s = world[name][0]
    a, b = _run_alone(dev, s, form), _run_alone(dev, s, form)
    assert a["count"] == b["count"] > 0
    for k in ("x", "y", "resp", "rank"):
        assert a[k].tobytes() == b[k].tobytes(), k
