"""k_octree keeps the counts of a (frame, level) item in 16 bits when the item lists at most 65535 candidates and leaves
the larger items to k_octree_wide (32-bit counts), launched behind it.  Through orbfe_debug_octree_device, form 1:

(a) the seam: n = 65535 and n = 65536 candidates on a few dozen distinct pixels of a small area with one root, so the
    root -- one node -- holds exactly 65535 keys (the largest 16-bit count) and 65536 keys (the first that needs 32 bits);
    one of the two sets of each size puts 65000 of them on ONE pixel, a count that stays that large down the tree;
(b) a narrow and a wide item as neighbouring frames of one launch;
(c) node lists filled to the end of the arrays: quotas N = 1 (mod 4) give a node capacity maxL = N + 3, and the sets
    end at N + 2 = maxL - 1 nodes, the longest list there is -- the largest-first pass starts one node short of N and
    its first split adds three before the early break.  The lattice sets of tests/octree_edges.py do exactly that.

Expected: the CPU oracle's DistributeOctTree (and the reference's recorded index lists for the lattice sets).  No
tolerance: count and ordered (x, y, response) are np.array_equal."""
import numpy as np
import pytest

import oracle_lib as orc
import ref_lib
from test_gpu_octree_edges import _assert_equals

pytestmark = pytest.mark.gpu

FORM = 1
# a 96 x 80 level: area 64 x 48, round(64 / 48) = 1 root
SMALL = (16, 80, 16, 64)
SEAM_N = 21  # 1 (mod 4): kpCap = maxL = 24


def _seam_set(name, n, heavy):
    """n candidates on 48 distinct pixels of the 64 x 48 area in raster order, responses 1..255, from a fixed seed;
    heavy: 65000 of them on the first pixel"""
    rng = np.random.default_rng([0x0C7EE16, heavy])
    pix = np.sort(rng.choice(64 * 48, 48, replace=False))
    if heavy:
        which = np.concatenate([np.zeros(65000, np.int64), rng.integers(1, 48, n - 65000)])
    else:
        which = rng.integers(0, 48, n)
    p = pix[np.sort(which)]
    return (name, p % 64, p // 64, rng.integers(1, 256, n), *SMALL, SEAM_N)


@pytest.fixture(scope="module")
def dev():
    from orb_slam2_annotate_amd import extractor
    return extractor


@pytest.fixture(scope="module")
def seam():
    """{name: (set, oracle index list)}, computed once and never written to"""
    out = {}
    for n in (65535, 65536):
        for heavy in (0, 1):
            s = _seam_set(f"n{n}_heavy{heavy}", n, heavy)
            idx = orc.distribute_octtree(*s[1:])
            idx.setflags(write=False)
            out[s[0]] = (s, idx)
    return out


def _run(dev, sets):
    assert len({s[4:9] for s in sets}) == 1
    return dev.debug_octree_device([s[1:4] for s in sets], *sets[0][4:9], form=FORM)


@pytest.mark.parametrize("heavy", (0, 1))
@pytest.mark.parametrize("n", (65535, 65536))
def test_count_type_seam(dev, seam, n, heavy):
    s, idx = seam[f"n{n}_heavy{heavy}"]
    assert len(s[1]) == n and len(idx) > 4
    assert dev.debug_octree_limits(*s[4:9], 1, n)["nIni"] == 1  # the root holds all n keys
    _assert_equals(_run(dev, [s])[0], s, idx)


@pytest.mark.parametrize("order", (("n65535_heavy0", "n65536_heavy1"), ("n65536_heavy0", "n65535_heavy1", "n65536_heavy1")))
def test_both_count_types_in_one_launch(dev, seam, order):
    sets = [seam[k][0] for k in order]
    for res, k in zip(_run(dev, sets), order):
        _assert_equals(res, *seam[k])


LATTICES = ("lattice_N5", "lattice_N17", "lattice_N65")


@pytest.mark.parametrize("name", LATTICES)
def test_node_list_filled_to_its_end(dev, name):
    s = {t[0]: t for t in ref_lib.octree_edge_sets()}[name]
    N = s[8]
    idx = orc.distribute_octtree(*s[1:])
    br = orc.octree_branch_counts()
    assert br["largest_first_entered"] == 1 and br["early_break"] == 1
    assert np.array_equal(ref_lib.recorded_octree_edges()[name], idx)
    d = dev.debug_octree_limits(*s[4:9], 1, len(s[1]))
    assert N % 4 == 1 and d["maxL"] == N + 3 and len(idx) == d["maxL"] - 1
    _assert_equals(_run(dev, [s])[0], s, idx)


def test_node_list_of_a_kitti_sized_level(dev):
    """the 4097 seeded pixels of octree_edges with the node capacity of a 2000-feature KITTI level (maxL = 440)"""
    s = {t[0]: t for t in ref_lib.octree_edge_sets()}["n4097"]
    s = (*s[:8], 437)
    idx = orc.distribute_octtree(*s[1:])
    br = orc.octree_branch_counts()
    assert br["largest_first_entered"] == 1 and br["early_break"] == 1
    assert dev.debug_octree_limits(*s[4:9], 1, 4097)["maxL"] == 440 and 437 <= len(idx) <= 439
    _assert_equals(_run(dev, [s])[0], s, idx)
