"""The engineered candidate sets of tests/octree_edges.py on the CPU: every new set gives the same ordered keypoints from
the oracle (orc_distribute_octtree), the product's host octree (orbfe_debug_octree_host) and, inside the reference's
domain, the reference's recorded index list (tests/golden/orbextractor_ref.npz); every engineered set, old and new,
reaches the branch it was built for (orc_octree_branch_counts), and every counter is reached by some set.

No branch is unreachable: octree_edges.UNREACHABLE is empty and test_every_counter_is_reached asserts all of them.
The GPU forms meet the same sets in tests/test_gpu_octree_edges.py."""
import ctypes as C

import numpy as np
import pytest

import octree_edges as oe
import oracle_lib as orc
import ref_lib
from test_orbextractor_ref import _assert_product_octree

BASE = oe.base_sets()


@pytest.fixture(scope="module")
def edge_sets():
    return ref_lib.octree_edge_sets()


@pytest.fixture(scope="module")
def counted(edge_sets):
    """{name: (oracle index list, counters)} of every set, old and new"""
    out = {}
    for s in BASE + edge_sets:
        idx = orc.distribute_octtree(*s[1:])
        out[s[0]] = (idx, orc.octree_branch_counts())
    return out


def test_names_and_sizes(edge_sets):
    assert tuple(s[0] for s in edge_sets) == oe.EDGE_NAMES and len(set(oe.EDGE_NAMES)) == len(oe.EDGE_NAMES)
    assert not set(oe.EDGE_NAMES) & {s[0] for s in BASE}
    by = {s[0]: s for s in edge_sets}
    for n in oe.SIZE_SEAMS:
        s = by[f"n{n}"]
        assert len(s[1]) == n and s[8] == 150 and s[4:8] == oe.AREA
        assert len(np.unique(s[2] * 608 + s[1])) == n and np.all(np.diff(s[2] * 608 + s[1]) > 0)  # distinct, raster order
    assert max(len(s[1]) for s in edge_sets) == 8193
    assert by["N_is_0"][8] == 0 and by["N_equals_n"][8] == len(by["N_equals_n"][1])
    assert by["N_is_n_plus_1"][8] == len(by["N_is_n_plus_1"][1]) + 1
    for s in edge_sets:
        assert s[1].min(initial=0) >= 0 and s[1].max(initial=0) <= s[5] - s[4], s[0]
        assert s[2].min(initial=0) >= 0 and s[2].max(initial=0) <= s[7] - s[6], s[0]
        assert s[3].min(initial=1) >= 1 and s[3].max(initial=1) <= 255, s[0]
    assert {8190, 8191, 8192, 8193} <= set(by["coord_x_8192"][1]) and {8190, 8191, 8192, 8193} <= set(by["coord_y_8192"][2])
    assert set(by["resp_all_255"][3]) == {255} and set(by["resp_all_1"][3]) == {1}


def test_node_list_seam_comes_from_the_library(edge_sets):
    from orb_slam2_annotate_amd.extractor import debug_octree_limits
    by = {s[0]: s for s in edge_sets}
    last, first = by[oe.NODELIST_SETS[0]], by[oe.NODELIST_SETS[1]]
    assert first[8] == last[8] + 1
    a, b = debug_octree_limits(*oe.AREA, last[8]), debug_octree_limits(*oe.AREA, first[8])
    assert a["lds_bytes"] <= a["lds_limit"] < b["lds_bytes"] and a["lds_limit"] == b["lds_limit"]
    assert a["form"] == 3 and b["form"] == 4  # form 0 of a one-frame launch moves to k_octree_global between the two
    assert debug_octree_limits(*oe.AREA, last[8], 9)["form"] == 1 and debug_octree_limits(*oe.AREA, first[8], 9)["form"] == 4
    assert debug_octree_limits(*oe.AREA, 150, 8)["form"] == 3 and debug_octree_limits(*oe.AREA, 150, 9)["form"] == 1
    assert len(last[1]) > b["kpCap"] >= a["kpCap"] == last[8] + 3  # enough points to fill either list


def test_out_of_domain_sets_are_marked(edge_sets):
    for s in edge_sets:
        if s[0] in oe.OUT_OF_DOMAIN:
            with pytest.raises(ValueError):
                ref_lib.check_octree_domain(*s[4:8])
        else:
            ref_lib.check_octree_domain(*s[4:8])
    assert [s[0] for s in ref_lib.octree_edge_sets_in_domain()] == [n for n in oe.EDGE_NAMES if n not in oe.OUT_OF_DOMAIN]


@pytest.mark.parametrize("name", oe.EDGE_NAMES)
def test_oracle_host_octree_and_recorded_reference_agree(edge_sets, counted, name):
    s = edge_sets[oe.EDGE_NAMES.index(name)]
    idx = counted[name][0]
    _assert_product_octree(s, idx)
    if name in oe.OUT_OF_DOMAIN:
        assert len(idx) == 0
    else:
        assert np.array_equal(ref_lib.recorded_octree_edges()[name], idx)
    if name in oe.CLUSTER_WINNERS:  # the cluster node is the last of the list
        assert idx[-1] == oe.CLUSTER_WINNERS[name]


def test_live_recording_of_the_edge_sets_equals_fresh_computation():
    if not ref_lib.reference_present():
        pytest.skip(f"no reference tree at {ref_lib.REF_TREE}")
    ref_lib.build_ref()
    rec = ref_lib.recorded_octree_edges()
    for s in ref_lib.octree_edge_sets_in_domain():
        assert np.array_equal(ref_lib.ref_octree(*s[1:]), rec[s[0]]), s[0]


def test_every_engineered_set_reaches_its_branch(edge_sets, counted):
    engineered = [s[0] for s in BASE if not s[0].startswith("random")] + list(oe.EDGE_NAMES)
    assert sorted(oe.TARGETS) == sorted(engineered)
    for name in engineered:
        c = counted[name][1]
        assert set(oe.TARGETS[name]) <= set(orc.OCTREE_BRANCHES), name
        for k, want in oe.TARGETS[name].items():
            assert (c[k] > 0) if want == 0 else (c[k] == want), (name, k, c[k])
    assert not any(counted["narrow_area_0_roots"][1].values())
    # the situations in words: the sets built around N end where they were meant to
    for N in (4, 16, 64, 256):
        assert len(counted[f"lattice_N{N}"][0]) == N
    for N in (3, 15, 63):
        assert len(counted[f"lattice_N{N}"][0]) == N + 1
    for N in (5, 17, 65):
        assert len(counted[f"lattice_N{N}"][0]) == N + 2
    assert len(counted["lattice_N257"][0]) == 256 and len(counted["N_is_0"][0]) == 4
    assert len(counted["N_equals_n"][0]) == len(counted["N_is_n_plus_1"][0]) == 299
    assert len(counted["largest_first_no_growth"][0]) == 4
    for n in oe.NODELIST_SETS:
        s = edge_sets[oe.EDGE_NAMES.index(n)]
        assert s[8] <= len(counted[n][0]) <= s[8] + 2


def test_every_counter_is_reached(counted):
    for k in orc.OCTREE_BRANCHES:
        hit = [n for n, (_, c) in counted.items() if c[k] > 0]
        if k in oe.UNREACHABLE:
            assert not hit, (k, hit[:3])
        else:
            assert hit, k
    assert set(oe.UNREACHABLE) <= set(orc.OCTREE_BRANCHES)


def test_counters_belong_to_the_last_call_and_change_no_result(edge_sets):
    by = {s[0]: s for s in BASE}
    a = orc.distribute_octtree(*by["equal_sized_nodes"][1:])
    c1 = orc.octree_branch_counts()
    orc.distribute_octtree(*by["one_point"][1:])
    assert orc.octree_branch_counts() != c1 and orc.octree_branch_counts()["roots"] == 1
    assert np.array_equal(orc.distribute_octtree(*by["equal_sized_nodes"][1:]), a) and orc.octree_branch_counts() == c1
    out = (C.c_int64 * 2)(-7, -7)
    assert orc.lib().orc_octree_branch_counts(out, 1) == len(orc.OCTREE_BRANCHES) and out[1] == -7
    # the recorded reference lists of the earlier sets were made before the counters existed: still the oracle's answers
    for s, rec in list(zip(BASE, ref_lib.recorded_octree()))[::7]:
        assert np.array_equal(orc.distribute_octtree(*s[1:]), rec), s[0]


def test_neighbour_and_small_item_lists():
    for F in (8, 9):
        fr = oe.neighbour_frames(F)
        assert len(fr) == F and {len(f[0]) for f in fr} == {0, 1, 4097, 144}
    items = oe.small_items(300)
    assert len(items) == 300 and max(len(i[0]) for i in items) <= 500
