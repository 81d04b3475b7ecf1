"""The node-array layout of the octree kernels (octree_carve, csrc/kernels.h) against octree_lds_bytes, on the host.

The kernels carve their LDS with octree_carve and octree_lds_bytes returns its end + 64, so the two cannot drift apart;
orbfe_debug_octree_carve hands out both.  Checked here for 16-bit (k_octree) and 32-bit counts: the arrays follow each
other without overlap at the element sizes the kernel uses, the alignments the kernel relies on hold, the byte budget is
what DESIGN.md states, and the 32-bit figure is the one the form choice (debug_octree_limits) reports."""
import pytest

from orb_slam2_annotate_amd import extractor as ex

ARRAYS = ("rect0", "rect1", "cnt0", "cnt1", "child", "scanA", "scanB", "order", "inS")
# node capacities: the smallest, KITTI / TUM sized ones, one above 64 KB of LDS, the largest the LDS forms take
CAPACITIES = (4, 8, 224, 440, 444, 1872, 2888)


def _sizes(M, c):
    """bytes of each array for M nodes and counts of c bytes, from the element types in octree_body"""
    return {"rect0": 8 * M, "rect1": 8 * M, "cnt0": c * M, "cnt1": c * M, "child": 4 * c * M, "scanA": c * M,
            "scanB": c * M, "order": 2 * M, "inS": M}


@pytest.mark.parametrize("narrow", (True, False))
@pytest.mark.parametrize("M", CAPACITIES)
def test_carve_is_dense_and_lds_bytes_is_its_end(M, narrow):
    c = 2 if narrow else 4
    cv, size = ex.debug_octree_carve(M, narrow), _sizes(M, c)
    at = 0
    for name in ARRAYS:  # each array starts where the one before ends
        assert cv[name] == at, (name, cv)
        at += size[name]
    # 32-bit counts keep two unused bytes per node (the size at which the forms move to global memory is pinned)
    assert cv["end"] == at + (0 if narrow else 2 * M)
    assert cv["lds_bytes"] == cv["end"] + 64
    assert cv["end"] == (35 if narrow else 53) * M
    if narrow:
        assert cv["end"] <= 36 * M  # the budget the 16-bit form was given


@pytest.mark.parametrize("narrow", (True, False))
@pytest.mark.parametrize("M", CAPACITIES)
def test_alignment_and_shared_storage(M, narrow):
    c = 2 if narrow else 4
    cv = ex.debug_octree_carve(M, narrow)
    assert cv["rect0"] % 8 == 0 and cv["rect1"] % 8 == 0      # 8-byte rectangles
    assert cv["child"] % 16 == 0                               # a node's four child counts are cleared together
    for name in ("cnt0", "cnt1", "child", "scanA", "scanB"):   # 16-bit counts are added as halves of aligned 32-bit words
        assert cv[name] % 4 == 0, name
    assert cv["order"] % 2 == 0
    # best[M] (int32) lies over child, skey[M] (uint32) over cnt[0] ++ cnt[1]
    assert cv["scanA"] - cv["child"] >= 4 * M
    assert cv["cnt1"] == cv["cnt0"] + c * M and cv["child"] - cv["cnt0"] >= 4 * M


def test_the_form_choice_reports_the_32_bit_figure():
    for N in (17, 437, 1000):
        d = ex.debug_octree_limits(16, 624, 16, 464, N)
        assert d["lds_bytes"] == ex.debug_octree_carve(d["maxL"], False)["lds_bytes"]
        assert ex.debug_octree_carve(d["maxL"], True)["lds_bytes"] < d["lds_bytes"]


def test_bad_capacities_are_refused():
    from orb_slam2_annotate_amd import _lib
    for M in (0, 3, 6, 65536):
        with pytest.raises(_lib.OrbfeError) as ei:
            ex.debug_octree_carve(M, True)
        assert ei.value.code == _lib.ERR_INVALID
