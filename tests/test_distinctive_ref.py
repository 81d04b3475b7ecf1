"""CPU: tests/distinctive_ref.py, the plain-Python restatement of MapPoint::ComputeDistinctiveDescriptors
(src/MapPoint.cc:269-333), pinned by answers worked out by hand and by the oracle library's orc_distinctive_descriptor.

The hand cases use descriptors whose first v bits are set, so the distance of two of them is |v - w| and every median can
be read off a line of numbers."""
import numpy as np

import distinctive_ref as dr
import oracle_lib as orc


def bits(v):
    """The 32-byte descriptor with the first v bits set: hamming(bits(v), bits(w)) = |v - w|."""
    return np.packbits(np.arange(256) < v).astype(np.uint8)


def world(values, ids=None, bad=()):
    """One key frame per value, kf slot k holding one descriptor bits(values[k]) at idx 0."""
    n = len(values)
    ids = list(range(10, 10 + n)) if ids is None else ids
    return ids, [k in bad for k in range(n)], [bits(v)[None] for v in values]


def winner(values, ids=None, bad=(), order=None, point_bad=False):
    kf_id, kf_bad, kf_desc = world(values, ids, bad)
    obs = [(k, 0) for k in (range(len(values)) if order is None else order)]
    r = dr.distinctive(point_bad, obs, kf_id, kf_bad, kf_desc)
    return None if r is None else r[0]


def test_hamming_of_the_line_descriptors():
    assert dr.hamming(bits(0), bits(256)) == 256 and dr.hamming(bits(7), bits(7)) == 0 and dr.hamming(bits(20), bits(9)) == 11


def test_one_and_two_descriptors():
    assert winner([5]) == 0
    # N = 2: k = int(0.5) = 0, both medians are the self-distance 0, the first row wins
    assert winner([0, 10]) == 0 and winner([10, 0]) == 0


def test_three_descriptors():
    # k = 1.  [0, 10, 4]: rows sorted (0 4 10), (0 6 10), (0 4 6) -> medians 4, 6, 4: the first of the tie
    assert winner([0, 10, 4]) == 0
    # [0, 10, 6]: (0 6 10), (0 4 10), (0 4 6) -> 6, 4, 4: row 1 before row 2
    assert winner([0, 10, 6]) == 1


def test_four_descriptors_take_the_lower_median():
    # k = int(1.5) = 1.  [0, 8, 9, 20]: (0 8 9 20), (0 1 8 12), (0 1 9 11), (0 11 12 20) -> 8, 1, 1, 11: row 1.
    assert winner([0, 8, 9, 20]) == 1
    # with k = 2 the medians would be 9, 8, 9, 12 -- also row 1; [0, 9, 8, 20] tells the two apart:
    # k = 1: (0 8 9 20), (0 1 9 11), (0 1 8 12), (0 11 12 20) -> 8, 1, 1, 11: row 1;  k = 2 -> 9, 9, 8, 12: row 2
    assert winner([0, 9, 8, 20]) == 1


def test_a_median_tie_goes_to_the_lowest_mnid_whatever_the_insertion_order():
    # kf slots 0, 1, 2 hold 4, 10, 0 and mnIds 30, 20, 10; observed in slot order = descending mnId.
    # In mnId order the row is [0, 10, 4] -> medians 4, 6, 4 -> the first: kf slot 2.  (Insertion order [4, 10, 0] would
    # give medians 4, 6, 4 as well -- and kf slot 0.)
    assert winner([4, 10, 0], ids=[30, 20, 10]) == 2
    assert winner([4, 10, 0], ids=[10, 20, 30]) == 0
    assert winner([4, 10, 0], ids=[30, 20, 10], order=[2, 0, 1]) == 2


def test_a_bad_key_frame_changes_n_and_k():
    # [0, 1, 8, 9, 20], N = 5, k = 2: medians 8, 7, 7, 8, 12 -> row 1 (the value 1)
    assert winner([0, 1, 8, 9, 20]) == 1
    # the key frame of value 1 bad: [0, 8, 9, 20], N = 4, k = 1 -> medians 8, 1, 1, 11 -> the value 8, kf slot 2
    assert winner([0, 1, 8, 9, 20], bad={1}) == 2
    # bad at the first and at the last place
    assert winner([0, 1, 8, 9, 20], bad={0}) == 2    # [1, 8, 9, 20]: (0 7 8 19), (0 1 7 12), (0 1 8 11), .. -> 7, 1, 1, 11
    assert winner([0, 1, 8, 9, 20], bad={4}) == 0    # [0, 1, 8, 9]: (0 1 8 9), (0 1 7 8), (0 1 7 8), (0 1 8 9) -> 1, 1, 1, 1


def test_where_the_reference_returns_early():
    assert winner([3, 4], point_bad=True) is None
    assert winner([3, 4], order=[]) is None
    assert winner([3, 4], bad={0, 1}) is None


def test_the_result_names_the_entry_and_its_bytes():
    kf_id, kf_bad = [7, 5], [False, False]
    kf_desc = [np.stack([bits(200), bits(3)]), np.stack([bits(9), bits(4), bits(100)])]
    # mnId order: kf 1 (idx 1: 4), kf 0 (idx 1: 3) -> N = 2: the first, kf slot 1
    assert dr.distinctive(False, [(0, 1), (1, 1)], kf_id, kf_bad, kf_desc) == (1, 1, bits(4).tobytes())


def test_agrees_with_the_oracle_on_seeded_lists():
    L = orc.lib()
    for seed in range(20):
        rng = np.random.default_rng(500 + seed)
        n = int(rng.integers(1, 40))
        proto = rng.integers(0, 256, size=(3, 32), dtype=np.uint8)
        d = proto[rng.integers(0, 3, n)] ^ np.packbits(rng.random((n, 256)) < (0.02 if seed % 2 else 0.2), axis=1)
        d = np.ascontiguousarray(d, dtype=np.uint8)
        assert dr.best_of([bytes(r) for r in d]) == L.orc_distinctive_descriptor(orc._p(d), n), seed
