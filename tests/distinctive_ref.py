"""MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333) restated in plain Python over the things the device
observation graph holds: a point's observations, the key frames' mnIds, bad flags and descriptors.  Lists, sorted(),
int(0.5 * (N - 1)) and a strict <, with the reference's line next to each step -- the yardstick of
tests/test_gpu_obsdesc.py, itself pinned by hand-computed answers and the oracle in tests/test_distinctive_ref.py."""


def hamming(a, b):
    """ORBmatcher::DescriptorDistance: the number of differing bits of two 32-byte descriptors."""
    return bin(int.from_bytes(bytes(a), "little") ^ int.from_bytes(bytes(b), "little")).count("1")


def best_of(descriptors):
    """:299-328 on vDescriptors -> BestIdx."""
    N = len(descriptors)                                                      # :300
    dist = [[hamming(descriptors[i], descriptors[j]) for j in range(N)] for i in range(N)]  # :303-312 (Distances[i][i] = 0)
    best_median, best_idx = 2 ** 31 - 1, 0                                    # :315-316
    for i in range(N):                                                        # :317
        v = sorted(dist[i])                                                   # :319-320
        median = v[int(0.5 * (N - 1))]                                        # :321
        if median < best_median:                                              # :323
            best_median, best_idx = median, i                                 # :325-326
    return best_idx


def distinctive(point_bad, observations, kf_id, kf_bad, kf_desc):
    """One map point.  observations: (kf_slot, idx) in any order; kf_id / kf_bad / kf_desc: per kf slot the mnId, isBad()
    and the [n, 32] descriptors.  -> (kf_slot, idx, 32 bytes) of the descriptor the point keeps, or None where the
    reference returns without writing mDescriptor."""
    if point_bad:                                                             # :278-279
        return None
    if not observations:                                                      # :283-284
        return None
    # :288: the map is walked in key order; the graph's documented order is ascending mnId (the reference's is pointer order)
    ordered = sorted(observations, key=lambda o: kf_id[o[0]])
    kept = [(k, i) for k, i in ordered if not kf_bad[k]]                       # :292-293
    if not kept:                                                              # :296-297
        return None
    descriptors = [bytes(bytearray(int(b) for b in kf_desc[k][i])) for k, i in kept]
    k, i = kept[best_of(descriptors)]
    return k, i, descriptors[kept.index((k, i))]                              # :332
