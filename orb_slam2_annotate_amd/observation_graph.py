"""Device-resident observation graph (include/orbfe.h: orbfe_obsgraph): ``MapPoint::mObservations`` -- map point -> the key
frames that see it -- kept in HBM, and the four loops over it: the votes of ``KeyFrame::UpdateConnections``
(src/KeyFrame.cc:311-403) and ``Tracking::UpdateLocalKeyFrames`` (src/Tracking.cc:1339-1455), the counts of
``LocalMapping::KeyFrameCulling`` (src/LocalMapping.cc:710-774) and ``MapPoint::UpdateNormalAndDepth``
(src/MapPoint.cc:360-404).  Points are addressed by the slots of a ``MapPoints`` table, key frames by kf slot; the caller
keeps both maps, the spanning tree and the map mutex.  Once ``enable_keyframe_points`` gave it a width the graph also holds
the opposite direction, ``KeyFrame::mvpMapPoints``, and runs the ordered union of ``Tracking::UpdateLocalPoints``
(src/Tracking.cc:1311-1334) and ``KeyFrame::TrackedMapPoints`` (src/KeyFrame.cc:264-289) over it."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr

OBS_DTYPE = np.dtype([("kf_slot", "<i4"), ("idx", "<u2"), ("octave", "u1"), ("flags", "u1")])
assert OBS_DTYPE.itemsize == 8


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).reshape(-1)


def _u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8).reshape(-1)


def _csr(lists, dtype):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype=dtype).reshape(-1) for x in lists]) if len(lists) and off[-1] else np.zeros(0, dtype)
    return off, np.ascontiguousarray(flat, dtype=dtype)


def update_connections(kf_id, weight):
    """KeyFrame::UpdateConnections :347-393 on one query's votes (orbfe_obsgraph_update_connections; host code) -> dict of
    ordered_id / ordered_weight (mvpOrderedConnectedKeyFrames / mvOrderedWeights), counter (mConnectedKeyFrameWeights as
    {id: weight}), connect_id / connect_weight (who receives AddConnection) and parent_id (front(), -1 when empty)."""
    ids = np.ascontiguousarray(kf_id, dtype=np.int64).reshape(-1)
    w = _i32(weight)
    if len(ids) != len(w):
        raise ValueError("update_connections: one weight per key frame")
    n = len(ids)
    oi, ow = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
    ci, cw = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int32)
    no, nc, parent = C.c_int(0), C.c_int(0), C.c_int64(-1)
    check(_lib.load().orbfe_obsgraph_update_connections(n, ptr(ids), ptr(w), ptr(oi), ptr(ow), C.byref(no), ptr(ci), ptr(cw),
                                                        C.byref(nc), C.byref(parent)))
    return {"ordered_id": oi[:no.value], "ordered_weight": ow[:no.value], "counter": dict(zip(ids.tolist(), w.tolist())),
            "connect_id": ci[:nc.value], "connect_weight": cw[:nc.value], "parent_id": parent.value}


def local_keyframes(kf_id, weight, bad, neighbours, neighbours_bad, children, children_bad, parent):
    """Tracking::UpdateLocalKeyFrames :1364-1454 on one frame's votes (orbfe_obsgraph_local_keyframes; host code).  Record
    i: key frame kf_id[i] with `weight[i]` votes, isBad() `bad[i]`, its ordered covisibles `neighbours[i]` (ids) with their
    bad flags, its children (ascending id) likewise, and its parent's id (-1: none) -> (local ids in order, reference id)."""
    ids = np.ascontiguousarray(kf_id, dtype=np.int64).reshape(-1)
    n = len(ids)
    w, b = _i32(weight), _u8(bad)
    par = np.ascontiguousarray(parent, dtype=np.int64).reshape(-1)
    if not (len(w) == len(b) == len(par) == len(neighbours) == len(neighbours_bad) == len(children) == len(children_bad) == n):
        raise ValueError("local_keyframes: one record per voted key frame")
    no, ni = _csr(neighbours, np.int64)
    _, nb = _csr(neighbours_bad, np.uint8)
    co, cid = _csr(children, np.int64)
    _, cb = _csr(children_bad, np.uint8)
    if len(nb) != len(ni) or len(cb) != len(cid):
        raise ValueError("local_keyframes: one bad flag per neighbour / child")
    cap = 3 * n + 1
    out = np.zeros(cap, np.int64)
    n_out, ref = C.c_int(0), C.c_int64(-1)
    check(_lib.load().orbfe_obsgraph_local_keyframes(n, ptr(ids), ptr(w), ptr(b), ptr(no), ptr(ni), ptr(nb), ptr(co), ptr(cid), ptr(cb),
                                                     ptr(par), ptr(out), cap, C.byref(n_out), C.byref(ref)))
    return out[:n_out.value], ref.value


class ObservationGraph:
    """`point_capacity` point slots with rows of `row_width` observations, `kf_capacity` key-frame slots.  Mutations change
    the host mirror alone; the calls that read the table on the device write the changed rows first.  After close() every
    method raises."""

    def __init__(self, point_capacity: int, kf_capacity: int, row_width: int = 64, device: int = 0):
        self._L = _lib.load()
        self._handle = C.c_void_p()
        check(self._L.orbfe_obsgraph_create(int(device), int(point_capacity), int(kf_capacity), int(row_width), C.byref(self._handle)))
        self.point_capacity, self.kf_capacity, self.row_width, self.device = int(point_capacity), int(kf_capacity), int(row_width), int(device)
        self._kf_id = {}  # kf slot -> mnId, for the replays
        self._kf_len = {}  # kf slot -> length of its mvpMapPoints row, to size the union's output

    @property
    def _h(self):
        if self._handle is None:
            raise ValueError("ObservationGraph is closed")
        return self._handle

    def close(self):
        if getattr(self, "_handle", None):
            self._L.orbfe_obsgraph_destroy(self._handle)
        self._handle = None

    __del__ = close

    def clear(self):
        check(self._L.orbfe_obsgraph_clear(self._h))
        self._kf_id.clear()
        self._kf_len.clear()

    def set_keyframes(self, kf_slot, kf_id, Ow, bad=None):
        k = _i32(kf_slot)
        ids = np.ascontiguousarray(kf_id, dtype=np.int64).reshape(-1)
        ow = np.ascontiguousarray(Ow, dtype=np.float32).reshape(-1, 3)
        b = np.zeros(len(k), np.uint8) if bad is None else _u8(bad)
        if not (len(ids) == len(ow) == len(b) == len(k)):
            raise ValueError("ObservationGraph.set_keyframes: one entry per kf slot")
        check(self._L.orbfe_obsgraph_set_keyframes(self._h, len(k), ptr(k), ptr(ids), ptr(ow), ptr(b)))
        self._kf_id.update(zip(k.tolist(), ids.tolist()))

    def set_points(self, slot, bad, ref_kf_slot):
        s, b, r = _i32(slot), _u8(bad), _i32(ref_kf_slot)
        if not (len(b) == len(r) == len(s)):
            raise ValueError("ObservationGraph.set_points: one entry per slot")
        check(self._L.orbfe_obsgraph_set_points(self._h, len(s), ptr(s), ptr(b), ptr(r)))

    def add_observations(self, slot, kf_slot, idx, octave, stereo):
        """MapPoint::AddObservation for each (slot, kf_slot); a full row raises OrbfeError(ERR_CAPACITY), nothing applied."""
        s, k = _i32(slot), _i32(kf_slot)
        i = np.ascontiguousarray(idx, dtype=np.uint16).reshape(-1)
        o, st = _u8(octave), _u8(stereo)
        if not (len(k) == len(i) == len(o) == len(st) == len(s)):
            raise ValueError("ObservationGraph.add_observations: one entry per observation")
        check(self._L.orbfe_obsgraph_add_observations(self._h, len(s), ptr(s), ptr(k), ptr(i), ptr(o), ptr(st)))

    def erase_observations(self, slot, kf_slot):
        """MapPoint::EraseObservation for each (slot, kf_slot) -> became_bad[n] (uint8)."""
        s, k = _i32(slot), _i32(kf_slot)
        if len(s) != len(k):
            raise ValueError("ObservationGraph.erase_observations: one kf slot per slot")
        bad = np.zeros(max(len(s), 1), np.uint8)
        check(self._L.orbfe_obsgraph_erase_observations(self._h, len(s), ptr(s), ptr(k), ptr(bad)))
        return bad[:len(s)]

    def erase_keyframe(self, kf_slot: int):
        """The map-point part of KeyFrame::SetBadFlag -> the slots of the points that became bad (ascending)."""
        out = np.zeros(self.point_capacity, np.int32)
        n = C.c_int(0)
        check(self._L.orbfe_obsgraph_erase_keyframe(self._h, int(kf_slot), ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def get_row(self, slot: int, from_device: bool = False):
        """-> dict of entries (OBS_DTYPE, the live ones), n_obs, bad, ref_kf_slot, from the mirror or from the device."""
        e = np.zeros(self.row_width, OBS_DTYPE)
        n, nobs, bad, ref = C.c_int32(0), C.c_int32(0), C.c_uint8(0), C.c_int32(0)
        check(self._L.orbfe_obsgraph_get_row(self._h, int(bool(from_device)), int(slot), ptr(e), C.byref(n), C.byref(nobs), C.byref(bad),
                                             C.byref(ref)))
        return {"entries": e[:n.value], "n_obs": nobs.value, "bad": bad.value, "ref_kf_slot": ref.value}

    def votes(self, queries, self_kf_slot=None, capacity=None):
        """The vote counts of len(queries) point-slot lists in one launch -> list of (kf_slot[], weight[]) per query, kf slots
        ascending.  capacity (default kf_capacity) below a query's count raises OrbfeError(ERR_CAPACITY) with .count set."""
        Q = len(queries)
        off, flat = _csr(queries, np.int32)
        me = np.full(Q, -1, np.int32) if self_kf_slot is None else _i32(self_kf_slot)
        if len(me) != Q:
            raise ValueError("ObservationGraph.votes: one self_kf_slot per query")
        cap = self.kf_capacity if capacity is None else int(capacity)
        kf = np.zeros(max(Q * cap, 1), np.int32)
        w = np.zeros(max(Q * cap, 1), np.int32)
        cnt = np.zeros(max(Q, 1), np.int32)
        try:
            check(self._L.orbfe_obsgraph_votes(self._h, Q, ptr(off), ptr(flat), ptr(me), cap, ptr(kf), ptr(w), ptr(cnt)))
        except _lib.OrbfeError as e:
            if e.code == _lib.ERR_CAPACITY:
                e.count = cnt[:Q].copy()
                e.partial = [(kf[q * cap:q * cap + min(cnt[q], cap)].copy(), w[q * cap:q * cap + min(cnt[q], cap)].copy()) for q in range(Q)]
            raise
        return [(kf[q * cap:q * cap + cnt[q]].copy(), w[q * cap:q * cap + cnt[q]].copy()) for q in range(Q)]

    def update_connections(self, kf_slot: int, point_slots):
        """KeyFrame::UpdateConnections for the key frame in `kf_slot` whose non-NULL mvpMapPoints are `point_slots`: the votes
        on the device, :347-393 on the host -> update_connections()'s dict, ids = mnIds."""
        (kf, w), = self.votes([point_slots], [kf_slot])
        return update_connections([self._kf_id[k] for k in kf.tolist()], w)

    def local_keyframes(self, point_slots, neighbours, children, parent, bad=None):
        """Tracking::UpdateLocalKeyFrames for a frame whose matched, non-NULL mvpMapPoints are `point_slots`.  neighbours /
        children: {mnId: [mnId, ...]} (ordered covisibles; children ascending), parent: {mnId: mnId}, bad: set of bad mnIds;
        only the voted key frames are looked up -> (local ids in order, reference id)."""
        (kf, w), = self.votes([point_slots])
        ids = [self._kf_id[k] for k in kf.tolist()]
        bad = set() if bad is None else set(bad)
        nb = [list(neighbours.get(i, [])) for i in ids]
        ch = [list(children.get(i, [])) for i in ids]
        return local_keyframes(ids, w, [i in bad for i in ids], nb, [[j in bad for j in x] for x in nb], ch,
                               [[j in bad for j in x] for x in ch], [parent.get(i, -1) for i in ids])

    def culling_counts(self, kf_slot, features):
        """KeyFrameCulling's counts for the candidates kf_slot[c] with features[c] = (point slots, octaves) that passed the
        host-side tests -> (n_mps[], n_redundant[])."""
        k = _i32(kf_slot)
        if len(features) != len(k):
            raise ValueError("ObservationGraph.culling_counts: one feature list per candidate")
        off, sl = _csr([f[0] for f in features], np.int32)
        _, oc = _csr([f[1] for f in features], np.uint8)
        if len(oc) != len(sl):
            raise ValueError("ObservationGraph.culling_counts: one octave per feature")
        nm, nr = np.zeros(max(len(k), 1), np.int32), np.zeros(max(len(k), 1), np.int32)
        check(self._L.orbfe_obsgraph_culling_counts(self._h, len(k), ptr(k), ptr(off), ptr(sl), ptr(oc), ptr(nm), ptr(nr)))
        return nm[:len(k)], nr[:len(k)]

    def keyframe_culling(self, candidates, features):
        """LocalMapping::KeyFrameCulling over the candidates (kf slots, in vpLocalKeyFrames order, mnId 0 left out by the
        caller), with the reference's order dependence replayed exactly: one launch for all remaining candidates; the first
        in order with n_redundant > 0.9 * n_mps (compared in double) is erased (erase_keyframe); the ones before it are
        final, the ones after it are counted again.  One launch plus one per culled key frame
        -> (culled kf slots in order, slots of the points that became bad)."""
        cand = [int(c) for c in candidates]
        culled, bad_points, start = [], [], 0
        while start < len(cand):
            nm, nr = self.culling_counts(cand[start:], features[start:])
            hit = next((i for i in range(len(nm)) if float(nr[i]) > 0.9 * float(nm[i])), None)
            if hit is None:
                break
            culled.append(cand[start + hit])
            bad_points.extend(self.erase_keyframe(cand[start + hit]).tolist())
            start += hit + 1
        return culled, bad_points

    # ---- KeyFrame::mvpMapPoints: key frame -> its points ----

    def enable_keyframe_points(self, kf_row_width: int):
        """Rows of `kf_row_width` point slots per kf slot (a multiple of 64 in 64 .. 16384); once per graph."""
        check(self._L.orbfe_obsgraph_enable_keyframe_points(self._h, int(kf_row_width)))
        self.kf_row_width = int(kf_row_width)

    def set_keyframe_points(self, kf_slot: int, slots):
        """The whole mvpMapPoints of a key frame (-1: NULL), as at the KeyFrame constructor."""
        s = _i32(slots)
        check(self._L.orbfe_obsgraph_set_keyframe_points(self._h, int(kf_slot), len(s), ptr(s)))
        self._kf_len[int(kf_slot)] = len(s)

    def assign_keyframe_points(self, kf_slot, idx, slot):
        """KeyFrame::AddMapPoint / ReplaceMapPointMatch (mvpMapPoints[idx] = slot) and EraseMapPointMatch(idx) (slot -1) per
        entry, in order; an invalid entry raises OrbfeError(ERR_INVALID) with nothing applied."""
        k, s = _i32(kf_slot), _i32(slot)
        i = np.ascontiguousarray(idx, dtype=np.uint16).reshape(-1)
        if not (len(i) == len(s) == len(k)):
            raise ValueError("ObservationGraph.assign_keyframe_points: one entry per assignment")
        check(self._L.orbfe_obsgraph_assign_keyframe_points(self._h, len(k), ptr(k), ptr(i), ptr(s)))

    def get_keyframe_points(self, kf_slot: int, from_device: bool = False):
        """-> the row's point slots (its length N; -1: NULL), from the mirror or from the device."""
        w = getattr(self, "kf_row_width", 0)
        out = np.full(max(w, 1), -1, np.int32)
        n = C.c_int32(0)
        check(self._L.orbfe_obsgraph_get_keyframe_points(self._h, int(bool(from_device)), int(kf_slot), ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def keyframe_points_union(self, queries, capacity=None):
        """The ordered union of the key frames' map points for len(queries) kf-slot lists in one call (Tracking::
        UpdateLocalPoints and its three siblings) -> list of point-slot arrays, each in visiting order with first occurrence
        kept.  capacity defaults to what the lists' row lengths allow; below a query's count it raises
        OrbfeError(ERR_CAPACITY) with .count and .partial set."""
        Q = len(queries)
        off, flat = _csr(queries, np.int32)
        if capacity is None:
            cap = max([min(sum(self._kf_len.get(int(k), 0) for k in q), self.point_capacity) for q in queries] + [1])
        else:
            cap = int(capacity)
        out = np.zeros(max(Q * cap, 1), np.int32)
        cnt = np.zeros(max(Q, 1), np.int32)
        try:
            check(self._L.orbfe_obsgraph_keyframe_points_union(self._h, Q, ptr(off), ptr(flat), cap, ptr(out), ptr(cnt)))
        except _lib.OrbfeError as e:
            if e.code == _lib.ERR_CAPACITY:
                e.count = cnt[:Q].copy()
                e.partial = [out[q * cap:q * cap + min(cnt[q], cap)].copy() for q in range(Q)]
            raise
        return [out[q * cap:q * cap + cnt[q]].copy() for q in range(Q)]

    def local_points(self, kf_slots):
        """Tracking::UpdateLocalPoints for mvpLocalKeyFrames = kf_slots -> mvpLocalMapPoints as point slots: the slot list
        MapPoints.search_local_points takes."""
        return self.keyframe_points_union([kf_slots])[0]

    def tracked_points(self, kf_slot, min_obs: int = 0):
        """KeyFrame::TrackedMapPoints(min_obs) for each kf slot in one launch -> counts (int32)."""
        k = _i32(kf_slot)
        cnt = np.zeros(max(len(k), 1), np.int32)
        check(self._L.orbfe_obsgraph_tracked_points(self._h, len(k), ptr(k), int(min_obs), ptr(cnt)))
        return cnt[:len(k)]

    # ---- KeyFrame::mDescriptors and MapPoint::ComputeDistinctiveDescriptors ----

    def enable_keyframe_descriptors(self, kf_desc_width: int):
        """A store of `kf_desc_width` descriptors per kf slot (a multiple of 64 in 64 .. 16384); once per graph."""
        check(self._L.orbfe_obsgraph_enable_keyframe_descriptors(self._h, int(kf_desc_width)))
        self.kf_desc_width = int(kf_desc_width)

    def set_keyframe_descriptors(self, kf_slot: int, desc):
        """mDescriptors of a key frame: an [n, 32] uint8 array from the host, or a ResidentFrame, whose descriptors are
        copied on the device (the frame may be closed afterwards).  Unlike the other mutations this touches the device."""
        if hasattr(desc, "_h") and hasattr(desc, "c"):  # a resident frame
            check(self._L.orbfe_obsgraph_set_keyframe_descriptors_frame(self._h, int(kf_slot), desc._h))
            return
        d = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        check(self._L.orbfe_obsgraph_set_keyframe_descriptors(self._h, int(kf_slot), len(d), ptr(d)))

    def get_keyframe_descriptors(self, kf_slot: int):
        """-> the [n, 32] descriptors the kf slot holds, read back from the device."""
        out = np.zeros((max(getattr(self, "kf_desc_width", 0), 1), 32), np.uint8)
        n = C.c_int32(0)
        check(self._L.orbfe_obsgraph_get_keyframe_descriptors(self._h, int(kf_slot), ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def distinctive_descriptors(self, slot, mp=None):
        """MapPoint::ComputeDistinctiveDescriptors for slot[] over the rows and the stored key-frame descriptors.  Without mp:
        -> (best_kf_slot, best_idx, desc [n, 32], valid); entries with valid = 0 hold -1 / -1 / zeros.  mp (a MapPoints table):
        the winners' bytes are written into the table's descriptors on the device -> (best_kf_slot, best_idx, valid)."""
        s = _i32(slot)
        n = len(s)
        kf, idx = np.full(max(n, 1), -1, np.int32), np.full(max(n, 1), -1, np.int32)
        valid = np.zeros(max(n, 1), np.uint8)
        if mp is not None:
            check(self._L.orbfe_obsgraph_distinctive_descriptors_mappoints(self._h, mp._h, n, ptr(s), ptr(kf), ptr(idx), ptr(valid)))
            return kf[:n], idx[:n], valid[:n]
        desc = np.zeros((max(n, 1), 32), np.uint8)
        check(self._L.orbfe_obsgraph_distinctive_descriptors(self._h, n, ptr(s), ptr(kf), ptr(idx), ptr(desc), ptr(valid)))
        return kf[:n], idx[:n], desc[:n], valid[:n]

    def update_normal_depth(self, slot, scale_factors, pos=None, mp=None):
        """MapPoint::UpdateNormalAndDepth for slot[].  pos ([n, 3]): the array form -> (normal [n, 3], min_dist, max_dist,
        valid); rows with valid = 0 hold zeros.  mp (a MapPoints table): positions are read from and the results written into
        the table on the device -> valid."""
        s = _i32(slot)
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32).reshape(-1)
        n = len(s)
        valid = np.zeros(max(n, 1), np.uint8)
        if (pos is None) == (mp is None):
            raise ValueError("ObservationGraph.update_normal_depth: give pos or mp")
        if mp is not None:
            check(self._L.orbfe_obsgraph_update_normal_depth_mappoints(self._h, mp._h, n, ptr(s), ptr(sf), len(sf), ptr(valid)))
            return valid[:n]
        p = np.ascontiguousarray(pos, dtype=np.float32).reshape(-1, 3)
        if len(p) != n:
            raise ValueError("ObservationGraph.update_normal_depth: one position per slot")
        normal = np.zeros((max(n, 1), 3), np.float32)
        lo, hi = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
        check(self._L.orbfe_obsgraph_update_normal_depth(self._h, n, ptr(s), ptr(p), ptr(sf), len(sf), ptr(normal), ptr(lo), ptr(hi),
                                                         ptr(valid)))
        return normal[:n], lo[:n], hi[:n], valid[:n]
