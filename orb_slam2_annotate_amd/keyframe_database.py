"""Python mirror of ``ORB_SLAM2::KeyFrameDatabase`` (reference: include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc) on
the device database of include/orbfe.h (orbfe_kfdb).  Key frames are their ids and BowVectors; the covisibility graph
stays with the caller, who hands in GetConnectedKeyFrames() / GetBestCovisibilityKeyFrames(10) as ids."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, ptr


def bow_arrays(bow):
    """A BowVector as (ascending uint32 word ids, float64 values): from the {word: value} dict ORBVocabulary.transform
    returns, or from an (ids, values) pair (taken as it is: the library checks the order)."""
    if isinstance(bow, dict):
        ids = np.fromiter(sorted(bow), dtype=np.uint32, count=len(bow))
        return ids, np.array([bow[int(w)] for w in ids], dtype=np.float64)
    ids, values = bow
    return np.ascontiguousarray(ids, dtype=np.uint32), np.ascontiguousarray(values, dtype=np.float64)


def _csr(lists, dtype):
    off = np.zeros(len(lists) + 1, np.int32)
    off[1:] = np.cumsum([len(x) for x in lists])
    flat = np.concatenate([np.asarray(x, dtype=dtype).reshape(-1) for x in lists]) if len(lists) else np.zeros(0, dtype)
    return off, np.ascontiguousarray(flat, dtype=dtype)


def group_candidates(mode, min_score, kf_ids, n_common, scores, neighbours):
    """orbfe_kfdb_group_candidates: the covisibility stage of Detect{Loop,Relocalization}Candidates
    (src/KeyFrameDatabase.cc:165-218, :293-346) over one query's scored set.  neighbours: a mapping or a callable
    kf_id -> ids (GetBestCovisibilityKeyFrames(10) in its order), asked only for scored key frames.  Host code."""
    kf_ids = np.ascontiguousarray(kf_ids, dtype=np.int64)
    n_common = np.ascontiguousarray(n_common, dtype=np.int32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    get = neighbours if callable(neighbours) else (lambda k: neighbours.get(k, ()))
    off, flat = _csr([list(get(int(k))) for k in kf_ids], np.int64)
    out = np.zeros(max(len(kf_ids), 1), np.int64)
    n_out = C.c_int(0)
    check(_lib.load().orbfe_kfdb_group_candidates(int(mode), float(min_score), len(kf_ids), ptr(kf_ids), ptr(n_common), ptr(scores),
                                                  ptr(off), ptr(flat), ptr(out), len(kf_ids), C.byref(n_out)))
    return out[:n_out.value].copy()


class KeyFrameDatabase:
    def __init__(self, voc=None, n_words: int | None = None, device: int | None = None):
        """voc: the ORBVocabulary whose words index the database (KeyFrameDatabase(const ORBVocabulary&), :33-37);
        or n_words for a database without a vocabulary object."""
        self._L = _lib.load()
        self._h = None
        if n_words is None:
            n_words = voc.info()["words"]
        if device is None:
            device = getattr(voc, "device", 0)
        h = C.c_void_p()
        check(self._L.orbfe_kfdb_create(int(n_words), int(device), C.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.orbfe_kfdb_destroy(self._h)
            self._h = None

    def __len__(self):
        return check(self._L.orbfe_kfdb_size(self._h))

    def add(self, kf_id: int, bow):
        ids, values = bow_arrays(bow)
        if len(ids) != len(values):
            raise ValueError("BowVector ids and values differ in length")
        check(self._L.orbfe_kfdb_add(self._h, int(kf_id), ptr(ids), ptr(values), len(ids)))

    def erase(self, kf_id: int) -> bool:
        return check(self._L.orbfe_kfdb_erase(self._h, int(kf_id))) == 1

    def clear(self):
        check(self._L.orbfe_kfdb_clear(self._h))

    def score(self, bow, kf_ids):
        """mpVoc->score(bow, BowVector of each named key frame): float64."""
        ids, values = bow_arrays(bow)
        kf = np.ascontiguousarray(kf_ids, dtype=np.int64)
        out = np.zeros(max(len(kf), 1), np.float64)
        check(self._L.orbfe_kfdb_score(self._h, ptr(ids), ptr(values), len(ids), len(kf), ptr(kf), ptr(out)))
        return out[:len(kf)]

    @staticmethod
    def pack_queries(bows, excluded=None):
        """The CSR operands of orbfe_kfdb_query for a list of BowVectors (and per query the excluded key-frame ids)."""
        arrs = [bow_arrays(b) for b in bows]
        q_off, q_words = _csr([a[0] for a in arrs], np.uint32)
        _, q_values = _csr([a[1] for a in arrs], np.float64)
        if excluded is not None:
            if len(excluded) != len(arrs):
                raise ValueError("one exclusion list per query")
            x_off, x_ids = _csr([list(x) for x in excluded], np.int64)
        else:
            x_off = x_ids = None
        return len(arrs), q_off, q_words, q_values, x_off, x_ids

    def query(self, bows, excluded=None, capacity: int = 256):
        """orbfe_kfdb_query for a list of BowVectors in ONE call; excluded: per query the key-frame ids that take no part
        (GetConnectedKeyFrames() of the loop form), or None.  Returns per query (kf_ids, n_common, scores float32) in the
        order of the reference's lKFsSharingWords."""
        return self.query_packed(self.pack_queries(bows, excluded), capacity)

    def query_packed(self, packed, capacity: int = 256):
        Q, q_off, q_words, q_values, x_off, x_ids = packed
        if Q == 0:
            return []
        while True:
            cap = max(int(capacity), 1)
            kf = np.zeros((Q, cap), np.int64)
            nc = np.zeros((Q, cap), np.int32)
            sc = np.zeros((Q, cap), np.float32)
            cnt = np.zeros(Q, np.int32)
            rc = self._L.orbfe_kfdb_query(self._h, Q, ptr(q_off), ptr(q_words), ptr(q_values), ptr(x_off), ptr(x_ids), cap,
                                          ptr(kf), ptr(nc), ptr(sc), ptr(cnt))
            if rc == _lib.ERR_CAPACITY:
                capacity = int(cnt.max())
                continue
            check(rc)
            return [(kf[q, :cnt[q]].copy(), nc[q, :cnt[q]].copy(), sc[q, :cnt[q]].copy()) for q in range(Q)]

    def DetectRelocalizationCandidates(self, bow, neighbours):
        """src/KeyFrameDatabase.cc:228-347 for a frame with BowVector `bow` -> candidate key-frame ids."""
        kf, nc, sc = self.query([bow])[0]
        return group_candidates(_lib.KFDB_RELOC, 0.0, kf, nc, sc, neighbours)

    def DetectLoopCandidates(self, kf_id: int, bow, connected, min_score: float, neighbours):
        """src/KeyFrameDatabase.cc:95-219 for key frame `kf_id` (BowVector `bow`, GetConnectedKeyFrames() = `connected`).
        The key frame itself takes part like any other unless `connected` names it (the reference's LoopClosing queries
        before it adds the key frame)."""
        kf, nc, sc = self.query([bow], excluded=[connected])[0]
        return group_candidates(_lib.KFDB_LOOP, min_score, kf, nc, sc, neighbours)
