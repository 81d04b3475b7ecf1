"""Plain-Python restatement of ORB-SLAM2's KeyFrameDatabase and DBoW2's L1 score: the comparator of the device database.

Written from the semantics, with the reference's data structures kept as they are: an inverted file with one list of key
frames per word (in insertion order), per-key-frame query marks and word counters, and the score as a merge walk over
two sorted (word, value) sequences.  Python floats are IEEE doubles and the score uses subtract, add, abs and / 2.0 only,
so it is exact without libm; numpy.float32 stands wherever the reference holds a `float`.
A BowVector here is a list of (word, value) pairs in ascending word order."""
from collections import defaultdict

import numpy as np

F32 = np.float32
RELOC, LOOP = 0, 1


def as_pairs(bow):
    """{word: value} or (ids, values) -> [(word, value)] ascending."""
    if isinstance(bow, dict):
        return [(int(w), float(bow[w])) for w in sorted(bow)]
    ids, values = bow
    return [(int(w), float(v)) for w, v in zip(ids, values)]


def l1_score(v1, v2):
    """L1Scoring::score: only words present in both vectors contribute, in ascending word order."""
    i, j, score = 0, 0, 0.0
    while i < len(v1) and j < len(v2):
        (w1, vi), (w2, wi) = v1[i], v2[j]
        if w1 == w2:
            score += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif w1 < w2:
            i += 1
        else:
            j += 1
    return -score / 2.0


class _KF:
    def __init__(self, kf_id, bow):
        self.id, self.bow = kf_id, bow
        self.query, self.words, self.score = None, 0, F32(0)


class Database:
    def __init__(self):
        self.inverted = defaultdict(list)  # word -> key frames, in insertion order
        self.kfs = {}
        self.nqueries = 0

    def add(self, kf_id, bow):
        assert kf_id not in self.kfs
        kf = _KF(kf_id, as_pairs(bow))
        self.kfs[kf_id] = kf
        for w, _ in kf.bow:
            self.inverted[w].append(kf)

    def erase(self, kf_id):
        kf = self.kfs.pop(kf_id)
        for w, _ in kf.bow:
            self.inverted[w].remove(kf)

    def clear(self):
        self.inverted.clear()
        self.kfs.clear()

    def score(self, bow, kf_ids):
        q = as_pairs(bow)
        return [l1_score(q, self.kfs[k].bow) for k in kf_ids]

    def sharing(self, bow, excluded=()):
        """The first stage of both Detect*Candidates: the list of key frames sharing a word with the query, in the order
        they are first met, with their word counters.  -> list of _KF"""
        self.nqueries += 1
        mark = self.nqueries  # a fresh query id: no key frame carries it yet
        excluded = set(excluded)
        sharing = []
        for w, _ in as_pairs(bow):
            for kf in self.inverted.get(w, ()):
                if kf.query != mark:
                    kf.words = 0
                    if kf.id not in excluded:
                        kf.query = mark
                        sharing.append(kf)
                kf.words += 1
        return sharing

    def scored(self, bow, excluded=()):
        """-> (kf_ids, n_common, scores as float32), and the sharing list's length, of the key frames that pass the
        word-count filter, in list order."""
        q = as_pairs(bow)
        sharing = self.sharing(bow, excluded)
        if not sharing:
            return ([], [], []), 0
        max_common = max(kf.words for kf in sharing)
        min_common = int(F32(max_common) * F32(0.8))
        ids, common, scores = [], [], []
        for kf in sharing:
            if kf.words > min_common:
                ids.append(kf.id)
                common.append(kf.words)
                scores.append(F32(l1_score(q, kf.bow)))
        return (ids, common, scores), len(sharing)


def group_candidates(mode, min_score, ids, scores, neighbours):
    """The covisibility stage: neighbours(kf_id) -> ids.  A neighbour counts only if it is in the scored set."""
    score_of = {k: F32(s) for k, s in zip(ids, scores)}
    min_score = F32(min_score)
    best_acc = min_score if mode == LOOP else F32(0)
    acc_and_match = []
    for k, s in zip(ids, scores):
        s = F32(s)
        if mode == LOOP and not s >= min_score:
            continue
        best_score, acc, best = s, s, k
        for k2 in neighbours(k):
            if k2 not in score_of:
                continue
            s2 = score_of[k2]
            acc = F32(acc + s2)
            if s2 > best_score:
                best, best_score = k2, s2
        acc_and_match.append((acc, best))
        if acc > best_acc:
            best_acc = acc
    retain = F32(F32(0.75) * best_acc)
    out = []
    for acc, best in acc_and_match:
        if acc > retain and best not in out:
            out.append(best)
    return out
