"""TEST INFRASTRUCTURE: a plain-Python restatement of the reference's KeyFrameDatabase
(src/KeyFrameDatabase.cc) and of L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).

It is built the way the reference is — an inverted file with one list of keyframes per word
(append on add, remove on erase) and per-keyframe query / words / score fields that a query
stamps while it walks the lists of its words — and so shares no structure with the
keyframe-major kernels of csrc/orb_kfdb.hip that it checks.  Doubles are Python floats; every
float step of the reference (si, accScore +=, maxCommonWords * 0.8f, 0.75f * bestAccScore) is an
np.float32 operation.

Choices that the reference leaves open and the library fixes (include/orb_abi.h): a keyframe's
mRelocScore starts at 0.0f, and every query has an id of its own.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32


def bow_items(bow):
    """[(word, value)] in ascending word order of a dict or a (words, values) pair."""
    if isinstance(bow, dict):
        return [(int(w), float(bow[w])) for w in sorted(bow)]
    w, v = bow
    return [(int(a), float(b)) for a, b in zip(w, v)]


def l1_terms(v1, v2):
    """The terms L1Scoring::score adds, in the order it adds them (both in ascending word order)."""
    out = []
    i = j = 0
    while i < len(v1) and j < len(v2):
        if v1[i][0] == v2[j][0]:
            vi, wi = v1[i][1], v2[j][1]
            out.append(abs(vi - wi) - abs(vi) - abs(wi))
            i += 1
            j += 1
        elif v1[i][0] < v2[j][0]:
            i += 1  # lower_bound(v2's word): the first element not below it
            while i < len(v1) and v1[i][0] < v2[j][0]:
                i += 1
        else:
            j += 1
            while j < len(v2) and v2[j][0] < v1[i][0]:
                j += 1
    return out


def l1_score(v1, v2, reverse: bool = False) -> float:
    score = 0.0
    terms = l1_terms(v1, v2)
    for t in (reversed(terms) if reverse else terms):
        score += t
    return -score / 2.0


class _KF:
    def __init__(self, kf_id, bow, seq):
        self.id = kf_id
        self.bow = bow
        self.seq = seq
        self.reloc_query = self.loop_query = -1
        self.reloc_words = self.loop_words = 0
        self.reloc_score = F32(0.0)  # the library's choice (the reference: uninitialised)
        self.loop_score = F32(0.0)
        self.first = None            # bookkeeping for the debug table only


class ModelDatabase:
    """Same methods as orbslam_jpminipc_amd.KeyFrameDatabase."""

    def __init__(self):
        self.inv = {}     # word -> list of keyframes, in add order (mvInvertedFile)
        self.kfs = {}     # live keyframes
        self.cov = {}     # id -> GetBestCovisibilityKeyFrames(10) as ids
        self.nquery = 0
        self.nadd = 0
        self.last = {}    # id -> (common, first, scored, score) of the last query's sharing list

    def __len__(self):
        return len(self.kfs)

    def add(self, kf_id, bow):
        assert kf_id not in self.kfs
        kf = _KF(kf_id, bow_items(bow), self.nadd)
        self.nadd += 1
        self.kfs[kf_id] = kf
        for w, _ in kf.bow:
            self.inv.setdefault(w, []).append(kf)

    def erase(self, kf_id):
        kf = self.kfs.pop(kf_id, None)
        if kf is None:
            return
        for w, _ in kf.bow:
            self.inv[w].remove(kf)

    def clear(self):
        self.inv = {}
        self.kfs = {}
        self.cov = {}

    def set_covisible(self, kf_id, neighbour_ids):
        assert len(neighbour_ids) <= 10
        self.cov[kf_id] = list(neighbour_ids)

    def _neighbours(self, kf):
        return [self.kfs[i] for i in self.cov.get(kf.id, []) if i in self.kfs]

    def _table(self, q, sharing, words_of, scored_of):
        self.last = {kf.id: (words_of(kf), kf.first, scored_of(kf), l1_score(q, kf.bow)) for kf in sharing}

    # KeyFrameDatabase.cc:198-308
    def DetectRelocalisationCandidates(self, bow):
        q = bow_items(bow)
        self.nquery += 1
        fid = self.nquery
        self.last = {}
        sharing = []
        for w, _ in q:
            for kf in self.inv.get(w, []):
                if kf.reloc_query != fid:
                    kf.reloc_words = 0
                    kf.reloc_query = fid
                    kf.first = w
                    sharing.append(kf)
                kf.reloc_words += 1
        if not sharing:
            return []
        max_common = 0
        for kf in sharing:
            if kf.reloc_words > max_common:
                max_common = kf.reloc_words
        min_common = int(F32(max_common) * F32(0.8))
        self._table(q, sharing, lambda k: k.reloc_words, lambda k: k.reloc_words > min_common)
        score_and_match = []
        for kf in sharing:
            if kf.reloc_words > min_common:
                si = F32(l1_score(q, kf.bow))
                kf.reloc_score = si
                score_and_match.append((si, kf))
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = F32(0.0)
        for si, kf in score_and_match:
            best, acc, best_kf = si, si, kf
            for kf2 in self._neighbours(kf):
                if kf2.reloc_query != fid:
                    continue
                acc = F32(acc + kf2.reloc_score)
                if kf2.reloc_score > best:
                    best_kf = kf2
                    best = kf2.reloc_score
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc)

    # KeyFrameDatabase.cc:75-196
    def DetectLoopCandidates(self, bow, connected_ids=(), min_score=0.0):
        q = bow_items(bow)
        min_score = F32(min_score)
        connected = set(connected_ids)
        self.nquery += 1
        fid = self.nquery
        self.last = {}
        sharing = []
        for w, _ in q:
            for kf in self.inv.get(w, []):
                if kf.loop_query != fid:
                    kf.loop_words = 0
                    if kf.id not in connected:
                        kf.loop_query = fid
                        kf.first = w
                        sharing.append(kf)
                kf.loop_words += 1
        if not sharing:
            return []
        max_common = 0
        for kf in sharing:
            if kf.loop_words > max_common:
                max_common = kf.loop_words
        min_common = int(F32(max_common) * F32(0.8))
        self._table(q, sharing, lambda k: k.loop_words, lambda k: k.loop_words > min_common)
        score_and_match = []
        for kf in sharing:
            if kf.loop_words > min_common:
                si = F32(l1_score(q, kf.bow))
                kf.loop_score = si
                if si >= min_score:
                    score_and_match.append((si, kf))
        if not score_and_match:
            return []
        acc_and_match = []
        best_acc = min_score
        for si, kf in score_and_match:
            best, acc, best_kf = si, si, kf
            for kf2 in self._neighbours(kf):
                if kf2.loop_query == fid and kf2.loop_words > min_common:
                    acc = F32(acc + kf2.loop_score)
                    if kf2.loop_score > best:
                        best_kf = kf2
                        best = kf2.loop_score
            acc_and_match.append((acc, best_kf))
            if acc > best_acc:
                best_acc = acc
        return self._retain(acc_and_match, best_acc)

    @staticmethod
    def _retain(acc_and_match, best_acc):
        min_to_retain = F32(0.75) * best_acc
        out, seen = [], set()
        for acc, kf in acc_and_match:
            if acc > min_to_retain and kf.id not in seen:
                out.append(kf.id)
                seen.add(kf.id)
        return out
