"""KeyFrameDatabase on the GPU (reference src/KeyFrameDatabase.cc), over the C ABI of
``include/orb_abi.h`` (csrc/orb_kfdb.hip).

The native database addresses keyframes by slot (dense integers below ``max_keyframes``); this
wrapper accepts any hashable keyframe id (the reference's ``mnId``) and gives every id it meets
the next free slot.  A slot stays with its id until ``clear()``: an erased keyframe may still
stand in another keyframe's covisibility list, where it is skipped as not live.  So
``max_keyframes`` bounds the ids met between two ``clear()`` calls.  BowVectors are dicts
{word id: value} or (words, values) pairs in ascending word order.  Only L1_NORM vocabularies
are supported.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._native import ORB_ERANGE, OrbError, check, hip_lib, ptr
from .vocabulary import bow_arrays


class KeyFrameDatabase:
    def __init__(self, voc, max_keyframes: int = 4096, max_entries: int | None = None):
        self._lib = hip_lib()
        self._h = None
        self.voc = voc  # keeps the vocabulary alive
        self.max_keyframes = int(max_keyframes)
        self.max_entries = int(max_entries) if max_entries is not None else 1024 * self.max_keyframes
        h = ctypes.c_void_p()
        check(self._lib.orb_kfdb_create(voc._h, self.max_keyframes, self.max_entries, voc.device, ctypes.byref(h)))
        self._h = h
        self._slot = {}
        self._id = []

    def close(self):
        if self._h:
            self._lib.orb_kfdb_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    # ---- ids <-> slots -------------------------------------------------------------------
    def slot_of(self, kf_id, create: bool = True) -> int:
        s = self._slot.get(kf_id)
        if s is None:
            if not create:
                return -1
            if len(self._id) >= self.max_keyframes:
                raise OrbError(ORB_ERANGE, f"more than max_keyframes = {self.max_keyframes} keyframe ids")
            s = len(self._id)
            self._slot[kf_id] = s
            self._id.append(kf_id)
        return s

    def ids_of(self, slots) -> list:
        return [self._id[int(s)] for s in slots]

    def __len__(self) -> int:
        return check(self._lib.orb_kfdb_size(self._h))

    # ---- KeyFrameDatabase::add / erase / clear ---------------------------------------------
    def add(self, kf_id, bow) -> None:
        w, v = bow_arrays(bow)
        check(self._lib.orb_kfdb_add(self._h, self.slot_of(kf_id), ptr(w), ptr(v), len(w)))

    def add_batch_device(self, kf_ids, bow_words, bow_values, bow_n, stream=None) -> None:
        """Frames 0 .. len(kf_ids)-1 of a batched transform ((B, cap) tensors, bow_n (B,)) become
        keyframes kf_ids, device to device."""
        import torch

        slots = np.array([self.slot_of(k) for k in kf_ids], np.int32)
        s = stream if stream is not None else torch.cuda.current_stream(bow_words.device)
        check(self._lib.orb_kfdb_add_batch_device(self._h, len(slots), ptr(slots), ptr(bow_words), ptr(bow_values),
                                                  ptr(bow_n), int(bow_words.shape[1]), ctypes.c_void_p(s.cuda_stream)))

    def erase(self, kf_id) -> None:
        s = self.slot_of(kf_id, create=False)
        if s >= 0:
            check(self._lib.orb_kfdb_erase(self._h, s))

    def clear(self) -> None:
        check(self._lib.orb_kfdb_clear(self._h))
        self._slot = {}
        self._id = []

    def set_covisible(self, kf_id, neighbour_ids) -> None:
        """GetBestCovisibilityKeyFrames(10) of kf_id, in its order."""
        nb = np.array([self.slot_of(k) for k in neighbour_ids], np.int32)
        check(self._lib.orb_kfdb_set_covisible(self._h, self.slot_of(kf_id), ptr(nb), len(nb)))

    # ---- queries ------------------------------------------------------------------------------
    def _host_query(self, call) -> list:
        out = np.zeros(max(len(self._id), 1), np.int32)
        n = ctypes.c_int()
        check(call(ptr(out), len(out), ctypes.byref(n)))
        return self.ids_of(out[: n.value])

    def DetectRelocalisationCandidates(self, bow) -> list:
        w, v = bow_arrays(bow)
        return self._host_query(lambda o, cap, n: self._lib.orb_kfdb_detect_relocalisation_candidates(
            self._h, ptr(w), ptr(v), len(w), o, cap, n))

    def DetectLoopCandidates(self, bow, connected_ids=(), min_score: float = 0.0) -> list:
        """bow = pKF->mBowVec, connected_ids = pKF->GetConnectedKeyFrames()."""
        w, v = bow_arrays(bow)
        conn = [self.slot_of(k, create=False) for k in connected_ids]
        conn = np.array([s for s in conn if s >= 0], np.int32)
        return self._host_query(lambda o, cap, n: self._lib.orb_kfdb_detect_loop_candidates(
            self._h, ptr(w), ptr(v), len(w), ptr(conn), len(conn), float(min_score), o, cap, n))

    def detect_relocalisation_candidates_batch_device(self, bow_words, bow_values, bow_n, out_cap: int = 32,
                                                      stream=None):
        """Q relocalisation queries ((Q, cap) tensors, bow_n (Q,)), equal to Q single calls in
        order.  Returns device tensors (slots (Q, out_cap) int32, n_out (Q,) int32): query q's
        candidates are ids_of(slots[q, :n_out[q]]); n_out[q] > out_cap means the row is cut."""
        import torch

        Q, cap = int(bow_words.shape[0]), int(bow_words.shape[1])
        dev = bow_words.device
        ids = torch.full((Q, out_cap), -1, dtype=torch.int32, device=dev)
        n_out = torch.zeros((Q,), dtype=torch.int32, device=dev)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        check(self._lib.orb_kfdb_detect_relocalisation_candidates_batch_device(
            self._h, Q, ptr(bow_words), ptr(bow_values), ptr(bow_n), cap, ptr(ids), int(out_cap), ptr(n_out),
            ctypes.c_void_p(s.cuda_stream)))
        return ids, n_out

    def debug_last_query(self, q: int = 0) -> dict:
        """Per-slot tables of the last query (include/orb_debug.h: orb_debug_kfdb_last_query)."""
        cap = max(len(self._id), 1)
        t = {"common": np.zeros(cap, np.int32), "first": np.zeros(cap, np.uint32), "seq": np.zeros(cap, np.uint32),
             "scored": np.zeros(cap, np.uint8), "score": np.zeros(cap, np.float64)}
        n = check(self._lib.orb_debug_kfdb_last_query(self._h, int(q), ptr(t["common"]), ptr(t["first"]), ptr(t["seq"]),
                                                      ptr(t["scored"]), ptr(t["score"]), cap))
        return {k: a[:n] for k, a in t.items()}
