"""Initializer's two-view model scoring on the GPU (reference src/Initializer.cc), over the C ABI
of ``include/orb_abi.h`` (csrc/orb_initializer.hip).

``CheckHomography`` / ``CheckFundamental`` for all RANSAC hypotheses of a frame pair in one call,
with the "keep the best" rule of ``FindHomography`` / ``FindFundamental``.  The hypotheses
(``ComputeH21`` / ``ComputeF21``, ``Normalize``, the ``T2inv*Hn*T1`` / ``inv()`` products) are the
caller's: arrays of shape (n_hyp, 3, 3) or (n_hyp, 9), float32, row-major.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._native import KEYPOINT_DTYPE, check, hip_lib, ptr


def _keys(F) -> np.ndarray:
    """mvKeysUn of a Frame, or a keypoint record array as it is."""
    return np.ascontiguousarray(getattr(F, "mvKeysUn", F), KEYPOINT_DTYPE)


def _hyp(a, n_hyp=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a, np.float32).reshape(-1, 9)
    if n_hyp is not None and len(a) != n_hyp:
        raise ValueError(f"{len(a)} hypotheses where the other arrays hold {n_hyp}")
    return a


class Initializer:
    """Initializer(ReferenceFrame, sigma, iterations) (Initializer.cc:33-42) without the frame:
    ``iterations`` is the default hypothesis count a caller generates (mMaxIterations); every call
    takes its count from the arrays it is given."""

    def __init__(self, sigma: float = 1.0, iterations: int = 200, device: int = 0):
        self._lib = hip_lib()
        self.mSigma = float(sigma)
        self.mSigma2 = self.mSigma * self.mSigma
        self.mMaxIterations = int(iterations)
        self.device = int(device)

    def check(self, F1, F2, matches12, H21=None, H12=None, F21=None) -> dict:
        """All hypotheses of one pair (host buffers, synchronous).  F1 / F2: Frames (mvKeysUn) or
        keypoint record arrays; matches12: vnMatches12 (len(F1) ints, -1 = unmatched).
        Returns a dict: n_matches; per given model scores_h / scores_f (n_hyp float32), best_h /
        best_f (index or -1), best_score_h / best_score_f (SH / SF), inliers_h / inliers_f
        (n_matches bools, by match ordinal); and RH = SH / (SH + SF) (Initializer.cc:110) as a
        float32 when both models are given, else None."""
        k1, k2 = _keys(F1), _keys(F2)
        m12 = np.ascontiguousarray(matches12, np.int32)
        if len(m12) != len(k1):
            raise ValueError(f"matches12 holds {len(m12)} entries for {len(k1)} keypoints")
        if (H21 is None) != (H12 is None):
            raise ValueError("H21 and H12 are given together")
        H21, H12, F21 = _hyp(H21), _hyp(H12), _hyp(F21)
        n_hyp = len(H21) if H21 is not None else (len(F21) if F21 is not None else 0)
        _hyp(H12, n_hyp), _hyp(F21, n_hyp)
        n1 = len(k1)
        sc = np.zeros((2, max(n_hyp, 1)), np.float32)
        best = np.full(2, -1, np.int32)
        bs = np.zeros(2, np.float32)
        inl = np.zeros((2, max(n1, 1)), np.uint8)
        nm = ctypes.c_int(0)
        check(self._lib.orb_initializer_check(
            ptr(k1), n1, ptr(k2), len(k2), ptr(m12), self.mSigma, n_hyp, ptr(H21), ptr(H12), ptr(F21), ptr(sc[0]),
            ptr(sc[1]), ptr(best[0:]), ptr(bs[0:]), ptr(inl[0]), ptr(best[1:]), ptr(bs[1:]), ptr(inl[1]),
            ctypes.byref(nm), self.device))
        out = {"n_matches": nm.value, "RH": None}
        if H21 is not None:
            out.update(scores_h=sc[0, :n_hyp].copy(), best_h=int(best[0]), best_score_h=np.float32(bs[0]),
                       inliers_h=inl[0, :nm.value].astype(bool))
        if F21 is not None:
            out.update(scores_f=sc[1, :n_hyp].copy(), best_f=int(best[1]), best_score_f=np.float32(bs[1]),
                       inliers_f=inl[1, :nm.value].astype(bool))
        if H21 is not None and F21 is not None:
            with np.errstate(invalid="ignore", divide="ignore"):
                out["RH"] = np.float32(bs[0]) / (np.float32(bs[0]) + np.float32(bs[1]))
        return out

    def check_batch_device(self, d_kps, d_counts, pair_f1, pair_f2, d_matches12, d_H21=None, d_H12=None, d_F21=None,
                           stream=None) -> dict:
        """P pairs on device-resident extractor and matcher output (orb_initializer_check_batch_device).

        d_kps (B, cap, 28) / d_counts (B,) as ORBextractor.extract_batch_device returns them (or
        mvKeysUn from camera.undistort_keypoints_batch_device); pair_f1 / pair_f2 int32 device
        tensors (P,); d_matches12 (P, cap) int32 as ORBmatcher.search_for_initialization_batch_device
        returns it; d_H21 / d_H12 / d_F21 float32 device tensors (P, n_hyp, 9) or (P, n_hyp, 3, 3).
        Returns a dict of device tensors: n_matches (P,) int32 and, per given model, scores_*
        (P, n_hyp) float32, best_* (P,) int32, best_score_* (P,) float32, inliers_* (P, cap) uint8
        (row p: entries [0, n_matches[p]) by match ordinal, the rest 0).  Asynchronous on `stream`.
        """
        import torch

        P, cap = int(d_matches12.shape[0]), int(d_kps.shape[1])
        if int(d_matches12.shape[1]) != cap:
            raise ValueError("d_matches12 must be (P, cap)")
        if (d_H21 is None) != (d_H12 is None):
            raise ValueError("d_H21 and d_H12 are given together")
        dev = d_kps.device
        hyp = [None if t is None else t.contiguous().reshape(P, -1, 9) for t in (d_H21, d_H12, d_F21)]
        given = [t for t in hyp if t is not None]
        n_hyp = int(given[0].shape[1]) if given else 0
        for t in given:
            if t.dtype != torch.float32 or int(t.shape[1]) != n_hyp:
                raise ValueError("hypotheses must be float32 tensors of one shape (P, n_hyp, 9)")
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        o = {}
        with torch.cuda.stream(s):  # the zero fills are ordered before the kernels
            out = {"n_matches": torch.zeros((P,), dtype=torch.int32, device=dev)}
            for tag, on in (("h", hyp[0] is not None), ("f", hyp[2] is not None)):
                if on:
                    out["scores_" + tag] = torch.empty((P, n_hyp), dtype=torch.float32, device=dev)
                    out["best_" + tag] = torch.empty((P,), dtype=torch.int32, device=dev)
                    out["best_score_" + tag] = torch.empty((P,), dtype=torch.float32, device=dev)
                    out["inliers_" + tag] = torch.zeros((P, cap), dtype=torch.uint8, device=dev)
                for name in ("scores_", "best_", "best_score_", "inliers_"):
                    o[name + tag] = ptr(out.get(name + tag))
        check(self._lib.orb_initializer_check_batch_device(
            ptr(d_kps), ptr(d_counts), cap, P, ptr(pair_f1), ptr(pair_f2), ptr(d_matches12), self.mSigma, n_hyp,
            ptr(hyp[0]), ptr(hyp[1]), ptr(hyp[2]), o["scores_h"], o["scores_f"], o["best_h"], o["best_score_h"],
            o["inliers_h"], o["best_f"], o["best_score_f"], o["inliers_f"], ptr(out["n_matches"]),
            ctypes.c_void_p(s.cuda_stream)))
        return out
