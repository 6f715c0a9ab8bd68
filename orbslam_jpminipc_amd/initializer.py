"""Initializer's two-view model scoring on the GPU (reference src/Initializer.cc), over the C ABI
of ``include/orb_abi.h`` (csrc/orb_initializer.hip).

``CheckHomography`` / ``CheckFundamental`` for all RANSAC hypotheses of a frame pair in one call,
with the "keep the best" rule of ``FindHomography`` / ``FindFundamental``.  The hypotheses
(``ComputeH21`` / ``ComputeF21``, ``Normalize``, the ``T2inv*Hn*T1`` / ``inv()`` products) are the
caller's in ``Initializer``: arrays of shape (n_hyp, 3, 3) or (n_hyp, 9), float32, row-major.
``InitializerRansac`` generates them on the device from the caller's rand() values and scores them
in the same call.
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


def initializer_minimal_sets(N: int, rand31) -> np.ndarray:
    """The minimal sets of Initializer::Initialize (Initializer.cc:80-95) for N matches: rand31
    holds n_hyp x 8 values that rand() returned; draw j of a set is RandomInt(0, N - j - 1) =
    (r * (N - j)) >> 31 on a list that loses the drawn *position* (the last entry moves into it), so
    a set never repeats an index.  Returns (n_hyp, 8) int32 match ordinals."""
    r = np.asarray(rand31, np.int64).reshape(-1, 8)
    if N < 8:
        raise ValueError("fewer than 8 matches: the reference would pop from an empty vector")
    if (r < 0).any() or (r >= 1 << 31).any():
        raise ValueError("rand31 values lie in [0, 2^31)")
    sets = np.zeros(r.shape, np.int32)
    for it in range(len(r)):
        avail = list(range(N))
        for j in range(8):
            randi = (int(r[it, j]) * len(avail)) >> 31
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


class InitializerRansac(Initializer):
    """Initializer::Initialize up to the ReconstructH / ReconstructF call (Initializer.cc:44-113) on
    the GPU: the minimal sets from the caller's rand() values, Normalize, ComputeH21 / ComputeF21
    (cv::SVDecomp as OpenCV 2.4's Jacobi SVD is read) and both checks.  The package
    owns no random generator: every call takes `rand31`, (n_hyp, 8) values that rand() returned.
    ``reconstruct`` is ReconstructH / ReconstructF on a given model (CheckRT, Triangulate, DecomposeE,
    DESIGN.md §18) and ``initialize`` the whole of Initialize; the ``*_batch_device`` forms do the same
    for P device-resident pairs."""

    def _pair(self, F1, F2, matches12):
        k1, k2 = _keys(F1), _keys(F2)
        m12 = np.ascontiguousarray(matches12, np.int32)
        if len(m12) != len(k1):
            raise ValueError(f"matches12 holds {len(m12)} entries for {len(k1)} keypoints")
        return k1, k2, m12

    def compute_hypotheses(self, F1, F2, matches12, rand31=None, sets=None) -> dict:
        """ComputeH21 / ComputeF21 of every iteration (host buffers, synchronous) from `rand31` or
        from given `sets` ((n_hyp, 8) match ordinals).  Returns n_matches, sets (n_hyp, 8) int32,
        H21, H12, F21 (what check() takes), Hn, Fn (n_hyp, 9) float32 and T1, T2 (3, 3).  With
        fewer than 8 matches the hypothesis and set rows are zeros."""
        k1, k2, m12 = self._pair(F1, F2, matches12)
        if (rand31 is None) == (sets is None):
            raise ValueError("exactly one of rand31 and sets is given")
        draws = np.ascontiguousarray(rand31 if sets is None else sets, np.int32).reshape(-1, 8)
        n_hyp = len(draws)
        hyp = {k: np.zeros((max(n_hyp, 1), 9), np.float32) for k in ("H21", "H12", "F21", "Hn", "Fn")}
        T = np.zeros((2, 9), np.float32)
        so = np.zeros((max(n_hyp, 1), 8), np.int32)
        nm = ctypes.c_int(0)
        check(self._lib.orb_initializer_compute_hypotheses(
            ptr(k1), len(k1), ptr(k2), len(k2), ptr(m12), n_hyp, ptr(draws if sets is not None else None),
            ptr(draws if sets is None else None), ptr(hyp["H21"]), ptr(hyp["H12"]), ptr(hyp["F21"]), ptr(hyp["Hn"]),
            ptr(hyp["Fn"]), ptr(T[0]), ptr(T[1]), ptr(so), ctypes.byref(nm), self.device))
        out = {k: v[:n_hyp] for k, v in hyp.items()}
        out.update(n_matches=nm.value, sets=so[:n_hyp], T1=T[0].reshape(3, 3), T2=T[1].reshape(3, 3))
        return out

    def find(self, F1, F2, matches12, rand31) -> dict:
        """One Initialize up to RH (host buffers, synchronous).  Returns what check() returns for
        the generated hypotheses, plus sets, H21, H12, F21, H / F (3, 3) float32 (the winners, NaN
        when the best index is -1), RH (float32) and use_h (RH > 0.40: ReconstructH would be
        tried)."""
        k1, k2, m12 = self._pair(F1, F2, matches12)
        draws = np.ascontiguousarray(rand31, np.int32).reshape(-1, 8)
        n_hyp, n1 = len(draws), len(k1)
        hyp = {k: np.zeros((max(n_hyp, 1), 9), np.float32) for k in ("H21", "H12", "F21")}
        so = np.zeros((max(n_hyp, 1), 8), np.int32)
        sc = np.zeros((2, max(n_hyp, 1)), np.float32)
        best = np.full(2, -1, np.int32)
        bs = np.zeros(2, np.float32)
        inl = np.zeros((2, max(n1, 1)), np.uint8)
        bm = np.zeros((2, 9), np.float32)
        rh = np.zeros(1, np.float32)
        use = np.zeros(1, np.int32)
        nm = ctypes.c_int(0)
        check(self._lib.orb_initializer_ransac(
            ptr(k1), n1, ptr(k2), len(k2), ptr(m12), self.mSigma, n_hyp, ptr(draws), ptr(hyp["H21"]), ptr(hyp["H12"]),
            ptr(hyp["F21"]), ptr(so), ptr(sc[0]), ptr(sc[1]), ptr(best[0:]), ptr(bs[0:]), ptr(inl[0]), ptr(best[1:]),
            ptr(bs[1:]), ptr(inl[1]), ptr(bm[0]), ptr(bm[1]), ptr(rh), ptr(use), ctypes.byref(nm), self.device))
        n = nm.value
        out = {k: v[:n_hyp] for k, v in hyp.items()}
        out.update(n_matches=n, sets=so[:n_hyp], scores_h=sc[0, :n_hyp].copy(), scores_f=sc[1, :n_hyp].copy(),
                   best_h=int(best[0]), best_f=int(best[1]), best_score_h=np.float32(bs[0]),
                   best_score_f=np.float32(bs[1]), inliers_h=inl[0, :n].astype(bool), inliers_f=inl[1, :n].astype(bool),
                   H=bm[0].reshape(3, 3), F=bm[1].reshape(3, 3), RH=np.float32(rh[0]), use_h=bool(use[0]))
        return out

    def find_batch_device(self, d_kps, d_counts, pair_f1, pair_f2, d_matches12, d_rand31, stream=None,
                          hypotheses=True) -> dict:
        """P pairs on device-resident extractor and matcher output (orb_initializer_ransac_batch_device):
        the arguments of check_batch_device with d_rand31 (P, n_hyp, 8) int32 (a negative value
        counts as 0) in place of the hypotheses.  Returns the device tensors of check_batch_device
        plus best_H21 / best_F21 (P, 9), RH (P,) float32, use_h (P,) int32 and, when `hypotheses`,
        H21 / H12 / F21 (P, n_hyp, 9) and sets (P, n_hyp, 8).  Asynchronous on `stream`."""
        import torch

        P, cap = int(d_matches12.shape[0]), int(d_kps.shape[1])
        if int(d_matches12.shape[1]) != cap:
            raise ValueError("d_matches12 must be (P, cap)")
        if d_rand31.dtype != torch.int32 or d_rand31.dim() != 3 or int(d_rand31.shape[0]) != P or int(d_rand31.shape[2]) != 8:
            raise ValueError("d_rand31 must be an int32 tensor (P, n_hyp, 8)")
        d_rand31 = d_rand31.contiguous()
        n_hyp = int(d_rand31.shape[1])
        dev = d_kps.device
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):  # the zero fills are ordered before the kernels
            out = {"n_matches": torch.zeros((P,), dtype=torch.int32, device=dev)}
            for t in "hf":
                out["scores_" + t] = torch.empty((P, n_hyp), dtype=torch.float32, device=dev)
                out["best_" + t] = torch.empty((P,), dtype=torch.int32, device=dev)
                out["best_score_" + t] = torch.empty((P,), dtype=torch.float32, device=dev)
                out["inliers_" + t] = torch.zeros((P, cap), dtype=torch.uint8, device=dev)
            out["best_H21"] = torch.empty((P, 9), dtype=torch.float32, device=dev)
            out["best_F21"] = torch.empty((P, 9), dtype=torch.float32, device=dev)
            out["RH"] = torch.empty((P,), dtype=torch.float32, device=dev)
            out["use_h"] = torch.empty((P,), dtype=torch.int32, device=dev)
            if hypotheses:
                for k in ("H21", "H12", "F21"):
                    out[k] = torch.empty((P, n_hyp, 9), dtype=torch.float32, device=dev)
                out["sets"] = torch.empty((P, n_hyp, 8), dtype=torch.int32, device=dev)
        g = lambda k: ptr(out.get(k))  # noqa: E731
        check(self._lib.orb_initializer_ransac_batch_device(
            ptr(d_kps), ptr(d_counts), cap, P, ptr(pair_f1), ptr(pair_f2), ptr(d_matches12), self.mSigma, n_hyp,
            ptr(d_rand31), g("H21"), g("H12"), g("F21"), g("sets"), g("scores_h"), g("scores_f"), g("best_h"),
            g("best_score_h"), g("inliers_h"), g("best_f"), g("best_score_f"), g("inliers_f"), g("n_matches"),
            g("best_H21"), g("best_F21"), g("RH"), g("use_h"), ctypes.c_void_p(s.cuda_stream)))
        return out

    # ---- ReconstructH / ReconstructF and the whole Initialize ----

    _REC_SHAPES = (("ok", (), "int32"), ("R21", (9,), "float32"), ("t21", (3,), "float32"), ("P3D", None, "float32"),
                   ("triangulated", None, "uint8"), ("n_motion", (), "int32"), ("motion_R", (72,), "float32"),
                   ("motion_t", (24,), "float32"), ("n_good", (8,), "int32"), ("cos_parallax", (8,), "float32"),
                   ("parallax_deg", (8,), "float32"), ("best", (), "int32"), ("n_inliers", (), "int32"))

    @staticmethod
    def _K4(K4) -> np.ndarray:
        K4 = np.ascontiguousarray(K4, np.float32).reshape(-1)
        if len(K4) != 4:
            raise ValueError("K4 holds fx, fy, cx, cy")
        return K4

    @classmethod
    def _rec_host(cls, n1):
        o = {}
        for name, shape, dt in cls._REC_SHAPES:
            if shape is None:
                shape = (max(n1, 1), 3) if name == "P3D" else (max(n1, 1),)
            o[name] = np.zeros(shape if shape else (1,), dt)
        return o

    @staticmethod
    def _rec_result(o, n1) -> dict:
        return dict(ok=bool(o["ok"][0]), R21=o["R21"].reshape(3, 3), t21=o["t21"], P3D=o["P3D"][:n1],
                    triangulated=o["triangulated"][:n1].astype(bool), n_motion=int(o["n_motion"][0]),
                    motion_R=o["motion_R"].reshape(8, 3, 3), motion_t=o["motion_t"].reshape(8, 3), n_good=o["n_good"],
                    cos_parallax=o["cos_parallax"], parallax_deg=o["parallax_deg"], best=int(o["best"][0]),
                    n_inliers=int(o["n_inliers"][0]))

    def reconstruct(self, F1, F2, matches12, M21, use_h, inliers, K4, min_parallax: float = 1.0,
                    min_triangulated: int = 50) -> dict:
        """ReconstructH (use_h) or ReconstructF on a given model (host buffers, synchronous).  M21:
        (3, 3) float32; inliers: the model's mask over match ordinals as find() returns inliers_h /
        inliers_f; K4: fx, fy, cx, cy.  Returns ok, R21 (3, 3), t21 (3,), P3D (n1, 3), triangulated
        (n1 bools) (zeros when not ok) and the diagnostics n_motion, motion_R (8, 3, 3), motion_t
        (8, 3), n_good, cos_parallax, parallax_deg (8 each), best and n_inliers."""
        k1, k2, m12 = self._pair(F1, F2, matches12)
        M = np.ascontiguousarray(M21, np.float32).reshape(-1)
        if len(M) != 9:
            raise ValueError("M21 is a 3 x 3 matrix")
        inl = np.ascontiguousarray(np.asarray(inliers).reshape(-1), np.uint8)
        n = int((m12 >= 0).sum())
        if len(inl) < n:
            raise ValueError(f"inliers holds {len(inl)} entries for {n} matches")
        n1 = len(k1)
        K4 = self._K4(K4)  # (kept alive across the call)
        o = self._rec_host(n1)
        check(self._lib.orb_initializer_reconstruct(
            ptr(k1), n1, ptr(k2), len(k2), ptr(m12), ptr(M), int(use_h), ptr(inl), ptr(K4), self.mSigma,
            float(min_parallax), int(min_triangulated), *[ptr(o[name]) for name, _, _ in self._REC_SHAPES], self.device))
        return self._rec_result(o, n1)

    def initialize(self, F1, F2, matches12, rand31, K4, min_parallax: float = 1.0, min_triangulated: int = 50) -> dict:
        """Initializer::Initialize in one call (host buffers, synchronous): what find() returns plus
        what reconstruct() returns for the model it chose."""
        k1, k2, m12 = self._pair(F1, F2, matches12)
        draws = np.ascontiguousarray(rand31, np.int32).reshape(-1, 8)
        n_hyp, n1 = len(draws), len(k1)
        hyp = {k: np.zeros((max(n_hyp, 1), 9), np.float32) for k in ("H21", "H12", "F21")}
        so = np.zeros((max(n_hyp, 1), 8), np.int32)
        sc = np.zeros((2, max(n_hyp, 1)), np.float32)
        best = np.full(2, -1, np.int32)
        bs = np.zeros(2, np.float32)
        inl = np.zeros((2, max(n1, 1)), np.uint8)
        bm = np.zeros((2, 9), np.float32)
        rh = np.zeros(1, np.float32)
        use = np.zeros(1, np.int32)
        nm = ctypes.c_int(0)
        K4 = self._K4(K4)  # (kept alive across the call)
        o = self._rec_host(n1)
        check(self._lib.orb_initializer_initialize(
            ptr(k1), n1, ptr(k2), len(k2), ptr(m12), self.mSigma, n_hyp, ptr(draws), ptr(K4),
            float(min_parallax), int(min_triangulated), ptr(hyp["H21"]), ptr(hyp["H12"]), ptr(hyp["F21"]), ptr(so),
            ptr(sc[0]), ptr(sc[1]), ptr(best[0:]), ptr(bs[0:]), ptr(inl[0]), ptr(best[1:]), ptr(bs[1:]), ptr(inl[1]),
            ptr(bm[0]), ptr(bm[1]), ptr(rh), ptr(use), ctypes.byref(nm),
            *[ptr(o[name]) for name, _, _ in self._REC_SHAPES], self.device))
        n = nm.value
        out = {k: v[:n_hyp] for k, v in hyp.items()}
        out.update(n_matches=n, sets=so[:n_hyp], scores_h=sc[0, :n_hyp].copy(), scores_f=sc[1, :n_hyp].copy(),
                   best_h=int(best[0]), best_f=int(best[1]), best_score_h=np.float32(bs[0]),
                   best_score_f=np.float32(bs[1]), inliers_h=inl[0, :n].astype(bool), inliers_f=inl[1, :n].astype(bool),
                   H=bm[0].reshape(3, 3), F=bm[1].reshape(3, 3), RH=np.float32(rh[0]), use_h=bool(use[0]))
        out.update(self._rec_result(o, n1))
        return out

    @classmethod
    def _rec_device(cls, torch, P, cap, dev) -> dict:
        o = {}
        for name, shape, dt in cls._REC_SHAPES:
            if shape is None:
                shape = (cap, 3) if name == "P3D" else (cap,)
            o[name] = torch.empty((P, *shape), dtype=getattr(torch, dt), device=dev)
        return o

    def reconstruct_batch_device(self, d_kps, d_counts, pair_f1, pair_f2, d_matches12, found: dict, K4,
                                 min_parallax: float = 1.0, min_triangulated: int = 50, stream=None) -> dict:
        """P pairs on what find_batch_device returned (`found`: best_H21, best_F21, use_h, inliers_h,
        inliers_f, n_matches), orb_initializer_reconstruct_batch_device.  Returns device tensors: ok,
        n_motion, best, n_inliers (P,) int32, R21 (P, 9), t21 (P, 3), P3D (P, cap, 3), triangulated
        (P, cap) uint8, motion_R (P, 72), motion_t (P, 24), n_good (P, 8) int32, cos_parallax and
        parallax_deg (P, 8).  Asynchronous on `stream`."""
        import torch

        P, cap = int(d_matches12.shape[0]), int(d_kps.shape[1])
        if int(d_matches12.shape[1]) != cap:
            raise ValueError("d_matches12 must be (P, cap)")
        dev = d_kps.device
        K4 = self._K4(K4)  # (kept alive across the call)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            o = self._rec_device(torch, P, cap, dev)
        check(self._lib.orb_initializer_reconstruct_batch_device(
            ptr(d_kps), ptr(d_counts), cap, P, ptr(pair_f1), ptr(pair_f2), ptr(d_matches12), ptr(found["best_H21"]),
            ptr(found["best_F21"]), ptr(found["use_h"]), ptr(found["inliers_h"]), ptr(found["inliers_f"]),
            ptr(found.get("n_matches")), ptr(K4), self.mSigma, float(min_parallax), int(min_triangulated),
            *[ptr(o[name]) for name, _, _ in self._REC_SHAPES], ctypes.c_void_p(s.cuda_stream)))
        return o

    def initialize_batch_device(self, d_kps, d_counts, pair_f1, pair_f2, d_matches12, d_rand31, K4,
                                min_parallax: float = 1.0, min_triangulated: int = 50, stream=None) -> dict:
        """Initialize for P pairs in one call with no host round trip
        (orb_initializer_initialize_batch_device): the tensors of find_batch_device(hypotheses=False)
        plus those of reconstruct_batch_device.  Asynchronous on `stream`."""
        import torch

        P, cap = int(d_matches12.shape[0]), int(d_kps.shape[1])
        if int(d_matches12.shape[1]) != cap:
            raise ValueError("d_matches12 must be (P, cap)")
        if d_rand31.dtype != torch.int32 or d_rand31.dim() != 3 or int(d_rand31.shape[0]) != P or int(d_rand31.shape[2]) != 8:
            raise ValueError("d_rand31 must be an int32 tensor (P, n_hyp, 8)")
        d_rand31 = d_rand31.contiguous()
        n_hyp = int(d_rand31.shape[1])
        dev = d_kps.device
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):  # the zero fills are ordered before the kernels
            out = {"n_matches": torch.zeros((P,), dtype=torch.int32, device=dev)}
            for t in "hf":
                out["scores_" + t] = torch.empty((P, n_hyp), dtype=torch.float32, device=dev)
                out["best_" + t] = torch.empty((P,), dtype=torch.int32, device=dev)
                out["best_score_" + t] = torch.empty((P,), dtype=torch.float32, device=dev)
                out["inliers_" + t] = torch.zeros((P, cap), dtype=torch.uint8, device=dev)
            out["best_H21"] = torch.empty((P, 9), dtype=torch.float32, device=dev)
            out["best_F21"] = torch.empty((P, 9), dtype=torch.float32, device=dev)
            out["RH"] = torch.empty((P,), dtype=torch.float32, device=dev)
            out["use_h"] = torch.empty((P,), dtype=torch.int32, device=dev)
            o = self._rec_device(torch, P, cap, dev)
        K4 = self._K4(K4)  # (kept alive across the call)
        g = lambda k: ptr(out.get(k))  # noqa: E731
        check(self._lib.orb_initializer_initialize_batch_device(
            ptr(d_kps), ptr(d_counts), cap, P, ptr(pair_f1), ptr(pair_f2), ptr(d_matches12), self.mSigma, n_hyp,
            ptr(d_rand31), ptr(K4), float(min_parallax), int(min_triangulated), g("H21"), g("H12"), g("F21"),
            g("sets"), g("scores_h"), g("scores_f"), g("best_h"), g("best_score_h"), g("inliers_h"), g("best_f"),
            g("best_score_f"), g("inliers_f"), g("n_matches"), g("best_H21"), g("best_F21"), g("RH"), g("use_h"),
            *[ptr(o[name]) for name, _, _ in self._REC_SHAPES], ctypes.c_void_p(s.cuda_stream)))
        out.update(o)
        return out
