"""The RANSAC consensus of PnPsolver and Sim3Solver on the GPU (reference src/PnPsolver.cc,
src/Sim3Solver.cc), over the C ABI of ``include/orb_abi.h`` (csrc/orb_solvers.hip).

``CheckInliers`` for all hypotheses of a solver in one call, with the constructors'
per-correspondence set-up and the keep-the-best rule of ``iterate``: ``PnPConsensus`` and
``Sim3Consensus`` score hypotheses the caller made.  ``PnPRansac`` and ``Sim3Ransac`` also draw the
minimal sets from the caller's ``rand()`` values and make the hypotheses on the device (EPnP's
``compute_pose`` and ``Refine``; Horn's ``computeT``), so a whole ``iterate`` is one call; the
iteration counters stay with the caller and the package owns no random generator.  ``pnp_ransac_parameters`` / ``sim3_ransac_parameters`` are the scalar arithmetic
of the two ``SetRansacParameters``.
"""
from __future__ import annotations

import ctypes
import math

import numpy as np

from ._native import check, hip_lib, ptr

_INT_MIN = -(2 ** 31)


def _iterations(probability: float, epsilon: np.float32, min_inliers: int, N: int, max_iterations: int) -> int:
    """max(1, min(ceil(log(1 - p) / log(1 - pow(eps, 3))), maxIterations)), the int conversion of a
    non-finite value taken as x86-64 makes it (INT_MIN)."""
    if min_inliers == N:
        n_it = 1
    else:
        try:
            e3 = math.pow(float(epsilon), 3)  # pow(float, int) promotes to double
            v = math.ceil(math.log(1 - probability) / math.log(1 - e3))
            n_it = v if -(2 ** 31) <= v < 2 ** 31 else _INT_MIN
        except (ValueError, ZeroDivisionError, OverflowError):
            n_it = _INT_MIN
    return max(1, min(n_it, int(max_iterations)))


def pnp_ransac_parameters(N: int, probability: float = 0.99, min_inliers: int = 8, max_iterations: int = 300,
                          min_set: int = 4, epsilon: float = 0.4, th2: float = 5.991) -> dict:
    """PnPsolver::SetRansacParameters (PnPsolver.cc:93-129) for N correspondences: the adjusted
    ``min_inliers``, ``epsilon`` (float32), ``max_iterations`` and ``th2`` (float32; mvMaxError =
    sigma2 * th2 is formed on the device).  Tracking.cc:940 calls it with (0.99, 10, 300, 4, 0.5,
    5.991)."""
    N = int(N)
    eps = np.float32(epsilon)
    n_min = int(np.float32(N) * eps)  # int nMinInliers = N*mRansacEpsilon
    n_min = max(n_min, int(min_inliers), int(min_set))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.float32(n_min) / np.float32(N)
    if eps < ratio:
        eps = ratio
    return {"min_inliers": n_min, "epsilon": eps, "max_iterations": _iterations(probability, eps, n_min, N, max_iterations),
            "th2": np.float32(th2)}


def sim3_ransac_parameters(N: int, probability: float = 0.99, min_inliers: int = 6, max_iterations: int = 300) -> dict:
    """Sim3Solver::SetRansacParameters (Sim3Solver.cc:114-138) for N correspondences.
    LoopClosing.cc:290 calls it with (0.99, 20, 300)."""
    N = int(N)
    with np.errstate(divide="ignore", invalid="ignore"):
        eps = np.float32(int(min_inliers)) / np.float32(N)
    return {"min_inliers": int(min_inliers), "epsilon": eps,
            "max_iterations": _iterations(probability, eps, int(min_inliers), N, max_iterations)}


def unpack_mask(words: np.ndarray, n: int) -> np.ndarray:
    """(..., W) uint64 mask rows -> (..., n) bools (bit i % 64 of word i // 64)."""
    words = np.ascontiguousarray(words, np.uint64)
    bits = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little")
    return bits[..., :n].astype(bool)


def _f32(a, cols):
    a = np.ascontiguousarray(a, np.float32)
    return a.reshape(-1, cols) if cols else a.reshape(-1)


def _host_outputs(n_hyp: int, n: int):
    W = (n + 63) // 64
    return (np.zeros(max(n_hyp, 1), np.int32), np.zeros((max(n_hyp, 1), max(W, 1)), np.uint64),
            np.full(max(n_hyp, 1), -1, np.int32), ctypes.c_int32(-1), W)


def _batch_outputs(torch, S, cap, n_hyp, dev):
    W = (cap + 63) // 64
    return {"n": torch.empty((S,), dtype=torch.int32, device=dev),
            "index": torch.empty((S, cap), dtype=torch.int32, device=dev),
            "counts": torch.empty((S, n_hyp), dtype=torch.int32, device=dev),
            "masks": torch.empty((S, n_hyp, W), dtype=torch.int64, device=dev),  # the uint64 words' bits
            "best_at": torch.empty((S, n_hyp), dtype=torch.int32, device=dev),
            "first": torch.empty((S,), dtype=torch.int32, device=dev)}


class PnPConsensus:
    """The consensus half of a PnPsolver (PnPsolver.cc).  fu, fv, uc, vc: the frame's calibration
    (kept as doubles, as the solver keeps them); min_inliers / th2: after ``pnp_ransac_parameters``."""

    def __init__(self, fu: float, fv: float, uc: float, vc: float, min_inliers: int = 8, th2: float = 5.991,
                 device: int = 0):
        self._lib = hip_lib()
        # F.fx etc. are floats widened to the solver's doubles (PnPsolver.cc:76-79)
        self.fu, self.fv, self.uc, self.vc = (float(np.float32(x)) for x in (fu, fv, uc, vc))
        self.min_inliers = int(min_inliers)
        self.th2 = float(np.float32(th2))
        self.device = int(device)

    def check(self, p3d, p2d, sigma2, R, t, best_in: int = 0, want_masks: bool = True) -> dict:
        """All hypotheses of one solver (host buffers, synchronous).  p3d (n, 3), p2d (n, 2), sigma2
        (n,) float32 as the constructor compacts them; R (n_hyp, 3, 3) / t (n_hyp, 3) float64.
        Returns counts (n_hyp,), masks (n_hyp, W) uint64, inliers (n_hyp, n) bool, best_at (n_hyp,),
        first_ok."""
        p3d, p2d, s2 = _f32(p3d, 3), _f32(p2d, 2), _f32(sigma2, 0)
        n = len(p3d)
        if len(p2d) != n or len(s2) != n:
            raise ValueError("p3d, p2d and sigma2 must hold one entry per correspondence")
        R = np.ascontiguousarray(R, np.float64).reshape(-1, 9)
        t = np.ascontiguousarray(t, np.float64).reshape(-1, 3)
        n_hyp = len(R)
        if len(t) != n_hyp:
            raise ValueError(f"{len(t)} translations for {n_hyp} rotations")
        counts, masks, best_at, first, W = _host_outputs(n_hyp, n)
        check(self._lib.orb_pnp_check_inliers(
            n, ptr(p3d), ptr(p2d), ptr(s2), self.th2, self.fu, self.fv, self.uc, self.vc, n_hyp, ptr(R), ptr(t),
            self.min_inliers, int(best_in), ptr(counts), ptr(masks) if want_masks else None, ptr(best_at),
            ctypes.byref(first), self.device))
        out = {"n": n, "counts": counts[:n_hyp], "best_at": best_at[:n_hyp], "first_ok": int(first.value)}
        if want_masks:
            # the library writes rows of W words; the array holds max(W, 1) per row
            m = masks.reshape(-1)[:n_hyp * W].reshape(n_hyp, W)
            out.update(masks=m, inliers=unpack_mask(m, n) if W else np.zeros((n_hyp, 0), bool))
        return out

    def check_batch_device(self, d_kps, d_counts, pair_kf, pair_f, d_match, d_mp_pos, d_mp_bad, level_sigma2, d_R, d_t,
                           d_best_in=None, stream=None) -> dict:
        """S solvers on device-resident extractor / SearchByBoW output
        (orb_pnp_check_inliers_batch_device).  d_kps (B, cap, 28) / d_counts (B,): the undistorted
        records; pair_kf / pair_f (S,) int32 device tensors; d_match (S, cap) int32 as
        ORBmatcher.search_by_bow_batch_device(kf_kf=False) returns it; d_mp_pos (B, cap, 3) float32;
        d_mp_bad (B, cap) uint8 or None; level_sigma2: host floats; d_R (S, n_hyp, 9) / d_t (S, n_hyp,
        3) float64.  Returns device tensors n, index, counts, masks (int64 holding the uint64 words),
        best_at, first_ok.  Asynchronous on `stream`."""
        import torch

        S, cap = int(d_match.shape[0]), int(d_kps.shape[1])
        if int(d_match.shape[1]) != cap:
            raise ValueError("d_match must be (S, cap)")
        dev = d_kps.device
        d_R = d_R.contiguous().reshape(S, -1, 9)
        d_t = d_t.contiguous().reshape(S, -1, 3)
        n_hyp = int(d_R.shape[1])
        if d_R.dtype != torch.float64 or d_t.dtype != torch.float64 or int(d_t.shape[1]) != n_hyp:
            raise ValueError("hypotheses must be float64 tensors (S, n_hyp, 9) and (S, n_hyp, 3)")
        ls2 = np.ascontiguousarray(level_sigma2, np.float32)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            out = _batch_outputs(torch, S, cap, n_hyp, dev)
        check(self._lib.orb_pnp_check_inliers_batch_device(
            ptr(d_kps), ptr(d_counts), cap, S, ptr(pair_kf), ptr(pair_f), ptr(d_match), ptr(d_mp_pos), ptr(d_mp_bad),
            ptr(ls2), len(ls2), self.th2, self.fu, self.fv, self.uc, self.vc, n_hyp, ptr(d_R), ptr(d_t),
            self.min_inliers, ptr(d_best_in), ptr(out["n"]), ptr(out["index"]), ptr(out["counts"]), ptr(out["masks"]),
            ptr(out["best_at"]), ptr(out["first"]), ctypes.c_void_p(s.cuda_stream)))
        out["first_ok"] = out.pop("first")
        return out


class Sim3Consensus:
    """The consensus half of a Sim3Solver (Sim3Solver.cc).  K1 / K2: (fx, fy, cx, cy) of the two
    keyframes; min_inliers as given to SetRansacParameters."""

    def __init__(self, K1, K2=None, min_inliers: int = 6, device: int = 0):
        self._lib = hip_lib()
        self.K1 = np.ascontiguousarray(K1, np.float32).reshape(4)
        self.K2 = self.K1 if K2 is None else np.ascontiguousarray(K2, np.float32).reshape(4)
        self.min_inliers = int(min_inliers)
        self.device = int(device)

    def check(self, x3dc1, x3dc2, sigma2_1, sigma2_2, T12, T21, best_in: int = 0, want_masks: bool = True) -> dict:
        """All hypotheses of one solver (host buffers, synchronous).  x3dc1 / x3dc2 (n, 3) float32
        (mvX3Dc1 / mvX3Dc2), sigma2_1 / sigma2_2 (n,); T12 / T21 (n_hyp, 3, 4) or (n_hyp, 12) float32,
        or 4x4 matrices whose rows 0-2 are taken.  Returns counts, masks, inliers, best_at,
        first_accept."""
        x1, x2, s1, s2 = _f32(x3dc1, 3), _f32(x3dc2, 3), _f32(sigma2_1, 0), _f32(sigma2_2, 0)
        n = len(x1)
        if len(x2) != n or len(s1) != n or len(s2) != n:
            raise ValueError("x3dc1, x3dc2 and the sigma2 arrays must hold one entry per correspondence")
        T12, T21 = _rows012(T12), _rows012(T21)
        n_hyp = len(T12)
        if len(T21) != n_hyp:
            raise ValueError(f"{len(T21)} inverse transforms for {n_hyp} transforms")
        counts, masks, best_at, first, W = _host_outputs(n_hyp, n)
        check(self._lib.orb_sim3_check_inliers(
            n, ptr(x1), ptr(x2), ptr(s1), ptr(s2), ptr(self.K1), ptr(self.K2), n_hyp, ptr(T12), ptr(T21),
            self.min_inliers, int(best_in), ptr(counts), ptr(masks) if want_masks else None, ptr(best_at),
            ctypes.byref(first), self.device))
        out = {"n": n, "counts": counts[:n_hyp], "best_at": best_at[:n_hyp], "first_accept": int(first.value)}
        if want_masks:
            m = masks.reshape(-1)[:n_hyp * W].reshape(n_hyp, W)
            out.update(masks=m, inliers=unpack_mask(m, n) if W else np.zeros((n_hyp, 0), bool))
        return out

    def check_batch_device(self, d_kps, d_counts, pair_1, pair_2, d_match, d_mp_pos, d_mp_bad, d_pose, level_sigma2,
                           d_T12, d_T21, d_best_in=None, stream=None) -> dict:
        """S solvers on device-resident data (orb_sim3_check_inliers_batch_device): as
        PnPConsensus.check_batch_device with d_match from search_by_bow_batch_device(kf_kf=True),
        d_pose (B, 12) float32 (Rcw row-major, then tcw), d_T12 / d_T21 (S, n_hyp, 12) float32 and K1
        as the one calibration.  Precondition: the match row's index pair stands for
        GetIndexInKeyFrame (include/orb_abi.h)."""
        import torch

        S, cap = int(d_match.shape[0]), int(d_kps.shape[1])
        if int(d_match.shape[1]) != cap:
            raise ValueError("d_match must be (S, cap)")
        dev = d_kps.device
        d_T12 = d_T12.contiguous().reshape(S, -1, 12)
        d_T21 = d_T21.contiguous().reshape(S, -1, 12)
        n_hyp = int(d_T12.shape[1])
        if d_T12.dtype != torch.float32 or d_T21.dtype != torch.float32 or int(d_T21.shape[1]) != n_hyp:
            raise ValueError("hypotheses must be float32 tensors (S, n_hyp, 12)")
        ls2 = np.ascontiguousarray(level_sigma2, np.float32)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            out = _batch_outputs(torch, S, cap, n_hyp, dev)
        check(self._lib.orb_sim3_check_inliers_batch_device(
            ptr(d_kps), ptr(d_counts), cap, S, ptr(pair_1), ptr(pair_2), ptr(d_match), ptr(d_mp_pos), ptr(d_mp_bad),
            ptr(d_pose), ptr(ls2), len(ls2), ptr(self.K1), n_hyp, ptr(d_T12), ptr(d_T21), self.min_inliers,
            ptr(d_best_in), ptr(out["n"]), ptr(out["index"]), ptr(out["counts"]), ptr(out["masks"]),
            ptr(out["best_at"]), ptr(out["first"]), ctypes.c_void_p(s.cuda_stream)))
        out["first_accept"] = out.pop("first")
        return out


def _rows012(T) -> np.ndarray:
    T = np.asarray(T, np.float32)
    if T.ndim >= 2 and T.shape[-2:] == (4, 4):
        T = T.reshape(-1, 4, 4)[:, :3, :]
    return np.ascontiguousarray(T, np.float32).reshape(-1, 12)


def sim3_minimal_sets(N: int, rand31, fixed: bool = False) -> np.ndarray:
    """The minimal sets of Sim3Solver::iterate (Sim3Solver.cc:163-177) for (n_hyp, 3) values of
    ``rand()``: draw i is ``RandomInt(0, size - 1) = (r * size) >> 31`` on the list of size N - i,
    and ``vAvailableIndices[idx] = back(); pop_back()`` overwrites the entry at the value drawn, not
    at the position, so a set may hold an index twice.  The list is N entries whose size shrinks;
    the write may land one slot past the size, where nothing reads it.  ``fixed`` removes by
    position instead (what the reference meant; for tests)."""
    return _minimal_sets(N, rand31, 3, fixed)


def _minimal_sets(N: int, rand31, K: int, fixed: bool) -> np.ndarray:
    # the one sampler of Sim3Solver (K = 3) and PnPsolver (K = 4)
    N = int(N)
    r = np.asarray(rand31, np.int64).reshape(-1, K)
    if N < K:
        raise ValueError(f"a minimal set is drawn from at least {K} correspondences")
    if r.size and (r.min() < 0 or r.max() >= 2 ** 31):
        raise ValueError("rand31 values must be in [0, 2^31)")
    sets = np.zeros((len(r), K), np.int32)
    for h in range(len(r)):
        avail = list(range(N))
        size = N
        for i in range(K):
            randi = (int(r[h, i]) * size) >> 31
            idx = avail[randi]
            sets[h, i] = idx
            avail[randi if fixed else idx] = avail[size - 1]
            size -= 1
    return sets


def _draws(sets, rand31):
    if (sets is None) == (rand31 is None):
        raise ValueError("exactly one of sets and rand31 must be given")
    a = np.asarray(sets if rand31 is None else rand31)
    if a.size and (a.min() < -(2 ** 31) or a.max() >= 2 ** 31):
        raise ValueError("rand31 values must be in [0, 2^31)")
    a = np.ascontiguousarray(a, np.int32).reshape(-1, 3)
    return (a, None, len(a)) if rand31 is None else (None, a, len(a))


class Sim3Ransac(Sim3Consensus):
    """A whole Sim3Solver::iterate on the GPU (Sim3Solver.cc:140-207): the minimal sets from the
    caller's ``rand()`` values, Horn's closed form (``computeT``) per set, ``CheckInliers`` and the
    keep-the-best rule, in one call.  K1 / K2 / min_inliers as for Sim3Consensus; min_inliers >= 3."""

    def compute_hypotheses(self, x3dc1, x3dc2, sets=None, rand31=None) -> dict:
        """``computeT`` alone (orb_sim3_compute_hypotheses; host buffers, synchronous) for (n_hyp, 3)
        ``sets`` of indices or ``rand31`` values.  Returns T12 / T21 (n_hyp, 3, 4), sim3 (n_hyp, 13: R
        row-major, t, s), quat (n_hyp, 4: the best eigenvector of Horn's N, w first) and sets."""
        x1, x2 = _f32(x3dc1, 3), _f32(x3dc2, 3)
        n = len(x1)
        if len(x2) != n:
            raise ValueError("x3dc1 and x3dc2 must hold one entry per correspondence")
        sets, rand31, n_hyp = _draws(sets, rand31)
        m = max(n_hyp, 1)
        T12, T21 = np.zeros((m, 3, 4), np.float32), np.zeros((m, 3, 4), np.float32)
        sim3, quat, sets_out = np.zeros((m, 13), np.float32), np.zeros((m, 4), np.float32), np.zeros((m, 3), np.int32)
        check(self._lib.orb_sim3_compute_hypotheses(n, ptr(x1), ptr(x2), n_hyp, ptr(sets), ptr(rand31), ptr(T12),
                                                    ptr(T21), ptr(sim3), ptr(quat), ptr(sets_out), self.device))
        return {"T12": T12[:n_hyp], "T21": T21[:n_hyp], "sim3": sim3[:n_hyp], "quat": quat[:n_hyp],
                "sets": sets_out[:n_hyp]}

    def iterate(self, x3dc1, x3dc2, sigma2_1, sigma2_2, sets=None, rand31=None, best_in: int = 0,
                want_masks: bool = True) -> dict:
        """One ``iterate(n_hyp, ...)`` without its early return (orb_sim3_ransac; host buffers,
        synchronous).  Returns what Sim3Consensus.check returns plus T12, T21, sim3, sets and
        ``accepted`` (13,): the Sim3 of hypothesis first_accept, or of best_at[-1] when nothing was
        accepted (NaN while the best is still an earlier call's)."""
        x1, x2, s1, s2 = _f32(x3dc1, 3), _f32(x3dc2, 3), _f32(sigma2_1, 0), _f32(sigma2_2, 0)
        n = len(x1)
        if len(x2) != n or len(s1) != n or len(s2) != n:
            raise ValueError("x3dc1, x3dc2 and the sigma2 arrays must hold one entry per correspondence")
        sets, rand31, n_hyp = _draws(sets, rand31)
        counts, masks, best_at, first, W = _host_outputs(n_hyp, n)
        m = max(n_hyp, 1)
        T12, T21 = np.zeros((m, 3, 4), np.float32), np.zeros((m, 3, 4), np.float32)
        sim3, sets_out, accepted = np.zeros((m, 13), np.float32), np.zeros((m, 3), np.int32), np.zeros(13, np.float32)
        check(self._lib.orb_sim3_ransac(
            n, ptr(x1), ptr(x2), ptr(s1), ptr(s2), ptr(self.K1), ptr(self.K2), n_hyp, ptr(sets), ptr(rand31),
            self.min_inliers, int(best_in), ptr(counts), ptr(masks) if want_masks else None, ptr(best_at),
            ctypes.byref(first), ptr(T12), ptr(T21), ptr(sim3), ptr(sets_out), ptr(accepted), self.device))
        out = {"n": n, "counts": counts[:n_hyp], "best_at": best_at[:n_hyp], "first_accept": int(first.value),
               "T12": T12[:n_hyp], "T21": T21[:n_hyp], "sim3": sim3[:n_hyp], "sets": sets_out[:n_hyp],
               "accepted": accepted}
        if want_masks:
            mm = masks.reshape(-1)[:n_hyp * W].reshape(n_hyp, W)
            out.update(masks=mm, inliers=unpack_mask(mm, n) if W else np.zeros((n_hyp, 0), bool))
        return out

    def iterate_batch_device(self, d_kps, d_counts, pair_1, pair_2, d_match, d_mp_pos, d_mp_bad, d_pose, level_sigma2,
                             d_rand31, d_best_in=None, stream=None) -> dict:
        """S solvers on device-resident data (orb_sim3_ransac_batch_device): as
        Sim3Consensus.check_batch_device with d_rand31 (S, n_hyp, 3) int32 in place of the
        hypotheses (a negative value is clamped to 0).  Returns its device tensors plus T12 / T21 (S,
        n_hyp, 12), sim3 (S, n_hyp, 13), sets (S, n_hyp, 3), accepted (S, 13: what
        Optimizer.optimize_sim3_batch_device takes as d_sim3_in) and accepted_mask (S, W) int64.
        Asynchronous on `stream`."""
        import torch

        S, cap = int(d_match.shape[0]), int(d_kps.shape[1])
        if int(d_match.shape[1]) != cap:
            raise ValueError("d_match must be (S, cap)")
        dev = d_kps.device
        if d_rand31.dtype != torch.int32 or d_rand31.dim() != 3 or int(d_rand31.shape[0]) != S or int(d_rand31.shape[2]) != 3:
            raise ValueError("d_rand31 must be an int32 tensor (S, n_hyp, 3)")
        d_rand31 = d_rand31.contiguous()
        n_hyp = int(d_rand31.shape[1])
        ls2 = np.ascontiguousarray(level_sigma2, np.float32)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            out = _batch_outputs(torch, S, cap, n_hyp, dev)
            W = (cap + 63) // 64
            out.update(T12=torch.empty((S, n_hyp, 12), dtype=torch.float32, device=dev),
                       T21=torch.empty((S, n_hyp, 12), dtype=torch.float32, device=dev),
                       sim3=torch.empty((S, n_hyp, 13), dtype=torch.float32, device=dev),
                       sets=torch.empty((S, n_hyp, 3), dtype=torch.int32, device=dev),
                       accepted=torch.empty((S, 13), dtype=torch.float32, device=dev),
                       accepted_mask=torch.empty((S, W), dtype=torch.int64, device=dev))
        check(self._lib.orb_sim3_ransac_batch_device(
            ptr(d_kps), ptr(d_counts), cap, S, ptr(pair_1), ptr(pair_2), ptr(d_match), ptr(d_mp_pos), ptr(d_mp_bad),
            ptr(d_pose), ptr(ls2), len(ls2), ptr(self.K1), n_hyp, ptr(d_rand31), self.min_inliers, ptr(d_best_in),
            ptr(out["n"]), ptr(out["index"]), ptr(out["counts"]), ptr(out["masks"]), ptr(out["best_at"]),
            ptr(out["first"]), ptr(out["T12"]), ptr(out["T21"]), ptr(out["sim3"]), ptr(out["sets"]),
            ptr(out["accepted"]), ptr(out["accepted_mask"]), ctypes.c_void_p(s.cuda_stream)))
        out["first_accept"] = out.pop("first")
        return out


def pnp_minimal_sets(N: int, rand31, fixed: bool = False) -> np.ndarray:
    """The minimal sets of PnPsolver::iterate (PnPsolver.cc:160-173) for (n_hyp, 4) values of ``rand()``:
    ``sim3_minimal_sets`` with four draws (the same removal by value)."""
    return _minimal_sets(N, rand31, 4, fixed)


def _draws4(sets, rand31):
    if (sets is None) == (rand31 is None):
        raise ValueError("exactly one of sets and rand31 must be given")
    a = np.asarray(sets if rand31 is None else rand31)
    if a.size and (a.min() < -(2 ** 31) or a.max() >= 2 ** 31):
        raise ValueError("rand31 values must be in [0, 2^31)")
    a = np.ascontiguousarray(a, np.int32).reshape(-1, 4)
    return (a, None, len(a)) if rand31 is None else (None, a, len(a))


class PnPRansac(PnPConsensus):
    """A whole PnPsolver::iterate on the GPU (PnPsolver.cc:137-277): the minimal sets from the caller's
    ``rand()`` values, EPnP's ``compute_pose`` per set, ``CheckInliers``, the keep-the-best rule and
    ``Refine`` at the iterations that replaced the best, in one call.  Arguments as for PnPConsensus;
    min_inliers >= 4."""

    @staticmethod
    def iterations(max_its: int, done: int, n_iterations: int) -> int:
        """How many iterations ``iterate(n_iterations, ...)`` runs at most: its loop goes on while
        ``mnIterations < mRansacMaxIts || nCurrentIterations < nIterations`` (PnPsolver.cc:154), an OR, so
        it is max(mRansacMaxIts - mnIterations, nIterations), the n_hyp to draw values for."""
        return max(int(max_its) - int(done), int(n_iterations))

    def compute_hypotheses(self, p3d, p2d, sets=None, rand31=None) -> dict:
        """``compute_pose`` on minimal sets alone (orb_pnp_compute_hypotheses; host buffers, synchronous)
        for (n_hyp, 4) ``sets`` of indices or ``rand31`` values.  Returns R (n_hyp, 3, 3), t (n_hyp, 3)
        float64, rep_error (n_hyp,) and sets."""
        p3d, p2d = _f32(p3d, 3), _f32(p2d, 2)
        n = len(p3d)
        if len(p2d) != n:
            raise ValueError("p3d and p2d must hold one entry per correspondence")
        sets, rand31, n_hyp = _draws4(sets, rand31)
        m = max(n_hyp, 1)
        R, t, rep, sets_out = np.zeros((m, 3, 3)), np.zeros((m, 3)), np.zeros(m), np.zeros((m, 4), np.int32)
        check(self._lib.orb_pnp_compute_hypotheses(n, ptr(p3d), ptr(p2d), self.fu, self.fv, self.uc, self.vc, n_hyp,
                                                   ptr(sets), ptr(rand31), ptr(R), ptr(t), ptr(rep), ptr(sets_out),
                                                   self.device))
        return {"R": R[:n_hyp], "t": t[:n_hyp], "rep_error": rep[:n_hyp], "sets": sets_out[:n_hyp]}

    def compute_pose(self, p3d, p2d, sel) -> dict:
        """``compute_pose`` on the correspondences ``sel`` in that order (orb_pnp_compute_pose_n): what
        ``Refine`` computes on the set bits of a mask.  Returns R (3, 3), t (3,), rep_error."""
        p3d, p2d = _f32(p3d, 3), _f32(p2d, 2)
        sel = np.ascontiguousarray(sel, np.int32).reshape(-1)
        R, t, rep = np.zeros((3, 3)), np.zeros(3), np.zeros(1)
        check(self._lib.orb_pnp_compute_pose_n(len(p3d), ptr(p3d), ptr(p2d), self.fu, self.fv, self.uc, self.vc,
                                               len(sel), ptr(sel), ptr(R), ptr(t), ptr(rep), self.device))
        return {"R": R, "t": t, "rep_error": float(rep[0])}

    def iterate(self, p3d, p2d, sigma2, sets=None, rand31=None, best_in: int = 0, want_masks: bool = True) -> dict:
        """One ``iterate`` over n_hyp iterations without its early return (orb_pnp_ransac; host buffers,
        synchronous).  Returns what PnPConsensus.check returns plus R, t, sets, refined_counts (n_hyp,:
        Refine's count at the replacing iterations, -1 elsewhere), first_refined (where iterate returns;
        first_refined + 1 sets of draws were consumed), pose (12,) float32 (Rcw row-major, tcw),
        pose_mask (W,), pose_in (n,) bool and pose_inliers."""
        p3d, p2d, s2 = _f32(p3d, 3), _f32(p2d, 2), _f32(sigma2, 0)
        n = len(p3d)
        if len(p2d) != n or len(s2) != n:
            raise ValueError("p3d, p2d and sigma2 must hold one entry per correspondence")
        sets, rand31, n_hyp = _draws4(sets, rand31)
        counts, masks, best_at, first, W = _host_outputs(n_hyp, n)
        m = max(n_hyp, 1)
        R, t, sets_out = np.zeros((m, 3, 3)), np.zeros((m, 3)), np.zeros((m, 4), np.int32)
        rc, fr, pin = np.zeros(m, np.int32), ctypes.c_int32(-1), ctypes.c_int32(0)
        pose, pmask = np.zeros(12, np.float32), np.zeros(max(W, 1), np.uint64)
        check(self._lib.orb_pnp_ransac(
            n, ptr(p3d), ptr(p2d), ptr(s2), self.th2, self.fu, self.fv, self.uc, self.vc, n_hyp, ptr(sets), ptr(rand31),
            self.min_inliers, int(best_in), ptr(counts), ptr(masks) if want_masks else None, ptr(best_at),
            ctypes.byref(first), ptr(R), ptr(t), ptr(sets_out), ptr(rc), ctypes.byref(fr), ptr(pose), ptr(pmask),
            ctypes.byref(pin), self.device))
        out = {"n": n, "counts": counts[:n_hyp], "best_at": best_at[:n_hyp], "first_ok": int(first.value),
               "R": R[:n_hyp], "t": t[:n_hyp], "sets": sets_out[:n_hyp], "refined_counts": rc[:n_hyp],
               "first_refined": int(fr.value), "pose": pose, "pose_mask": pmask[:W],
               "pose_in": unpack_mask(pmask[:W], n) if W else np.zeros(0, bool), "pose_inliers": int(pin.value)}
        if want_masks:
            mm = masks.reshape(-1)[:n_hyp * W].reshape(n_hyp, W)
            out.update(masks=mm, inliers=unpack_mask(mm, n) if W else np.zeros((n_hyp, 0), bool))
        return out

    def iterate_batch_device(self, d_kps, d_counts, pair_kf, pair_f, d_match, d_mp_pos, d_mp_bad, level_sigma2, d_rand31,
                             d_best_in=None, stream=None) -> dict:
        """S solvers on device-resident data (orb_pnp_ransac_batch_device): as
        PnPConsensus.check_batch_device with d_rand31 (S, n_hyp, 4) int32 in place of the hypotheses (a
        negative value is clamped to 0).  Returns its device tensors plus R (S, n_hyp, 9), t (S, n_hyp,
        3) float64, sets (S, n_hyp, 4), refined_counts (S, n_hyp), first_refined (S,), pose (S, 12)
        float32 (what Optimizer.pose_optimization_batch_device takes as its input pose), pose_mask (S,
        W) int64 and pose_inliers (S,).  Asynchronous on `stream`."""
        import torch

        S, cap = int(d_match.shape[0]), int(d_kps.shape[1])
        if int(d_match.shape[1]) != cap:
            raise ValueError("d_match must be (S, cap)")
        dev = d_kps.device
        if d_rand31.dtype != torch.int32 or d_rand31.dim() != 3 or int(d_rand31.shape[0]) != S or int(d_rand31.shape[2]) != 4:
            raise ValueError("d_rand31 must be an int32 tensor (S, n_hyp, 4)")
        d_rand31 = d_rand31.contiguous()
        n_hyp = int(d_rand31.shape[1])
        ls2 = np.ascontiguousarray(level_sigma2, np.float32)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            out = _batch_outputs(torch, S, cap, n_hyp, dev)
            W = (cap + 63) // 64
            out.update(R=torch.empty((S, n_hyp, 9), dtype=torch.float64, device=dev),
                       t=torch.empty((S, n_hyp, 3), dtype=torch.float64, device=dev),
                       sets=torch.empty((S, n_hyp, 4), dtype=torch.int32, device=dev),
                       refined_counts=torch.empty((S, n_hyp), dtype=torch.int32, device=dev),
                       first_refined=torch.empty((S,), dtype=torch.int32, device=dev),
                       pose=torch.empty((S, 12), dtype=torch.float32, device=dev),
                       pose_mask=torch.empty((S, W), dtype=torch.int64, device=dev),
                       pose_inliers=torch.empty((S,), dtype=torch.int32, device=dev))
        check(self._lib.orb_pnp_ransac_batch_device(
            ptr(d_kps), ptr(d_counts), cap, S, ptr(pair_kf), ptr(pair_f), ptr(d_match), ptr(d_mp_pos), ptr(d_mp_bad),
            ptr(ls2), len(ls2), self.th2, self.fu, self.fv, self.uc, self.vc, n_hyp, ptr(d_rand31), self.min_inliers,
            ptr(d_best_in), ptr(out["n"]), ptr(out["index"]), ptr(out["counts"]), ptr(out["masks"]), ptr(out["best_at"]),
            ptr(out["first"]), ptr(out["R"]), ptr(out["t"]), ptr(out["sets"]), ptr(out["refined_counts"]),
            ptr(out["first_refined"]), ptr(out["pose"]), ptr(out["pose_mask"]), ptr(out["pose_inliers"]),
            ctypes.c_void_p(s.cuda_stream)))
        out["first_ok"] = out.pop("first")
        return out
