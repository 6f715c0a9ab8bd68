"""Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:154-285, csrc/orb_optimizer.hip),
Optimizer::OptimizeSim3 (Optimizer.cc:1721-1917, csrc/orb_sim3opt.hip),
Optimizer::LocalBundleAdjustment (Optimizer.cc:287-536, csrc/orb_localba.hip) and
Optimizer::OptimizeEssentialGraph (Optimizer.cc:1470-1719, csrc/orb_essgraph.hip) on the GPU, over the C
ABI of ``include/orb_abi.h``.

The motion-only optimisation of one frame's pose against its keypoint <-> MapPoint associations:
the whole g2o schedule (four rounds of Levenberg with the outlier classification between them)
runs in one launch per call, one workgroup per problem.  The Sim3 optimisation of a loop candidate
(two optimize() calls with the pair classification between and after them) likewise, and so does
the local bundle adjustment of a window of keyframes and points (both optimize() calls with the
Schur complement, and both outlier classifications).  The essential graph of a loop
correction is one synchronous call whose Levenberg state stays on the device.  Global
bundle adjustment is not part of this package.
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._native import KEYPOINT_DTYPE, check, hip_lib, ptr
from .views import View


class PoseOptInfo(ctypes.Structure):
    """orb_pose_opt_info_t."""

    _fields_ = [("n_initial", ctypes.c_int32), ("n_bad", ctypes.c_int32), ("rounds", ctypes.c_int32),
                ("iterations", ctypes.c_int32 * 4), ("trials", ctypes.c_int32), ("lambda_", ctypes.c_double),
                ("chi2", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"n_initial": self.n_initial, "n_bad": self.n_bad, "rounds": self.rounds,
                "iterations": list(self.iterations), "trials": self.trials, "lambda": self.lambda_, "chi2": self.chi2}


INFO_DTYPE = np.dtype([("n_initial", "<i4"), ("n_bad", "<i4"), ("rounds", "<i4"), ("iterations", "<i4", (4,)),
                       ("trials", "<i4"), ("lambda", "<f8"), ("chi2", "<f8")])
assert INFO_DTYPE.itemsize == ctypes.sizeof(PoseOptInfo) == 48


class Sim3OptInfo(ctypes.Structure):
    """orb_sim3_opt_info_t."""

    _fields_ = [("n_correspondences", ctypes.c_int32), ("n_bad", ctypes.c_int32), ("more_iterations", ctypes.c_int32),
                ("iterations", ctypes.c_int32 * 2), ("trials", ctypes.c_int32), ("lambda_", ctypes.c_double),
                ("chi2", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"n_correspondences": self.n_correspondences, "n_bad": self.n_bad,
                "more_iterations": self.more_iterations, "iterations": list(self.iterations), "trials": self.trials,
                "lambda": self.lambda_, "chi2": self.chi2}


SIM3_INFO_DTYPE = np.dtype([("n_correspondences", "<i4"), ("n_bad", "<i4"), ("more_iterations", "<i4"),
                            ("iterations", "<i4", (2,)), ("trials", "<i4"), ("lambda", "<f8"), ("chi2", "<f8")])
assert SIM3_INFO_DTYPE.itemsize == ctypes.sizeof(Sim3OptInfo) == 40


class LocalBARound(ctypes.Structure):
    """orb_local_ba_round_t."""

    _fields_ = [("iterations", ctypes.c_int32), ("trials", ctypes.c_int32), ("active_edges", ctypes.c_int32),
                ("active_points", ctypes.c_int32), ("active_keyframes", ctypes.c_int32), ("refused", ctypes.c_int32),
                ("lambda_", ctypes.c_double), ("chi2_before", ctypes.c_double), ("chi2_after", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"iterations": self.iterations, "trials": self.trials, "active_edges": self.active_edges,
                "active_points": self.active_points, "active_keyframes": self.active_keyframes,
                "refused": self.refused, "lambda": self.lambda_, "chi2_before": self.chi2_before,
                "chi2_after": self.chi2_after}


class LocalBAInfo(ctypes.Structure):
    """orb_local_ba_info_t."""

    _fields_ = [("status", ctypes.c_int32), ("n_free_kf", ctypes.c_int32), ("round", LocalBARound * 2)]

    def as_dict(self) -> dict:
        return {"status": self.status, "n_free_kf": self.n_free_kf, "round": [r.as_dict() for r in self.round]}


LOCAL_BA_ROUND_DTYPE = np.dtype([("iterations", "<i4"), ("trials", "<i4"), ("active_edges", "<i4"),
                                 ("active_points", "<i4"), ("active_keyframes", "<i4"), ("refused", "<i4"),
                                 ("lambda", "<f8"), ("chi2_before", "<f8"), ("chi2_after", "<f8")])
LOCAL_BA_INFO_DTYPE = np.dtype([("status", "<i4"), ("n_free_kf", "<i4"), ("round", LOCAL_BA_ROUND_DTYPE, (2,))])
assert LOCAL_BA_INFO_DTYPE.itemsize == ctypes.sizeof(LocalBAInfo) == 104
LOCAL_BA_MAX_FREE_KF = 64  # ORB_LBA_MAX_FREE_KF


EG_MAX_TRIALS = 200  # ORB_EG_MAX_TRIALS
EG_MAX_KF = 65536  # ORB_EG_MAX_KF
EG_MAX_PROFILE_BYTES = 256 << 20  # ORB_EG_MAX_PROFILE_BYTES


class EssentialGraphInfo(ctypes.Structure):
    """orb_essential_graph_info_t."""

    _fields_ = [("status", ctypes.c_int32), ("n_active", ctypes.c_int32), ("n_free", ctypes.c_int32),
                ("n_edges", ctypes.c_int32), ("profile_bytes", ctypes.c_int64), ("iterations", ctypes.c_int32),
                ("trials", ctypes.c_int32), ("refused", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("lambda_", ctypes.c_double), ("chi2_before", ctypes.c_double), ("chi2_after", ctypes.c_double),
                ("trial_rho", ctypes.c_double * EG_MAX_TRIALS), ("trial_chi2", ctypes.c_double * EG_MAX_TRIALS),
                ("trial_accepted", ctypes.c_uint8 * EG_MAX_TRIALS)]

    def as_dict(self) -> dict:
        n = min(self.trials, EG_MAX_TRIALS)
        return {"status": self.status, "n_active": self.n_active, "n_free": self.n_free, "n_edges": self.n_edges,
                "profile_bytes": self.profile_bytes, "iterations": self.iterations, "trials": self.trials,
                "refused": self.refused, "lambda": self.lambda_, "chi2_before": self.chi2_before,
                "chi2_after": self.chi2_after, "trial_rho": list(self.trial_rho[:n]),
                "trial_chi2": list(self.trial_chi2[:n]), "trial_accepted": [int(v) for v in self.trial_accepted[:n]]}


assert ctypes.sizeof(EssentialGraphInfo) == 3464


def _sim3_table(table, flags, n):
    """(n, 8) doubles and (n,) u8 flags, or (None, None) where the caller has no such table."""
    if table is None:
        return None, None
    t = np.ascontiguousarray(table, np.float64).reshape(-1, 8)
    f = np.ones(n, np.uint8) if flags is None else np.ascontiguousarray(flags, np.uint8).reshape(-1)
    if len(t) != n or len(f) != n:
        raise ValueError("a Sim3 table holds one row and one flag per keyframe")
    return t, f


def _sim3_13(sim3) -> np.ndarray:
    """13 floats (R row-major, t, s) from that, or from a (R, t, s) triple."""
    if isinstance(sim3, (tuple, list)) and len(sim3) == 3:
        R, t, s = sim3
        sim3 = np.concatenate([np.asarray(R, np.float32).reshape(9), np.asarray(t, np.float32).reshape(3),
                               np.float32([s])])
    return np.ascontiguousarray(sim3, np.float32).reshape(13)


def inv_level_sigma2(level_sigma2) -> np.ndarray:
    """mvInvLevelSigma2[i] = 1 / mvLevelSigma2[i], a float division (Frame.cc:105-107)."""
    return (np.float32(1.0) / np.ascontiguousarray(level_sigma2, np.float32)).astype(np.float32)


def _pose12(pose) -> np.ndarray:
    p = np.asarray(pose, np.float32)
    if p.shape == (4, 4):
        p = np.concatenate([p[:3, :3].reshape(9), p[:3, 3]])
    return np.ascontiguousarray(p, np.float32).reshape(12)


class Optimizer:
    """The GPU half of the reference's Optimizer: ``pose_optimization``, ``optimize_sim3``,
    ``local_bundle_adjustment`` and their batch forms, ``OptimizeEssentialGraph`` and
    ``sim3_correct_points``."""

    def __init__(self, device: int = 0):
        self._lib = hip_lib()
        self.device = int(device)

    def pose_optimization(self, frame, mp_pos, has_mp=None, pose_in=None, K=None, inv_level_sigma2_=None,
                          inv_sigma2=None, want_info: bool = True) -> dict:
        """One frame (host buffers, synchronous).  `frame`: a ``View`` (its keypoints, calibration,
        pose and level table are used), keypoint records (KEYPOINT_DTYPE; give K, pose_in and
        inv_level_sigma2_, an octave outside the table is clamped) or an (n, 2) float32 array of
        undistorted positions (give K, pose_in and the per-keypoint inv_sigma2).  mp_pos (n, 3):
        the MapPoint of keypoint i; has_mp (n,) flags, None = all.  pose_in: 12 floats (Rcw
        row-major, tcw) or a 4x4 Tcw.  Returns pose (12,) float32, pose_f64 (12,), Tcw (4, 4)
        float32, outlier (n,) bool, n_inliers and info."""
        if isinstance(frame, View):
            kps = frame.kps
            K = (frame.fx, frame.fy, frame.cx, frame.cy) if K is None else K
            if pose_in is None:
                pose_in = np.concatenate([frame.Rcw.reshape(9), frame.tcw])
            if inv_level_sigma2_ is None and inv_sigma2 is None:
                inv_level_sigma2_ = inv_level_sigma2(frame.mvLevelSigma2[:frame.nlevels])
        else:
            kps = np.asarray(frame)
        if K is None or pose_in is None:
            raise ValueError("K and pose_in are needed unless a View carries them")
        if kps.dtype == KEYPOINT_DTYPE:
            obs = np.ascontiguousarray(np.stack([kps["x"], kps["y"]], 1), np.float32).reshape(-1, 2)
            if inv_sigma2 is None:
                if inv_level_sigma2_ is None:
                    raise ValueError("keypoint records need inv_level_sigma2_ or inv_sigma2")
                tab = np.ascontiguousarray(inv_level_sigma2_, np.float32)
                inv_sigma2 = tab[np.clip(kps["octave"], 0, len(tab) - 1)]
        else:
            obs = np.ascontiguousarray(kps, np.float32).reshape(-1, 2)
            if inv_sigma2 is None:
                raise ValueError("positions need the per-keypoint inv_sigma2")
        n = len(obs)
        p3d = np.ascontiguousarray(mp_pos, np.float32).reshape(-1, 3)
        s = np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1)
        hm = None if has_mp is None else np.ascontiguousarray(has_mp, np.uint8).reshape(-1)
        if len(p3d) != n or len(s) != n or (hm is not None and len(hm) != n):
            raise ValueError("mp_pos, inv_sigma2 and has_mp must hold one entry per keypoint")
        pin = _pose12(pose_in)
        pose, pose64 = np.zeros(12, np.float32), np.zeros(12, np.float64)
        outl, ninl, info = np.zeros(max(n, 1), np.uint8), ctypes.c_int32(0), PoseOptInfo()
        check(self._lib.orb_pose_optimization(
            n, ptr(p3d), ptr(obs), ptr(s), ptr(hm), float(K[0]), float(K[1]), float(K[2]), float(K[3]), ptr(pin),
            ptr(pose), ptr(pose64), ptr(outl), ctypes.addressof(ninl),
            ctypes.addressof(info) if want_info else None, self.device))
        Tcw = np.eye(4, dtype=np.float32)
        Tcw[:3, :3], Tcw[:3, 3] = pose[:9].reshape(3, 3), pose[9:]
        out = {"pose": pose, "pose_f64": pose64, "Tcw": Tcw, "outlier": outl[:n].astype(bool),
               "n_inliers": int(ninl.value)}
        if want_info:
            out["info"] = info.as_dict()
        return out

    def pose_optimization_batch_device(self, d_kps, d_counts, frame_of, d_mp_pos, d_has_mp, inv_level_sigma2_, K,
                                       d_pose_in, want_f64: bool = True, want_info: bool = True, stream=None) -> dict:
        """S problems on device-resident extractor output (orb_pose_optimization_batch_device).
        d_kps (B, cap, 28) / d_counts (B,): the undistorted records; frame_of (S,) int32 device
        tensor: the frame of each problem; d_mp_pos (S, cap, 3) float32 and d_has_mp (S, cap) uint8
        per problem; inv_level_sigma2_ / K: host floats; d_pose_in (S, 12) float32.  Returns device
        tensors pose (S, 12) float32, pose_f64 (S, 12), outlier (S, cap) uint8, n_inliers (S,) and
        info (S, 48) uint8 (view it as INFO_DTYPE on the host).  Asynchronous on `stream`."""
        import torch

        S, cap = int(frame_of.shape[0]), int(d_kps.shape[1])
        if tuple(d_mp_pos.shape) != (S, cap, 3) or tuple(d_has_mp.shape) != (S, cap) or tuple(d_pose_in.shape) != (S, 12):
            raise ValueError("d_mp_pos must be (S, cap, 3), d_has_mp (S, cap) and d_pose_in (S, 12)")
        if d_mp_pos.dtype != torch.float32 or d_has_mp.dtype != torch.uint8 or d_pose_in.dtype != torch.float32:
            raise ValueError("d_mp_pos / d_pose_in must be float32 and d_has_mp uint8")
        dev = d_kps.device
        tab = np.ascontiguousarray(inv_level_sigma2_, np.float32)
        K4 = np.ascontiguousarray(K, np.float32).reshape(4)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            out = {"pose": torch.empty((S, 12), dtype=torch.float32, device=dev),
                   "outlier": torch.empty((S, cap), dtype=torch.uint8, device=dev),
                   "n_inliers": torch.empty((S,), dtype=torch.int32, device=dev)}
            if want_f64:
                out["pose_f64"] = torch.empty((S, 12), dtype=torch.float64, device=dev)
            if want_info:
                out["info"] = torch.empty((S, INFO_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        check(self._lib.orb_pose_optimization_batch_device(
            ptr(d_kps), ptr(d_counts), cap, S, ptr(frame_of), ptr(d_mp_pos.contiguous()), ptr(d_has_mp.contiguous()),
            ptr(tab), len(tab), ptr(K4), ptr(d_pose_in.contiguous()), ptr(out["pose"]), ptr(out.get("pose_f64")),
            ptr(out["outlier"]), ptr(out["n_inliers"]), ptr(out.get("info")), ctypes.c_void_p(s.cuda_stream)))
        return out

    def optimize_sim3(self, x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, sigma2_2, K1, K2, sim3_in, th2: float = 10.0,
                      usable=None, want_info: bool = True) -> dict:
        """One loop candidate (host buffers, synchronous): Optimizer::OptimizeSim3(pKF1, pKF2,
        vpMatches1, g2oS12, th2).  Slot i is keypoint i of KF1: x3dc1 / x3dc2 (n, 3) the two
        MapPoints in their own keyframe's camera frame, obs1 / obs2 (n, 2) the undistorted positions
        of keypoint i and of its partner i2 in KF2, inv_sigma2_1 (n,) = GetInvSigma2(octave1),
        sigma2_2 (n,) = GetSigma2(octave2) (the reference weights e21 with sigma2, not its
        inverse); usable (n,) flags, None = all.  K1 / K2: fx, fy, cx, cy.  sim3_in: 13 floats (R
        row-major, t, s) or an (R, t, s) triple.  Returns kept (n,) bool (the slot is still matched),
        n_inliers (0 when fewer than 10 pairs survive the first classification: the Sim3 is then the
        input's), sim3 (13,) float32, sim3_f64 (8,) = qx qy qz qw t s, R, t, s and info."""
        x1 = np.ascontiguousarray(x3dc1, np.float32).reshape(-1, 3)
        x2 = np.ascontiguousarray(x3dc2, np.float32).reshape(-1, 3)
        o1 = np.ascontiguousarray(obs1, np.float32).reshape(-1, 2)
        o2 = np.ascontiguousarray(obs2, np.float32).reshape(-1, 2)
        w1 = np.ascontiguousarray(inv_sigma2_1, np.float32).reshape(-1)
        w2 = np.ascontiguousarray(sigma2_2, np.float32).reshape(-1)
        us = None if usable is None else np.ascontiguousarray(usable, np.uint8).reshape(-1)
        n = len(x1)
        if any(len(a) != n for a in (x2, o1, o2, w1, w2)) or (us is not None and len(us) != n):
            raise ValueError("every per-slot array must hold one entry per slot")
        k1 = np.ascontiguousarray(K1, np.float32).reshape(4)
        k2 = np.ascontiguousarray(K2, np.float32).reshape(4)
        sin = _sim3_13(sim3_in)
        kept, out64, out32 = np.zeros(max(n, 1), np.uint8), np.zeros(8, np.float64), np.zeros(13, np.float32)
        ninl, info = ctypes.c_int32(0), Sim3OptInfo()
        check(self._lib.orb_optimize_sim3(
            n, ptr(x1), ptr(x2), ptr(o1), ptr(o2), ptr(w1), ptr(w2), ptr(us), ptr(k1), ptr(k2), float(th2), ptr(sin),
            ptr(kept), ptr(out64), ptr(out32), ctypes.addressof(ninl),
            ctypes.addressof(info) if want_info else None, self.device))
        out = {"kept": kept[:n].astype(bool), "n_inliers": int(ninl.value), "sim3": out32, "sim3_f64": out64,
               "R": out32[:9].reshape(3, 3), "t": out32[9:12], "s": float(out32[12])}
        if want_info:
            out["info"] = info.as_dict()
        return out

    def optimize_sim3_batch_device(self, d_kps, d_counts, pair_a, pair_b, d_match, d_mp_pos, d_mp_bad, d_pose,
                                   level_sigma2, K, d_sim3_in, th2: float = 10.0, want_f64: bool = True,
                                   want_info: bool = True, stream=None) -> dict:
        """S loop candidates on device-resident data (orb_optimize_sim3_batch_device), laid out as
        for ``Sim3Consensus.check_batch_device``: d_kps (B, cap, 28) / d_counts (B,), pair_a /
        pair_b (S,) int32 device tensors, d_match (S, cap) int32 as SearchByBoW (kf_kf) or
        SearchBySim3 leaves it, d_mp_pos (B, cap, 3) float32, d_mp_bad (B, cap) uint8 or None, d_pose
        (B, 12) float32; level_sigma2: the host level table (its float inverse is taken here as
        Frame.cc:105-107 does), K: fx, fy, cx, cy; d_sim3_in (S, 13) float32.  Returns device tensors
        match (S, cap) int32 (the row with the cleared slots at -1), sim3 (S, 13) float32, sim3_f64
        (S, 8), n_inliers (S,) and info (S, 40) uint8 (view it as SIM3_INFO_DTYPE on the host).
        Asynchronous on `stream`."""
        import torch

        S, cap = int(pair_a.shape[0]), int(d_kps.shape[1])
        B = int(d_kps.shape[0])
        if tuple(d_match.shape) != (S, cap) or tuple(d_mp_pos.shape) != (B, cap, 3) or tuple(d_pose.shape) != (B, 12) \
                or tuple(d_sim3_in.shape) != (S, 13) or (d_mp_bad is not None and tuple(d_mp_bad.shape) != (B, cap)):
            raise ValueError("d_match must be (S, cap), d_mp_pos (B, cap, 3), d_mp_bad (B, cap), d_pose (B, 12) "
                             "and d_sim3_in (S, 13)")
        if d_match.dtype != torch.int32 or d_mp_pos.dtype != torch.float32 or d_pose.dtype != torch.float32 \
                or d_sim3_in.dtype != torch.float32 or (d_mp_bad is not None and d_mp_bad.dtype != torch.uint8):
            raise ValueError("d_match must be int32, d_mp_pos / d_pose / d_sim3_in float32 and d_mp_bad uint8")
        dev = d_kps.device
        tab = np.ascontiguousarray(level_sigma2, np.float32).reshape(-1)
        inv = inv_level_sigma2(tab)
        K4 = np.ascontiguousarray(K, np.float32).reshape(4)
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            out = {"match": torch.empty((S, cap), dtype=torch.int32, device=dev),
                   "sim3": torch.empty((S, 13), dtype=torch.float32, device=dev),
                   "n_inliers": torch.empty((S,), dtype=torch.int32, device=dev)}
            if want_f64:
                out["sim3_f64"] = torch.empty((S, 8), dtype=torch.float64, device=dev)
            if want_info:
                out["info"] = torch.empty((S, SIM3_INFO_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        check(self._lib.orb_optimize_sim3_batch_device(
            ptr(d_kps), ptr(d_counts), cap, S, ptr(pair_a), ptr(pair_b), ptr(d_match.contiguous()),
            ptr(d_mp_pos.contiguous()), ptr(d_mp_bad.contiguous()) if d_mp_bad is not None else None,
            ptr(d_pose.contiguous()), ptr(tab), ptr(inv), len(tab), ptr(K4), float(th2), ptr(d_sim3_in.contiguous()),
            ptr(out["match"]), ptr(out["sim3"]), ptr(out.get("sim3_f64")), ptr(out["n_inliers"]),
            ptr(out.get("info")), ctypes.c_void_p(s.cuda_stream)))
        return out

    def local_bundle_adjustment(self, kf_pose, kf_K, kf_fixed, pt_pos, pt_nobs, edge_pt, edge_kf, edge_obs,
                                edge_inv_sigma2, want_info: bool = True) -> dict:
        """One window (host buffers, synchronous): Optimizer::LocalBundleAdjustment on the graph of
        Optimizer.cc:356-447 as flat arrays.  kf_pose (n_kf, 12) (Rcw row-major, tcw) or (n_kf, 4, 4),
        local keyframes first, then fixed; kf_K (n_kf, 4) fx fy cx cy; kf_fixed (n_kf,) flags; pt_pos
        (n_pt, 3); pt_nobs (n_pt,) = mObservations.size() at entry; the edges in creation order, those
        of a point contiguous and the points ascending: edge_pt / edge_kf (n_edge,) indices, edge_obs
        (n_edge, 2) undistorted positions, edge_inv_sigma2 (n_edge,).  Returns kf_pose (n_kf, 12)
        float32, kf_pose_f64, pt_pos (n_pt, 3) float32, pt_pos_f64, edge_erased (n_edge,) uint8 (0
        kept, 1 / 2 the round after which the edge was erased; walk it in edge order to mutate the
        map as the reference does), pt_bad (n_pt,) uint8 and info."""
        kp = np.asarray(kf_pose, np.float32)
        if kp.ndim == 3 and kp.shape[1:] == (4, 4):
            kp = np.concatenate([kp[:, :3, :3].reshape(-1, 9), kp[:, :3, 3]], 1)
        kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 12)
        kK = np.ascontiguousarray(kf_K, np.float32).reshape(-1, 4)
        kf = np.ascontiguousarray(kf_fixed, np.uint8).reshape(-1)
        pp = np.ascontiguousarray(pt_pos, np.float32).reshape(-1, 3)
        pn = np.ascontiguousarray(pt_nobs, np.int32).reshape(-1)
        ep = np.ascontiguousarray(edge_pt, np.int32).reshape(-1)
        ek = np.ascontiguousarray(edge_kf, np.int32).reshape(-1)
        eo = np.ascontiguousarray(edge_obs, np.float32).reshape(-1, 2)
        es = np.ascontiguousarray(edge_inv_sigma2, np.float32).reshape(-1)
        nk, npt, ne = len(kp), len(pp), len(ep)
        if len(kK) != nk or len(kf) != nk or len(pn) != npt or len(ek) != ne or len(eo) != ne or len(es) != ne:
            raise ValueError("the keyframe, point and edge arrays must hold one entry per keyframe, point and edge")
        out = {"kf_pose": np.zeros((nk, 12), np.float32), "kf_pose_f64": np.zeros((nk, 12), np.float64),
               "pt_pos": np.zeros((npt, 3), np.float32), "pt_pos_f64": np.zeros((npt, 3), np.float64),
               "edge_erased": np.zeros(ne, np.uint8), "pt_bad": np.zeros(npt, np.uint8)}
        info = LocalBAInfo()
        check(self._lib.orb_local_bundle_adjustment(
            nk, ptr(kp), ptr(kK), ptr(kf), npt, ptr(pp), ptr(pn), ne, ptr(ep), ptr(ek), ptr(eo), ptr(es),
            ptr(out["kf_pose"]), ptr(out["kf_pose_f64"]), ptr(out["pt_pos"]), ptr(out["pt_pos_f64"]),
            ptr(out["edge_erased"]), ptr(out["pt_bad"]), ctypes.addressof(info) if want_info else None, self.device))
        if want_info:
            out["info"] = info.as_dict()
        return out

    def OptimizeEssentialGraph(self, kf_pose, kf_fixed, edge_i, edge_j, edge_kind, kf_corrected=None,
                               kf_has_corrected=None, kf_noncorrected=None, kf_has_noncorrected=None, pt_pos=None,
                               pt_ref=None, pt_skip=None, n_iterations: int = 20, want_info: bool = True) -> dict:
        """Optimizer::OptimizeEssentialGraph on the pose graph as flat arrays (host buffers,
        synchronous).  kf_pose (n_kf, 12) (Rcw row-major, tcw) or (n_kf, 4, 4) in the
        caller's order; kf_fixed (n_kf,) flags; kf_corrected / kf_noncorrected (n_kf, 8) doubles (q x y z
        w, t, s) with their (n_kf,) flags (a table without flags applies to every keyframe); the edges
        in the order the reference adds them: edge_i (vertex 0), edge_j (vertex 1), edge_kind (0 a loop
        connection, 1 a spanning-tree, loop or covisibility edge).  pt_pos (n_pt, 3), pt_ref (n_pt,) the
        reference keyframe's index or -1, pt_skip (n_pt,) flags of bad points, whose rows come back as
        they went in.  Returns kf_sim3 (n_kf, 8), kf_pose (n_kf, 12) float32, kf_pose_f64, pt_pos (n_pt,
        3) float32, pt_pos_f64 and info."""
        kp = np.asarray(kf_pose, np.float32)
        if kp.ndim == 3 and kp.shape[1:] == (4, 4):
            kp = np.concatenate([kp[:, :3, :3].reshape(-1, 9), kp[:, :3, 3]], 1)
        kp = np.ascontiguousarray(kp, np.float32).reshape(-1, 12)
        nk = len(kp)
        kf = np.ascontiguousarray(kf_fixed, np.uint8).reshape(-1)
        ei = np.ascontiguousarray(edge_i, np.int32).reshape(-1)
        ej = np.ascontiguousarray(edge_j, np.int32).reshape(-1)
        ek = np.ascontiguousarray(edge_kind, np.uint8).reshape(-1)
        ne = len(ei)
        pp = np.zeros((0, 3), np.float32) if pt_pos is None else np.ascontiguousarray(pt_pos, np.float32).reshape(-1, 3)
        npt = len(pp)
        pr = np.zeros(0, np.int32) if pt_ref is None else np.ascontiguousarray(pt_ref, np.int32).reshape(-1)
        ps = None if pt_skip is None else np.ascontiguousarray(pt_skip, np.uint8).reshape(-1)
        if len(kf) != nk or len(ej) != ne or len(ek) != ne or len(pr) != npt or (ps is not None and len(ps) != npt):
            raise ValueError("the keyframe, edge and point arrays must hold one entry per keyframe, edge and point")
        kc, hc = _sim3_table(kf_corrected, kf_has_corrected, nk)
        kn, hn = _sim3_table(kf_noncorrected, kf_has_noncorrected, nk)
        out = {"kf_sim3": np.zeros((nk, 8), np.float64), "kf_pose": np.zeros((nk, 12), np.float32),
               "kf_pose_f64": np.zeros((nk, 12), np.float64), "pt_pos": pp.copy(), "pt_pos_f64": pp.astype(np.float64)}
        info = EssentialGraphInfo()
        check(self._lib.orb_optimize_essential_graph(
            nk, ptr(kp), ptr(kc), ptr(hc), ptr(kn), ptr(hn), ptr(kf), ne, ptr(ei), ptr(ej), ptr(ek), npt, ptr(pp),
            ptr(pr), ptr(ps), int(n_iterations), ptr(out["kf_sim3"]), ptr(out["kf_pose"]), ptr(out["kf_pose_f64"]),
            ptr(out["pt_pos"]), ptr(out["pt_pos_f64"]), ctypes.addressof(info) if want_info else None, self.device))
        if want_info:
            out["info"] = info.as_dict()
        return out

    def sim3_correct_points(self, pt_pos, pt_pair, sim3_from, sim3_to) -> dict:
        """to[pair]^-1.map(from[pair].map(P)) per point (LoopClosing::CorrectLoop lines 466-495;
        host buffers, synchronous).  pt_pos (n_pt, 3); pt_pair (n_pt,) the row of the two (n_pair, 8)
        Sim3 tables, -1 leaves the point as it is.  Returns pt_pos (n_pt, 3) float32 and pt_pos_f64."""
        pp = np.ascontiguousarray(pt_pos, np.float32).reshape(-1, 3)
        pr = np.ascontiguousarray(pt_pair, np.int32).reshape(-1)
        sf = np.ascontiguousarray(sim3_from, np.float64).reshape(-1, 8)
        st = np.ascontiguousarray(sim3_to, np.float64).reshape(-1, 8)
        if len(pr) != len(pp) or len(sf) != len(st):
            raise ValueError("one pair index per point and one row of each table per pair")
        out = {"pt_pos": np.zeros((len(pp), 3), np.float32), "pt_pos_f64": np.zeros((len(pp), 3), np.float64)}
        check(self._lib.orb_sim3_correct_points(len(pp), ptr(pp), ptr(pr), len(sf), ptr(sf), ptr(st), ptr(out["pt_pos"]),
                                                ptr(out["pt_pos_f64"]), self.device))
        return out

    def local_bundle_adjustment_batch_device(self, kf_off, pt_off, edge_off, d_kf_pose, d_kf_K, d_kf_fixed, d_pt_pos,
                                             d_pt_nobs, d_edge_pt, d_edge_kf, d_edge_obs, d_edge_inv_sigma2,
                                             want_f64: bool = True, want_info: bool = True, stream=None,
                                             out: dict = None) -> dict:
        """S windows on device arrays (orb_local_bundle_adjustment_batch_device).  kf_off / pt_off /
        edge_off: (S + 1,) int32 device tensors of offsets into the concatenated keyframe, point and
        edge tensors (d_kf_pose (NK, 12), d_kf_K (NK, 4), d_kf_fixed (NK,) uint8, d_pt_pos (NP, 3),
        d_pt_nobs (NP,) int32, d_edge_pt / d_edge_kf (NE,) int32 problem-local, d_edge_obs (NE, 2),
        d_edge_inv_sigma2 (NE,)); rows past the last offset are not read.  Returns device tensors in
        the same layout: kf_pose (NK, 12) float32, kf_pose_f64, pt_pos (NP, 3), pt_pos_f64,
        edge_erased (NE,) uint8, pt_bad (NP,) uint8 and info (S, 104) uint8 (view it as
        LOCAL_BA_INFO_DTYPE on the host; its status names a problem that was refused and left
        unwritten).  `out`: tensors to write into instead of new ones.  Asynchronous on `stream`."""
        import torch

        S = int(kf_off.shape[0]) - 1
        if S < 0 or int(pt_off.shape[0]) != S + 1 or int(edge_off.shape[0]) != S + 1:
            raise ValueError("kf_off, pt_off and edge_off must hold S + 1 offsets each")
        for t, dt, tail in ((kf_off, torch.int32, ()), (pt_off, torch.int32, ()), (edge_off, torch.int32, ()),
                            (d_kf_pose, torch.float32, (12,)), (d_kf_K, torch.float32, (4,)),
                            (d_kf_fixed, torch.uint8, ()), (d_pt_pos, torch.float32, (3,)), (d_pt_nobs, torch.int32, ()),
                            (d_edge_pt, torch.int32, ()), (d_edge_kf, torch.int32, ()), (d_edge_obs, torch.float32, (2,)),
                            (d_edge_inv_sigma2, torch.float32, ())):
            if t.dtype != dt or tuple(t.shape[1:]) != tail or not t.is_contiguous():
                raise ValueError("a tensor has the wrong dtype or shape, or is not contiguous")
        NK, NP, NE = int(d_kf_pose.shape[0]), int(d_pt_pos.shape[0]), int(d_edge_pt.shape[0])
        if int(d_kf_K.shape[0]) != NK or int(d_kf_fixed.shape[0]) != NK or int(d_pt_nobs.shape[0]) != NP or \
                int(d_edge_kf.shape[0]) != NE or int(d_edge_obs.shape[0]) != NE or int(d_edge_inv_sigma2.shape[0]) != NE:
            raise ValueError("the keyframe, point and edge tensors must hold one row per keyframe, point and edge")
        dev = d_kf_pose.device
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        if out is None:
            with torch.cuda.stream(s):
                out = {"kf_pose": torch.empty((NK, 12), dtype=torch.float32, device=dev),
                       "pt_pos": torch.empty((NP, 3), dtype=torch.float32, device=dev),
                       "edge_erased": torch.empty((NE,), dtype=torch.uint8, device=dev),
                       "pt_bad": torch.empty((NP,), dtype=torch.uint8, device=dev)}
                if want_f64:
                    out["kf_pose_f64"] = torch.empty((NK, 12), dtype=torch.float64, device=dev)
                    out["pt_pos_f64"] = torch.empty((NP, 3), dtype=torch.float64, device=dev)
                if want_info:
                    out["info"] = torch.empty((S, LOCAL_BA_INFO_DTYPE.itemsize), dtype=torch.uint8, device=dev)
        check(self._lib.orb_local_bundle_adjustment_batch_device(
            S, ptr(kf_off), ptr(pt_off), ptr(edge_off), NK, NP, NE, ptr(d_kf_pose), ptr(d_kf_K), ptr(d_kf_fixed),
            ptr(d_pt_pos), ptr(d_pt_nobs), ptr(d_edge_pt), ptr(d_edge_kf), ptr(d_edge_obs), ptr(d_edge_inv_sigma2),
            ptr(out.get("kf_pose")), ptr(out.get("kf_pose_f64")), ptr(out.get("pt_pos")), ptr(out.get("pt_pos_f64")),
            ptr(out.get("edge_erased")), ptr(out.get("pt_bad")), ptr(out.get("info")), ctypes.c_void_p(s.cuda_stream)))
        return out
