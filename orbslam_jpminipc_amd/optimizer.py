"""Optimizer::PoseOptimization(Frame*) on the GPU (reference src/Optimizer.cc:154-285), over the C
ABI of ``include/orb_abi.h`` (csrc/orb_optimizer.hip).

The motion-only optimisation of one frame's pose against its keypoint <-> MapPoint associations:
the whole g2o schedule (four rounds of Levenberg with the outlier classification between them)
runs in one launch per call, one workgroup per problem.  Local and global bundle adjustment are
not part of this package.
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


def inv_level_sigma2(level_sigma2) -> np.ndarray:
    """mvInvLevelSigma2[i] = 1 / mvLevelSigma2[i], a float division (Frame.cc:105-107)."""
    return (np.float32(1.0) / np.ascontiguousarray(level_sigma2, np.float32)).astype(np.float32)


def _pose12(pose) -> np.ndarray:
    p = np.asarray(pose, np.float32)
    if p.shape == (4, 4):
        p = np.concatenate([p[:3, :3].reshape(9), p[:3, 3]])
    return np.ascontiguousarray(p, np.float32).reshape(12)


class Optimizer:
    """The GPU half of the reference's Optimizer: ``pose_optimization`` and its batch form."""

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
