"""MapPoint-level helpers over the C ABI (csrc/orb_mappoint.hip)."""
from __future__ import annotations

import ctypes

import numpy as np

from ._native import check, hip_lib, ptr


def compute_distinctive_descriptors(offsets, desc, usable=None, current=None, device: int = 0):
    """MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:185-250) for many points.

    offsets (M + 1,): point m observes rows offsets[m] .. offsets[m+1]-1 of desc (R, 32), in
    the order of its observations map; usable (R,) = keyframe not bad (None = all); current
    (M, 32) = the points' descriptors before the call (kept where no row is usable).
    Returns (best_row (M,) int32, -1 = unchanged; descriptors (M, 32) uint8).
    """
    off = np.ascontiguousarray(np.asarray(offsets, np.int32))
    d = np.ascontiguousarray(np.asarray(desc, np.uint8).reshape(-1, 32))
    M = len(off) - 1
    u = None if usable is None else np.ascontiguousarray(np.asarray(usable, np.uint8).reshape(-1))
    if u is not None and len(u) != len(d):
        raise ValueError("usable must have one flag per row")
    out = (np.zeros((max(M, 1), 32), np.uint8) if current is None
           else np.ascontiguousarray(np.array(current, np.uint8).reshape(-1, 32)))
    best = np.full(max(M, 1), -1, np.int32)
    check(hip_lib().orb_compute_distinctive_descriptors(M, ptr(off), ptr(d), ptr(u), ptr(best), ptr(out), device))
    return best[:M], out[:M]


def compute_distinctive_descriptors_device(d_offsets, d_desc, d_usable, max_obs, d_best_row, d_out_desc, stream=None):
    """orb_compute_distinctive_descriptors_device on device tensors: d_offsets (M + 1,) int32,
    d_desc (R, 32) uint8 (16-byte aligned), d_usable (R,) uint8 or None, max_obs >= the largest
    offsets[m+1] - offsets[m] (the kernel's LDS is sized from it: the caller must not understate
    it), d_best_row (M,) int32 and d_out_desc (M, 32) uint8 written in place (rows of points with
    no usable observation are left alone, best_row -1); enqueued on `stream`."""
    import torch

    M = int(d_offsets.shape[0]) - 1
    s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
    check(hip_lib().orb_compute_distinctive_descriptors_device(M, ptr(d_offsets), ptr(d_desc), ptr(d_usable),
                                                               int(max_obs), ptr(d_best_row), ptr(d_out_desc),
                                                               ctypes.c_void_p(s.cuda_stream)))
    return d_best_row, d_out_desc


def update_normal_and_depth(offsets, obs_Ow, pos, ref_Ow, ref_level, scale_factors, device: int = 0):
    """MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:273-312) for many points.

    offsets (M + 1,): point m is observed from the camera centres obs_Ow rows offsets[m] ..
    offsets[m+1]-1 ((R, 3), GetCameraCenter of each observing keyframe), in the order of its
    observations map: the float sum of the unit vectors depends on that order, which is the caller's.
    pos (M, 3), ref_Ow (M, 3) the reference keyframe's centre, ref_level (M,) the octave of the point's
    keypoint there, scale_factors (nlevels,) the reference keyframe's mvScaleFactors.
    Returns (normal (M, 3), dmin (M,), dmax (M,)) float32; a point without an observation has a NaN
    normal, as the reference's 0 * inf gives."""
    off = np.ascontiguousarray(np.asarray(offsets, np.int32))
    ow = np.ascontiguousarray(np.asarray(obs_Ow, np.float32).reshape(-1, 3))
    p = np.ascontiguousarray(np.asarray(pos, np.float32).reshape(-1, 3))
    ro = np.ascontiguousarray(np.asarray(ref_Ow, np.float32).reshape(-1, 3))
    lv = np.ascontiguousarray(np.asarray(ref_level, np.int32).reshape(-1))
    sf = np.ascontiguousarray(np.asarray(scale_factors, np.float32).reshape(-1))
    M = len(off) - 1
    if len(p) != M or len(ro) != M or len(lv) != M:
        raise ValueError("pos, ref_Ow and ref_level must have one row per point")
    normal, dmin, dmax = np.zeros((max(M, 1), 3), np.float32), np.zeros(max(M, 1), np.float32), np.zeros(max(M, 1), np.float32)
    check(hip_lib().orb_update_normal_and_depth(M, ptr(off), ptr(ow), ptr(p), ptr(ro), ptr(lv), ptr(sf), len(sf),
                                                ptr(normal), ptr(dmin), ptr(dmax), device))
    return normal[:M], dmin[:M], dmax[:M]


def update_normal_and_depth_device(d_offsets, d_obs_Ow, d_pos, d_ref_Ow, d_ref_level, scale_factors, max_obs, d_normal,
                                   d_dmin, d_dmax, stream=None):
    """orb_update_normal_and_depth_device on device tensors: d_offsets (M + 1,) int32, d_obs_Ow (R, 3),
    d_pos / d_ref_Ow (M, 3) float32, d_ref_level (M,) int32; scale_factors stays a host table; max_obs >=
    the largest offsets[m+1] - offsets[m] (no point is walked further); d_normal (M, 3), d_dmin, d_dmax
    (M,) written in place (any may be None); enqueued on `stream`."""
    import torch

    M = int(d_offsets.shape[0]) - 1
    sf = np.ascontiguousarray(np.asarray(scale_factors, np.float32).reshape(-1))
    s = stream if stream is not None else torch.cuda.current_stream(d_offsets.device)
    check(hip_lib().orb_update_normal_and_depth_device(M, ptr(d_offsets), ptr(d_obs_Ow), ptr(d_pos), ptr(d_ref_Ow),
                                                       ptr(d_ref_level), ptr(sf), len(sf), int(max_obs), ptr(d_normal),
                                                       ptr(d_dmin), ptr(d_dmax), ctypes.c_void_p(s.cuda_stream)))
    return d_normal, d_dmin, d_dmax
