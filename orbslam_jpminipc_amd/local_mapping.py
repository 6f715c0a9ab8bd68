"""LocalMapping::CreateNewMapPoints over the C ABI (csrc/orb_localmap.hip):
ComputeF12, ComputeSceneMedianDepth, the triangulation of a matched pair with all its gates, and the
reference's neighbour loop on top of ORBmatcher.SearchForTriangulation.  The thread, the map mutation
and the culling stay with the caller (local BA is Optimizer.local_bundle_adjustment): results are
indices, points and status codes."""
from __future__ import annotations

import ctypes
import math

import numpy as np

from ._native import check, hip_lib, ptr
from .matcher import ORBmatcher
from .views import FeatureVector, View, flags

# status codes of a slot of the current keyframe: the statement that ended the match
NO_MATCH, ACCEPTED, RAY_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, ZERO_DIST, SCALE_RATIO = range(10)


class LocalMapping:
    """The arithmetic of LocalMapping (reference src/LocalMapping.cc) on device `device`."""

    def __init__(self, device: int = 0):
        self._lib = hip_lib()
        self.device = int(device)

    def compute_f12(self, KF1: View, KF2: View) -> np.ndarray:
        """ComputeF12 (LocalMapping.cc:474-491): (3, 3) float32 with x1^T F12 x2 = 0."""
        F = np.zeros((3, 3), np.float32)
        check(self._lib.orb_compute_f12(KF1.ref(), KF2.ref(), ptr(F)))
        return F

    def scene_median_depth(self, KF: View, mp_pos, has_mp, q: int = 2) -> float:
        """KeyFrame::ComputeSceneMedianDepth(q) (KeyFrame.cc:659-689): mp_pos (n, 3) world positions of
        the keyframe's slots, has_mp (n,) = the slot holds a MapPoint.  A keyframe without one is
        refused (-22), where the reference indexes an empty vector."""
        pos = np.ascontiguousarray(np.asarray(mp_pos, np.float32).reshape(-1, 3))
        has = flags(has_mp, KF.n)
        if len(pos) != KF.n:
            raise ValueError("mp_pos must have one row per keypoint")
        d = np.zeros(1, np.float32)
        check(self._lib.orb_scene_median_depth(KF.ref(), ptr(pos), ptr(has), int(q), ptr(d), self.device))
        return float(d[0])

    def triangulate(self, KF1: View, KF2: View, match12, mp_pos2=None, has_mp2=None) -> dict:
        """The neighbour-loop body for one pair past the matcher (LocalMapping.cc:256-265, 276-391):
        match12 (n1,) = idx2 or -1.  mp_pos2 / has_mp2 (KF2's MapPoints) feed the baseline gate; None: no
        gate.  Returns x3d (n1, 3), status (n1,) uint8 (the module's codes), cos_rays (n1,), n_new,
        new_idx1 / new_idx2 (n_new,) ascending idx1, skipped, median_depth."""
        n1 = KF1.n
        m12 = np.ascontiguousarray(np.asarray(match12, np.int32).reshape(-1))
        if len(m12) != n1:
            raise ValueError("match12 must have one entry per KF1 keypoint")
        pos = has = None
        if mp_pos2 is not None:
            pos = np.ascontiguousarray(np.asarray(mp_pos2, np.float32).reshape(-1, 3))
            has = flags(has_mp2, KF2.n)
            if len(pos) != KF2.n:
                raise ValueError("mp_pos2 must have one row per KF2 keypoint")
        m = max(n1, 1)
        x3d, status, cosr = np.zeros((m, 3), np.float32), np.zeros(m, np.uint8), np.zeros(m, np.float32)
        i1, i2 = np.full(m, -1, np.int32), np.full(m, -1, np.int32)
        s = np.zeros(2, np.int32)
        med = np.zeros(1, np.float32)
        check(self._lib.orb_create_new_map_points(KF1.ref(), KF2.ref(), ptr(m12), ptr(pos), ptr(has), ptr(x3d), ptr(status),
                                                  ptr(cosr), ptr(s[0:1]), ptr(i1), ptr(i2), ptr(s[1:2]), ptr(med),
                                                  self.device))
        n = int(s[0])
        return dict(x3d=x3d[:n1], status=status[:n1], cos_rays=cosr[:n1], n_new=n, new_idx1=i1[:n], new_idx2=i2[:n],
                    skipped=int(s[1]), median_depth=float(med[0]))

    def scene_median_depth_batch_device(self, d_counts, cap, d_pose, d_mp_pos, d_has_mp, q=2, d_depth=None, d_n=None,
                                        stream=None):
        """orb_scene_median_depth_batch_device on device tensors: one workgroup per keyframe of the batch."""
        import torch

        B = int(d_counts.shape[0])
        st = stream if stream is not None else torch.cuda.current_stream(d_counts.device)
        check(self._lib.orb_scene_median_depth_batch_device(ptr(d_counts), int(cap), B, ptr(d_pose), ptr(d_mp_pos),
                                                            ptr(d_has_mp), int(q), ptr(d_depth), ptr(d_n),
                                                            ctypes.c_void_p(st.cuda_stream)))
        return d_depth, d_n

    def create_new_map_points_batch_device(self, d_kps, d_counts, cap, d_pair_a, d_pair_b, d_match, d_pose,
                                           scale_factors, level_sigma2, K4, d_mp_pos=None, d_has_mp=None, out=None,
                                           stream=None) -> dict:
        """orb_create_new_map_points_batch_device: P pairs (d_pair_a[p] = current keyframe, d_pair_b[p] =
        neighbour) of a device-resident batch, one workgroup per pair, asynchronous on `stream`.

        The match rows (d_match, P x cap) are taken as given, and deliberately so: the reference's
        neighbour loop is sequential, a slot of the current keyframe that neighbour i filled is has_mp1 for
        neighbour i + 1, so the rows of one current keyframe cannot come from a single matching batch
        without that dependence.  Rows of different current keyframes, or rows the caller has made with
        the dependence respected, batch freely.

        out: a dict of preallocated device tensors (any subset of x3d, status, cos_rays, n_new, new_idx1,
        new_idx2, skipped, median_depth, F12); missing ones are allocated.  d_mp_pos / d_has_mp: the
        baseline gate's inputs (B x cap x 3, B x cap) or None."""
        import torch

        P = int(d_pair_a.shape[0])
        dev = d_kps.device
        sf = np.ascontiguousarray(scale_factors, np.float32)
        s2 = np.ascontiguousarray(level_sigma2, np.float32)
        K = np.ascontiguousarray(K4, np.float32)
        if len(sf) != len(s2) or len(K) != 4:
            raise ValueError("scale_factors and level_sigma2 hold nlevels floats each, K4 four")
        shapes = dict(x3d=((P, cap, 3), torch.float32), status=((P, cap), torch.uint8),
                      cos_rays=((P, cap), torch.float32), n_new=((P,), torch.int32), new_idx1=((P, cap), torch.int32),
                      new_idx2=((P, cap), torch.int32), skipped=((P,), torch.int32),
                      median_depth=((P,), torch.float32), F12=((P, 3, 3), torch.float32))
        o = dict(out or {})
        for k, (shape, dt) in shapes.items():
            if k not in o:
                o[k] = torch.full(shape, float("nan"), dtype=dt, device=dev) if k == "median_depth" else \
                    torch.zeros(shape, dtype=dt, device=dev)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        check(self._lib.orb_create_new_map_points_batch_device(
            ptr(d_kps), ptr(d_counts), int(cap), P, ptr(d_pair_a), ptr(d_pair_b), ptr(d_match), ptr(d_pose),
            ptr(d_mp_pos), ptr(d_has_mp), ptr(sf), ptr(s2), len(sf), ptr(K), ptr(o["x3d"]), ptr(o["status"]),
            ptr(o["cos_rays"]), ptr(o["n_new"]), ptr(o["new_idx1"]), ptr(o["new_idx2"]), ptr(o["skipped"]),
            ptr(o["median_depth"]), ptr(o["F12"]), ctypes.c_void_p(st.cuda_stream)))
        return o

    def baseline_gate(self, cur: View, KF2: View, mp_pos2, has_mp2):
        """The gate in front of the matcher (LocalMapping.cc:258-265) alone: one median call on the
        device, then three scalars on the host with the reference's types (the baseline is cv::norm's
        double narrowed to float, the ratio a float quotient compared with the double 0.01).  Returns
        (skipped, median_depth): 0 go on, 1 short baseline, 2 KF2 holds no MapPoint (median NaN)."""
        has = flags(has_mp2, KF2.n)
        if not has.any():
            return 2, float("nan")
        median = np.float32(self.scene_median_depth(KF2, mp_pos2, has, 2))
        vb = KF2.Ow.astype(np.float32) - cur.Ow.astype(np.float32)
        s = 0.0
        for v in vb:
            s += float(v) * float(v)
        baseline = np.float32(math.sqrt(s))
        with np.errstate(all="ignore"):
            ratio = baseline / median
        return (1 if float(ratio) < 0.01 else 0), float(median)

    def create_new_map_points(self, cur: View, cur_fv: FeatureVector, cur_has_mp, neighbours, nnratio: float = 0.6):
        """The neighbour loop of CreateNewMapPoints (LocalMapping.cc:252-392) for the current keyframe
        `cur` (has_mp (n,) on entry; a copy is updated as the loop fills slots).  neighbours: a list of
        (View, FeatureVector, mp_pos (n2, 3), has_mp (n2,)) in the order of GetBestCovisibilityKeyFrames.
        Per neighbour: the baseline gate, compute_f12, ORBmatcher(0.6, False).SearchForTriangulation,
        triangulate.  Returns a list of dicts, one per neighbour, as triangulate() gives them plus match12
        and F12 (None for a skipped neighbour), and the final has_mp of `cur`.  The neighbour's own has_mp
        is the caller's to update between calls (its slot new_idx2 holds the new point afterwards).
        A neighbour that holds no MapPoint, where the reference indexes an empty vector, is reported
        skipped = 2 with a NaN median, as the batch form does, and the loop goes on."""
        has1 = flags(cur_has_mp, cur.n).copy()
        matcher = ORBmatcher(nnratio, False)
        results = []
        for KF2, fv2, pos2, has2 in neighbours:
            has2 = flags(has2, KF2.n)
            skipped, median = self.baseline_gate(cur, KF2, pos2, has2)
            if skipped:
                n1 = cur.n
                results.append(dict(x3d=np.zeros((n1, 3), np.float32), status=np.zeros(n1, np.uint8),
                                    cos_rays=np.full(n1, np.nan, np.float32), n_new=0,
                                    new_idx1=np.zeros(0, np.int32), new_idx2=np.zeros(0, np.int32), skipped=skipped,
                                    median_depth=median, match12=None, F12=None))
                continue
            F12 = self.compute_f12(cur, KF2)
            _, m12 = matcher.SearchForTriangulation(cur, has1, cur_fv, KF2, has2, fv2, F12, self.device)
            r = self.triangulate(cur, KF2, m12)
            r.update(match12=m12, F12=F12, median_depth=median)
            has1[r["new_idx1"]] = 1  # mpCurrentKeyFrame->AddMapPoint(pMP, idx1)
            results.append(r)
        return results, has1
