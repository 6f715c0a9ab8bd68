"""TEST INFRASTRUCTURE: seeded keyframe pairs for the CreateNewMapPoints tests.  A pair is two
orbslam_jpminipc_amd.views.View with known world points behind some of their keypoints and a match12 row as
SearchForTriangulation would leave it; the second keyframe's keypoints are permuted, so a match's ordinal, idx1
and idx2 all differ.  Pixels are projected in float64 and may lie outside the image: CreateNewMapPoints has no
image-bounds test."""
from __future__ import annotations

import numpy as np

from orbslam_jpminipc_amd import KEYPOINT_DTYPE
from orbslam_jpminipc_amd.views import View, frame_scale_tables

W, H = 640, 480
CALIB = (520.9, 521.0, 325.1, 249.7)
NLEVELS = 8
SF, SIGMA2 = frame_scale_tables(NLEVELS, 1.2)


def rot(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose_at(R, centre):
    """(Rcw, tcw) of a camera with rotation Rcw at world position `centre`."""
    R = np.asarray(R, np.float64)
    return R, -R @ np.asarray(centre, np.float64)


R1, T1 = pose_at(rot([0.2, 1.0, 0.1], 0.05), [0.1, -0.05, 0.2])


def project(R, t, X):
    """Pixels of world points X (m, 3) and their depths, in float64; a negative depth projects too."""
    Xc = np.asarray(X, np.float64) @ R.T + t
    return np.stack([CALIB[0] * Xc[:, 0] / Xc[:, 2] + CALIB[2], CALIB[1] * Xc[:, 1] / Xc[:, 2] + CALIB[3]], 1), Xc[:, 2]


def world_of(R, t, uvz):
    """World points at pixel (u, v) and depth z of camera (R, t)."""
    uvz = np.asarray(uvz, np.float64)
    Xc = np.stack([(uvz[:, 0] - CALIB[2]) / CALIB[0] * uvz[:, 2], (uvz[:, 1] - CALIB[3]) / CALIB[1] * uvz[:, 2], uvz[:, 2]], 1)
    return (Xc - t) @ R


def make_pair(seed, n1, n2, X, oct1, oct2, R2, t2, noise=0.0, off1=None, off2=None, calib2=None):
    """Keyframes of n1 and n2 keypoints; world point X[k] is seen by keypoint idx1[k] of the first (octave
    oct1[k], pixel offset off1[k]) and idx2[k] of the second.  Returns a dict: V1, V2, match12, idx1, idx2
    (idx1 ascending: k is the match ordinal), X."""
    rng = np.random.default_rng(seed)
    m = len(X)
    assert m <= min(n1, n2)
    idx1 = np.sort(rng.choice(n1, m, replace=False))
    idx2 = rng.permutation(n2)[:m]
    views = []
    for n, idx, octs, (R, t), off in ((n1, idx1, oct1, (R1, T1), off1), (n2, idx2, oct2, (R2, t2), off2)):
        k = np.zeros(n, KEYPOINT_DTYPE)
        k["x"], k["y"] = rng.uniform(0, W - 1, n), rng.uniform(0, H - 1, n)
        k["octave"] = rng.integers(0, NLEVELS, n)
        if m:
            uv, _ = project(R, t, X)
            uv = uv + rng.normal(0, noise, (m, 2)) + (0 if off is None else np.asarray(off, np.float64))
            k["x"][idx], k["y"][idx] = uv[:, 0], uv[:, 1]
            k["octave"][idx] = octs
        k["size"] = 31 * SF[k["octave"]]
        k["angle"] = rng.uniform(0, 360, n)
        k["response"] = rng.integers(1, 100, n)
        k["class_id"] = -1
        views.append(View(k, rng.integers(0, 256, (n, 32), dtype=np.uint8), (0, W, 0, H), NLEVELS, 1.2,
                          CALIB if calib2 is None or len(views) == 0 else calib2, R, t))
    match12 = np.full(n1, -1, np.int32)
    match12[idx1] = idx2
    return dict(V1=views[0], V2=views[1], match12=match12, idx1=idx1, idx2=idx2, X=np.asarray(X, np.float64))


def sideways(baseline=0.5):
    """The neighbour `baseline` to the right of the first camera, turned a little."""
    c1 = -R1.T @ T1
    return pose_at(rot([0.1, 1.0, 0.0], -0.04) @ R1, c1 + R1.T @ np.array([baseline, 0.03 * baseline, 0.05 * baseline]))


def accept_scene(m=130, n1=147, n2=139, seed=11, noise=0.3, baseline=0.5):
    """m matches of points 3 to 8 deep in front of both cameras, equal octaves: nearly all accepted."""
    rng = np.random.default_rng(seed + 1000)
    R2, t2 = sideways(baseline)
    X = world_of(R1, T1, np.stack([rng.uniform(40, W - 40, m), rng.uniform(40, H - 40, m), rng.uniform(3, 8, m)], 1))
    octs = rng.integers(0, 5, m)
    return make_pair(seed, n1, n2, X, octs, octs, R2, t2, noise)


def gates_scene(seed=23):
    """A neighbour 3 m ahead of the first camera and a little to the side, so that a point between the two
    is in front of one and behind the other.  Groups, in order of the match ordinal mixed by idx1: 40 good
    points, then 6 each meant for the ray-parallax gate (very far), z1 <= 0 (behind both), z2 <= 0 (between
    the cameras), the reprojection gate of KF1 (a 14 px offset across the epipolar line at octave 0), that
    of KF2 (an 8 px offset, KF1's keypoint at octave 6 and KF2's at 0) and the scale ratio (octaves 7 and
    0).  `kind` names the intended group of each match; the model decides what each really is."""
    rng = np.random.default_rng(seed + 1000)
    c1 = -R1.T @ T1
    R2, t2 = pose_at(rot([0.0, 1.0, 0.2], 0.03) @ R1, c1 + R1.T @ np.array([0.35, 0.1, 3.0]))

    def cam1(x, y, z):
        return (np.stack([x, y, z], 1) - T1) @ R1

    good = cam1(rng.uniform(-4, 4, 40), rng.uniform(-3, 3, 40), rng.uniform(7, 12, 40))
    far = cam1(rng.uniform(-50, 50, 6), rng.uniform(-50, 50, 6), rng.uniform(2000, 4000, 6))
    behind = cam1(rng.uniform(-2, 2, 6), rng.uniform(-2, 2, 6), rng.uniform(-6, -3, 6))
    between = cam1(rng.uniform(0.8, 1.5, 6) * rng.choice([-1, 1], 6), rng.uniform(-0.5, 0.5, 6), rng.uniform(1.2, 2.2, 6))
    rep = cam1(rng.uniform(-4, 4, 18), rng.uniform(-3, 3, 18), rng.uniform(7, 12, 18))
    X = np.concatenate([good, far, behind, between, rep])
    kind = np.repeat([1, 2, 4, 5, 6, 7, 9], [40, 6, 6, 6, 6, 6, 6])
    m = len(X)
    o1 = rng.integers(0, 4, m)
    o2 = o1.copy()
    off1, off2 = np.zeros((m, 2)), np.zeros((m, 2))
    # across the epipolar line: the epipole of a forward motion is near the image centre, so "across" is
    # the tangent of the circle around it
    uv, _ = project(R1, T1, X)
    tang = np.stack([-(uv[:, 1] - CALIB[3]), uv[:, 0] - CALIB[2]], 1)
    tang /= np.linalg.norm(tang, axis=1)[:, None]
    o1[kind == 6], o2[kind == 6] = 0, 0
    off1[kind == 6] = 14.0 * tang[kind == 6]
    o1[kind == 7], o2[kind == 7] = 6, 0
    off1[kind == 7] = 8.0 * tang[kind == 7]
    o1[kind == 9], o2[kind == 9] = 7, 0
    s = make_pair(seed, 147, 139, X, o1, o2, R2, t2, 0.2, off1, off2)
    s["kind"] = kind
    return s


def map_points_of(V, seed, depth=5.0, frac=0.6):
    """mp_pos (n, 3) and has_mp (n,) for a keyframe: a share of its slots hold a MapPoint about `depth` deep."""
    rng = np.random.default_rng(seed)
    n = V.n
    R, t = V.Rcw.astype(np.float64), V.tcw.astype(np.float64)
    z = depth * rng.uniform(0.6, 1.6, n)
    pos = world_of(R, t, np.stack([V.kps["x"].astype(np.float64), V.kps["y"].astype(np.float64), z], 1)).astype(np.float32)
    has = (rng.random(n) < frac).astype(np.uint8)
    if n and not has.any():
        has[0] = 1
    return pos, has
