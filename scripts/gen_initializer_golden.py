#!/usr/bin/env python3
"""Writes tests/golden/initializer_320x240.npz: 200 homography and 200 fundamental-matrix
hypotheses for the committed frame pair (scene_320x240_nf500 / _f1 with the matches of
match_320x240_f0_f1) and the CPU model's answer for them (tests/initializer_model.py).

The hypotheses follow Initializer::FindHomography / FindFundamental (reference
src/Initializer.cc:122-221) in numpy float32 (Normalize, an 8-match minimal set, the DLT by SVD,
T2inv*Hn*T1 and its inverse, T2t*Fn*T1) under a fixed seed.  They are only data: the file stores
them, and nothing depends on numpy's SVD giving the same bits elsewhere.

The script refuses a seed for which a pairwise float32 sum of the model's terms equals the
sequential sum for every hypothesis of a kind: with such data a GPU test could not tell a wrong
summation order from the right one.
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import initializer_model as model  # noqa: E402

GOLD = ROOT / "tests" / "golden"
SEED = 20240611
N_HYP = 200
SIGMA = 1.0
f32 = np.float32


def normalize(pts):
    """Initializer::Normalize (Initializer.cc:747-794): zero mean, unit mean absolute deviation."""
    mean = pts.mean(0, dtype=f32)
    d = pts - mean
    s = f32(1.0) / np.abs(d).mean(0, dtype=f32)
    T = np.array([[s[0], 0, -mean[0] * s[0]], [0, s[1], -mean[1] * s[1]], [0, 0, 1]], f32)
    return (d * s).astype(f32), T


def compute_h21(p1, p2):
    A = np.zeros((16, 9), f32)
    for i, ((u1, v1), (u2, v2)) in enumerate(zip(p1, p2)):
        A[2 * i] = [0, 0, 0, -u1, -v1, -1, v2 * u1, v2 * v1, v2]
        A[2 * i + 1] = [u1, v1, 1, 0, 0, 0, -u2 * u1, -u2 * v1, -u2]
    return np.linalg.svd(A)[2][8].reshape(3, 3).astype(f32)


def compute_f21(p1, p2):
    A = np.zeros((8, 9), f32)
    for i, ((u1, v1), (u2, v2)) in enumerate(zip(p1, p2)):
        A[i] = [u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1]
    Fpre = np.linalg.svd(A)[2][8].reshape(3, 3).astype(f32)
    u, w, vt = np.linalg.svd(Fpre)
    w[2] = 0
    return (u @ np.diag(w) @ vt).astype(f32)


def pairwise_sum(t):
    t = np.asarray(t, f32)
    while len(t) > 1:
        if len(t) & 1:
            t = np.concatenate([t, np.zeros(1, f32)])
        t = (t[0::2] + t[1::2]).astype(f32)
    return t[0] if len(t) else f32(0)


def main():
    k1 = np.load(GOLD / "scene_320x240_nf500.npz")["kps"]
    k2 = np.load(GOLD / "scene_320x240_nf500_f1.npz")["kps"]
    m12 = np.load(GOLD / "match_320x240_f0_f1.npz")["m12"]
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE

    x1 = model.xy(np.ascontiguousarray(k1).view(KEYPOINT_DTYPE).reshape(-1))
    x2 = model.xy(np.ascontiguousarray(k2).view(KEYPOINT_DTYPE).reshape(-1))
    idx = np.flatnonzero(m12 >= 0)
    N = len(idx)
    assert N >= 8, N
    n1, T1 = normalize(x1)
    n2, T2 = normalize(x2)
    T2inv, T2t = np.linalg.inv(T2).astype(f32), T2.T.copy()
    rng = np.random.default_rng(SEED)
    H21 = np.zeros((N_HYP, 3, 3), f32)
    H12 = np.zeros_like(H21)
    F21 = np.zeros_like(H21)
    for it in range(N_HYP):
        pick = idx[rng.choice(N, 8, replace=False)]
        a, b = n1[pick], n2[m12[pick]]
        H21[it] = T2inv @ compute_h21(a, b) @ T1
        H12[it] = np.linalg.inv(H21[it]).astype(f32)
        F21[it] = T2t @ compute_f21(a, b) @ T1
    r = model.check(x1, x2, m12, SIGMA, H21, H12, F21, terms=True)
    assert r["n_matches"] == N
    for t in "hf":
        differ = sum(pairwise_sum(r["terms_" + t][h]).tobytes() != r["scores_" + t][h].tobytes() for h in range(N_HYP))
        print(f"{t}: best {r['best_' + t]} score {r['best_score_' + t]!r}, {int(r['inliers_' + t].sum())}/{N} inliers, "
              f"{differ}/{N_HYP} scores change under pairwise summation")
        assert differ >= 1, "change SEED: summation order would be untestable on this data"
        assert r["best_" + t] >= 0
    np.savez_compressed(
        GOLD / "initializer_320x240.npz", sigma=f32(SIGMA), H21=H21.reshape(N_HYP, 9), H12=H12.reshape(N_HYP, 9),
        F21=F21.reshape(N_HYP, 9), n_matches=np.int32(N), scores_h=r["scores_h"], scores_f=r["scores_f"],
        best_h=np.int32(r["best_h"]), best_f=np.int32(r["best_f"]), best_score_h=r["best_score_h"],
        best_score_f=r["best_score_f"], inliers_h=r["inliers_h"], inliers_f=r["inliers_f"])
    print("wrote", GOLD / "initializer_320x240.npz")


if __name__ == "__main__":
    main()
