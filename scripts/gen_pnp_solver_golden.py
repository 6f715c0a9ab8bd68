#!/usr/bin/env python3
"""Writes tests/golden/pnp_solver_320x240.npz: one PnPsolver::iterate of 300 iterations on the PnP
correspondences of the solvers fixture (tests/golden/solvers_320x240.npz), with the draws and the CPU
model's answer (tests/native/pnp_solver_model.cpp), and prints the tolerances that
tests/test_pnp_solver_model.py holds the model to:

  model against an independent numpy float64 EPnP (n >= 6 points in general position): the largest
  difference of R and of t seen, times 10 for unseen inputs;
  n = 4, noise-free non-coplanar sets: the largest deviation of R from an orthonormal matrix and of its
  determinant from +1, times 10; the median reprojection error, times 10.

It refuses to write when no Refine succeeds, or when fewer than 4 sets hold a correspondence twice (the
reference's removal quirk must show in the fixture)."""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import pnp_solver_model as pm  # noqa: E402

N_HYP, N_QUIRK = 300, 8
NUMPY_CASES, N4_CASES = 200, 300


def r_for(randi, size):
    return (randi * 2 ** 31 + 2 ** 30) // size


def measure():
    K = np.float64(np.float32(pm.K_CAM))
    dR = dt = 0.0
    for seed in range(NUMPY_CASES):
        p3, p2, _, _ = pm.scene(6 + seed % 40, seed)
        m = pm.compute_pose(p3, p2, K)
        Rn, tn = pm.numpy_epnp(p3, p2, K)
        dR, dt = max(dR, float(np.abs(m["R"] - Rn).max())), max(dt, float(np.abs(m["t"] - tn).max()))
    orth = det = 0.0
    reps = []
    for seed in range(N4_CASES):
        p3, p2, _, _ = pm.scene(4, 1000 + seed)
        m = pm.compute_pose(p3, p2, K)
        orth = max(orth, float(np.abs(m["R"] @ m["R"].T - np.eye(3)).max()))
        det = max(det, abs(float(np.linalg.det(m["R"])) - 1))
        reps.append(m["rep_error"])
    return {"numpy_dR": dR, "numpy_dt": dt, "n4_orth": orth, "n4_det": det, "n4_rep_median": float(np.median(reps)),
            "n4_rep_worst": float(np.max(reps))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=4)
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "pnp_solver_320x240.npz"))
    a = ap.parse_args()
    for k, v in measure().items():
        print(f"measured {k} = {v:.3e}   (x 10 = {10 * v:.3e})")
    g = np.load(ROOT / "tests" / "golden" / "solvers_320x240.npz")
    p3d, p2d, sigma2, K, th2 = g["p3d"], g["p2d"], g["pnp_sigma2"], g["K"], g["th2"]
    N, mi = len(p3d), int(g["pnp_min"])
    rng = np.random.default_rng(2000 + a.seed)
    rand31 = rng.integers(0, 2 ** 31, (N_HYP, 4))
    rand31[0], rand31[1] = 0, 2 ** 31 - 1
    # random draws all but never land on an overwritten entry; these do: the later draws hit the
    # position of the first, which gives (i0, N - 1, N - 1, ..)
    for k in range(N_QUIRK):
        h, i0 = 10 + 31 * k, int(rng.integers(0, N - 4))
        rand31[h] = [r_for(i0, N), r_for(i0, N - 1), r_for(i0, N - 2), rng.integers(0, 2 ** 31)]
    rand31 = rand31.astype(np.int32)
    want = pm.ransac(p3d, p2d, sigma2, th2, np.float64(K), mi, rand31=rand31)
    repeated = sum(len(set(s)) < 4 for s in want["sets"].tolist())
    print(f"N = {N}, min_inliers = {mi}: first_ok {want['first_ok']}, first_refined {want['first_refined']}, "
          f"pose_inliers {want['pose_inliers']}, Refine calls of the reference {want['refine_calls']}, "
          f"replacing iterations {int((want['best_at'] == np.arange(N_HYP)).sum())}, sets with a repeated index {repeated}")
    if want["first_refined"] < 0:
        sys.exit("refused: no Refine succeeds")
    if repeated < 4:
        sys.exit("refused: the removal quirk does not show in the sets")
    np.savez_compressed(a.out, p3d=p3d, p2d=p2d, sigma2=sigma2, K=K, th2=th2, min_inliers=np.int32(mi), rand31=rand31,
                        **{k: want[k] for k in ("counts", "masks", "best_at", "R", "t", "rep_error", "sets", "branches",
                                                "refined_counts", "pose", "pose_mask")},
                        **{k: np.int32(want[k]) for k in ("first_ok", "first_refined", "pose_inliers")})
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
