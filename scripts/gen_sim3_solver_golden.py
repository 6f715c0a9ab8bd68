#!/usr/bin/env python3
"""Writes tests/golden/sim3_solver_320x240.npz: one Sim3Solver::iterate of 300 iterations on a
synthetic 320x240 two-view cloud, with the CPU model's answer (tests/native/sim3_solver_model.cpp,
tests/native/solvers_model.cpp) and the tolerances that tests/test_gpu_sim3_solver.py applies.

  tol_T12 / tol_T21 / tol_sim3  4 x the largest deviation of the model's outputs among its 26
                                variants that move the results of atan2, cos and sin by one ulp
  margin_px                     2 x that tolerance propagated to pixels at the cloud's depth range

It refuses to write when a consensus error of any hypothesis lies closer to its bound than the
margin (or changes sides under a libm variant), when fewer than 8 of the sets hold an index twice,
or when fewer than 8 would differ under a sampler that removes by position: counts and masks must
be exact on the GPU, and the reference's removal quirk must show in the fixture.
"""
import argparse
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import sim3_solver_model as s3  # noqa: E402

K = np.float32([260, 260, 160, 120])
N, N_HYP, MIN_INLIERS, N_QUIRK = 200, 300, 20, 12


def r_for(randi, size):
    return (randi * 2 ** 31 + 2 ** 30) // size


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "sim3_solver_320x240.npz"))
    a = ap.parse_args()
    c = s3.cloud(N, seed=a.seed, scale=1.7, angle=0.4, noise=0.01, outliers=0.3)
    x1, x2, g1, g2 = c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"]
    rng = np.random.default_rng(1000 + a.seed)
    rand31 = rng.integers(0, 2 ** 31, (N_HYP, 3))
    rand31[0], rand31[1] = 0, 2 ** 31 - 1
    # random draws at N = 200 all but never land on an overwritten entry; these do: the second and
    # third draw hit the position of the first, which gives (i0, N - 1, N - 1)
    for k in range(N_QUIRK):
        h, i0 = 10 + 23 * k, int(rng.integers(0, N - 3))
        rand31[h] = [r_for(i0, N), r_for(i0, N - 1), r_for(i0, N - 2)]
    want = s3.iterate(x1, x2, g1, g2, K, K, rand31, MIN_INLIERS, errors=True)
    sets = want["sets"]
    repeated = sum(len(set(s)) < 3 for s in sets.tolist())
    differ = int((s3.sets(N, rand31, s3.FIXED_SAMPLER) != sets).any(1).sum())
    print(f"sets with a repeated index: {repeated}; sets that differ under the fixed sampler: {differ}")
    if repeated < 8 or differ < 8:
        sys.exit("refused: the removal quirk does not show in the sets")
    # the tolerance: the libm variants
    tol = {"T12": 0.0, "T21": 0.0, "sim3": 0.0}
    b1 = np.float32(np.floor(9.210 * g1.astype(np.float64)))
    b2 = np.float32(np.floor(9.210 * g2.astype(np.float64)))
    in0 = (want["err1"] < b1) & (want["err2"] < b2)
    assert np.array_equal(in0, want["inliers"])
    for v in s3.LIBM_VARIANTS:
        m = s3.iterate(x1, x2, g1, g2, K, K, rand31, MIN_INLIERS, variant=v, errors=True)
        for k in tol:
            if not np.array_equal(np.isnan(m[k]), np.isnan(want[k])):
                sys.exit("refused: a libm variant moves a NaN")
            with np.errstate(invalid="ignore"):
                d = np.abs(m[k].astype(np.float64) - want[k].astype(np.float64))
            tol[k] = max(tol[k], float(np.nanmax(d)))
        if not np.array_equal(m["inliers"], want["inliers"]):
            sys.exit(f"refused: an error changes sides under libm variant {v}")
    measured = dict(tol)
    tol = {k: 4 * v for k, v in tol.items()}
    # propagated to pixels: P = sR X + t moves by 3 tol |X| + tol, its image by fx (dP / Z)(1 + |X| / Z)
    xmax = float(max(np.abs(x1).max(), np.abs(x2).max()))
    zmin = float(min(x1[:, 2].min(), x2[:, 2].min()))
    tmax = max(tol["T12"], tol["T21"])
    margin_px = 2 * float(K[0]) * (3 * tmax * xmax + tmax) / zmin * (1 + xmax / zmin)
    print(f"measured deviation {measured}; tolerance {tol}; depth >= {zmin:.3f}, |X| <= {xmax:.3f}; "
          f"margin {margin_px:.3e} px")
    with np.errstate(invalid="ignore"):
        gap1 = np.abs(np.sqrt(want["err1"].astype(np.float64)) - np.sqrt(b1.astype(np.float64)))
        gap2 = np.abs(np.sqrt(want["err2"].astype(np.float64)) - np.sqrt(b2.astype(np.float64)))
    closest = float(min(np.nanmin(gap1), np.nanmin(gap2)))
    print(f"closest error to its bound: {closest:.3e} px")
    if not closest >= margin_px:
        sys.exit("refused: a consensus error lies inside the margin of its bound; try another --seed")
    print(f"counts: max {want['counts'].max()}, first_accept {want['first_accept']}, NaN hypotheses "
          f"{int(np.isnan(want['sim3']).any(1).sum())}")
    np.savez_compressed(
        a.out, K=K, min_inliers=np.int32(MIN_INLIERS), x3dc1=x1, x3dc2=x2, sigma2_1=g1, sigma2_2=g2,
        rand31=rand31.astype(np.int32), sets=sets, T12=want["T12"], T21=want["T21"], sim3=want["sim3"],
        quat=want["quat"], counts=want["counts"], masks=want["masks"], best_at=want["best_at"],
        first_accept=np.int32(want["first_accept"]), accepted=want["accepted"],
        tol_T12=np.float64(tol["T12"]), tol_T21=np.float64(tol["T21"]), tol_sim3=np.float64(tol["sim3"]),
        measured_T12=np.float64(measured["T12"]), measured_T21=np.float64(measured["T21"]),
        measured_sim3=np.float64(measured["sim3"]), margin_px=np.float64(margin_px), closest_px=np.float64(closest))
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
