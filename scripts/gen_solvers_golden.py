#!/usr/bin/env python3
"""Writes tests/golden/solvers_320x240.npz: a PnP and a Sim3 consensus problem on the committed
frame pair (scene_320x240_nf500 / _f1 with the matches of match_320x240_f0_f1) and the CPU
model's answers for them (tests/solvers_model.py).

The scene is made up around the real keypoints and matches: every matched keypoint of frame 0 gets
a depth under a fixed seed and is a MapPoint; frame 1 sits at a chosen pose (PnP), and the two
frames' camera coordinates are related by a chosen similarity (Sim3).  The hypotheses are that pose
/ similarity perturbed by growing amounts.  All of it is only data: the file stores the compact
solver inputs, the hypotheses and the model's counts, masks, best_at and first indices.

The fixture must make the float pattern visible, so the data is then tuned at the decision
boundary, and the script refuses to write unless, for each model, at least 8 (hypothesis,
correspondence) flags differ between the true pattern and the model's `plain` variant (no fused
operation), and for Sim3 at least 8 more between the truncated and the untruncated bound:
  PnP   for 16 correspondences, one hypothesis each, sigma2 is chosen so that sigma2 * th2 lands
        between the error2 of the two variants (sigma2 is per correspondence in the solver);
        and 4 more correspondences, each with a hypothesis of its own, are built so that the first
        row sum lands on a float rounding tie exactly when its products are rounded one by one
        (row_visible_points): the narrowing to float hides the row's fused operations everywhere
        else, about 2^-29 of all values apart;
  Sim3  the bound is an integer, so the boundary is scanned: for every (hypothesis,
        correspondence) the depth of the first camera's point is bisected to the adjacent float
        pair where the flag flips, and a correspondence is moved there when the two variants
        disagree at one of the pair; likewise to the 9.21 * sigma2 boundary of the untruncated
        variant.  The script prints how many boundary points it looked at.
"""
import pathlib
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import solvers_model as model  # noqa: E402

GOLD = ROOT / "tests" / "golden"
SEED = 20240702
N_HYP = 96
K = np.array([260.0, 260.0, 160.0, 120.0], np.float32)  # fx, fy, cx, cy of the 320x240 frames
TH2 = np.float32(5.991)
PNP_MIN, SIM3_MIN = 10, 20
NEED = 8
f32 = np.float32


def hypotheses(rng, R0, t0, s0):
    R = np.zeros((N_HYP, 3, 3))
    t = np.zeros((N_HYP, 3))
    s = np.zeros(N_HYP)
    for h in range(N_HYP):
        e = 0.0015 * (h % 13)
        R[h] = model.rodrigues(rng.normal(0, e + 1e-4, 3)) @ R0
        t[h] = t0 + rng.normal(0, 2 * e + 1e-4, 3)
        s[h] = s0 * (1 + rng.normal(0, e + 1e-4))
    return R, t, s


def tune_pnp(p3d, p2d, sigma2, R, t):
    """sigma2 of 16 correspondences moved so that the bound separates the two variants' error2."""
    args = (p3d, p2d, sigma2, TH2, K, R, t, PNP_MIN)
    e_true = model.pnp(*args, errors=True)["err"]
    e_plain = model.pnp(*args, variant=model.PLAIN, errors=True)["err"]
    sigma2 = sigma2.copy()
    done = 0
    for i in range(len(p3d)):
        if done == 16:
            break
        for h in np.flatnonzero(e_true[:, i] != e_plain[:, i]):
            hi = max(e_true[h, i], e_plain[h, i])
            # a float sigma2 whose float product with th2 is exactly the larger error: lo < bound <= hi
            s = f32(hi / TH2)
            cand = [c for c in (s, np.nextafter(s, f32(0)), np.nextafter(s, f32(np.inf))) if f32(c * TH2) == hi]
            if cand and 0.25 < cand[0] < 64:
                sigma2[i] = cand[0]
                done += 1
                break
    return sigma2


def row_visible_points(count):
    """(X, r) pairs, X a float and r a double: with the row (r * 2^-24, 1, 0) and the point (X, 1, Z)
    the exact product r * X is 1 + 2^-29 + e with 0 < e < 2^-53.  Fused, 1 + 2^-24 * (r * X) rounds
    above the tie between the floats 1 and 1 + 2^-23; with the product rounded first, e is lost, the
    double sum is the tie itself and the float is 1."""
    from fractions import Fraction

    T, out = 1 + Fraction(1, 2 ** 29), []
    for m in range(1, 4000):
        X = 1 + Fraction(m, 2 ** 23)
        r = float(T / X)
        for r in (np.nextafter(r, 0), r, np.nextafter(r, 2)):
            if T < Fraction(float(r)) * X < T + Fraction(1, 2 ** 53):
                out.append((float(X), float(r)))
                break
        if len(out) == count:
            return out
    sys.exit("no row-visible points found")


def scan_sim3(c, variant_a, variant_b, taken, want):
    """Bisects x3dc1[:, 2] of every free correspondence, per hypothesis, to the adjacent float pair
    where `variant_a`'s flag flips; moves a correspondence to a point of the pair where variant_b's
    flag differs from variant_a's.  Returns (moved, boundary points looked at)."""
    n = len(c["x3dc1"])
    moved = looked = 0

    def flags(z, h, variant):
        x1 = c["x3dc1"].copy()
        x1[:, 2] = z
        return model.sim3(x1, c["x3dc2"], c["sigma2_1"], c["sigma2_2"], K, K, c["T12"][h:h + 1], c["T21"][h:h + 1],
                          SIM3_MIN, variant=variant)["inliers"][0]

    for h in range(N_HYP):
        if moved >= want:
            break
        lo = c["x3dc1"][:, 2].copy()
        hi = (lo * f32(1.6)).astype(f32)
        ok = flags(lo, h, variant_a) & ~flags(hi, h, variant_a) & ~taken
        lo_i, hi_i = lo.view(np.int32).copy(), hi.view(np.int32).copy()
        while np.any(ok & (hi_i - lo_i > 1)):
            mid = lo_i + (hi_i - lo_i) // 2
            inside = flags(mid.view(f32), h, variant_a)
            lo_i = np.where(inside, mid, lo_i)
            hi_i = np.where(inside, hi_i, mid)
        looked += int(ok.sum())
        for z_i in (lo_i, hi_i):
            z = z_i.view(f32)
            differ = ok & (flags(z, h, variant_a) != flags(z, h, variant_b)) & ~taken
            for i in np.flatnonzero(differ):
                if moved < want:
                    c["x3dc1"][i, 2] = z[i]
                    taken[i] = True
                    moved += 1
    return moved, looked


def main():
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE

    k1 = np.ascontiguousarray(np.load(GOLD / "scene_320x240_nf500.npz")["kps"]).view(KEYPOINT_DTYPE).reshape(-1)
    k2 = np.ascontiguousarray(np.load(GOLD / "scene_320x240_nf500_f1.npz")["kps"]).view(KEYPOINT_DTYPE).reshape(-1)
    m12 = np.load(GOLD / "match_320x240_f0_f1.npz")["m12"]
    i1 = np.flatnonzero(m12 >= 0)
    i2 = m12[i1]
    n = len(i1)
    rng = np.random.default_rng(SEED)
    ls2 = model.LEVEL_SIGMA2

    # ---- PnP: frame 0's matched keypoints are MapPoints (world = camera 0), frame 1 is at (Rt, tt)
    Rt, tt = model.rodrigues(rng.normal(0, 0.05, 3)), rng.normal(0, 0.1, 3)
    depth = rng.uniform(2, 8, n)
    x2 = np.stack([k2["x"][i2], k2["y"][i2]], 1).astype(np.float64)
    Pc = np.stack([(x2[:, 0] - K[2]) / K[0] * depth, (x2[:, 1] - K[3]) / K[1] * depth, depth], 1)
    Pw = (Pc - tt) @ Rt
    order = np.argsort(i2)  # the solver lists the frame's keypoints in ascending order
    p3d = Pw[order].astype(f32)
    p2d = x2[order].astype(f32)
    pnp_sigma2 = ls2[k2["octave"][i2][order]].astype(f32)
    R, t, _ = hypotheses(rng, Rt, tt, 1.0)
    pnp_sigma2 = tune_pnp(p3d, p2d, pnp_sigma2, R, t)
    # the row-visible correspondences and their hypotheses: Xc is 1 + 2^-23 (fused) or 1, Yc .5, Zc 2;
    # ue = 130 * Xc + 160, measured 1.25 px to its right; the bound sits between the two error2
    for X, r in row_visible_points(4):
        Rv = np.array([[r * 2.0 ** -24, 1, 0], [0, 0.5, 0], [0, 0, 1]])
        R, t = np.concatenate([R, Rv[None]]), np.concatenate([t, np.zeros((1, 3))])
        p3d = np.concatenate([p3d, f32([[X, 1, 2]])])
        p2d = np.concatenate([p2d, f32([[291.25, 185]])])
        pnp_sigma2 = np.concatenate([pnp_sigma2, f32([1.56248 / 5.991])])
    pa = (p3d, p2d, pnp_sigma2, TH2, K, R, t, PNP_MIN)
    rp = model.pnp(*pa)
    d_pnp = int((rp["inliers"] != model.pnp(*pa, variant=model.PLAIN)["inliers"]).sum())
    d_row = int((rp["inliers"] != model.pnp(*pa, variant=model.ROW_PLAIN)["inliers"]).sum())
    print(f"pnp: n {len(p3d)}, counts {rp['counts'].min()}..{rp['counts'].max()}, first_ok {rp['first_ok']}, "
          f"{d_pnp} flags differ under the plain variant, {d_row} with only the row sums unfused")
    if d_row < 4:
        sys.exit("refusing to write: the PnP row sums' fused operations would be invisible")

    # ---- Sim3: camera-1 points from frame 0's keypoints, camera-2 points through a similarity
    R12, t12, s12 = model.rodrigues(rng.normal(0, 0.1, 3)), rng.normal(0, 0.2, 3), 1.1
    x1 = np.stack([k1["x"][i1], k1["y"][i1]], 1).astype(np.float64)
    d1 = rng.uniform(2, 8, n)
    X1 = np.stack([(x1[:, 0] - K[2]) / K[0] * d1, (x1[:, 1] - K[3]) / K[1] * d1, d1], 1)
    X2 = ((X1 - t12) @ R12) / s12 + rng.normal(0, 0.004, (n, 3))
    Rh, th, sh = hypotheses(rng, R12, t12, s12)
    T12 = np.zeros((N_HYP, 3, 4), f32)
    T21 = np.zeros((N_HYP, 3, 4), f32)
    for h in range(N_HYP):
        T12[h, :, :3], T12[h, :, 3] = sh[h] * Rh[h], th[h]
        T21[h, :, :3], T21[h, :, 3] = Rh[h].T / sh[h], -(Rh[h].T / sh[h]) @ th[h]
    c = {"x3dc1": X1.astype(f32), "x3dc2": X2.astype(f32), "sigma2_1": ls2[k1["octave"][i1]].astype(f32),
         "sigma2_2": ls2[k2["octave"][i2]].astype(f32), "T12": T12, "T21": T21}
    taken = np.zeros(n, bool)
    m_plain, looked = scan_sim3(c, 0, model.PLAIN, taken, 14)
    m_bound, looked_b = scan_sim3(c, model.UNTRUNCATED, 0, taken, 14)
    sa = (c["x3dc1"], c["x3dc2"], c["sigma2_1"], c["sigma2_2"], K, K, T12, T21, SIM3_MIN)
    rs = model.sim3(*sa)
    d_plain = int((rs["inliers"] != model.sim3(*sa, variant=model.PLAIN)["inliers"]).sum())
    d_bound = int((rs["inliers"] != model.sim3(*sa, variant=model.UNTRUNCATED)["inliers"]).sum())
    print(f"sim3: n {n}, counts {rs['counts'].min()}..{rs['counts'].max()}, first_accept {rs['first_accept']}; "
          f"{looked} boundary points scanned, {m_plain} correspondences moved, {d_plain} flags differ under the "
          f"plain variant; {looked_b} scanned for the bound, {m_bound} moved, {d_bound} differ untruncated")
    if d_pnp < NEED or d_plain < NEED or d_bound < NEED:
        sys.exit("refusing to write: the fixture would not show the float pattern (change SEED or N_HYP)")
    np.savez_compressed(
        GOLD / "solvers_320x240.npz", K=K, th2=TH2, pnp_min=np.int32(PNP_MIN), sim3_min=np.int32(SIM3_MIN),
        index1=i1.astype(np.int32), index2=i2[order].astype(np.int32),
        p3d=p3d, p2d=p2d, pnp_sigma2=pnp_sigma2, R=R.reshape(-1, 9), t=t,
        pnp_counts=rp["counts"], pnp_masks=rp["masks"], pnp_best_at=rp["best_at"], pnp_first_ok=np.int32(rp["first_ok"]),
        x3dc1=c["x3dc1"], x3dc2=c["x3dc2"], sigma2_1=c["sigma2_1"], sigma2_2=c["sigma2_2"],
        T12=T12.reshape(N_HYP, 12), T21=T21.reshape(N_HYP, 12),
        sim3_counts=rs["counts"], sim3_masks=rs["masks"], sim3_best_at=rs["best_at"],
        sim3_first_accept=np.int32(rs["first_accept"]))
    print("wrote", GOLD / "solvers_320x240.npz")


if __name__ == "__main__":
    main()
