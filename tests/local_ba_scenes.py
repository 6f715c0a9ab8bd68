"""Synthetic local bundle adjustment windows for the tests of DESIGN.md §21: cameras on an arc that
look at a point cloud, 320x240 calibration, level-dependent pixel noise (sigma 0.5 px at level 0), a
share of gross outliers of 10 to 40 px, a few points behind one camera.  Every case carries the CPU
model's answer and is decisive: the model alone decides every flag (local_ba_model.decisive)."""
from __future__ import annotations

import numpy as np

import local_ba_model as lbm

K_DEFAULT = (np.float32(320.0), np.float32(318.5), np.float32(159.5), np.float32(119.25))
LEVEL_SIGMA2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2
RADIUS = 8.0  # the arc's radius = the scene's depth and scale
MAX_SEED_SKIPS = 20
MAX_FREE_KF = 64


def rot(w) -> np.ndarray:
    """Rodrigues' rotation matrix of the axis-angle vector w (float64)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * Wx @ Wx


def look_at(C) -> tuple:
    """Rcw, tcw of a camera at C that looks at the origin."""
    z = -C / np.linalg.norm(C)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    return R, -R @ C


def project(R, t, K, X):
    Xc = X @ R.T + t
    return np.stack([Xc[:, 0] / Xc[:, 2] * K[0] + K[2], Xc[:, 1] / Xc[:, 2] * K[1] + K[3]], 1), Xc[:, 2]


def build_scene(seed, n_free, n_fixed, n_pt, obs_per_pt, outliers=0.1, behind=0, noise=0.5, local_fixed=None,
                force_kf=None, perturb=1.0, K=K_DEFAULT) -> dict:
    """One window (no model run).  n_free local keyframes come first (`local_fixed`: the index of a
    further local keyframe that is fixed, the reference's mnId == 0), then n_fixed fixed ones.
    `force_kf`: a keyframe that point 0 observes."""
    rng = np.random.default_rng(seed)
    fixed = [0] * n_free
    if local_fixed is not None:
        fixed.insert(local_fixed, 1)
    fixed += [1] * n_fixed
    n_kf = len(fixed)
    ang = np.linspace(-0.6, 0.6, n_kf) + rng.normal(0, 0.01, n_kf) if n_kf > 1 else np.zeros(1)
    ang = rng.permutation(ang)
    Rs, ts = [], []
    for a in ang:
        C = np.array([RADIUS * np.sin(a), rng.normal(0, 0.3), -RADIUS * np.cos(a)])
        R, t = look_at(C)
        Rs.append(R), ts.append(t)
    X = rng.uniform(-1.5, 1.5, (n_pt, 3))
    for p in range(min(behind, n_pt)):  # behind camera 0 (a free one unless local_fixed == 0)
        X[p] = -Rs[0].T @ ts[0] - Rs[0][2] * rng.uniform(1.0, 3.0) + rng.normal(0, 0.2, 3)
    ept, ekf, obs, inv_s2, nobs = [], [], [], [], []
    for p in range(n_pt):
        m = min(obs_per_pt, n_kf)
        kfs = rng.choice(n_kf, m, replace=False)
        if p < behind and 0 not in kfs:
            kfs[0] = 0
        if p == 0 and force_kf is not None and force_kf not in kfs:
            kfs[-1] = force_kf
        for i in kfs:
            uv, _ = project(Rs[i], ts[i], K, X[p:p + 1])
            octave = int(rng.integers(0, 8))
            uv = uv[0] + rng.normal(0, noise, 2) * np.sqrt(float(LEVEL_SIGMA2[octave]))
            if rng.random() < outliers:
                d = rng.normal(0, 1, 2)
                uv = uv + d / np.linalg.norm(d) * rng.uniform(10, 40)
            ept.append(p), ekf.append(int(i)), obs.append(uv)
            inv_s2.append(np.float32(1.0) / LEVEL_SIGMA2[octave])
        nobs.append(m + (1 if rng.random() < 0.2 else 0))  # an observation in a bad keyframe has no edge
    pose = np.zeros((n_kf, 12))
    for i in range(n_kf):
        R, t = Rs[i], ts[i]
        if not fixed[i]:
            R = rot(rng.normal(0, 0.004 * perturb, 3)) @ R
            t = t + rng.normal(0, 0.03 * perturb, 3)
        pose[i] = np.concatenate([R.reshape(9), t])
    X0 = X + rng.normal(0, 0.03 * perturb, X.shape)
    return {"kf_pose": pose.astype(np.float32), "kf_K": np.tile(np.array(K, np.float32), (n_kf, 1)),
            "kf_fixed": np.array(fixed, np.uint8), "pt_pos": X0.astype(np.float32), "pt_nobs": np.array(nobs, np.int32),
            "edge_pt": np.array(ept, np.int32), "edge_kf": np.array(ekf, np.int32),
            "edge_obs": np.array(obs, np.float32).reshape(-1, 2), "edge_inv_sigma2": np.array(inv_s2, np.float32),
            "scale": RADIUS, "seed": seed}


def make_scene(seed, *args, **kw) -> dict:
    """build_scene at the first of the seeds seed, seed + 1, ... whose model run is decisive; at most
    MAX_SEED_SKIPS seeds are skipped."""
    for s in range(seed, seed + MAX_SEED_SKIPS + 1):
        g = build_scene(s, *args, **kw)
        g["model"] = lbm.local_bundle_adjustment(g)
        assert g["model"]["status"] == 0, g["model"]["status"]
        if lbm.decisive(g["model"], g["scale"]):
            g["skipped"] = s - seed
            return g
    raise AssertionError(f"no decisive seed within {MAX_SEED_SKIPS} of {seed}")


# name -> (seed, n_free, n_fixed, n_pt, obs_per_pt, keywords).  The free keyframe counts straddle the
# Cholesky panel (two keyframes: 1, 2, 3) and reach the capacity; the point counts straddle a wave (64)
# and the workgroup (256).
HOST_CASES = {
    "free_1_pts_65": (1000, 1, 2, 65, 3, {}),
    "free_2_pts_63": (1020, 2, 2, 63, 3, {}),
    "free_3_pts_64": (1040, 3, 2, 64, 3, {}),
    "free_8_pts_255": (1060, 8, 2, 255, 3, {}),
    "free_9_pts_257_obs_12": (1080, 9, 4, 257, 12, {}),
    "free_64_bit_63": (1100, MAX_FREE_KF, 2, 300, 12, {"force_kf": MAX_FREE_KF - 1, "outliers": 0.05}),
    "fixed_1": (1120, 3, 1, 100, 3, {}),
    "fixed_40_obs_12": (1140, 4, 40, 200, 12, {}),
    "pts_1_obs_2": (1160, 2, 2, 1, 2, {"outliers": 0.0}),
    "pts_256": (1180, 3, 2, 256, 3, {}),
    "pts_2000": (1200, 5, 3, 2000, 3, {}),
    "obs_2": (1220, 3, 2, 120, 2, {}),
    "outliers_points_go_bad": (1240, 4, 2, 150, 3, {"outliers": 0.25}),
    "behind_camera": (1260, 3, 2, 100, 4, {"behind": 5}),
    "keyframe_0_window": (1280, 4, 2, 100, 3, {"local_fixed": 1}),
}
GAUGE_FREE_CASE = ("fixed_0", (1300, 3, 0, 100, 3, {}))
_cache = {}


def host_case(name) -> dict:
    if name not in _cache:
        seed, nf, nx, npt, nobs, kw = dict([GAUGE_FREE_CASE], **HOST_CASES)[name]
        _cache[name] = make_scene(seed, nf, nx, npt, nobs, **kw)
    return _cache[name]


def fixture_scene(seed=1400) -> dict:
    """The scene of tests/golden/local_ba_320x240.npz (scripts/gen_local_ba_golden.py picks the seed)."""
    return make_scene(seed, 6, 3, 180, 4, outliers=0.2, behind=6)


def threshold_case(above=False) -> dict:
    """Four edges whose chi2 is 5.991 to the bit at both classifications.  A free and a fixed keyframe at
    the identity pose (cx = cy = 0) see two points at (0, 0, 1); the free keyframe sees point 0 at +e and
    point 1 at -e, the fixed one the other way round, with e = (e0, e1) and invSigma2 = s floats chosen
    so that e0 (s e0) + e1 (s e1) == 5.991 in double arithmetic.  Each vertex's two contributions to b
    cancel exactly in any order, so the step is exactly 0, the trial ends where it began (rho == 0:
    rejected, terminate) and every chi2 stays what it was.  `>` keeps all four edges (Optimizer.cc:461);
    `>=` would erase them.  `above`: invSigma2 one float up, every chi2 above the threshold."""
    s, e0, e1 = (np.array([b], np.uint32).view(np.float32)[0] for b in (0x3F800011, 0x401CA649, 0x3A869775))
    assert np.float64(e0) * (np.float64(s) * np.float64(e0)) + np.float64(e1) * (np.float64(s) * np.float64(e1)) == 5.991
    if above:
        s = np.nextafter(s, np.float32(2))
    I12 = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(np.float32)
    e = np.array([e0, e1], np.float32)
    return {"kf_pose": np.stack([I12, I12]), "kf_K": np.tile(np.float32([320, 320, 0, 0]), (2, 1)),
            "kf_fixed": np.array([0, 1], np.uint8), "pt_pos": np.float32([[0, 0, 1], [0, 0, 1]]),
            "pt_nobs": np.int32([2, 2]), "edge_pt": np.int32([0, 0, 1, 1]), "edge_kf": np.int32([0, 1, 0, 1]),
            "edge_obs": np.stack([e, -e, -e, e]), "edge_inv_sigma2": np.full(4, s, np.float32), "scale": 1.0}


GRAPH_KEYS = ("kf_pose", "kf_K", "kf_fixed", "pt_pos", "pt_nobs", "edge_pt", "edge_kf", "edge_obs", "edge_inv_sigma2")


def pose_spread(a, b) -> float:
    return float(np.max(np.abs(a["kf_pose_f64"] - b["kf_pose_f64"]), initial=0.0))


def point_spread(a, b) -> float:
    return float(np.max(np.abs(a["pt_pos_f64"] - b["pt_pos_f64"]), initial=0.0))


def chi2_spread(a, b) -> float:
    """Largest difference of a classified chi2, relative to 5.991 or to the chi2 itself where that is
    larger, over the pairs finite in both."""
    with np.errstate(invalid="ignore"):
        d = np.abs(a["chi2"] - b["chi2"]) / np.maximum(lbm.CHI2_TH, np.abs(a["chi2"]))
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0
