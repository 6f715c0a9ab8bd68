"""ctypes loader of build/libpose_optimization_model.so (tests/native/pose_optimization_model.cpp):
the CPU model of Optimizer::PoseOptimization that the GPU tests compare against, and the synthetic
cases they share."""
from __future__ import annotations

import ctypes
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB_PATH = ROOT / "build" / "libpose_optimization_model.so"

CHI2_TH = np.array([9.210, 7.378, 5.991, 5.991], np.float32).astype(np.float64)
# every edge of a test case keeps this relative distance from the round's threshold at every
# classification, so the model alone decides the flag (checked by `decisive`)
FLAG_MARGIN = 1e-5


class Info(ctypes.Structure):
    """orb_pose_opt_info_t (include/orb_abi.h)."""

    _fields_ = [("n_initial", ctypes.c_int32), ("n_bad", ctypes.c_int32), ("rounds", ctypes.c_int32),
                ("iterations", ctypes.c_int32 * 4), ("trials", ctypes.c_int32), ("lambda_", ctypes.c_double),
                ("chi2", ctypes.c_double)]


_vp, _i, _f, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
_libs = {}


def lib(path=LIB_PATH):
    if path not in _libs:
        L = ctypes.CDLL(str(path))
        L.pom_pose_optimization.restype = _i
        L.pom_pose_optimization.argtypes = [_i, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _vp, _i, _i, _vp, _vp, _vp, _vp,
                                            _vp, _vp]
        L.pom_pose_from_float.argtypes = [_vp, _vp]
        L.pom_pose_to_matrix.argtypes = [_vp, _vp]
        L.pom_exp_update.argtypes = [_vp, _vp, _vp]
        L.pom_edge.argtypes = [_vp, _vp, _vp, _vp, _d, _vp, _vp, _vp]
        L.pom_build.restype = _d
        L.pom_build.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp]
        L.pom_solve.restype = _i
        L.pom_solve.argtypes = [_vp, _vp, _d, _vp]
        L.pom_huber.argtypes = [_d, _vp]
        _libs[path] = L
    return _libs[path]


def _p(a):
    return None if a is None else a.ctypes.data


def pose_optimization(p3d, obs, inv_sigma2, has_mp, K, pose_in, sum_order=0, variant=0, path=LIB_PATH) -> dict:
    """The model's answer: pose (12,) float32, pose_f64 (12,), outlier (n,) uint8, n_inliers, info
    and chi2 (4, n): every edge's chi2 at each classification (NaN: no edge / round not run)."""
    p3d = np.ascontiguousarray(p3d, np.float32).reshape(-1, 3)
    obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 2)
    s = np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1)
    n = len(p3d)
    hm = None if has_mp is None else np.ascontiguousarray(has_mp, np.uint8)
    pin = np.ascontiguousarray(pose_in, np.float32).reshape(12)
    pose, pose64 = np.zeros(12, np.float32), np.zeros(12, np.float64)
    outl, chi2 = np.zeros(max(n, 1), np.uint8), np.zeros((4, max(n, 1)), np.float64)
    ninl, info = ctypes.c_int32(0), Info()
    lib(path).pom_pose_optimization(n, _p(p3d), _p(obs), _p(s), _p(hm), K[0], K[1], K[2], K[3], _p(pin), sum_order,
                                    variant, _p(pose), _p(pose64), _p(outl), ctypes.addressof(ninl),
                                    ctypes.addressof(info), _p(chi2))
    return {"pose": pose, "pose_f64": pose64, "outlier": outl[:n], "n_inliers": int(ninl.value), "info": info,
            "chi2": chi2.reshape(-1)[:4 * n].reshape(4, n)}


def decisive(res) -> bool:
    """Every classified chi2 lies at least FLAG_MARGIN (relative) from its round's threshold."""
    c = res["chi2"]
    with np.errstate(invalid="ignore"):
        near = np.abs(c - CHI2_TH[:, None]) < FLAG_MARGIN * CHI2_TH[:, None]
    return not bool(near.any())


def rot(w) -> np.ndarray:
    """Rodrigues' rotation matrix of the axis-angle vector w (float64)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * Wx @ Wx


LEVEL_SIGMA2 = (np.float32(1.2) ** np.arange(8, dtype=np.float32)) ** 2
K_DEFAULT = (np.float32(320.0), np.float32(318.5), np.float32(159.5), np.float32(119.25))


def make_case(seed, n, edges=None, outliers=0.2, levels=8, K=K_DEFAULT, perturb=0.02, octave_out=False) -> dict:
    """A synthetic problem: true pose, points at depth 4..12 in front of the camera, level-dependent
    pixel noise, a share of gross outliers, a perturbed float32 start pose.  `edges`: how many of
    the n keypoints carry a map point (None: all).  Seeds are advanced until the model is
    decisive (FLAG_MARGIN)."""
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        Rt = rot(rng.normal(0, 0.2, 3))
        tt = rng.normal(0, 0.5, 3)
        z = rng.uniform(4, 12, n)
        u = rng.uniform(0, 2 * K[2], n)
        v = rng.uniform(0, 2 * K[3], n)
        Xc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)
        Xw = (Xc - tt) @ Rt  # Rt^T (Xc - t)
        octave = rng.integers(0, levels, n)
        sig = np.sqrt(LEVEL_SIGMA2[octave].astype(np.float64))
        obs = np.stack([u, v], 1) + rng.normal(0, 1, (n, 2)) * sig[:, None]
        bad = rng.random(n) < outliers
        obs[bad] += rng.uniform(-40, 40, (int(bad.sum()), 2))
        inv_s2 = (np.float32(1.0) / LEVEL_SIGMA2[octave]).astype(np.float32)
        if octave_out:  # an octave outside the table is clamped to its last level
            octave = octave.copy()
            octave[::3] = levels + 3
            inv_s2[::3] = np.float32(1.0) / LEVEL_SIGMA2[levels - 1]
        has = np.ones(n, np.uint8)
        if edges is not None:
            has[:] = 0
            has[rng.choice(n, edges, replace=False)] = 1
        R0 = rot(rng.normal(0, perturb, 3)) @ Rt
        t0 = tt + rng.normal(0, perturb * 5, 3)
        pose_in = np.concatenate([R0.reshape(9), t0]).astype(np.float32)
        case = {"p3d": Xw.astype(np.float32), "obs": obs.astype(np.float32), "inv_sigma2": inv_s2, "has_mp": has,
                "octave": octave.astype(np.int32), "K": K, "pose_in": pose_in, "seed": s,
                "pose_true": np.concatenate([Rt.reshape(9), tt])}
        case["model"] = pose_optimization(case["p3d"], case["obs"], inv_s2, has, K, pose_in)
        if decisive(case["model"]):
            return case
    raise AssertionError("no decisive seed found")


def _decisive_or_fail(case):
    case["model"] = pose_optimization(case["p3d"], case["obs"], case["inv_sigma2"], case["has_mp"], case["K"],
                                      case["pose_in"])
    assert decisive(case["model"]), "case is not decisive: change its seed"
    return case


EDGE_COUNTS = [0, 1, 5, 9, 10, 63, 64, 65, 255, 256, 257, 1000, 8192]  # 256: the kernels' stride


def host_cases() -> dict:
    """name -> case: every synthetic problem of tests/test_gpu_pose_optimization.py (the tolerance of
    DESIGN.md §13 is measured over exactly these)."""
    out = {}
    for n in EDGE_COUNTS:
        out[f"edges_{n}"] = make_case(100 + n, n)
    out["holes_5_of_2000"] = make_case(300, 2000, edges=5)
    out["holes_300_of_2000"] = make_case(301, 2000, edges=300)
    out["holes_257_of_1025"] = make_case(302, 1025, edges=257)
    out["outliers_0"] = make_case(310, 300, outliers=0.0)
    out["outliers_50"] = make_case(311, 300, outliers=0.5)
    out["level_0_only"] = make_case(320, 300, levels=1)
    # nothing fits: every edge is an outlier after round 1, rounds 2-4 have no active edge
    c = make_case(330, 40)
    rng = np.random.default_rng(330)
    c["obs"] = (c["obs"] + rng.choice([-1, 1], c["obs"].shape) * rng.uniform(60, 120, c["obs"].shape)).astype(np.float32)
    out["all_outliers_after_round_1"] = _decisive_or_fail(c)
    # a point at the camera centre of an identity start pose (0 / 0: NaN chi2) and one in its
    # plane (x / 0: inf)
    for name, X0 in (("z_zero_nan", [0, 0, 0]), ("z_zero_inf", [1, 1, 0])):
        c = make_case(340, 30)
        c["pose_in"] = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(np.float32)
        c["p3d"][0] = X0
        out[name] = _decisive_or_fail(c)
    # a third of the points behind the camera
    c = make_case(350, 120)
    R, t = c["pose_true"][:9].reshape(3, 3), c["pose_true"][9:]
    Xc = c["p3d"][::3].astype(np.float64) @ R.T + t
    Xc[:, 2] *= -1
    c["p3d"][::3] = ((Xc - t) @ R).astype(np.float32)
    out["behind_camera"] = _decisive_or_fail(c)
    # all points identical: H has rank 2
    c = make_case(360, 50)
    c["p3d"][:] = c["p3d"][0]
    out["identical_points"] = _decisive_or_fail(c)
    return out


def pose_spread(a, b) -> float:
    with np.errstate(invalid="ignore"):
        d = np.abs(a["pose_f64"] - b["pose_f64"])
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def chi2_spread(a, b) -> float:
    """Largest difference of a classified chi2, relative to its round's threshold, over finite pairs."""
    with np.errstate(invalid="ignore"):
        d = np.abs(a["chi2"] - b["chi2"]) / CHI2_TH[:, None]
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0
