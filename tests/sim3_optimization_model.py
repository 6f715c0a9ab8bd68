"""ctypes loader of build/libsim3_optimization_model.so (tests/native/sim3_optimization_model.cpp):
the CPU model of Optimizer::OptimizeSim3 that the GPU tests compare against, and the synthetic cases
they share."""
from __future__ import annotations

import ctypes
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB_PATH = ROOT / "build" / "libsim3_optimization_model.so"

TH2 = np.float32(10.0)  # LoopClosing.cc:340
# every edge of a test case keeps this relative distance from th2 at both classifications, so the
# model alone decides each slot (checked by `decisive`); DESIGN.md §14: at least 10 x the chi2 spread
MARGIN = 5e-4
f32 = np.float32


class Info(ctypes.Structure):
    """orb_sim3_opt_info_t (include/orb_abi.h)."""

    _fields_ = [("n_correspondences", ctypes.c_int32), ("n_bad", ctypes.c_int32), ("more_iterations", ctypes.c_int32),
                ("iterations", ctypes.c_int32 * 2), ("trials", ctypes.c_int32), ("lambda_", ctypes.c_double),
                ("chi2", ctypes.c_double)]


_vp, _i, _f, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
_libs = {}


def lib(path=LIB_PATH):
    if path not in _libs:
        L = ctypes.CDLL(str(path))
        L.s3m_optimize_sim3.restype = _i
        L.s3m_optimize_sim3.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _i, _vp, _vp, _vp,
                                        _vp, _vp, _vp]
        L.s3m_from_float.argtypes = [_vp, _vp]
        L.s3m_to_13.argtypes = [_vp, _vp]
        L.s3m_exp.restype = _i
        L.s3m_exp.argtypes = [_vp, _vp]
        L.s3m_oplus.restype = _i
        L.s3m_oplus.argtypes = [_vp, _vp, _vp]
        L.s3m_map.argtypes = [_vp, _vp, _vp]
        L.s3m_inverse.argtypes = [_vp, _vp]
        L.s3m_mul.argtypes = [_vp, _vp, _vp]
        L.s3m_edge.argtypes = [_vp, _vp, _vp, _vp, _d, _i, _vp, _vp, _vp]
        L.s3m_build.restype = _d
        L.s3m_build.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _i, _vp, _vp]
        L.s3m_solve.restype = _i
        L.s3m_solve.argtypes = [_vp, _vp, _d, _vp]
        L.s3m_huber.argtypes = [_f, _d, _vp, _vp]
        L.s3m_last_branches.restype = _i
        _libs[path] = L
    return _libs[path]


def _p(a):
    return None if a is None else a.ctypes.data


def optimize_sim3(x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, sigma2_2, usable, K1, K2, th2, sim3_in, sum_order=0,
                  variant=0, path=LIB_PATH) -> dict:
    """The model's answer: kept (n,) uint8, n_inliers, sim3 (13,) float32, sim3_f64 (8,), info, chi2
    (2, 2, n): every edge's chi2 at each classification (classification, e12 / e21, slot; NaN: no edge
    / not run) and branches: bit k set when an accepted update took branch k of Sim3(update)."""
    x1 = np.ascontiguousarray(x3dc1, f32).reshape(-1, 3)
    x2 = np.ascontiguousarray(x3dc2, f32).reshape(-1, 3)
    o1 = np.ascontiguousarray(obs1, f32).reshape(-1, 2)
    o2 = np.ascontiguousarray(obs2, f32).reshape(-1, 2)
    w1 = np.ascontiguousarray(inv_sigma2_1, f32).reshape(-1)
    w2 = np.ascontiguousarray(sigma2_2, f32).reshape(-1)
    us = None if usable is None else np.ascontiguousarray(usable, np.uint8)
    k1, k2 = np.ascontiguousarray(K1, f32).reshape(4), np.ascontiguousarray(K2, f32).reshape(4)
    sin = np.ascontiguousarray(sim3_in, f32).reshape(13)
    n = len(x1)
    kept, o64, o32 = np.zeros(max(n, 1), np.uint8), np.zeros(8), np.zeros(13, f32)
    chi2 = np.zeros(4 * max(n, 1))
    ninl, info = ctypes.c_int32(0), Info()
    L = lib(path)
    L.s3m_optimize_sim3(n, _p(x1), _p(x2), _p(o1), _p(o2), _p(w1), _p(w2), _p(us), _p(k1), _p(k2), float(th2), _p(sin),
                        sum_order, variant, _p(kept), _p(o64), _p(o32), ctypes.addressof(ninl), ctypes.addressof(info),
                        _p(chi2))
    return {"kept": kept[:n], "n_inliers": int(ninl.value), "sim3": o32, "sim3_f64": o64, "info": info,
            "chi2": chi2[:4 * n].reshape(2, 2, n), "branches": int(L.s3m_last_branches())}


def run_case(c, sum_order=0, variant=0, path=LIB_PATH) -> dict:
    return optimize_sim3(c["x3dc1"], c["x3dc2"], c["obs1"], c["obs2"], c["inv_sigma2_1"], c["sigma2_2"], c["usable"],
                         c["K1"], c["K2"], c["th2"], c["sim3_in"], sum_order, variant, path)


def decisive(res, th2=TH2) -> bool:
    """Every classified chi2 lies at least MARGIN (relative) from th2."""
    t = float(f32(th2))
    with np.errstate(invalid="ignore"):
        near = np.abs(res["chi2"] - t) < MARGIN * t
    return not bool(near.any())


def rot(w) -> np.ndarray:
    """Rodrigues' rotation matrix of the axis-angle vector w (float64)."""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    Wx = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + Wx
    return np.eye(3) + np.sin(th) / th * Wx + (1 - np.cos(th)) / th ** 2 * Wx @ Wx


LEVEL_SIGMA2 = (f32(1.2) ** np.arange(8, dtype=f32)) ** 2
INV_LEVEL_SIGMA2 = (f32(1.0) / LEVEL_SIGMA2).astype(f32)
K_DEFAULT = f32([320.0, 318.5, 159.5, 119.25])
K_SECOND = f32([300.0, 301.5, 161.25, 118.5])
IDENTITY13 = np.concatenate([np.eye(3).reshape(9), np.zeros(3), [1.0]]).astype(f32)


def sim3_13(R, t, s) -> np.ndarray:
    return np.concatenate([np.asarray(R).reshape(9), np.asarray(t).reshape(3), [s]]).astype(f32)


def make_case(seed, n, usable=None, outliers=0.1, levels=8, scale=1.0, perturb=0.02, K1=K_DEFAULT, K2=K_SECOND,
              th2=TH2, require=None, tries=60, moderate=0.0) -> dict:
    """A synthetic loop candidate: a true S12 (rotation, translation, `scale`), points at depth 4..12
    of camera 1 and their images under S21 in camera 2, level-dependent pixel noise (on the second
    side scaled down by sigma2, as e21 is weighted with sigma2 itself), a share of gross outliers
    and a perturbed float32 start.  `moderate`: a share of pairs whose second observation is 1.5 to 3
    pixels off, which e21's sigma2 weight makes an outlier at the higher levels and 1 / sigma2 would
    not.  `usable`: None (all) or an (n,) flag array.  Seeds are advanced
    until the model is decisive (MARGIN) and `require(case)` holds."""
    for s in range(seed, seed + tries):
        rng = np.random.default_rng(s)
        R12, t12 = rot(rng.normal(0, 0.1, 3)), rng.normal(0, 0.4, 3)
        z = rng.uniform(4, 12, n)
        u1, v1 = rng.uniform(0, 2 * K1[2], n), rng.uniform(0, 2 * K1[3], n)
        X1 = np.stack([(u1 - K1[2]) / K1[0] * z, (v1 - K1[3]) / K1[1] * z, z], 1)
        X2 = ((X1 - t12) @ R12) / scale  # S21 * X1
        X2[:, 2] = np.maximum(X2[:, 2], 1.0)
        X1 = scale * (X2 @ R12.T) + t12
        oct1, oct2 = rng.integers(0, levels, n), rng.integers(0, levels, n)
        w1, w2 = INV_LEVEL_SIGMA2[oct1], LEVEL_SIGMA2[oct2]
        obs1 = np.stack([X1[:, 0] / X1[:, 2] * K1[0] + K1[2], X1[:, 1] / X1[:, 2] * K1[1] + K1[3]], 1)
        obs2 = np.stack([X2[:, 0] / X2[:, 2] * K2[0] + K2[2], X2[:, 1] / X2[:, 2] * K2[1] + K2[3]], 1)
        obs1 += rng.normal(0, 0.7, (n, 2)) / np.sqrt(w1.astype(np.float64))[:, None]
        obs2 += rng.normal(0, 0.7, (n, 2)) / np.sqrt(w2.astype(np.float64))[:, None]
        bad = rng.random(n) < outliers if isinstance(outliers, float) else np.arange(n) < int(outliers)
        k = int(bad.sum())
        side = rng.random(k) < 0.5  # the gross error sits in one image or the other
        off = rng.choice([-1, 1], (k, 2)) * rng.uniform(25, 60, (k, 2))
        obs1[bad] += off * side[:, None]
        obs2[bad] += off * ~side[:, None]
        if moderate:
            mod = rng.random(n) < moderate
            ang = rng.uniform(0, 2 * np.pi, int(mod.sum()))
            obs2[mod] += (rng.uniform(1.5, 3, int(mod.sum())) * np.stack([np.cos(ang), np.sin(ang)])).T
        R0 = rot(rng.normal(0, perturb, 3)) @ R12
        t0 = t12 + rng.normal(0, perturb * 5, 3)
        s0 = scale * (1 + rng.normal(0, perturb))
        us = np.ones(n, np.uint8) if usable is None else np.ascontiguousarray(usable, np.uint8)
        case = {"x3dc1": X1.astype(f32), "x3dc2": X2.astype(f32), "obs1": obs1.astype(f32), "obs2": obs2.astype(f32),
                "inv_sigma2_1": w1.copy(), "sigma2_2": w2.copy(), "usable": us, "K1": K1, "K2": K2, "th2": th2,
                "sim3_in": sim3_13(R0, t0, s0), "oct1": oct1.astype(np.int32), "oct2": oct2.astype(np.int32),
                "seed": s, "true": sim3_13(R12, t12, scale).astype(np.float64), "bad": bad}
        case["model"] = run_case(case)
        if decisive(case["model"], th2) and (require is None or require(case)):
            return case
    raise AssertionError("no decisive seed found")


def _decisive_or_fail(case):
    case["model"] = run_case(case)
    assert decisive(case["model"], case["th2"]), "case is not decisive: change its seed"
    return case


PAIR_COUNTS = [0, 1, 9, 10, 11, 63, 64, 65, 255, 256, 257, 1000, 8192]  # 256: the kernels' stride

_cases = None


def host_cases() -> dict:
    """name -> case: every synthetic problem of tests/test_gpu_sim3_optimization.py (the tolerance of
    DESIGN.md §14 is measured over exactly these)."""
    global _cases
    if _cases is not None:
        return _cases
    out = {}
    for n in PAIR_COUNTS:
        out[f"pairs_{n}"] = make_case(100 + n, n, outliers=0.1 if n >= 63 else 0.0)
    out["holes_300"] = make_case(300, 300, usable=(np.arange(300) % 3 != 2))
    out["outliers_0"] = make_case(310, 200, outliers=0.0)
    out["outliers_10"] = make_case(311, 200, outliers=0.10)
    out["outliers_45"] = make_case(312, 200, outliers=0.45)
    # the first classification leaves exactly 9 / exactly 10 pairs of 20
    out["survivors_9"] = make_case(320, 20, outliers=11,
                                   require=lambda c: c["model"]["info"].n_bad == 11 and c["model"]["n_inliers"] == 0)
    out["survivors_10"] = make_case(321, 20, outliers=10,
                                    require=lambda c: c["model"]["info"].n_bad == 10 and c["model"]["n_inliers"] == 10)
    out["octaves"] = make_case(330, 200, moderate=0.3, require=lambda c: len(set(c["oct1"])) == 8 and len(set(c["oct2"])) == 8)
    for sc in (0.5, 1.0, 2.0):
        out[f"scale_{sc}"] = make_case(340, 150, scale=sc)
    # update branch: started far from the optimum an accepted update has theta >= 1e-5 (branch 1 or
    # 3); started at the float32 rounding of the optimum every accepted one has theta < 1e-5
    far = make_case(350, 150, outliers=0.0, require=lambda c: c["model"]["branches"] & 0b1010)
    out["start_far"] = far
    near = dict(far)
    q = far["model"]["sim3"].copy()
    near["sim3_in"] = q
    near = _decisive_or_fail(near)
    assert near["model"]["branches"] and not near["model"]["branches"] & 0b1010, near["model"]["branches"]
    out["start_near"] = near
    # z = 0 after the map from an identity start: x / 0 (inf) on e12 of pair 0, and 0 / 0 (NaN) on
    # both edges of pair 0
    for name, X0 in (("z_zero_inf", [1, 1, 0]), ("nan_pair", [0, 0, 0])):
        c = make_case(360, 40, outliers=0.0)
        c["sim3_in"] = IDENTITY13.copy()
        c["x3dc2"][0] = X0
        if name == "nan_pair":
            c["x3dc1"][0] = X0
        out[name] = _decisive_or_fail(c)
    _cases = out
    return out


def threshold_case(w=TH2):
    """12 pairs at an identity start.  Pairs 0 and 1 look at the point (0, 0, 1) and observe it one
    pixel to the right and to the left in image 1 with information `w`, exactly in image 2; pairs 2..11
    observe (0, 0, 2) exactly in both.  The e21 rows and those of pairs 2..11 are exactly 0, the e12
    rows of pairs 0 and 1 are each other's negative (one Jacobian, opposite residuals), so b is
    exactly 0 in any summation order, the step is 0 and chi2(e12) of pairs 0 and 1 is 1 * (w * 1) = w
    to the bit."""
    n = 12
    X = np.zeros((n, 3), f32)
    X[:, 2] = 2
    X[:2, 2] = 1
    K = K_DEFAULT
    obs = np.tile(f32([K[2], K[3]]), (n, 1))
    obs1 = obs.copy()
    obs1[0, 0] += 1
    obs1[1, 0] -= 1
    w1 = np.ones(n, f32)
    w1[:2] = w
    return {"x3dc1": X, "x3dc2": X.copy(), "obs1": obs1, "obs2": obs, "inv_sigma2_1": w1, "sigma2_2": np.ones(n, f32),
            "usable": np.ones(n, np.uint8), "K1": K, "K2": K, "th2": TH2, "sim3_in": IDENTITY13.copy()}


def gemm3_add(T12, X) -> np.ndarray:
    """Rcw * X + tcw as the batch form takes it: float row sums left to right, then the
    add in double, narrowed."""
    T12, X = np.asarray(T12, f32), np.asarray(X, f32).reshape(-1, 3)
    R = T12[:9].reshape(3, 3)
    out = np.zeros_like(X)
    for i in range(3):
        s = R[i, 0] * X[:, 0]
        s = s + R[i, 1] * X[:, 1]
        s = s + R[i, 2] * X[:, 2]
        out[:, i] = (s.astype(np.float64) + np.float64(T12[9 + i])).astype(f32)
    return out


def batch_setup(kps1, n1, kps2, n2, row, pos1, bad1, pos2, bad2, pose1, pose2) -> dict:
    """The host arrays of one problem of the batch form (slot = keypoint of keyframe 1, n1 slots):
    what Optimizer.cc:1774-1853 reads for each slot."""
    row = np.asarray(row[:n1], np.int64)
    ok = (row >= 0) & (row < n2)
    m = np.where(ok, row, 0)
    if bad1 is not None:
        ok &= (bad1[:n1] == 0) & (bad2[m] == 0)
    k2 = kps2[m]
    return {"x3dc1": gemm3_add(pose1, pos1[:n1]), "x3dc2": gemm3_add(pose2, pos2[m]),
            "obs1": np.stack([kps1["x"][:n1], kps1["y"][:n1]], 1).astype(f32),
            "obs2": np.stack([k2["x"], k2["y"]], 1).astype(f32),
            "inv_sigma2_1": INV_LEVEL_SIGMA2[np.clip(kps1["octave"][:n1], 0, 7)],
            "sigma2_2": LEVEL_SIGMA2[np.clip(k2["octave"], 0, 7)], "usable": ok.astype(np.uint8)}


def sim3_spread(a, b) -> float:
    with np.errstate(invalid="ignore"):
        d = np.abs(a["sim3_f64"] - b["sim3_f64"])
    return float(np.nanmax(d)) if np.isfinite(d).any() else 0.0


def chi2_spread(a, b, th2=TH2) -> float:
    """Largest difference of a classified chi2, relative to th2, over finite pairs."""
    with np.errstate(invalid="ignore"):
        d = np.abs(a["chi2"] - b["chi2"]) / float(th2)
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0
