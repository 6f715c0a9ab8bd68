"""ctypes loader of the CPU model of the PnP / Sim3 consensus (tests/native/solvers_model.cpp, built
to build/libsolvers_model.so by __graft_entry__.build()).  Python has no fma, so the model that
restates the constructors' set-up, the two CheckInliers and the keep-the-best loops is C++.

Also the shared synthetic cases of the solver tests (CPU and GPU)."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB = ROOT / "build" / "libsolvers_model.so"
PLAIN, UNTRUNCATED, ROW_PLAIN = 1, 2, 4  # variant bits (tests only)
_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
            sys.path.insert(0, str(ROOT))
            import __graft_entry__ as ge

            LIB.parent.mkdir(exist_ok=True)
            subprocess.run(ge.SOLVERS_MODEL_CMD(LIB), check=True)
        _lib = ctypes.CDLL(str(LIB))
        vp, i, d, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
        _lib.solvers_model_pnp.restype = i
        _lib.solvers_model_pnp.argtypes = [i, vp, vp, vp, f, d, d, d, d, i, vp, vp, i, i, i, vp, vp, vp, vp, vp]
        _lib.solvers_model_sim3.restype = i
        _lib.solvers_model_sim3.argtypes = [i, vp, vp, vp, vp, vp, vp, i, vp, vp, i, i, i, vp, vp, vp, vp, vp, vp]
        _lib.solvers_model_pnp_setup.restype = i
        _lib.solvers_model_pnp_setup.argtypes = [vp, vp, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
        _lib.solvers_model_sim3_setup.restype = i
        _lib.solvers_model_sim3_setup.argtypes = [vp, i, vp, i] + [vp] * 13
    return _lib


def _p(a):
    return ctypes.c_void_p(None if a is None else a.ctypes.data)


def _f32(a, cols=0):
    a = np.ascontiguousarray(a, np.float32)
    return a.reshape(-1, cols) if cols else a.reshape(-1)


def unpack(masks, n):
    masks = np.ascontiguousarray(masks, np.uint64)
    return np.unpackbits(masks.view(np.uint8), axis=-1, bitorder="little")[..., :n].astype(bool)


def pnp(p3d, p2d, sigma2, th2, K, R, t, min_inliers, best_in=0, variant=0, errors=False) -> dict:
    """The model's answer in the shape of orbslam_jpminipc_amd.PnPConsensus.check (plus `err`
    (n_hyp, n) error2 when `errors`).  K: fu, fv, uc, vc (float32 values, widened)."""
    p3d, p2d, s2 = _f32(p3d, 3), _f32(p2d, 2), _f32(sigma2)
    R = np.ascontiguousarray(R, np.float64).reshape(-1, 9)
    t = np.ascontiguousarray(t, np.float64).reshape(-1, 3)
    n, n_hyp = len(p3d), len(R)
    W = (n + 63) // 64
    counts = np.zeros(n_hyp, np.int32)
    masks = np.zeros((n_hyp, max(W, 1)), np.uint64)
    best_at = np.zeros(n_hyp, np.int32)
    first = np.zeros(1, np.int32)
    err = np.zeros((n_hyp, max(n, 1)), np.float32) if errors else None
    fu, fv, uc, vc = (float(np.float32(x)) for x in K)
    r = lib().solvers_model_pnp(n, _p(p3d), _p(p2d), _p(s2), float(np.float32(th2)), fu, fv, uc, vc, n_hyp, _p(R), _p(t),
                                int(min_inliers), int(best_in), int(variant), _p(counts), _p(masks) if W else None,
                                _p(best_at), _p(first), _p(err))
    assert r == 0
    masks = masks[:, :W]
    out = {"n": n, "counts": counts, "masks": masks, "inliers": unpack(masks, n) if W else np.zeros((n_hyp, 0), bool),
           "best_at": best_at, "first_ok": int(first[0])}
    if errors:
        out["err"] = err[:, :n]
    return out


def sim3(x3dc1, x3dc2, sigma2_1, sigma2_2, K1, K2, T12, T21, min_inliers, best_in=0, variant=0, errors=False) -> dict:
    """The model's answer in the shape of Sim3Consensus.check (plus err1 / err2 (n_hyp, n))."""
    x1, x2, s1, s2 = _f32(x3dc1, 3), _f32(x3dc2, 3), _f32(sigma2_1), _f32(sigma2_2)
    K1, K2 = _f32(K1), _f32(K2)
    T12, T21 = _f32(T12, 12), _f32(T21, 12)
    n, n_hyp = len(x1), len(T12)
    W = (n + 63) // 64
    counts = np.zeros(n_hyp, np.int32)
    masks = np.zeros((n_hyp, max(W, 1)), np.uint64)
    best_at = np.zeros(n_hyp, np.int32)
    first = np.zeros(1, np.int32)
    e1 = np.zeros((n_hyp, max(n, 1)), np.float32) if errors else None
    e2 = np.zeros((n_hyp, max(n, 1)), np.float32) if errors else None
    r = lib().solvers_model_sim3(n, _p(x1), _p(x2), _p(s1), _p(s2), _p(K1), _p(K2), n_hyp, _p(T12), _p(T21),
                                 int(min_inliers), int(best_in), int(variant), _p(counts), _p(masks) if W else None,
                                 _p(best_at), _p(first), _p(e1), _p(e2))
    assert r == 0
    masks = masks[:, :W]
    out = {"n": n, "counts": counts, "masks": masks, "inliers": unpack(masks, n) if W else np.zeros((n_hyp, 0), bool),
           "best_at": best_at, "first_accept": int(first[0])}
    if errors:
        out["err1"], out["err2"] = e1[:, :n], e2[:, :n]
    return out


def pnp_setup(f_kps, n_f, n_kf, match, mp_pos, mp_bad, level_sigma2) -> dict:
    """PnPsolver's constructor over one SearchByBoW(KF, F) row.  f_kps: the frame's keypoint records
    (capacity rows, n_f valid); match: the row; mp_pos (cap, 3) / mp_bad (cap,) of the keyframe."""
    cap = len(match)
    xy = np.ascontiguousarray(np.stack([f_kps["x"], f_kps["y"]], 1), np.float32)
    octv = np.ascontiguousarray(f_kps["octave"], np.int32)
    match = np.ascontiguousarray(match, np.int32)
    pos = _f32(mp_pos, 3)
    bad = None if mp_bad is None else np.ascontiguousarray(mp_bad, np.uint8)
    ls2 = _f32(level_sigma2)
    p3d, p2d, s2, idx = (np.zeros((cap, 3), np.float32), np.zeros((cap, 2), np.float32), np.zeros(cap, np.float32),
                         np.full(cap, -1, np.int32))
    N = lib().solvers_model_pnp_setup(_p(xy), _p(octv), int(n_f), int(n_kf), _p(match), _p(pos), _p(bad), _p(ls2),
                                      _p(p3d), _p(p2d), _p(s2), _p(idx))
    return {"n": N, "p3d": p3d[:N], "p2d": p2d[:N], "sigma2": s2[:N], "index": idx}


def sim3_setup(kps1, n1, kps2, n2, match12, pos1, bad1, pos2, bad2, pose1, pose2, level_sigma2) -> dict:
    """Sim3Solver's constructor over one SearchByBoW(KF1, KF2) row."""
    cap = len(match12)
    o1 = np.ascontiguousarray(kps1["octave"], np.int32)
    o2 = np.ascontiguousarray(kps2["octave"], np.int32)
    match12 = np.ascontiguousarray(match12, np.int32)
    pos1, pos2 = _f32(pos1, 3), _f32(pos2, 3)
    bad1 = None if bad1 is None else np.ascontiguousarray(bad1, np.uint8)
    bad2 = None if bad2 is None else np.ascontiguousarray(bad2, np.uint8)
    pose1, pose2, ls2 = _f32(pose1), _f32(pose2), _f32(level_sigma2)
    x1, x2, s1, s2, idx = (np.zeros((cap, 3), np.float32), np.zeros((cap, 3), np.float32), np.zeros(cap, np.float32),
                           np.zeros(cap, np.float32), np.full(cap, -1, np.int32))
    N = lib().solvers_model_sim3_setup(_p(o1), int(n1), _p(o2), int(n2), _p(match12), _p(pos1), _p(bad1), _p(pos2),
                                       _p(bad2), _p(pose1), _p(pose2), _p(ls2), _p(x1), _p(x2), _p(s1), _p(s2), _p(idx))
    return {"n": N, "x3dc1": x1[:N], "x3dc2": x2[:N], "sigma2_1": s1[:N], "sigma2_2": s2[:N], "index": idx}


def same_result(got: dict, want: dict, first_key: str) -> None:
    """Asserts that two check() results agree exactly in counts, masks, best_at and the first index."""
    assert got["n"] == want["n"]
    assert np.array_equal(got["counts"], want["counts"]), np.flatnonzero(got["counts"] != want["counts"])[:8]
    if "masks" in got and "masks" in want:
        assert got["masks"].shape == want["masks"].shape
        assert np.array_equal(got["masks"], want["masks"])
    assert np.array_equal(got["best_at"], want["best_at"])
    assert got[first_key] == want[first_key]


# ---- synthetic cases ---------------------------------------------------------------------------------
K_TUM = (517.306408, 516.469215, 318.643040, 255.313989)  # fx, fy, cx, cy (a TUM1-like calibration)
LEVEL_SIGMA2 = np.float32(1.2) ** (2 * np.arange(8, dtype=np.float32))  # mvLevelSigma2 of 8 levels at 1.2


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pnp_case(n, n_hyp, seed, K=K_TUM, noise=1.5, outliers=0.3):
    """n world points seen by a camera at a known pose, pixel noise and gross outliers; hypotheses
    = the true pose perturbed by growing amounts (the first few near it)."""
    rng = np.random.default_rng(seed)
    Rt, tt = rodrigues(rng.normal(0, 0.2, 3)), rng.normal(0, 0.3, 3)
    Pc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(2, 8, n)], 1)
    Pw = (Pc - tt) @ Rt  # Pc = R Pw + t
    lev = rng.integers(0, 8, n)
    u = K[0] * Pc[:, 0] / Pc[:, 2] + K[2] + rng.normal(0, noise, n) * np.sqrt(LEVEL_SIGMA2[lev])
    v = K[1] * Pc[:, 1] / Pc[:, 2] + K[3] + rng.normal(0, noise, n) * np.sqrt(LEVEL_SIGMA2[lev])
    bad = rng.random(n) < outliers
    u[bad] += rng.uniform(-60, 60, bad.sum())
    v[bad] += rng.uniform(-60, 60, bad.sum())
    R = np.zeros((n_hyp, 3, 3))
    t = np.zeros((n_hyp, 3))
    for h in range(n_hyp):
        s = 0.002 * (h % 17)
        R[h] = rodrigues(rng.normal(0, s + 1e-4, 3)) @ Rt
        t[h] = tt + rng.normal(0, 2 * s + 1e-4, 3)
    return {"p3d": Pw.astype(np.float32), "p2d": np.stack([u, v], 1).astype(np.float32),
            "sigma2": LEVEL_SIGMA2[lev].astype(np.float32), "R": R, "t": t, "K": K}


def sim3_case(n, n_hyp, seed, K=K_TUM, noise=0.01, outliers=0.3):
    """n points in two camera frames related by a similarity, noise and outliers; hypotheses = the
    true transform perturbed by growing amounts, each with its inverse."""
    rng = np.random.default_rng(seed)
    R12, t12, s12 = rodrigues(rng.normal(0, 0.3, 3)), rng.normal(0, 0.5, 3), float(rng.uniform(0.8, 1.25))
    X2 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(3, 9, n)], 1)
    X1 = s12 * X2 @ R12.T + t12 + rng.normal(0, noise, (n, 3))
    bad = rng.random(n) < outliers
    X1[bad] += rng.normal(0, 0.8, (bad.sum(), 3))
    T12 = np.zeros((n_hyp, 3, 4), np.float32)
    T21 = np.zeros((n_hyp, 3, 4), np.float32)
    for h in range(n_hyp):
        e = 0.002 * (h % 17)
        R = rodrigues(rng.normal(0, e + 1e-4, 3)) @ R12
        s = s12 * (1 + rng.normal(0, e + 1e-4))
        t = t12 + rng.normal(0, 2 * e + 1e-4, 3)
        T12[h, :, :3], T12[h, :, 3] = s * R, t
        T21[h, :, :3], T21[h, :, 3] = R.T / s, -(R.T / s) @ t
    l1, l2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
    return {"x3dc1": X1.astype(np.float32), "x3dc2": X2.astype(np.float32), "sigma2_1": LEVEL_SIGMA2[l1].astype(np.float32),
            "sigma2_2": LEVEL_SIGMA2[l2].astype(np.float32), "T12": T12, "T21": T21,
            "K1": np.asarray(K, np.float32), "K2": np.asarray(K, np.float32)}
