"""ctypes loader of build/liblocal_ba_model.so (tests/native/local_ba_model.cpp): the CPU model of
Optimizer::LocalBundleAdjustment that the GPU tests compare against."""
from __future__ import annotations

import ctypes
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB_PATH = ROOT / "build" / "liblocal_ba_model.so"

CHI2_TH = 5.991
# every classified chi2 keeps this relative distance from 5.991 and every depth this distance,
# relative to the scene's depth, from 0, so the model alone decides the flags (checked by `decisive`)
FLAG_MARGIN = 1e-5


class Round(ctypes.Structure):
    """orb_local_ba_round_t (include/orb_abi.h)."""

    _fields_ = [("iterations", ctypes.c_int32), ("trials", ctypes.c_int32), ("active_edges", ctypes.c_int32),
                ("active_points", ctypes.c_int32), ("active_keyframes", ctypes.c_int32), ("refused", ctypes.c_int32),
                ("lambda_", ctypes.c_double), ("chi2_before", ctypes.c_double), ("chi2_after", ctypes.c_double)]

    def as_dict(self) -> dict:
        return {"iterations": self.iterations, "trials": self.trials, "active_edges": self.active_edges,
                "active_points": self.active_points, "active_keyframes": self.active_keyframes,
                "refused": self.refused, "lambda": self.lambda_, "chi2_before": self.chi2_before,
                "chi2_after": self.chi2_after}


class Info(ctypes.Structure):
    """orb_local_ba_info_t."""

    _fields_ = [("status", ctypes.c_int32), ("n_free_kf", ctypes.c_int32), ("round", Round * 2)]

    def as_dict(self) -> dict:
        return {"status": self.status, "n_free_kf": self.n_free_kf, "round": [r.as_dict() for r in self.round]}


_vp, _i, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
_libs = {}


def lib(path=LIB_PATH):
    if path not in _libs:
        L = ctypes.CDLL(str(path))
        graph = [_i, _vp, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _vp, _vp]
        L.lbm_max_free_kf.restype = _i
        L.lbm_local_bundle_adjustment.restype = _i
        L.lbm_local_bundle_adjustment.argtypes = graph + [_i, _i] + [_vp] * 10
        L.lbm_step.restype = _i
        L.lbm_step.argtypes = graph + [_d, _i] + [_vp] * 7
        L.lbm_pose_from_float.argtypes = [_vp, _vp]
        L.lbm_pose_to_matrix.argtypes = [_vp, _vp]
        L.lbm_exp_update.argtypes = [_vp, _vp, _vp]
        L.lbm_edge.argtypes = [_vp, _vp, _vp, _vp, _d, _vp, _vp, _vp, _vp]
        L.lbm_erase_walk.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _vp, _i]
        L.lbm_cholesky_solve.restype = _i
        L.lbm_cholesky_solve.argtypes = [_i, _vp, _vp, _vp]
        _libs[path] = L
    return _libs[path]


def _p(a):
    return None if a is None else a.ctypes.data


def graph_arrays(g: dict) -> dict:
    """The graph `g` as the contiguous arrays of the C interfaces."""
    out = {"kf_pose": np.ascontiguousarray(g["kf_pose"], np.float32).reshape(-1, 12),
           "kf_K": np.ascontiguousarray(g["kf_K"], np.float32).reshape(-1, 4),
           "kf_fixed": np.ascontiguousarray(g["kf_fixed"], np.uint8).reshape(-1),
           "pt_pos": np.ascontiguousarray(g["pt_pos"], np.float32).reshape(-1, 3),
           "pt_nobs": np.ascontiguousarray(g["pt_nobs"], np.int32).reshape(-1),
           "edge_pt": np.ascontiguousarray(g["edge_pt"], np.int32).reshape(-1),
           "edge_kf": np.ascontiguousarray(g["edge_kf"], np.int32).reshape(-1),
           "edge_obs": np.ascontiguousarray(g["edge_obs"], np.float32).reshape(-1, 2),
           "edge_inv_sigma2": np.ascontiguousarray(g["edge_inv_sigma2"], np.float32).reshape(-1)}
    assert len(out["kf_K"]) == len(out["kf_fixed"]) == len(out["kf_pose"]) and len(out["pt_nobs"]) == len(out["pt_pos"])
    assert len(out["edge_kf"]) == len(out["edge_obs"]) == len(out["edge_inv_sigma2"]) == len(out["edge_pt"])
    return out


def _graph_args(a):
    return [len(a["kf_pose"]), _p(a["kf_pose"]), _p(a["kf_K"]), _p(a["kf_fixed"]), len(a["pt_pos"]), _p(a["pt_pos"]),
            _p(a["pt_nobs"]), len(a["edge_pt"]), _p(a["edge_pt"]), _p(a["edge_kf"]), _p(a["edge_obs"]),
            _p(a["edge_inv_sigma2"])]


def local_bundle_adjustment(g, sum_order=0, variant=0, path=LIB_PATH) -> dict:
    """The model's answer: status, kf_pose (n_kf, 12) float32 and kf_pose_f64, pt_pos (n_pt, 3) and
    pt_pos_f64, edge_erased, pt_bad, info, and chi2 / depth (2, n_edge): what each classification
    read (NaN: the edge was not in that round's optimisation), and kf_pose_round1_f64: the poses
    after the first optimize()."""
    a = graph_arrays(g)
    nk, npt, ne = len(a["kf_pose"]), len(a["pt_pos"]), len(a["edge_pt"])
    out = {"kf_pose": np.zeros((nk, 12), np.float32), "kf_pose_f64": np.zeros((nk, 12)),
           "pt_pos": np.zeros((npt, 3), np.float32), "pt_pos_f64": np.zeros((npt, 3)),
           "edge_erased": np.zeros(ne, np.uint8), "pt_bad": np.zeros(npt, np.uint8),
           "kf_pose_round1_f64": np.zeros((nk, 12))}
    chi2, depth = np.full((2, max(ne, 1)), np.nan), np.full((2, max(ne, 1)), np.nan)
    info = Info()
    out["status"] = lib(path).lbm_local_bundle_adjustment(
        *_graph_args(a), sum_order, variant, _p(out["kf_pose"]), _p(out["kf_pose_f64"]), _p(out["pt_pos"]),
        _p(out["pt_pos_f64"]), _p(out["edge_erased"]), _p(out["pt_bad"]), ctypes.addressof(info), _p(chi2), _p(depth),
        _p(out["kf_pose_round1_f64"]))
    out["info"] = info.as_dict()
    out["chi2"] = chi2.reshape(-1)[:2 * ne].reshape(2, ne)
    out["depth"] = depth.reshape(-1)[:2 * ne].reshape(2, ne)
    return out


def step(g, lam, sum_order=0) -> dict:
    """The system at the input estimates with every edge active and one damped step at `lam`."""
    a = graph_arrays(g)
    nk, npt, ne = len(a["kf_pose"]), len(a["pt_pos"]), len(a["edge_pt"])
    out = {"Hpp": np.zeros((nk, 6, 6)), "bp": np.zeros((nk, 6)), "Hll": np.zeros((npt, 3, 3)), "bl": np.zeros((npt, 3)),
           "Hpl": np.zeros((max(ne, 1), 6, 3)), "xp": np.zeros((nk, 6)), "xl": np.zeros((npt, 3))}
    out["status"] = lib().lbm_step(*_graph_args(a), float(lam), sum_order, *[_p(out[k]) for k in
                                                                           ("Hpp", "bp", "Hll", "bl", "Hpl", "xp", "xl")])
    out["Hpl"] = out["Hpl"][:ne]
    return out


def pose7(p12) -> np.ndarray:
    out = np.zeros(7)
    p = np.ascontiguousarray(p12, np.float32).reshape(12)
    lib().lbm_pose_from_float(_p(p), _p(out))
    return out


def pose_matrix(p7) -> np.ndarray:
    out, p = np.zeros(12), np.ascontiguousarray(p7, np.float64)
    lib().lbm_pose_to_matrix(_p(p), _p(out))
    return out


def exp_update(x6, p7) -> np.ndarray:
    out, x, p = np.zeros(7), np.ascontiguousarray(x6, np.float64), np.ascontiguousarray(p7, np.float64)
    lib().lbm_exp_update(_p(x), _p(p), _p(out))
    return out


def edge(p7, K4, X, obs, inv_sigma2):
    """e (2,), chi2, A (2, 3), B (2, 6) of one edge."""
    p, K, X, obs = (np.ascontiguousarray(v, np.float64) for v in (p7, K4, X, obs))
    e, c, A, B = np.zeros(2), ctypes.c_double(0), np.zeros((2, 3)), np.zeros((2, 6))
    lib().lbm_edge(_p(p), _p(K), _p(X), _p(obs), float(inv_sigma2), _p(e), ctypes.addressof(c), _p(A), _p(B))
    return e, c.value, A, B


def erase_walk(edge_pt, pt_nobs, chi2, depth, erased, bad, rnd):
    """One classification on the given tables; returns (erased, bad, nobs) after it."""
    ept = np.ascontiguousarray(edge_pt, np.int32)
    nobs = np.ascontiguousarray(pt_nobs, np.int32).copy()
    c, d = np.ascontiguousarray(chi2, np.float64), np.ascontiguousarray(depth, np.float64)
    er, bd = np.ascontiguousarray(erased, np.uint8).copy(), np.ascontiguousarray(bad, np.uint8).copy()
    lib().lbm_erase_walk(len(ept), _p(ept), _p(nobs), _p(c), _p(d), _p(er), _p(bd), int(rnd))
    return er, bd, nobs


def cholesky_solve(S, b):
    S, b = np.ascontiguousarray(S, np.float64), np.ascontiguousarray(b, np.float64)
    x = np.zeros(len(b))
    ok = lib().lbm_cholesky_solve(len(b), _p(S), _p(b), _p(x))
    return bool(ok), x


def decisive(res, depth_scale) -> bool:
    """Every chi2 and depth that a classification read lies at least FLAG_MARGIN from its threshold."""
    c, d = res["chi2"], res["depth"]
    with np.errstate(invalid="ignore"):
        near = (np.abs(c - CHI2_TH) < FLAG_MARGIN * CHI2_TH) | (np.abs(d) < FLAG_MARGIN * depth_scale)
    return not bool(near.any())
