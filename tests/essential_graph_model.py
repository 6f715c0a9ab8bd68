"""ctypes loader of build/libessential_graph_model.so (tests/native/essential_graph_model.cpp): the CPU
model of Optimizer::OptimizeEssentialGraph that the GPU tests compare against, and of
build/libg2o_sim3_host.so (the Sim3 part of csrc/orb_g2o_math.h compiled for the host)."""
from __future__ import annotations

import ctypes
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB_PATH = ROOT / "build" / "libessential_graph_model.so"
HOST_PATH = ROOT / "build" / "libg2o_sim3_host.so"

MAX_TRIALS = 200
EINVAL, ENOTSUP = -22, -95
MAX_PROFILE_BYTES = 256 << 20
# every evaluation of log() keeps this relative distance from its two eps tests, and every trial of a
# case whose counters are compared exactly this relative distance between chi2 and the trial's chi2
LOG_MARGIN = 1e-3
TRIAL_MARGIN = 1e-9
# ... which says something only while chi2 stands above its own rounding: an error entry carries about
# 1e-15 (1e-16 of pose entries of size 5 to 10 through a handful of products), so a chi2 of c over n edges
# carries about 2e-15 sqrt(n c), and that stays under TRIAL_MARGIN c only for c > 4e-12 n.  1e-8 covers the
# 1285 edges of the largest listed case.
TRIAL_CHI2_FLOOR = 1e-8
SEQUENTIAL, PAIRWISE, REVERSED = 0, 1, 2
DENSE, PROFILE = 0, 1
# the mutants of DESIGN.md §22
V_KIND_IGNORED, V_MEAS_SWAPPED, V_LAMBDA_DIAG, V_FIXED_BLOCK, V_T_NOT_DIVIDED, V_LOG_SWAPPED, V_SECOND_VSCW = range(1, 8)


class Info(ctypes.Structure):
    """orb_essential_graph_info_t (include/orb_abi.h)."""

    _fields_ = [("status", ctypes.c_int32), ("n_active", ctypes.c_int32), ("n_free", ctypes.c_int32),
                ("n_edges", ctypes.c_int32), ("profile_bytes", ctypes.c_int64), ("iterations", ctypes.c_int32),
                ("trials", ctypes.c_int32), ("refused", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("lambda_", ctypes.c_double), ("chi2_before", ctypes.c_double), ("chi2_after", ctypes.c_double),
                ("trial_rho", ctypes.c_double * MAX_TRIALS), ("trial_chi2", ctypes.c_double * MAX_TRIALS),
                ("trial_accepted", ctypes.c_uint8 * MAX_TRIALS)]

    def as_dict(self) -> dict:
        n = min(self.trials, MAX_TRIALS)
        return {"status": self.status, "n_active": self.n_active, "n_free": self.n_free, "n_edges": self.n_edges,
                "profile_bytes": self.profile_bytes, "iterations": self.iterations, "trials": self.trials,
                "refused": self.refused, "lambda": self.lambda_, "chi2_before": self.chi2_before,
                "chi2_after": self.chi2_after, "trial_rho": list(self.trial_rho[:n]),
                "trial_chi2": list(self.trial_chi2[:n]), "trial_accepted": [int(v) for v in self.trial_accepted[:n]]}


class Margins(ctypes.Structure):
    _fields_ = [("sigma", ctypes.c_double), ("d", ctypes.c_double), ("trial", ctypes.c_double),
                ("min_chi2", ctypes.c_double), ("branch", ctypes.c_int64 * 4)]


_vp, _i = ctypes.c_void_p, ctypes.c_int
_libs = {}


def lib(path=LIB_PATH):
    if path not in _libs:
        L = ctypes.CDLL(str(path))
        L.eg_model_run.restype = _i
        L.eg_model_run.argtypes = [_i] + [_vp] * 6 + [_i, _vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i] + [_vp] * 7
        L.eg_model_log.restype = _i
        L.eg_model_log.argtypes = [_vp, _vp, _i]
        for name, n in (("eg_model_exp", 2), ("eg_model_from_pose", 2), ("eg_model_to_pose", 2), ("eg_model_mul", 3),
                        ("eg_model_inverse", 2), ("eg_model_edge", 6)):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [_vp] * n
        L.eg_model_correct_points.restype = None
        L.eg_model_correct_points.argtypes = [_i] + [_vp] * 6
        _libs[path] = L
    return _libs[path]


def host(path=HOST_PATH):
    if path not in _libs:
        L = ctypes.CDLL(str(path))
        for name, n in (("s3h_from_pose", 2), ("s3h_to_pose", 2), ("s3h_mul", 3), ("s3h_inverse", 2), ("s3h_map", 3),
                        ("s3h_lu3_solve", 3)):
            getattr(L, name).restype = None
            getattr(L, name).argtypes = [_vp] * n
        L.s3h_log.restype = _i
        L.s3h_log.argtypes = [_vp, _vp]
        _libs[path] = L
    return _libs[path]


def _p(a):
    return None if a is None else a.ctypes.data


def _d(v, n=None):
    a = np.ascontiguousarray(v, np.float64)
    assert n is None or a.size == n
    return a


def graph_arrays(g: dict) -> dict:
    """The graph `g` as the contiguous arrays of the C interfaces (missing tables: None)."""
    nk = len(g["kf_pose"])
    out = {"kf_pose": np.ascontiguousarray(g["kf_pose"], np.float32).reshape(-1, 12),
           "kf_fixed": np.ascontiguousarray(g["kf_fixed"], np.uint8).reshape(-1),
           "edge_i": np.ascontiguousarray(g["edge_i"], np.int32).reshape(-1),
           "edge_j": np.ascontiguousarray(g["edge_j"], np.int32).reshape(-1),
           "edge_kind": np.ascontiguousarray(g["edge_kind"], np.uint8).reshape(-1),
           "pt_pos": np.ascontiguousarray(g.get("pt_pos", np.zeros((0, 3))), np.float32).reshape(-1, 3),
           "pt_ref": np.ascontiguousarray(g.get("pt_ref", np.zeros(0)), np.int32).reshape(-1)}
    for t, f in (("kf_corrected", "kf_has_corrected"), ("kf_noncorrected", "kf_has_noncorrected")):
        if g.get(t) is None:
            out[t] = out[f] = None
        else:
            out[t] = np.ascontiguousarray(g[t], np.float64).reshape(nk, 8)
            out[f] = np.ascontiguousarray(g[f], np.uint8).reshape(nk)
    out["pt_skip"] = None if g.get("pt_skip") is None else np.ascontiguousarray(g["pt_skip"], np.uint8).reshape(-1)
    assert len(out["kf_fixed"]) == nk and len(out["edge_j"]) == len(out["edge_kind"]) == len(out["edge_i"])
    assert len(out["pt_ref"]) == len(out["pt_pos"])
    return out


def run(g, n_iterations=20, sum_order=SEQUENTIAL, variant=0, solver=PROFILE, path=LIB_PATH) -> dict:
    """The model's answer: status, kf_sim3 (n_kf, 8), kf_pose (n_kf, 12) float32, kf_pose_f64, pt_pos
    (n_pt, 3) float32 (a skipped point: its input), pt_pos_f64, info and margins (sigma, d, trial: the
    smallest relative distances met; branch: log() evaluations per branch)."""
    a = graph_arrays(g)
    nk, ne, npt = len(a["kf_pose"]), len(a["edge_i"]), len(a["pt_pos"])
    out = {"kf_sim3": np.zeros((nk, 8)), "kf_pose": np.zeros((nk, 12), np.float32), "kf_pose_f64": np.zeros((nk, 12)),
           "pt_pos": a["pt_pos"].copy(), "pt_pos_f64": a["pt_pos"].astype(np.float64)}
    info, m = Info(), Margins()
    out["status"] = lib(path).eg_model_run(
        nk, _p(a["kf_pose"]), _p(a["kf_corrected"]), _p(a["kf_has_corrected"]), _p(a["kf_noncorrected"]),
        _p(a["kf_has_noncorrected"]), _p(a["kf_fixed"]), ne, _p(a["edge_i"]), _p(a["edge_j"]), _p(a["edge_kind"]), npt,
        _p(a["pt_pos"]), _p(a["pt_ref"]), _p(a["pt_skip"]), int(n_iterations), int(sum_order), int(variant), int(solver),
        _p(out["kf_sim3"]), _p(out["kf_pose"]), _p(out["kf_pose_f64"]), _p(out["pt_pos"]), _p(out["pt_pos_f64"]),
        ctypes.addressof(info), ctypes.addressof(m))
    out["info"] = info.as_dict()
    out["margins"] = {"sigma": m.sigma, "d": m.d, "trial": m.trial, "min_chi2": m.min_chi2, "branch": list(m.branch)}
    return out


def decisive_log(res) -> bool:
    """Every evaluation of log() kept LOG_MARGIN from both eps tests."""
    return res["margins"]["sigma"] >= LOG_MARGIN and res["margins"]["d"] >= LOG_MARGIN


def decisive_trials(res) -> bool:
    """Every trial's chi2 differs from the chi2 it is compared with by TRIAL_MARGIN, relative, and both
    stand above TRIAL_CHI2_FLOOR."""
    return res["margins"]["trial"] >= TRIAL_MARGIN and res["margins"]["min_chi2"] >= TRIAL_CHI2_FLOOR


def exp(u) -> np.ndarray:
    out, u = np.zeros(8), _d(u, 7)
    lib().eg_model_exp(_p(u), _p(out))
    return out


def log(s, variant=0):
    """(log (7,), branch) of a Sim3: branch bit 0 |sigma| >= eps, bit 1 d <= 1 - eps."""
    out, s = np.zeros(7), _d(s, 8)
    br = lib().eg_model_log(_p(s), _p(out), variant)
    return out, br


def from_pose(p12) -> np.ndarray:
    out, p = np.zeros(8), np.ascontiguousarray(p12, np.float32).reshape(12)
    lib().eg_model_from_pose(_p(p), _p(out))
    return out


def to_pose(s) -> np.ndarray:
    out, s = np.zeros(12), _d(s, 8)
    lib().eg_model_to_pose(_p(s), _p(out))
    return out


def mul(a, b) -> np.ndarray:
    out, a, b = np.zeros(8), _d(a, 8), _d(b, 8)
    lib().eg_model_mul(_p(a), _p(b), _p(out))
    return out


def inverse(a) -> np.ndarray:
    out, a = np.zeros(8), _d(a, 8)
    lib().eg_model_inverse(_p(a), _p(out))
    return out


def edge(C, vi, vj):
    """err (7,), Ji (7, 7), Jj (7, 7) of one EdgeSim3 with both vertices free."""
    C, vi, vj = _d(C, 8), _d(vi, 8), _d(vj, 8)
    err, Ji, Jj = np.zeros(7), np.zeros((7, 7)), np.zeros((7, 7))
    lib().eg_model_edge(_p(C), _p(vi), _p(vj), _p(err), _p(Ji), _p(Jj))
    return err, Ji, Jj


def correct_points(pt_pos, pt_pair, sim3_from, sim3_to):
    """(float32 (n, 3), float64 (n, 3)): to[pair]^-1.map(from[pair].map(P))."""
    pp = np.ascontiguousarray(pt_pos, np.float32).reshape(-1, 3)
    pr = np.ascontiguousarray(pt_pair, np.int32).reshape(-1)
    sf, st = _d(sim3_from).reshape(-1, 8), _d(sim3_to).reshape(-1, 8)
    o32, o64 = np.zeros((len(pp), 3), np.float32), np.zeros((len(pp), 3))
    lib().eg_model_correct_points(len(pp), _p(pp), _p(pr), _p(sf), _p(st), _p(o32), _p(o64))
    return o32, o64
