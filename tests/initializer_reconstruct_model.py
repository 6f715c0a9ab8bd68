"""ctypes loader of the CPU model of the Initializer's reconstruction
(tests/native/initializer_reconstruct_model.cpp, built to build/libinitializer_reconstruct_model.so
by __graft_entry__.build()): ReconstructF / ReconstructH, CheckRT, Triangulate and DecomposeE with
the OpenCV 2.4 expressions they use as read.  `initialize` puts the model of Initialize up to RH
(tests/initializer_ransac_model.py) in front of it, as Initializer::Initialize does."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np

import initializer_model as check_model
import initializer_ransac_model as ransac_model
from initializer_ransac_model import same_bits  # noqa: F401

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB = ROOT / "build" / "libinitializer_reconstruct_model.so"
_lib = None
f32 = np.float32
# compared with no tolerance (NaN as "is NaN"); parallax_deg has the recorded acosf bound
EXACT_KEYS = ("ok", "R21", "t21", "P3D", "triangulated", "n_motion", "motion_R", "motion_t", "n_good", "cos_parallax",
              "best", "n_inliers")


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
            sys.path.insert(0, str(ROOT))
            import __graft_entry__ as ge

            LIB.parent.mkdir(exist_ok=True)
            subprocess.run(ge.INITIALIZER_RECONSTRUCT_MODEL_CMD(LIB), check=True)
        _lib = ctypes.CDLL(str(LIB))
        vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        _lib.initializer_reconstruct_model_rule_f.restype = i
        _lib.initializer_reconstruct_model_rule_f.argtypes = [vp, vp, i, f, i]
        _lib.initializer_reconstruct_model_rule_h.restype = i
        _lib.initializer_reconstruct_model_rule_h.argtypes = [vp, vp, i, f, i]
        _lib.initializer_reconstruct_model_triangulate.restype = None
        _lib.initializer_reconstruct_model_triangulate.argtypes = [vp] * 5
        _lib.initializer_reconstruct_model_decompose_e.restype = None
        _lib.initializer_reconstruct_model_decompose_e.argtypes = [vp] * 4
        _lib.initializer_reconstruct_model_motions.restype = i
        _lib.initializer_reconstruct_model_motions.argtypes = [vp, i, vp, vp, vp, vp]
        _lib.initializer_reconstruct_model.restype = i
        _lib.initializer_reconstruct_model.argtypes = [vp, i, vp, i, vp, vp, i, vp, vp, f, f, i, i] + [vp] * 16
    return _lib


def _p(a):
    return ctypes.c_void_p(None if a is None else a.ctypes.data)


def rule_f(n_good, parallax, N, min_parallax=1.0, min_triangulated=50) -> int:
    """ReconstructF's acceptance rule on tables of 4: the chosen hypothesis or -1."""
    g, p = np.ascontiguousarray(n_good, np.int32), np.ascontiguousarray(parallax, f32)
    assert len(g) == 4 and len(p) == 4
    return lib().initializer_reconstruct_model_rule_f(_p(g), _p(p), int(N), float(min_parallax), int(min_triangulated))


def rule_h(n_good, parallax, N, min_parallax=1.0, min_triangulated=50) -> int:
    """ReconstructH's acceptance rule on tables of 8: the chosen hypothesis or -1."""
    g, p = np.ascontiguousarray(n_good, np.int32), np.ascontiguousarray(parallax, f32)
    assert len(g) == 8 and len(p) == 8
    return lib().initializer_reconstruct_model_rule_h(_p(g), _p(p), int(N), float(min_parallax), int(min_triangulated))


def triangulate(kp1, kp2, P1, P2) -> np.ndarray:
    a = [np.ascontiguousarray(x, f32).reshape(-1) for x in (kp1, kp2, P1, P2)]
    x = np.zeros(3, f32)
    lib().initializer_reconstruct_model_triangulate(*[_p(v) for v in a], _p(x))
    return x


def decompose_e(E):
    E = np.ascontiguousarray(E, f32).reshape(9)
    R1, R2, t = np.zeros(9, f32), np.zeros(9, f32), np.zeros(3, f32)
    lib().initializer_reconstruct_model_decompose_e(_p(E), _p(R1), _p(R2), _p(t))
    return R1.reshape(3, 3), R2.reshape(3, 3), t


def motions(M21, use_h, K4):
    """n_motion, R (8, 3, 3), t (8, 3) and, for H, the three singular values."""
    M = np.ascontiguousarray(M21, f32).reshape(9)
    K4 = np.ascontiguousarray(K4, f32)
    R, t, d = np.zeros((8, 3, 3), f32), np.zeros((8, 3), f32), np.zeros(3, f32)
    n = lib().initializer_reconstruct_model_motions(_p(M), int(bool(use_h)), _p(K4), _p(R), _p(t), _p(d))
    return n, R, t, d


def reconstruct(kps1, kps2, matches12, M21, use_h, inliers, K4, sigma=1.0, min_parallax=1.0, min_triangulated=50,
                acos_variant=0) -> dict:
    """The model's answer in the shape of InitializerRansac.reconstruct, plus hyp_P3D (8, n1, 3),
    hyp_good (8, n1) and hyp_err (8, n1, 2): vP3D, vbGood and the squared reprojection errors of every
    hypothesis.  acos_variant: +1 / -1 move acosf's result by one ulp, 2 drops the reprojection's
    fused multiply-adds."""
    k1, k2 = check_model.xy(kps1), check_model.xy(kps2)
    m12 = np.ascontiguousarray(matches12, np.int32)
    n1 = len(k1)
    assert len(m12) == n1
    M = np.ascontiguousarray(M21, f32).reshape(9)
    K4 = np.ascontiguousarray(K4, f32)
    inl = np.zeros(max(n1, 1), np.uint8)
    src = np.asarray(inliers).astype(np.uint8).reshape(-1)
    inl[:len(src)] = src
    o = dict(ok=np.zeros(1, np.int32), R21=np.zeros((3, 3), f32), t21=np.zeros(3, f32), P3D=np.zeros((n1, 3), f32),
             triangulated=np.zeros(n1, np.uint8), n_motion=np.zeros(1, np.int32), motion_R=np.zeros((8, 3, 3), f32),
             motion_t=np.zeros((8, 3), f32), n_good=np.zeros(8, np.int32), cos_parallax=np.zeros(8, f32),
             parallax_deg=np.zeros(8, f32), best=np.zeros(1, np.int32), n_inliers=np.zeros(1, np.int32),
             hyp_P3D=np.zeros((8, n1, 3), f32), hyp_good=np.zeros((8, n1), np.uint8),
             hyp_err=np.zeros((8, n1, 2), f32))
    st = lib().initializer_reconstruct_model(
        _p(k1), n1, _p(k2), len(k2), _p(m12), _p(M), int(bool(use_h)), _p(inl), _p(K4), float(sigma),
        float(min_parallax), int(min_triangulated), int(acos_variant), *[_p(v) for v in o.values()])
    if st:
        raise ValueError(f"initializer reconstruct model: status {st}")
    for k in ("ok", "n_motion", "best", "n_inliers"):
        o[k] = int(o[k][0])
    o["ok"] = bool(o["ok"])
    o["triangulated"] = o["triangulated"].astype(bool)
    o["hyp_good"] = o["hyp_good"].astype(bool)
    return o


def initialize(kps1, kps2, matches12, rand31, K4, sigma=1.0, min_parallax=1.0, min_triangulated=50) -> dict:
    """Initializer::Initialize: find, then ReconstructH or ReconstructF by use_h."""
    r = ransac_model.find(kps1, kps2, matches12, rand31, sigma)
    use_h = r["use_h"]
    rec = reconstruct(kps1, kps2, matches12, r["H"] if use_h else r["F"], use_h,
                      r["inliers_h"] if use_h else r["inliers_f"], K4, sigma, min_parallax, min_triangulated)
    r.update(rec)
    return r


def same_reconstruction(got: dict, want: dict, parallax_bound: float) -> None:
    """Every exact key bit for bit (NaN as "is NaN"), parallax_deg within the recorded bound."""
    for k in EXACT_KEYS:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            assert same_bits(np.asarray(g).astype(w.dtype), w), (k, g, w)
        else:
            assert g == w, (k, g, w)
    g, w = np.asarray(got["parallax_deg"], np.float64), np.asarray(want["parallax_deg"], np.float64)
    nan = np.isnan(w)
    assert np.all(np.isnan(g[nan])) and np.all(np.abs(g[~nan] - w[~nan]) <= parallax_bound), ("parallax_deg", g, w)
