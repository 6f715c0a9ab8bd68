"""ctypes loader of the CPU model of the Initializer's hypothesis generation
(tests/native/initializer_ransac_model.cpp, built to build/libinitializer_ransac_model.so by
__graft_entry__.build()): the minimal sets, Normalize, ComputeH21 / ComputeF21 with OpenCV 2.4's
SVDecomp, inv() and 3x3 products as read.  `find` puts the model of the two checks
(tests/initializer_model.py) behind it, as Initializer::Initialize does."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np

import initializer_model as check_model

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB = ROOT / "build" / "libinitializer_ransac_model.so"
_lib = None
f32 = np.float32
HYP_KEYS = ("H21", "H12", "F21", "Hn", "Fn", "Fpre")


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
            sys.path.insert(0, str(ROOT))
            import __graft_entry__ as ge

            LIB.parent.mkdir(exist_ok=True)
            subprocess.run(ge.INITIALIZER_RANSAC_MODEL_CMD(LIB), check=True)
        _lib = ctypes.CDLL(str(LIB))
        vp, i = ctypes.c_void_p, ctypes.c_int
        _lib.initializer_ransac_model_sets.restype = i
        _lib.initializer_ransac_model_sets.argtypes = [i, i, vp, vp]
        _lib.initializer_ransac_model_hypotheses.restype = i
        _lib.initializer_ransac_model_hypotheses.argtypes = [vp, i, vp, i, vp, i] + [vp] * 12
        _lib.initializer_ransac_model_compute.restype = i
        _lib.initializer_ransac_model_compute.argtypes = [vp] * 6 + [i]
        _lib.initializer_ransac_model_inv3.restype = None
        _lib.initializer_ransac_model_inv3.argtypes = [vp, vp]
        _lib.initializer_ransac_model_mul3.restype = None
        _lib.initializer_ransac_model_mul3.argtypes = [vp, vp, vp]
        _lib.initializer_ransac_model_svd.restype = None
        _lib.initializer_ransac_model_svd.argtypes = [vp, i, i, vp, vp, vp]
    return _lib


def _p(a):
    return ctypes.c_void_p(None if a is None else a.ctypes.data)


def minimal_sets(N, rand31) -> np.ndarray:
    r = np.ascontiguousarray(rand31, np.int32).reshape(-1, 8)
    sets = np.zeros(r.shape, np.int32)
    st = lib().initializer_ransac_model_sets(int(N), len(r), _p(r), _p(sets))
    if st:
        raise ValueError(f"initializer ransac model: status {st}")
    return sets


def hypotheses(kps1, kps2, matches12, rand31=None, sets=None) -> dict:
    """The model's answer in the shape of InitializerRansac.compute_hypotheses, plus Fpre (the
    fundamental matrix before the rank-2 enforcement)."""
    k1, k2 = check_model.xy(kps1), check_model.xy(kps2)
    m12 = np.ascontiguousarray(matches12, np.int32)
    assert len(m12) == len(k1) and (rand31 is None) != (sets is None)
    draws = np.ascontiguousarray(rand31 if sets is None else sets, np.int32).reshape(-1, 8)
    n_hyp = len(draws)
    out = {k: np.zeros((n_hyp, 9), f32) for k in HYP_KEYS}
    T = np.zeros((2, 9), f32)
    so = np.zeros((n_hyp, 8), np.int32)
    nm = np.zeros(1, np.int32)
    st = lib().initializer_ransac_model_hypotheses(
        _p(k1), len(k1), _p(k2), len(k2), _p(m12), n_hyp, _p(draws if sets is not None else None),
        _p(draws if sets is None else None), *[_p(out[k]) for k in HYP_KEYS], _p(T[0]), _p(T[1]), _p(so), _p(nm))
    if st:
        raise ValueError(f"initializer ransac model: status {st}")
    out.update(n_matches=int(nm[0]), sets=so, T1=T[0].reshape(3, 3), T2=T[1].reshape(3, 3))
    return out


def find(kps1, kps2, matches12, rand31, sigma=1.0) -> dict:
    """Initialize up to RH, in the shape of InitializerRansac.find."""
    h = hypotheses(kps1, kps2, matches12, rand31=rand31)
    r = check_model.check(kps1, kps2, matches12, sigma, h["H21"], h["H12"], h["F21"])
    r.update({k: h[k] for k in ("H21", "H12", "F21", "sets")})
    nan = np.full((3, 3), np.nan, f32)
    r["H"] = h["H21"][r["best_h"]].reshape(3, 3) if r["best_h"] >= 0 else nan
    r["F"] = h["F21"][r["best_f"]].reshape(3, 3) if r["best_f"] >= 0 else nan
    r["RH"] = f32(r["RH"])
    r["use_h"] = bool(np.float64(r["RH"]) > 0.40)  # Initializer.cc:113: the float against the double 0.40
    return r


def compute(p1, p2):
    """ComputeH21 / ComputeF21 on 8 normalised correspondences: Hn, Fn, Fpre (3, 3) and the signs
    the generator handed out inside ComputeF21."""
    p1 = np.ascontiguousarray(p1, f32).reshape(8, 2)
    p2 = np.ascontiguousarray(p2, f32).reshape(8, 2)
    Hn, Fn, Fp = (np.zeros(9, f32) for _ in range(3))
    sg = np.zeros(4096, np.int32)
    n = lib().initializer_ransac_model_compute(_p(p1), _p(p2), _p(Hn), _p(Fn), _p(Fp), _p(sg), len(sg))
    return Hn.reshape(3, 3), Fn.reshape(3, 3), Fp.reshape(3, 3), sg[:min(n, len(sg))].copy()


def inv3(S):
    S = np.ascontiguousarray(S, f32).reshape(9)
    D = np.zeros(9, f32)
    lib().initializer_ransac_model_inv3(_p(S), _p(D))
    return D.reshape(3, 3)


def mul3(a, b):
    a, b = (np.ascontiguousarray(x, f32).reshape(9) for x in (a, b))
    d = np.zeros(9, f32)
    lib().initializer_ransac_model_mul3(_p(a), _p(b), _p(d))
    return d.reshape(3, 3)


def svd(A):
    """cv::SVDecomp(A, w, u, vt, MODIFY_A | FULL_UV) of a float32 matrix."""
    A = np.ascontiguousarray(A, f32)
    r, c = A.shape
    w, u, vt = np.zeros(min(r, c), f32), np.zeros((r, r), f32), np.zeros((c, c), f32)
    lib().initializer_ransac_model_svd(_p(A), r, c, _p(w), _p(u), _p(vt))
    return w, u, vt


def same_bits(got, want) -> bool:
    """Bit for bit where the model's value is not NaN, "is NaN" where it is."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.all(np.isnan(got[nan]))) and got[~nan].tobytes() == want[~nan].tobytes()
