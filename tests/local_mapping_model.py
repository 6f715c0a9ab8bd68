"""ctypes loader of the CPU model of LocalMapping::CreateNewMapPoints, ComputeF12,
ComputeSceneMedianDepth and MapPoint::UpdateNormalAndDepth (tests/native/local_mapping_model.cpp, built
to build/liblocal_mapping_model.so by __graft_entry__.build()), with the OpenCV 2.4 expressions they use
as read."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB = ROOT / "build" / "liblocal_mapping_model.so"
_lib = None
f32 = np.float32
# compared with no tolerance (NaN as "is NaN")
EXACT_KEYS = ("x3d", "status", "cos_rays", "n_new", "new_idx1", "new_idx2", "skipped", "median_depth")


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
            sys.path.insert(0, str(ROOT))
            import __graft_entry__ as ge

            LIB.parent.mkdir(exist_ok=True)
            subprocess.run(ge.LOCAL_MAPPING_MODEL_CMD(LIB), check=True)
        _lib = ctypes.CDLL(str(LIB))
        vp, i = ctypes.c_void_p, ctypes.c_int
        _lib.local_mapping_model_compute_f12.restype = None
        _lib.local_mapping_model_compute_f12.argtypes = [vp] * 7
        _lib.local_mapping_model_center.restype = None
        _lib.local_mapping_model_center.argtypes = [vp, vp]
        _lib.local_mapping_model_median.restype = i
        _lib.local_mapping_model_median.argtypes = [vp, vp, vp, i, i, vp]
        _lib.local_mapping_model_triangulate4.restype = i
        _lib.local_mapping_model_triangulate4.argtypes = [vp] * 5
        _lib.local_mapping_model_create.restype = i
        _lib.local_mapping_model_create.argtypes = ([vp, vp, i, vp, vp, i] + [vp] * 9 + [i, vp, vp, i, vp, vp, i] + [vp] * 9)
        _lib.local_mapping_model_update_normal_and_depth.restype = None
        _lib.local_mapping_model_update_normal_and_depth.argtypes = [i] + [vp] * 6 + [i] + [vp] * 3
    return _lib


def _p(a):
    return ctypes.c_void_p(None if a is None else a.ctypes.data)


def same_bits(a, b) -> bool:
    """Equal bit for bit, except that a NaN equals any NaN."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))


def pose12(V) -> np.ndarray:
    """Rcw row-major, then tcw: the 12 floats the batch form takes per keyframe."""
    return np.ascontiguousarray(np.concatenate([V.Rcw.reshape(9), V.tcw.reshape(3)]).astype(f32))


def K4(V) -> np.ndarray:
    return np.array([V.fx, V.fy, V.cx, V.cy], f32)


def center(pose) -> np.ndarray:
    """GetCameraCenter as the batch form computes it: -Rcw.t()*tcw, one gemm with alpha = -1."""
    T = np.ascontiguousarray(pose, f32).reshape(12)
    O = np.zeros(3, f32)
    lib().local_mapping_model_center(_p(T), _p(O))
    return O


def compute_f12(V1, V2) -> np.ndarray:
    a = [np.ascontiguousarray(x, f32).reshape(-1) for x in (V1.Rcw, V1.tcw, V2.Rcw, V2.tcw, K4(V1), K4(V2))]
    F = np.zeros((3, 3), f32)
    lib().local_mapping_model_compute_f12(*[_p(v) for v in a], _p(F))
    return F


def median(V, mp_pos, has_mp, q=2):
    """(sorted depths[(n - 1) / q] or NaN, the number of depths)."""
    T = pose12(V)
    pos = np.ascontiguousarray(mp_pos, f32).reshape(-1, 3)
    has = np.ascontiguousarray(has_mp, np.uint8).reshape(-1)
    d = np.zeros(1, f32)
    n = lib().local_mapping_model_median(_p(T), _p(pos), _p(has), len(has), int(q), _p(d))
    return d[0], n


def triangulate4(xn1, xn2, Tcw1, Tcw2):
    """The Euclidean point of lines 310-325 from two normalised points and two 3 x 4 poses, or None
    when the fourth coordinate is 0."""
    a = [np.ascontiguousarray(x, f32).reshape(-1) for x in (xn1, xn2, Tcw1, Tcw2)]
    x = np.zeros(3, f32)
    ok = lib().local_mapping_model_triangulate4(*[_p(v) for v in a], _p(x))
    return x if ok else None


def create(V1, V2, match12, mp_pos2=None, has_mp2=None, variant=0, Ow1=None, Ow2=None) -> dict:
    """The model's answer in the shape of LocalMapping.triangulate, plus dbg (n1, 6): the two squared
    reprojection errors, ratioDist, ratioOctave, z1, z2.  Ow1 / Ow2 default to the views' own centres
    (the host form); the batch form's are center(pose12(V)).  variant 2 drops the fused multiply-adds."""
    n1, n2 = V1.n, V2.n
    k1 = np.ascontiguousarray(np.stack([V1.kps["x"], V1.kps["y"]], 1).astype(f32))
    k2 = np.ascontiguousarray(np.stack([V2.kps["x"], V2.kps["y"]], 1).astype(f32))
    o1 = np.ascontiguousarray(V1.kps["octave"].astype(np.int32))
    o2 = np.ascontiguousarray(V2.kps["octave"].astype(np.int32))
    m12 = np.ascontiguousarray(match12, np.int32)
    assert len(m12) == n1
    T1, T2 = pose12(V1), pose12(V2)
    O1 = np.ascontiguousarray(V1.Ow if Ow1 is None else Ow1, f32)
    O2 = np.ascontiguousarray(V2.Ow if Ow2 is None else Ow2, f32)
    Ka, Kb = K4(V1), K4(V2)
    sf1, s21 = np.ascontiguousarray(V1.mvScaleFactors, f32), np.ascontiguousarray(V1.mvLevelSigma2, f32)
    sf2, s22 = np.ascontiguousarray(V2.mvScaleFactors, f32), np.ascontiguousarray(V2.mvLevelSigma2, f32)
    pos = has = None
    if mp_pos2 is not None:
        pos = np.ascontiguousarray(mp_pos2, f32).reshape(-1, 3)
        has = np.ascontiguousarray(has_mp2, np.uint8).reshape(-1)
        assert len(pos) == n2 and len(has) == n2
    m = max(n1, 1)
    o = dict(x3d=np.zeros((m, 3), f32), status=np.zeros(m, np.uint8), cos_rays=np.zeros(m, f32),
             n_new=np.zeros(1, np.int32), new_idx1=np.zeros(m, np.int32), new_idx2=np.zeros(m, np.int32),
             skipped=np.zeros(1, np.int32), median_depth=np.zeros(1, f32), dbg=np.zeros((m, 6), f32))
    st = lib().local_mapping_model_create(_p(k1), _p(o1), n1, _p(k2), _p(o2), n2, _p(m12), _p(T1), _p(O1), _p(T2), _p(O2),
                                          _p(Ka), _p(Kb), _p(sf1), _p(s21), V1.nlevels, _p(sf2), _p(s22), V2.nlevels,
                                          _p(pos), _p(has), int(variant), *[_p(v) for v in o.values()])
    if st:
        raise ValueError(f"local mapping model: status {st}")
    n = int(o["n_new"][0])
    o.update(n_new=n, skipped=int(o["skipped"][0]), median_depth=float(o["median_depth"][0]))
    for k in ("x3d", "status", "cos_rays", "dbg"):
        o[k] = o[k][:n1]
    o["new_idx1"], o["new_idx2"] = o["new_idx1"][:n], o["new_idx2"][:n]
    return o


def update_normal_and_depth(offsets, obs_Ow, pos, ref_Ow, ref_level, scale_factors):
    off = np.ascontiguousarray(offsets, np.int32)
    M = len(off) - 1
    ow = np.ascontiguousarray(obs_Ow, f32).reshape(-1, 3)
    p, ro = np.ascontiguousarray(pos, f32).reshape(-1, 3), np.ascontiguousarray(ref_Ow, f32).reshape(-1, 3)
    lv, sf = np.ascontiguousarray(ref_level, np.int32), np.ascontiguousarray(scale_factors, f32)
    normal, dmin, dmax = np.zeros((M, 3), f32), np.zeros(M, f32), np.zeros(M, f32)
    lib().local_mapping_model_update_normal_and_depth(M, _p(off), _p(ow), _p(p), _p(ro), _p(lv), _p(sf), len(sf),
                                                      _p(normal), _p(dmin), _p(dmax))
    return normal, dmin, dmax


def same_result(got: dict, want: dict) -> None:
    """Every output bit for bit (NaN as "is NaN")."""
    for k in EXACT_KEYS:
        g, w = got[k], want[k]
        if isinstance(w, np.ndarray):
            assert same_bits(np.asarray(g).astype(w.dtype), w), (k, g, w)
        elif isinstance(w, float):
            assert same_bits(np.float32(g), np.float32(w)), (k, g, w)
        else:
            assert g == w, (k, g, w)
