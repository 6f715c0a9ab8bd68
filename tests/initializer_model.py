"""ctypes loader of the CPU model of the Initializer checks (tests/native/initializer_model.cpp,
built to build/libinitializer_model.so by __graft_entry__.build()).  Python has no fmaf, so the
model that restates Initializer::CheckHomography / CheckFundamental and the best-of loops is C++."""
import ctypes
import pathlib
import subprocess
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
LIB = ROOT / "build" / "libinitializer_model.so"
_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        if not LIB.exists():  # build() makes it; a tree that skipped build() compiles it here (g++, seconds)
            sys.path.insert(0, str(ROOT))
            import __graft_entry__ as ge

            LIB.parent.mkdir(exist_ok=True)
            subprocess.run(ge.INITIALIZER_MODEL_CMD(LIB), check=True)
        _lib = ctypes.CDLL(str(LIB))
        vp, i = ctypes.c_void_p, ctypes.c_int
        _lib.initializer_model_check.restype = i
        _lib.initializer_model_check.argtypes = [vp, i, vp, i, vp, ctypes.c_float, i] + [vp] * 14
    return _lib


def _p(a):
    return ctypes.c_void_p(None if a is None else a.ctypes.data)


def xy(kps) -> np.ndarray:
    """(n, 2) float32 pt.x, pt.y of a keypoint record array (or of an (n, 2) array)."""
    kps = np.asarray(kps)
    if kps.dtype.names:
        return np.ascontiguousarray(np.stack([kps["x"], kps["y"]], 1).astype(np.float32)).reshape(-1, 2)
    return np.ascontiguousarray(kps, np.float32).reshape(-1, 2)


def check(kps1, kps2, matches12, sigma, H21=None, H12=None, F21=None, terms=False) -> dict:
    """The model's answer in the shape of orbslam_jpminipc_amd.Initializer.check (plus terms_h /
    terms_f (n_hyp, 2 N): the accepted terms in add order, 0 where rejected, when `terms`)."""
    k1, k2 = xy(kps1), xy(kps2)
    m12 = np.ascontiguousarray(matches12, np.int32)
    assert len(m12) == len(k1)
    hyp = [None if a is None else np.ascontiguousarray(a, np.float32).reshape(-1, 9) for a in (H21, H12, F21)]
    n_hyp = next(len(a) for a in hyp if a is not None)
    n1 = len(k1)
    sc = np.zeros((2, n_hyp), np.float32)
    best = np.full(2, -1, np.int32)
    bs = np.zeros(2, np.float32)
    inl = np.zeros((2, max(n1, 1)), np.uint8)
    nm = np.zeros(1, np.int32)
    tm = np.zeros((2, n_hyp, 2 * max(n1, 1)), np.float32) if terms else None
    r = lib().initializer_model_check(_p(k1), n1, _p(k2), len(k2), _p(m12), float(sigma), n_hyp, _p(hyp[0]), _p(hyp[1]),
                                      _p(hyp[2]), _p(sc[0]), _p(sc[1]), _p(best[0:]), _p(bs[0:]), _p(inl[0]),
                                      _p(best[1:]), _p(bs[1:]), _p(inl[1]), _p(nm), _p(tm[0]) if terms else None,
                                      _p(tm[1]) if terms else None)
    if r:
        raise ValueError(f"initializer model: status {r}")
    N = int(nm[0])
    out = {"n_matches": N, "RH": None}
    if hyp[0] is not None:
        out.update(scores_h=sc[0].copy(), best_h=int(best[0]), best_score_h=np.float32(bs[0]),
                   inliers_h=inl[0, :N].astype(bool))
        if terms:
            out["terms_h"] = tm[0, :, :2 * N].copy()
    if hyp[2] is not None:
        out.update(scores_f=sc[1].copy(), best_f=int(best[1]), best_score_f=np.float32(bs[1]),
                   inliers_f=inl[1, :N].astype(bool))
        if terms:
            out["terms_f"] = tm[1, :, :2 * N].copy()
    if hyp[0] is not None and hyp[2] is not None:
        with np.errstate(invalid="ignore", divide="ignore"):
            out["RH"] = np.float32(bs[0]) / (np.float32(bs[0]) + np.float32(bs[1]))
    return out


def same_scores(got, want) -> bool:
    """Bitwise where the model's score is not NaN, "is NaN" where it is (NaN bit patterns differ
    between x86 and the GPU)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return (got.shape == want.shape and bool(np.all(np.isnan(got[nan])))
            and got[~nan].tobytes() == want[~nan].tobytes())


def same_result(got: dict, want: dict) -> None:
    """Asserts that two check() results agree in every field both hold."""
    assert got["n_matches"] == want["n_matches"]
    for t in "hf":
        if "scores_" + t not in want:
            assert "scores_" + t not in got
            continue
        assert same_scores(got["scores_" + t], want["scores_" + t]), t
        assert got["best_" + t] == want["best_" + t], (t, got["best_" + t], want["best_" + t])
        assert np.float32(got["best_score_" + t]).tobytes() == np.float32(want["best_score_" + t]).tobytes(), t
        assert np.array_equal(got["inliers_" + t], want["inliers_" + t]), t
