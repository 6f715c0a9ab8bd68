"""The CPU model of the Initializer checks (tests/native/initializer_model.cpp) on cases whose
answer is known by hand, the float-division equality the kernel relies on, the declared surface,
and the committed golden file."""
import pathlib

import numpy as np

import initializer_model as model

ROOT = pathlib.Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden"
f32 = np.float32
TH = f32(5.991)
I3 = np.eye(3, dtype=f32).reshape(1, 9)


def _seq_sum(terms):
    s = f32(0)
    for t in terms:
        s = f32(s + f32(t))
    return s


def test_identity_homography_scores_every_term_in_order():
    rng = np.random.default_rng(1)
    N = 37
    pts = (rng.random((N, 2)) * [320, 240]).astype(f32)
    r = model.check(pts, pts, np.arange(N), 1.0, I3, I3, None, terms=True)
    assert r["n_matches"] == N and r["best_h"] == 0
    assert r["inliers_h"].all() and len(r["inliers_h"]) == N
    want = _seq_sum([TH] * (2 * N))
    assert r["scores_h"][0].tobytes() == want.tobytes() == f32(r["best_score_h"]).tobytes()
    assert (r["terms_h"][0] == TH).all()
    assert r["RH"] is None


def test_shifted_pair_by_hand():
    p1 = np.array([[10.0, 20.0]], f32)
    # homography: identity, the point one pixel to the right: both squared distances are 1
    r = model.check(p1, np.array([[11.0, 20.0]], f32), [0], 1.0, I3, I3, None)
    assert r["scores_h"][0].tobytes() == f32(f32(TH - f32(1)) + f32(TH - f32(1))).tobytes()
    assert r["inliers_h"].tolist() == [True]
    # sigma 0.5: chi = 4 for both terms, still below 5.991
    r = model.check(p1, np.array([[11.0, 20.0]], f32), [0], 0.5, I3, I3, None)
    assert r["scores_h"][0].tobytes() == f32(f32(TH - f32(4)) + f32(TH - f32(4))).tobytes()
    # fundamental matrix of a pure x translation: l2 = (0, -1, v1), distance |v2 - v1| = 1.5
    F = np.array([[0, 0, 0, 0, 0, -1, 0, 1, 0]], f32)
    r = model.check(p1, np.array([[11.0, 21.5]], f32), [0], 1.0, None, None, F)
    t = f32(TH - f32(2.25))
    assert r["scores_f"][0].tobytes() == f32(t + t).tobytes() and r["best_f"] == 0
    assert r["inliers_f"].tolist() == [True]
    # 2 pixels off the line: chi = 4 > 3.841, an outlier in both images; nothing scores above 0
    r = model.check(p1, np.array([[11.0, 22.0]], f32), [0], 1.0, None, None, F)
    assert r["scores_f"][0] == 0 and r["best_f"] == -1 and r["best_score_f"] == 0
    assert r["inliers_f"].tolist() == [False]
    # the same 2 pixels pass the homography's 5.991 (chi = 4)
    r = model.check(p1, np.array([[10.0, 22.0]], f32), [0], 1.0, I3, I3, None)
    assert r["inliers_h"].tolist() == [True]


def test_holes_order_and_first_maximum():
    k1 = np.array([[0, 0], [5, 5], [9, 9], [50, 60]], f32)
    k2 = np.array([[50, 60], [0, 0], [5, 5.5]], f32)
    m12 = [1, 2, -1, 0]  # ordinals 0, 1, 2 <- indices 0, 1, 3
    far = np.array([[1, 0, 1000, 0, 1, 0, 0, 0, 1]], f32)
    near = np.array([[1, 0, -1000, 0, 1, 0, 0, 0, 1]], f32)
    H21 = np.concatenate([far, I3, I3])
    H12 = np.concatenate([near, I3, I3])
    r = model.check(k1, k2, m12, 1.0, H21, H12, None)
    assert r["n_matches"] == 3
    assert r["scores_h"][0] == 0 and r["scores_h"][1] == r["scores_h"][2] > 0
    assert r["best_h"] == 1  # the first of two equal maxima
    assert r["inliers_h"].tolist() == [True, True, True]
    r = model.check(k1, k2, m12, 1.0, far, near, None)
    assert r["best_h"] == -1 and r["best_score_h"] == 0 and r["inliers_h"].tolist() == [False] * 3


def test_nan_and_infinity():
    pts = np.array([[10, 20], [30, 40], [70, 5]], f32)
    m12 = [0, 1, 2]
    Z = np.zeros((1, 9), f32)
    row3zero = np.array([[1, 0, 0, 0, 1, 0, 0, 0, 0]], f32)  # w = 1/0 = inf, distance inf: outliers
    r = model.check(pts, pts, m12, 1.0, row3zero, row3zero, None)
    assert r["scores_h"][0] == 0 and r["best_h"] == -1 and not r["inliers_h"].any()
    # all zero: 0 * inf = NaN, which is not > th: the score is NaN and never wins
    for order in ([Z, I3], [I3, Z]):
        H = np.concatenate(order)
        r = model.check(pts, pts, m12, 1.0, H, H, H)
        nan = 0 if order[0] is Z else 1
        assert np.isnan(r["scores_h"][nan]) and np.isnan(r["scores_f"][nan])
        assert r["best_h"] == 1 - nan and r["inliers_h"].all()
        # F = identity: l = x, num = |x|^2 + 1, far from 0: outliers, score 0; nothing wins
        assert r["scores_f"][1 - nan] == 0 and r["best_f"] == -1 and not r["inliers_f"].any()


def test_invalid_matches_are_refused():
    pts = np.zeros((2, 2), f32)
    for bad in ([0, 2], [-2, 0]):
        try:
            model.check(pts, pts, bad, 1.0, I3, I3, None)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_double_reciprocal_rounded_equals_float_reciprocal():
    """(float)(1.0 / (double)x) == 1.0f / x for float x: double keeps more than 2 * 24 + 2 bits,
    so rounding twice is innocuous.  The reference divides in double, the kernel in float."""
    rng = np.random.default_rng(20240611)
    bits = rng.integers(0, 2**32, 400_000, dtype=np.uint64).astype(np.uint32)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000,
                        0x3F800000, 0x3F800001, 0x3F7FFFFF, 0x7E800000, 0x7EFFFFFF, 0x00400000, 0x00200000], np.uint32)
    x = np.concatenate([bits, special]).view(f32)
    with np.errstate(all="ignore"):
        a = (f32(1.0) / x).astype(f32)
        b = (1.0 / x.astype(np.float64)).astype(f32)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    assert a[~nan].tobytes() == b[~nan].tobytes()


def test_surface_is_declared():
    header = (ROOT / "include" / "orb_abi.h").read_text()
    for name in ("orb_initializer_check", "orb_initializer_check_batch_device"):
        assert f"int {name}(" in header
    from orbslam_jpminipc_amd import Initializer, _native

    assert "orb_initializer_check" in _native.HIP_SIGNATURES
    assert "orb_initializer_check_batch_device" in _native.HIP_SIGNATURES
    assert callable(Initializer.check) and callable(Initializer.check_batch_device)
    assert "class Initializer" in (ROOT / "include" / "orb_slam_gpu.hpp").read_text()


def golden_inputs():
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE

    k1 = np.ascontiguousarray(np.load(GOLD / "scene_320x240_nf500.npz")["kps"]).view(KEYPOINT_DTYPE).reshape(-1)
    k2 = np.ascontiguousarray(np.load(GOLD / "scene_320x240_nf500_f1.npz")["kps"]).view(KEYPOINT_DTYPE).reshape(-1)
    m12 = np.load(GOLD / "match_320x240_f0_f1.npz")["m12"]
    return k1, k2, m12, dict(np.load(GOLD / "initializer_320x240.npz"))


def golden_as_result(g) -> dict:
    return {"n_matches": int(g["n_matches"]), "scores_h": g["scores_h"], "scores_f": g["scores_f"],
            "best_h": int(g["best_h"]), "best_f": int(g["best_f"]), "best_score_h": g["best_score_h"],
            "best_score_f": g["best_score_f"], "inliers_h": g["inliers_h"], "inliers_f": g["inliers_f"]}


def test_golden_equals_a_fresh_model_run():
    k1, k2, m12, g = golden_inputs()
    r = model.check(k1, k2, m12, float(g["sigma"]), g["H21"], g["H12"], g["F21"])
    assert not np.isnan(g["scores_h"]).any() and not np.isnan(g["scores_f"]).any()
    assert g["best_h"] >= 0 and g["best_f"] >= 0
    model.same_result(r, golden_as_result(g))
    model.same_result(golden_as_result(g), r)
