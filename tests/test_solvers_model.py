"""The CPU model of the PnP / Sim3 consensus (tests/native/solvers_model.cpp) against cases worked by
hand, the scalar RANSAC parameters of the wrappers, and the committed fixture.  No GPU."""
import pathlib
import re

import numpy as np
import pytest

import solvers_model as model

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
I3 = np.eye(3).reshape(1, 9)
T0 = np.zeros((1, 3))
K100 = (100.0, 100.0, 0.0, 0.0)
TI = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(f32).reshape(1, 12)  # rows 0-2 of the identity


def pnp1(p3d, p2d, sigma2, th2=1.0, **kw):
    return model.pnp(np.array([p3d], f32), np.array([p2d], f32), np.array([sigma2], f32), th2, K100, I3, T0, 1,
                     errors=True, **kw)


def test_pnp_by_hand():
    # (0.5, 0.25, 2): Xc .5, Yc .25, invZc .5 -> ue = 100*.5*.5 = 25, ve = 12.5; measured (26, 12.5): error2 = 1
    r = pnp1((0.5, 0.25, 2), (26, 12.5), 2.0)
    assert r["err"][0, 0] == 1.0 and r["counts"][0] == 1 and r["inliers"][0, 0]
    # (0, 0, 1) measured at (3, 4): error2 = 25 exactly
    r = pnp1((0, 0, 1), (3, 4), 30.0)
    assert r["err"][0, 0] == 25.0 and r["counts"][0] == 1


def test_pnp_exactly_at_the_bound_is_an_outlier():
    # mvMaxError = 25 * 1: error2 < bound is false at equality, true one float above
    assert pnp1((0, 0, 1), (3, 4), 25.0)["counts"][0] == 0
    assert pnp1((0, 0, 1), (3, 4), np.nextafter(f32(25), f32(26)))["counts"][0] == 1
    # the bound is the float product sigma2 * th2
    assert pnp1((0, 0, 1), (3, 4), 5.0, th2=5.0)["counts"][0] == 0


def test_pnp_nan_and_infinite_projection_are_outliers():
    r = pnp1((0, 0, 0), (0, 0), 1e30)  # Xc = 0, 1/0 = inf: 0 * inf = NaN
    assert np.isnan(r["err"][0, 0]) and r["counts"][0] == 0
    r = pnp1((1, 1, 0), (0, 0), 1e30)  # ue = inf: error2 = inf
    assert np.isinf(r["err"][0, 0]) and r["counts"][0] == 0


def test_pnp_point_behind_the_camera_counts():
    r = pnp1((0.5, 0.25, -2), (26, 12.5), 2.0)  # Zc = -2: ue = 100 * .5 * -.5 = -25
    assert r["counts"][0] == 0
    r = pnp1((0.5, 0.25, -2), (-24, -12.5), 2.0)
    assert r["err"][0, 0] == 1.0 and r["counts"][0] == 1, "the reference does not test the depth's sign"


def sim3_1(x1, x2, s1=1.0, s2=1.0, K=(96.0, 96.0, 0.0, 0.0), **kw):
    return model.sim3(np.array([x1], f32), np.array([x2], f32), [s1], [s2], K, K, TI, TI, 0, errors=True, **kw)


def test_sim3_by_hand_and_level0_bound_is_9():
    # identity transforms, fx = 96: (0, 0, 1) -> (0, 0); (1/32, 0, 1) -> (3, 0): err1 = err2 = 9
    r = sim3_1((0, 0, 1), (1 / 32, 0, 1))
    assert r["err1"][0, 0] == 9.0 and r["err2"][0, 0] == 9.0
    # mvnMaxError is a vector<size_t>: 9.21 * 1 truncates to 9, and 9 < 9 is false
    assert r["counts"][0] == 0
    assert sim3_1((0, 0, 1), (1 / 32, 0, 1), variant=model.UNTRUNCATED)["counts"][0] == 1
    # one float below 9 is inside
    x = np.nextafter(f32(1 / 32), f32(0))
    r = sim3_1((0, 0, 1), (x, 0, 1))
    assert r["err1"][0, 0] < 9.0 and r["counts"][0] == 1
    # level 1: 9.21 * 1.44 = 13.26 -> 13; (3.625)^2 = 13.14 is outside, under the untruncated bound inside
    x = 3.625 / 96
    assert sim3_1((0, 0, 1), (x, 0, 1), f32(1.44), f32(1.44))["counts"][0] == 0
    assert sim3_1((0, 0, 1), (x, 0, 1), f32(1.44), f32(1.44), variant=model.UNTRUNCATED)["counts"][0] == 1
    # both errors must pass: the second keypoint at level 0
    assert sim3_1((0, 0, 1), (3.5 / 96, 0, 1), f32(1.44), f32(1.44))["counts"][0] == 1
    assert sim3_1((0, 0, 1), (3.5 / 96, 0, 1), f32(1.44), f32(1.0))["counts"][0] == 0


def test_sim3_nan_infinite_and_behind_camera():
    r = sim3_1((0, 0, 1), (0, 0, 0))  # 0 * (1/0) = NaN
    assert np.isnan(r["err1"][0, 0]) and r["counts"][0] == 0
    r = sim3_1((0, 0, 1), (1, 1, 0))  # x = y = inf
    assert np.isinf(r["err1"][0, 0]) and r["counts"][0] == 0
    r = sim3_1((0.25, 0, -1), (0.25, 0, -1))  # behind both cameras, consistent: an inlier
    assert r["err1"][0, 0] == 0.0 and r["counts"][0] == 1


def test_ransac_parameters_by_hand():
    from orbslam_jpminipc_amd.solvers import pnp_ransac_parameters, sim3_ransac_parameters

    reloc = (0.99, 10, 300, 4, 0.5, 5.991)  # Tracking.cc:940
    # N 100: int(100 * .5) = 50; eps .5; ceil(log(.01) / log(1 - .125)) = ceil(34.49) = 35
    p = pnp_ransac_parameters(100, *reloc)
    assert (p["min_inliers"], p["max_iterations"]) == (50, 35) and p["epsilon"] == f32(0.5)
    # N 15: int(7.5) = 7 -> 10; eps = 10/15; ceil(4.60517 / 0.35140) = ceil(13.1) = 14
    p = pnp_ransac_parameters(15, *reloc)
    assert (p["min_inliers"], p["max_iterations"]) == (10, 14) and p["epsilon"] == f32(10) / f32(15)
    assert pnp_ransac_parameters(10, *reloc)["max_iterations"] == 1  # minInliers == N
    assert pnp_ransac_parameters(3, 0.99, 2, 300, 4, 0.5, 5.991)["min_inliers"] == 4  # minSet
    assert pnp_ransac_parameters(100, *reloc)["th2"] == f32(5.991)
    loop = (0.99, 20, 300)  # LoopClosing.cc:290
    # N 100: eps .2; ceil(4.60517 / 0.0080322) = 574 -> capped at 300
    assert sim3_ransac_parameters(100, *loop) == {"min_inliers": 20, "epsilon": f32(0.2), "max_iterations": 300}
    assert sim3_ransac_parameters(40, *loop)["max_iterations"] == 35  # eps .5
    assert sim3_ransac_parameters(25, *loop)["max_iterations"] == 7   # eps .8: ceil(4.60517 / 0.71744)
    assert sim3_ransac_parameters(20, *loop)["max_iterations"] == 1
    assert sim3_ransac_parameters(0, *loop)["max_iterations"] == 1    # eps inf: the NaN converts to INT_MIN


def _identical(n_hyp=5):
    c = model.pnp_case(40, 1, 3, outliers=0.5)
    s = model.sim3_case(40, 1, 4, outliers=0.5)
    rep = lambda a: np.repeat(np.asarray(a).reshape(1, -1), n_hyp, 0)  # noqa: E731
    return c, rep(c["R"]), rep(c["t"]), s, rep(s["T12"]), rep(s["T21"])


def test_keep_the_best_on_identical_hypotheses():
    c, R, t, s, T12, T21 = _identical()
    r = model.pnp(c["p3d"], c["p2d"], c["sigma2"], 5.991, c["K"], R, t, 4)
    assert r["counts"][0] >= 4 and len(set(r["counts"])) == 1
    assert list(r["best_at"]) == [0] * 5, "PnP replaces on a strict >: the first maximum wins"
    assert r["first_ok"] == 0
    r = model.sim3(s["x3dc1"], s["x3dc2"], s["sigma2_1"], s["sigma2_2"], s["K1"], s["K2"], T12, T21, 4)
    assert r["counts"][0] > 4 and len(set(r["counts"])) == 1
    assert list(r["best_at"]) == [0, 1, 2, 3, 4], "Sim3 replaces on >=: the last maximum wins"
    assert r["first_accept"] == 0


def test_count_equal_to_min_inliers():
    c, R, t, s, T12, T21 = _identical()
    n_in = int(model.pnp(c["p3d"], c["p2d"], c["sigma2"], 5.991, c["K"], R, t, 1)["counts"][0])
    r = model.pnp(c["p3d"], c["p2d"], c["sigma2"], 5.991, c["K"], R, t, n_in)
    assert r["first_ok"] == 0 and r["best_at"][0] == 0, "count >= min qualifies"
    r = model.pnp(c["p3d"], c["p2d"], c["sigma2"], 5.991, c["K"], R, t, n_in + 1)
    assert r["first_ok"] == -1 and list(r["best_at"]) == [-1] * 5
    sa = (s["x3dc1"], s["x3dc2"], s["sigma2_1"], s["sigma2_2"], s["K1"], s["K2"], T12, T21)
    n_in = int(model.sim3(*sa, 1)["counts"][0])
    r = model.sim3(*sa, n_in)
    assert r["first_accept"] == -1, "count > min is needed to accept"
    assert list(r["best_at"]) == [0, 1, 2, 3, 4], "but the best is still replaced"
    assert model.sim3(*sa, n_in - 1)["first_accept"] == 0


def test_best_in_carry():
    c, R, t, s, T12, T21 = _identical()
    pa = (c["p3d"], c["p2d"], c["sigma2"], 5.991, c["K"], R, t, 4)
    n_in = int(model.pnp(*pa)["counts"][0])
    r = model.pnp(*pa, best_in=n_in)
    assert list(r["best_at"]) == [-2] * 5 and r["first_ok"] == 0, "an equal count does not replace the earlier best"
    assert list(model.pnp(*pa, best_in=n_in - 1)["best_at"]) == [0] * 5
    sa = (s["x3dc1"], s["x3dc2"], s["sigma2_1"], s["sigma2_2"], s["K1"], s["K2"], T12, T21, 4)
    n_in = int(model.sim3(*sa)["counts"][0])
    r = model.sim3(*sa, best_in=n_in + 1)
    assert list(r["best_at"]) == [-2] * 5 and r["first_accept"] == -1
    r = model.sim3(*sa, best_in=n_in)
    assert list(r["best_at"]) == [0, 1, 2, 3, 4] and r["first_accept"] == 0, "an equal count replaces it"


def test_mixed_counts_running_best():
    c = model.pnp_case(120, 40, 5)
    # (the case's hypotheses start at the best one: run them backwards)
    r = model.pnp(c["p3d"], c["p2d"], c["sigma2"], 5.991, c["K"], c["R"][::-1], c["t"][::-1], 30)
    best, holder, first = 0, -1, -1
    for h, n in enumerate(r["counts"]):
        if n >= 30:
            if n > best:
                best, holder = n, h
            if first < 0:
                first = h
        assert r["best_at"][h] == holder
    assert r["first_ok"] == first and len(set(r["best_at"])) > 2


def test_setup_compacts_in_index_order():
    from orbslam_jpminipc_amd._native import KEYPOINT_DTYPE

    kps = np.zeros(6, KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["octave"] = np.arange(6) * 10, np.arange(6) * 10 + 1, [0, 1, 2, 3, 0, 1]
    pos = np.arange(15, dtype=f32).reshape(5, 3)
    #        j: 0   1  2  3  4  5(beyond n_f)
    match = [3, -1, 9, 1, 0, 2]  # 9: beyond the keyframe's count; keyframe point 1 is bad
    s = model.pnp_setup(kps, 5, 5, match, pos, [0, 1, 0, 0, 0], model.LEVEL_SIGMA2)
    assert s["n"] == 2 and list(s["index"][:2]) == [0, 4]
    assert s["p3d"].tolist() == [pos[3].tolist(), pos[0].tolist()] and s["p2d"].tolist() == [[0, 1], [40, 41]]
    assert s["sigma2"].tolist() == [1.0, 1.0]
    pose = np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0.5, 0, 0], f32)
    q = model.sim3_setup(kps, 5, kps, 5, match[:5] + [0], pos, [0, 0, 0, 1, 0], pos, [0, 0, 0, 0, 0], pose, pose,
                         model.LEVEL_SIGMA2)
    assert q["n"] == 2 and list(q["index"][:2]) == [0, 4]  # i1 = 3 is bad, 2 points outside
    assert q["x3dc1"].tolist() == [[0.5, 1, 2], [12.5, 13, 14]] and q["x3dc2"].tolist() == [[9.5, 10, 11], [0.5, 1, 2]]
    assert q["sigma2_2"].tolist() == [model.LEVEL_SIGMA2[3], 1.0]


def test_golden_fixture_and_its_visibility():
    g = np.load(ROOT / "tests" / "golden" / "solvers_320x240.npz")
    pa = (g["p3d"], g["p2d"], g["pnp_sigma2"], g["th2"], g["K"], g["R"], g["t"], int(g["pnp_min"]))
    r = model.pnp(*pa)
    assert np.array_equal(r["counts"], g["pnp_counts"]) and np.array_equal(r["masks"], g["pnp_masks"])
    assert np.array_equal(r["best_at"], g["pnp_best_at"]) and r["first_ok"] == int(g["pnp_first_ok"])
    assert (r["inliers"] != model.pnp(*pa, variant=model.PLAIN)["inliers"]).sum() >= 8
    assert (r["inliers"] != model.pnp(*pa, variant=model.ROW_PLAIN)["inliers"]).sum() >= 4
    sa = (g["x3dc1"], g["x3dc2"], g["sigma2_1"], g["sigma2_2"], g["K"], g["K"], g["T12"], g["T21"], int(g["sim3_min"]))
    r = model.sim3(*sa)
    assert np.array_equal(r["counts"], g["sim3_counts"]) and np.array_equal(r["masks"], g["sim3_masks"])
    assert np.array_equal(r["best_at"], g["sim3_best_at"]) and r["first_accept"] == int(g["sim3_first_accept"])
    assert (r["inliers"] != model.sim3(*sa, variant=model.PLAIN)["inliers"]).sum() >= 8
    assert (r["inliers"] != model.sim3(*sa, variant=model.UNTRUNCATED)["inliers"]).sum() >= 8


@pytest.mark.parametrize("name", ["orb_pnp_check_inliers", "orb_sim3_check_inliers",
                                  "orb_pnp_check_inliers_batch_device", "orb_sim3_check_inliers_batch_device"])
def test_abi_names(name):
    from orbslam_jpminipc_amd import _native

    header = (ROOT / "include" / "orb_abi.h").read_text()
    assert re.search(r"^int " + name + r"\(", header, re.M), name + " is not declared in orb_abi.h"
    assert name in _native.HIP_SIGNATURES
