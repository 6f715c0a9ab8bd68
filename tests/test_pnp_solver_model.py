"""The CPU model of the PnPsolver hypotheses and RANSAC (tests/native/pnp_solver_model.cpp over
csrc/orb_epnp_math.h) held to hand cases, to an independent numpy float64 EPnP and to a sanitizer run.

Tolerances (scripts/gen_pnp_solver_golden.py measures and prints them): the largest
difference between the model and the numpy EPnP over 200 noise-free scenes of 6 to 45 points was
3.480e-06 on R and 2.243e-06 on t (the pixel coordinates are float32, so the scenes are exact to 3e-5
px only, and the two solutions weigh that differently); the bounds are 10 x those.  On 300 noise-free
4-point sets R R^T deviated from the identity by at most 2.442e-15 and det R from +1 by 1.110e-15
(bounds 10 x); the median reprojection error was 0.156 px (bound 10 x) while one set in ten ends
above 40 px and the worst at 136 px: with four points the null space has four dimensions and the
three beta approximations do not always find the pose.  The reference behaves so; RANSAC absorbs it."""
import subprocess
import sys
import pathlib

import numpy as np

import orbslam_jpminipc_amd as orb
import pnp_solver_model as pm

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
K64 = np.float64(f32(pm.K_CAM))
TOL_R, TOL_T = 3.480e-05, 2.243e-05
TOL_ORTH, TOL_DET, TOL_REP_MEDIAN = 2.442e-14, 1.110e-14, 1.557


def r_for(randi, size):
    return (randi * 2 ** 31 + 2 ** 30) // size


# ---- the minimal sets --------------------------------------------------------------------------------
def test_set_mapping_hand_cases():
    # r = 0: position 0 every time.  [0] = 5 after the first draw; the second draw takes that 5 and
    # writes past the end, so position 0 still holds 5 for the third and fourth: a repeated index
    assert pm.sets(6, [[0, 0, 0, 0]]).tolist() == [[0, 5, 5, 5]]
    # r = 2^31 - 1: the last position every time, whose value is its own index
    top = 2 ** 31 - 1
    assert pm.sets(6, [[top] * 4]).tolist() == [[5, 4, 3, 2]]
    # the second draw lands on the entry the first one overwrote
    assert pm.sets(10, [[r_for(2, 10), r_for(2, 9), r_for(7, 8), r_for(2, 7)]]).tolist() == [[2, 9, 7, 9]]
    for N, r in ((6, [[0, 0, 0, 0]]), (6, [[top] * 4]), (10, [[r_for(2, 10), r_for(2, 9), r_for(7, 8), r_for(2, 7)]])):
        assert np.array_equal(pm.sets(N, r), pm.mapping(4, N, r))
        assert np.array_equal(pm.sets(N, r), orb.pnp_minimal_sets(N, r))
    # removal by position (what the reference meant) gives another set
    assert orb.pnp_minimal_sets(6, [[0, 0, 0, 0]], fixed=True).tolist() == [[0, 5, 4, 3]]


def test_closed_form_mapping_equals_the_vector_sampler():
    rng = np.random.default_rng(3)
    for N in (4, 5, 6, 7, 9, 58, 8192):
        r = rng.integers(0, 2 ** 31, (3000, 4)).astype(np.int32)
        r[:500] = [[r_for(int(rng.integers(0, N - k)), N - k) for k in range(4)] for _ in range(500)]
        r[0], r[1] = 0, 2 ** 31 - 1
        want = pm.sets(N, r)
        assert np.array_equal(want, pm.mapping(4, N, r)), N
        assert np.array_equal(want[:200], orb.pnp_minimal_sets(N, r[:200])), N
        if N <= 9:
            assert any(len(set(s)) < 4 for s in want.tolist()), "the removal quirk must show"
    # the same mapping with three draws is Sim3Solver's
    for N in (3, 4, 5, 40):
        r = rng.integers(0, 2 ** 31, (500, 3)).astype(np.int32)
        assert np.array_equal(pm.mapping(3, N, r), orb.sim3_minimal_sets(N, r)), N


# ---- qr_solve ------------------------------------------------------------------------------------------
def test_qr_solve_hand_cases():
    # A = [I; 0]: every column has eta = 1, sigma = 1, the diagonal becomes 2, A1 = 2, A2 = -1 and no
    # column touches another; Qt b negates b[0..3]; X = -b / -1
    A = np.zeros((6, 4))
    A[:4] = np.eye(4)
    x, br = pm.qr_solve(A, [3, -5, 7, 11, 13, 17])
    assert x.tolist() == [3, -5, 7, 11] and not br & pm.BR["QR_ETA0"] and not br & pm.BR["QR_SIGMA_NEG"]
    # a negative pivot: sigma = -1, the diagonal becomes -2, A1 = 2, A2 = 1; Qt b negates b[0..3]; X = -b / 1
    x, br = pm.qr_solve(-A, [3, -5, 7, 11, 13, 17])
    assert x.tolist() == [-3, 5, -7, -11] and br & pm.BR["QR_SIGMA_NEG"]
    # a zero first column: the early return, X as it was
    Z = A.copy()
    Z[0, 0] = 0
    x, br = pm.qr_solve(Z, [1, 2, 3, 4, 5, 6], x0=[9, 8, 7, 6])
    assert x.tolist() == [9, 8, 7, 6] and br & pm.BR["QR_ETA0"]
    # the scan for eta never looks at the last row: a column whose only entry sits there counts as zero
    Z[5, 0] = 4.0
    x, br = pm.qr_solve(Z, [1, 2, 3, 4, 5, 6], x0=[9, 8, 7, 6])
    assert x.tolist() == [9, 8, 7, 6] and br & pm.BR["QR_ETA0"]


def test_qr_solve_is_least_squares():
    rng = np.random.default_rng(5)
    for _ in range(50):
        A, b = rng.normal(size=(6, 4)), rng.normal(size=6)
        x, _ = pm.qr_solve(A, b)
        assert np.abs(x - np.linalg.lstsq(A, b, rcond=None)[0]).max() < 1e-12


# ---- compute_pose against an independent EPnP -------------------------------------------------------
def test_n_point_pose_equals_numpy_epnp():
    worst = [0.0, 0.0]
    for seed in list(range(0, 200, 7)) + list(range(5000, 5060)):
        n = 6 + seed % 40
        p3, p2, R, t = pm.scene(n, seed)
        m = pm.compute_pose(p3, p2, K64)
        Rn, tn = pm.numpy_epnp(p3, p2, K64)
        worst = [max(worst[0], np.abs(m["R"] - Rn).max()), max(worst[1], np.abs(m["t"] - tn).max())]
        # and both are the scene's pose
        assert np.abs(m["R"] - R).max() < 1e-5 and np.abs(m["t"] - t).max() < 1e-4 and m["rep_error"] < 1e-3
    print(f"model against numpy: R {worst[0]:.3e} (bound {TOL_R:.3e}), t {worst[1]:.3e} (bound {TOL_T:.3e})")
    assert worst[0] <= TOL_R and worst[1] <= TOL_T


def test_four_point_pose_is_a_rotation():
    orth = det = 0.0
    reps = []
    for seed in list(range(1000, 1300, 5)) + list(range(7000, 7100)):
        p3, p2, _, _ = pm.scene(4, seed)
        m = pm.compute_pose(p3, p2, K64)
        orth = max(orth, np.abs(m["R"] @ m["R"].T - np.eye(3)).max())
        det = max(det, abs(np.linalg.det(m["R"]) - 1))
        reps.append(m["rep_error"])
    print(f"n = 4: orthonormality {orth:.3e}, determinant {det:.3e}, median reprojection error {np.median(reps):.3e} px, "
          f"worst {np.max(reps):.3e} px")
    assert orth <= TOL_ORTH and det <= TOL_DET and np.median(reps) <= TOL_REP_MEDIAN


def test_degenerate_sets_flow_on():
    p3, p2, _, _ = pm.scene(12, 7)
    m = pm.compute_pose(p3, p2, K64, [3, 3, 3, 3])  # qr_solve returns early on the first Gauss-Newton step
    assert m["branches"] & pm.BR["QR_ETA0"] and m["branches"] & pm.BR["SVD_FILL"] and m["branches"] & pm.BR["BKSB_SKIP"]
    nan = p3.copy()
    nan[1, 1] = np.nan
    m = pm.compute_pose(nan, p2, K64, [0, 1, 2, 3])
    assert np.isnan(m["R"]).all() and np.isnan(m["t"]).all() and np.isnan(m["rep_error"])


# ---- iterate and Refine --------------------------------------------------------------------------------
def test_refine_is_strict():
    p3, p2, _, _ = pm.scene(40, 5, noise=1.2, outliers=0.35)
    s2, r = np.ones(40, f32), pm.draws(40, 5)
    # iteration 31 sets the best; Refine on its mask counts 20
    fails = pm.ransac(p3, p2, s2, 5.991, K64, 20, rand31=r)
    assert fails["refined_counts"][31] == 20 and fails["first_refined"] == -1  # 20 > 20 is false: the loop goes on
    h = int(fails["best_at"][-1])
    assert h == 31 and fails["pose_inliers"] == fails["counts"][h] and np.array_equal(fails["pose_mask"], fails["masks"][h])
    assert np.array_equal(fails["pose"], f32(np.concatenate([fails["R"][h], fails["t"][h]])))
    # every later qualifying iteration refined the same mask again and got the same answer
    later = int((fails["counts"][32:] >= 20).sum())
    assert fails["refine_calls"] == 1 + later
    ok = pm.ransac(p3, p2, s2, 5.991, K64, 19, rand31=r)
    assert ok["refined_counts"][31] == 20 and ok["first_refined"] == 31 and ok["pose_inliers"] == 20
    assert np.array_equal(ok["pose"], f32(np.concatenate([ok["refined_R"][31], ok["refined_t"][31]])))
    # a later replacing iteration is the first whose Refine succeeds
    p3, p2, _, _ = pm.scene(40, 78, noise=1.2, outliers=0.35)
    o = pm.ransac(p3, p2, s2, 5.991, K64, 25, rand31=pm.draws(40, 78))
    assert o["refined_counts"][[1, 10]].tolist() == [25, 27] and o["first_refined"] == 10


def test_golden_equals_a_fresh_model_run():
    g = dict(np.load(ROOT / "tests" / "golden" / "pnp_solver_320x240.npz"))
    m = pm.ransac(g["p3d"], g["p2d"], g["sigma2"], g["th2"], np.float64(g["K"]), int(g["min_inliers"]), rand31=g["rand31"])
    for k in ("counts", "masks", "best_at", "sets", "branches", "refined_counts", "pose_mask"):
        assert np.array_equal(m[k], g[k]), k
    for k in ("R", "t", "rep_error", "pose"):
        assert np.array_equal(m[k], g[k], equal_nan=True), k
    assert (m["first_ok"], m["first_refined"], m["pose_inliers"]) == (int(g["first_ok"]), int(g["first_refined"]),
                                                                      int(g["pose_inliers"]))
    assert g["rand31"].shape == (300, 4) and m["first_refined"] >= 0
    assert sum(len(set(s)) < 4 for s in m["sets"].tolist()) >= 4


def test_sanitized_model_program(tmp_path):
    """The model as a stand-alone program under AddressSanitizer and UBSan: general sets, the degenerate
    ones (coplanar, repeated, identical, behind the camera, NaN) and a whole RANSAC; between them they
    visit every branch."""
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = tmp_path / "pnp_solver_model_san"
    subprocess.run(ge.PNP_SOLVER_MODEL_CMD(exe, ("-DPNP_SOLVER_MODEL_MAIN", "-g", "-fsanitize=address,undefined",
                                                 "-fno-sanitize-recover=all")), check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "status 0" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
    assert f"branches 0x{pm.BR_ALL:x} of 0x{pm.BR_ALL:x}" in r.stdout, r.stdout
