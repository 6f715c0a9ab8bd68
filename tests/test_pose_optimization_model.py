"""The CPU model of Optimizer::PoseOptimization (tests/native/pose_optimization_model.cpp) on cases
worked by hand: the GPU tests compare the kernels with this model, so the model itself is proven
here against numpy and against the statements of DESIGN.md §13."""
import numpy as np
import pytest

import pose_optimization_model as pom

f32, f64 = np.float32, np.float64
K = pom.K_DEFAULT
K64 = np.array(K, f64)
DELTA = float(f32(np.sqrt(5.991)))
P = lambda a: a.ctypes.data  # noqa: E731


@pytest.fixture(scope="module")
def L():
    return pom.lib()


def pose7(L, pose12):
    out = np.zeros(7)
    p = np.ascontiguousarray(pose12, f32)
    L.pom_pose_from_float(P(p), P(out))
    return out


def edge(L, T7, X, obs, s):
    e, c, J = np.zeros(2), np.zeros(1), np.zeros(12)
    X, obs = np.ascontiguousarray(X, f64), np.ascontiguousarray(obs, f64)
    L.pom_edge(P(T7), P(K64), P(X), P(obs), float(s), P(e), P(c), P(J))
    return e, float(c[0]), J.reshape(2, 6)


def exp_update(L, x, T7):
    out = np.zeros(7)
    x = np.ascontiguousarray(x, f64)
    L.pom_exp_update(P(x), P(T7), P(out))
    return out


def start_pose(rng, amp=0.1):
    return np.concatenate([pom.rot(rng.normal(0, amp, 3)).reshape(9), rng.normal(0, 0.3, 3)]).astype(f32)


def test_pose_round_trip_and_quaternion_sign(L):
    rng = np.random.default_rng(1)
    for w in (rng.normal(0, 0.3, 3), np.array([3.1, 0, 0]), np.array([0, 3.0, 0.5]), np.array([0.2, 0.1, 3.1])):
        R = pom.rot(w)
        p12 = np.concatenate([R.reshape(9), [0.5, -1, 2]]).astype(f32)
        T7 = pose7(L, p12)
        assert T7[3] >= 0 and abs(np.linalg.norm(T7[:4]) - 1) < 1e-15
        M = np.zeros(12)
        L.pom_pose_to_matrix(P(T7), P(M))
        assert np.allclose(M, p12.astype(f64), atol=2e-7)  # the float input is not exactly orthonormal
        assert abs(np.linalg.det(M[:9].reshape(3, 3)) - 1) < 1e-14


def test_jacobian_against_central_differences(L):
    rng = np.random.default_rng(2)
    T7 = pose7(L, start_pose(rng))
    for _ in range(5):
        X, obs = rng.uniform(-1, 1, 3) + [0, 0, 6], rng.uniform(0, 300, 2)
        _, _, J = edge(L, T7, X, obs, 1.0)
        h = 1e-6
        for j in range(6):
            d = np.zeros(6)
            d[j] = h
            ep, _, _ = edge(L, exp_update(L, d, T7), X, obs, 1.0)
            em, _, _ = edge(L, exp_update(L, -d, T7), X, obs, 1.0)
            assert np.allclose((ep - em) / (2 * h), J[:, j], rtol=1e-6, atol=1e-6), j
        assert J[0, 4] == 0 and J[1, 3] == 0


def test_exp_small_angle_branch_and_group_law(L):
    I7 = np.array([0, 0, 0, 1, 0, 0, 0], f64)
    x = np.array([3e-6, -2e-6, 1e-6, 0.1, 0.2, 0.3])  # theta < 1e-5: R = I + Omega + Omega^2, V = R
    T = exp_update(L, x, I7)
    O = np.array([[0, -x[2], x[1]], [x[2], 0, -x[0]], [-x[1], x[0], 0]])
    assert np.allclose(T[4:], (np.eye(3) + O + O @ O) @ x[3:], rtol=0, atol=1e-16)
    x = np.array([0.3, -0.2, 0.1, 0.5, -0.4, 0.3])
    T = exp_update(L, x, I7)
    M = np.zeros(12)
    L.pom_pose_to_matrix(P(T), P(M))
    assert np.allclose(M[:9].reshape(3, 3), pom.rot(x[:3]), atol=1e-15)
    back = exp_update(L, -x, T)  # exp(-x) exp(x) = identity
    assert np.allclose(back, I7, atol=1e-15)


def test_huber(L):
    rho = np.zeros(3)
    L.pom_huber(DELTA * DELTA, P(rho))
    assert rho.tolist() == [DELTA * DELTA, 1.0, 0.0]  # e <= dsqr: the bound is an inlier
    assert DELTA * DELTA != 5.991  # the delta is a float: dsqr is not 5.991
    L.pom_huber(16.0, P(rho))
    assert rho[0] == 2 * 4.0 * DELTA - DELTA * DELTA and rho[1] == DELTA / 4.0


def numpy_system(L, T7, X, obs, s):
    H, b, chi = np.zeros((6, 6)), np.zeros(6), 0.0
    for i in range(len(X)):
        e, c, J = edge(L, T7, X[i], obs[i], s[i])
        assert c == pytest.approx(s[i] * e @ e, rel=1e-15)
        if c <= DELTA * DELTA:
            r0, r1 = c, 1.0
        else:
            r0, r1 = 2 * np.sqrt(c) * DELTA - DELTA * DELTA, DELTA / np.sqrt(c)
        H += J.T @ (r1 * s[i] * np.eye(2)) @ J
        b += J.T @ (-s[i] * e * r1)
        chi += r0
    return H, b, chi


def build(L, T7, X, obs, s, order=0):
    H, b = np.zeros(36), np.zeros(6)
    X, obs, s = (np.ascontiguousarray(a, f64) for a in (X, obs, s))
    chi = L.pom_build(len(s), P(X), P(obs), P(s), P(K64), P(T7), order, P(H), P(b))
    return H.reshape(6, 6), b, chi


def test_one_levenberg_step_of_three_edges_against_numpy(L):
    rng = np.random.default_rng(3)
    T7 = pose7(L, start_pose(rng, 0.02))
    X = rng.uniform(-2, 2, (3, 3)) + [0, 0, 7]
    # one inlier-sized and two Huber-sized residuals
    obs = np.array([edge(L, T7, X[i], [0, 0], 1)[0] * -1 for i in range(3)]) + [[0.5, -0.3], [6, 2], [-9, 4]]
    s = np.array([1.0, 1 / 1.44, 1 / 2.0736])
    Hn, bn, chin = numpy_system(L, T7, X, obs, s)
    H, b, chi = build(L, T7, X, obs, s)
    assert np.allclose(H, Hn, rtol=1e-13, atol=1e-9) and np.allclose(b, bn, rtol=1e-13) and chi == pytest.approx(chin, rel=1e-14)
    assert np.array_equal(H, H.T)
    lam = 1e-5 * np.abs(np.diag(H)).max()
    x = np.zeros(6)
    assert L.pom_solve(P(np.ascontiguousarray(H)), P(b), lam, P(x)) == 1
    xn = np.linalg.solve(Hn + lam * np.eye(6), bn)  # rank 6 needs 3 edges; H + lambda I is regular anyway
    assert np.allclose(x, xn, rtol=1e-6)
    assert np.allclose((H + lam * np.eye(6)) @ x, b, rtol=1e-9, atol=1e-9 * np.abs(b).max())
    # not positive: refused, x untouched
    x[:] = 7
    assert L.pom_solve(P(np.ascontiguousarray(-H)), P(b), 0.0, P(x)) == 0 and (x == 7).all()


def levenberg_round(L, T7, X, obs, s, its):
    """optimization_algorithm_levenberg.cpp:61-189 over the model's pieces, every edge active."""
    lam, ni, bad, x = -1.0, 2.0, 0, np.zeros(6)
    log = {"iterations": 0, "trials": 0, "factors": []}
    for it in range(its):
        log["iterations"] += 1
        H, b, cur = build(L, T7, X, obs, s)
        ini = cur
        if it == 0:
            lam, ni, bad = 1e-5 * np.abs(np.diag(H)).max(), 2.0, 0
        rho, q = 0.0, 0
        while True:
            ok = L.pom_solve(P(np.ascontiguousarray(H)), P(b), lam, P(x))
            Tn = exp_update(L, x, T7)
            tmp = build(L, Tn, X, obs, s)[2] if ok else np.finfo(f64).max
            rho = (cur - tmp) / (float(np.sum(x * (lam * x + b))) + 1e-3)
            if rho > 0 and np.isfinite(tmp):
                f = max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3))
                log["factors"].append(f)
                lam, ni, cur, T7 = lam * f, 2.0, tmp, Tn
            else:
                lam, ni = lam * ni, ni * 2
            q += 1
            log["trials"] += 1
            if not (rho < 0 and q < 10):
                break
        if q == 10 or rho == 0:
            break
        bad = bad + 1 if (ini - cur) * 1e3 < ini else 0
        if bad >= 3:
            break
    log["lambda"] = lam
    return T7, log


def exact_case(rng, n):
    Rt, tt = pom.rot(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3)
    Xc = np.stack([rng.uniform(-2, 2, n), rng.uniform(-1.5, 1.5, n), rng.uniform(4, 12, n)], 1)
    Xw = ((Xc - tt) @ Rt).astype(f32)  # float points; the observations are exact for them
    Xc = Xw.astype(f64) @ Rt.T + tt
    obs = np.stack([Xc[:, 0] / Xc[:, 2] * K64[0] + K64[2], Xc[:, 1] / Xc[:, 2] * K64[1] + K64[3]], 1)
    start = np.concatenate([(pom.rot(rng.normal(0, 0.02, 3)) @ Rt).reshape(9), tt + rng.normal(0, 0.1, 3)]).astype(f32)
    return Xw, obs, start, np.concatenate([Rt.reshape(9), tt])


def test_exact_data_converges_and_lambda_shrinks_by_a_third(L):
    Xw, obs, start, truth = exact_case(np.random.default_rng(4), 9)
    obs32 = obs.astype(f32)
    r = pom.pose_optimization(Xw, obs32, np.ones(9, f32), None, K, start)
    # float observations: the residual is their rounding, 1e-5 pixels
    assert np.allclose(r["pose_f64"], truth, atol=2e-6)
    assert not r["outlier"].any() and r["n_inliers"] == 9 and r["info"].n_bad == 0
    assert np.array_equal(r["pose"], r["pose_f64"].astype(f32))
    # the same round over the pieces: same pose, same counters, same lambda
    T7, log = levenberg_round(L, pose7(L, start), Xw.astype(f64), obs32.astype(f64), np.ones(9), 10)
    M = np.zeros(12)
    L.pom_pose_to_matrix(P(T7), P(M))
    assert np.array_equal(M, r["pose_f64"])
    assert (r["info"].iterations[0], r["info"].trials) == (log["iterations"], log["trials"])
    assert r["info"].lambda_ == log["lambda"]
    # while the steps are good (rho near 1: the first two, before the residual reaches the rounding
    # of the float observations) lambda shrinks by 1/3 per step; no accepted step leaves [1/3, 2/3]
    assert log["factors"][:2] == [1 / 3] * 2 and all(1 / 3 <= f <= 2 / 3 for f in log["factors"])


def test_nine_edges_run_one_round_ten_run_four():
    rng = np.random.default_rng(5)
    Xw, obs, start, _ = exact_case(rng, 10)
    obs = (obs + rng.normal(0, 0.5, obs.shape)).astype(f32)
    s = np.ones(10, f32)
    r10 = pom.pose_optimization(Xw, obs, s, None, K, start)
    assert r10["info"].rounds == 4 and all(r10["info"].iterations[k] > 0 for k in range(4))
    assert not np.isnan(r10["chi2"]).any()
    has = np.ones(10, np.uint8)
    has[4] = 0  # ten keypoints, nine edges: edges().size() < 10
    r9 = pom.pose_optimization(Xw, obs, s, has, K, start)
    assert r9["info"].rounds == 1 and r9["info"].n_initial == 9 and list(r9["info"].iterations)[1:] == [0, 0, 0]
    assert np.isnan(r9["chi2"][1:]).all() and np.isnan(r9["chi2"][0, 4]) and not r9["outlier"][4]


def test_a_round_without_active_edges_leaves_the_pose(L):
    rng = np.random.default_rng(6)
    Xw, obs, start, _ = exact_case(rng, 12)
    obs = (obs + rng.choice([-1, 1], obs.shape) * rng.uniform(30, 60, obs.shape)).astype(f32)  # nothing fits
    r = pom.pose_optimization(Xw, obs, np.ones(12, f32), None, K, start)
    assert r["outlier"].all() and r["n_inliers"] == 0 and r["info"].rounds == 4
    assert list(r["info"].iterations)[1:] == [0, 0, 0]
    T7, log = levenberg_round(L, pose7(L, start), Xw.astype(f64), obs.astype(f64), np.ones(12), 10)
    M = np.zeros(12)
    L.pom_pose_to_matrix(P(T7), P(M))
    assert np.array_equal(M, r["pose_f64"]), "rounds 2-4 must not move the pose"
    # the flagged edges are re-evaluated at that pose before each classification
    assert np.array_equal(r["chi2"][0], r["chi2"][3]) and (r["chi2"] > 9.21).all()


def test_an_edge_with_z_zero_keeps_its_flag():
    rng = np.random.default_rng(7)
    I12 = np.concatenate([np.eye(3).reshape(9), np.zeros(3)]).astype(f32)
    Xc = np.stack([rng.uniform(-2, 2, 12), rng.uniform(-1.5, 1.5, 12), rng.uniform(4, 12, 12)], 1).astype(f32)
    obs = np.stack([Xc[:, 0] / Xc[:, 2] * K[0] + K[2], Xc[:, 1] / Xc[:, 2] * K[1] + K[3]], 1).astype(f32)
    obs[3] += 40  # would be an outlier
    Xc[0] = 0     # 0 / 0: its chi2 is NaN, and so is every sum it takes part in
    r = pom.pose_optimization(Xc, obs, np.ones(12, f32), None, K, I12)
    # every trial ends at a NaN pose and is rejected; the errors it left are NaN, which match
    # neither > nor <=: all flags stay as they were, nothing is counted bad
    assert np.isnan(r["chi2"]).all() and not r["outlier"].any() and r["info"].n_bad == 0 and r["n_inliers"] == 12
    assert np.array_equal(r["pose"], I12) and list(r["info"].iterations) == [10, 10, 7, 5] and r["info"].trials == 32
    # x / 0 instead: the edge's chi2 is +inf, its Huber weight 0 and its Jacobian infinite, so H is
    # NaN all the same (0 * inf) and the run goes the same way: the +inf is never classified,
    # because the errors that the classification reads are those of the rejected NaN trial
    Xc[0] = [1, 1, 0]
    r = pom.pose_optimization(Xc, obs, np.ones(12, f32), None, K, I12)
    assert np.isnan(r["chi2"]).all() and not r["outlier"].any() and r["n_inliers"] == 12
    assert np.array_equal(r["pose"], I12)


def test_sum_orders_agree_closely_and_flags_do_not_depend_on_them():
    c = pom.make_case(11, 300)
    a = (c["p3d"], c["obs"], c["inv_sigma2"], c["has_mp"], c["K"], c["pose_in"])
    r0 = c["model"]
    assert 0.1 < r0["outlier"].mean() < 0.35
    assert np.allclose(r0["pose_f64"], c["pose_true"], atol=5e-2)
    for order in (1, 2):
        r = pom.pose_optimization(*a, sum_order=order)
        assert np.array_equal(r["outlier"], r0["outlier"])
        assert np.abs(r["pose_f64"] - r0["pose_f64"]).max() < 1e-8
        assert not np.array_equal(r["pose_f64"], r0["pose_f64"]) or order == 0
