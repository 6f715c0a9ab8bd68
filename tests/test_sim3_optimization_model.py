"""The CPU model of Optimizer::OptimizeSim3 (tests/native/sim3_optimization_model.cpp) on cases worked
by hand: the GPU tests compare the kernels with this model, so the model itself is proven here
against numpy and against the statements of DESIGN.md §14."""
import numpy as np
import pytest

import sim3_optimization_model as s3m

f32, f64 = np.float32, np.float64
K1, K2 = np.array(s3m.K_DEFAULT, f64), np.array(s3m.K_SECOND, f64)
TH2 = s3m.TH2
P = lambda a: a.ctypes.data  # noqa: E731
ND = 1e-9  # the step of g2o's numeric Jacobian


@pytest.fixture(scope="module")
def L():
    return s3m.lib()


def state(L, R, t, s, normalise=True):
    """8 doubles (qx qy qz qw t s) of Sim3(R, t, s); normalise: with the quaternion scaled to unit
    length in double (the model itself never does that)."""
    out = np.zeros(8)
    L.s3m_from_float(P(s3m.sim3_13(R, t, s)), P(out))
    if normalise:
        out[:4] /= np.linalg.norm(out[:4])
    return out


def Rmat(L, s8):
    o = np.zeros(13)
    L.s3m_to_13(P(np.ascontiguousarray(s8)), P(o))
    return o[:9].reshape(3, 3)


def smap(L, s8, X):
    o = np.zeros(3)
    L.s3m_map(P(np.ascontiguousarray(s8)), P(np.ascontiguousarray(X, f64)), P(o))
    return o


def inverse(L, s8):
    o = np.zeros(8)
    L.s3m_inverse(P(np.ascontiguousarray(s8)), P(o))
    return o


def oplus(L, u, s8):
    o = np.zeros(8)
    br = L.s3m_oplus(P(np.ascontiguousarray(u, f64)), P(np.ascontiguousarray(s8)), P(o))
    return o, br


def edge(L, s8, K, X, obs, w, inv):
    e, c, J = np.zeros(2), np.zeros(1), np.zeros(14)
    L.s3m_edge(P(np.ascontiguousarray(s8)), P(K), P(np.ascontiguousarray(X, f64)), P(np.ascontiguousarray(obs, f64)),
               float(w), int(inv), P(e), P(c), P(J))
    return e, float(c[0]), J.reshape(2, 7)


def expm(A):
    """Matrix exponential by scaling and squaring of a Taylor series (float64)."""
    k = max(0, int(np.ceil(np.log2(max(np.abs(A).sum(1).max(), 1e-30)))) + 4)
    B = A / 2.0 ** k
    E, T = np.eye(len(A)), np.eye(len(A))
    for i in range(1, 25):
        T = T @ B / i
        E = E + T
    for _ in range(k):
        E = E @ E
    return E


def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], f64)


@pytest.mark.parametrize("u, branch", [
    ([3e-6, -2e-6, 1e-6, 0.1, 0.2, 0.3, 4e-6], 0),     # |sigma| < 1e-5, theta < 1e-5
    ([0.3, -0.2, 0.1, 0.1, 0.2, 0.3, -4e-6], 1),       # |sigma| < 1e-5
    ([3e-6, -2e-6, 1e-6, 0.1, 0.2, 0.3, 0.25], 2),     # theta < 1e-5
    ([0.3, -0.2, 0.1, 0.1, 0.2, 0.3, -0.4], 3),
    ([ND, 0, 0, 0, 0, 0, 0], 0), ([0, 0, 0, 0, 0, 0, -ND], 0),  # the perturbations of the numeric Jacobian
])
def test_exp_update_in_all_four_branches(L, u, branch):
    """Sim3(update) against the matrix exponential of the sim(3) generator [[Omega + sigma I, upsilon],
    [0, 0]] = [[s R, t], [0, 1]], and against a numpy restatement of the branch's own coefficients.
    The three short branches drop the first-order terms of their small quantity (C = 1 for (e^sigma -
    1) / sigma, A = 1/2, B = 1/6, R = I + Omega + Omega^2 with a whole Omega^2): against the exponential
    t is off by up to 1e-5 |upsilon| and R by theta^2 / 2 <= 5e-11; those are the bounds."""
    u = np.array(u, f64)
    out = np.zeros(8)
    assert L.s3m_exp(P(u), P(out)) == branch
    G = np.zeros((4, 4))
    G[:3, :3] = skew(u[:3]) + u[6] * np.eye(3)
    G[:3, 3] = u[3:6]
    E = expm(G)
    assert abs(out[7] - np.exp(u[6])) <= 1e-16 * 2
    assert np.allclose(out[7] * Rmat(L, out), E[:3, :3], rtol=0, atol=2e-10 if branch in (0, 2) else 1e-14)
    assert np.allclose(out[4:7], E[:3, 3], rtol=0, atol=1e-14 if branch == 3 else 1e-5 * np.linalg.norm(u[3:6]))
    # the coefficients as sim3.h:92-135 writes them
    th, sg, s_ = np.linalg.norm(u[:3]), u[6], np.exp(u[6])
    if branch == 0:
        A, B, C = 0.5, 1. / 6., 1.0
    elif branch == 1:
        A, B, C = (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3, 1.0
    elif branch == 2:
        A, B, C = ((sg - 1) * s_ + 1) / sg ** 2, ((0.5 * sg ** 2 - sg + 1) * s_) / sg ** 3, (s_ - 1) / sg
    else:
        a, b, c = s_ * np.sin(th), s_ * np.cos(th), th ** 2 + sg ** 2
        C = (s_ - 1) / sg
        A, B = (a * sg + (1 - b) * th) / (th * c), (C - ((b - 1) * sg + a * th) / c) / th ** 2
    O = skew(u[:3])
    assert np.allclose(out[4:7], (A * O + B * O @ O + C * np.eye(3)) @ u[3:6], rtol=1e-14, atol=1e-18)
    if branch in (0, 2):  # the quaternion is that of I + Omega + Omega^2 exactly as Eigen converts it
        O = skew(u[:3])
        R = np.eye(3) + O + O @ O
        t = np.sqrt(np.trace(R) + 1.0)
        assert out[3] == 0.5 * t and out[0] == (R[2, 1] - R[1, 2]) * (0.5 / t)


def test_update_is_left_multiplication_in_omega_upsilon_sigma_order(L):
    rng = np.random.default_rng(3)
    S = state(L, s3m.rot(rng.normal(0, 0.3, 3)), rng.normal(0, 1, 3), 1.3)
    u = np.array([0.02, -0.01, 0.03, 0.1, -0.2, 0.05, 0.07])
    T, br = oplus(L, u, S)
    assert br == 3
    E = np.zeros(8)
    L.s3m_exp(P(u), P(E))
    X = rng.normal(0, 1, 3) + [0, 0, 5]
    assert np.allclose(smap(L, T, X), smap(L, E, smap(L, S, X)), rtol=0, atol=1e-14)
    assert T[7] == E[7] * S[7]
    # sigma is the last entry: it alone scales
    T2, _ = oplus(L, [0, 0, 0, 0, 0, 0, 0.5], S)
    assert np.allclose(smap(L, T2, X), np.exp(0.5) * smap(L, S, X), rtol=0, atol=1e-14)
    # upsilon is entries 3..5: it alone translates
    T3, _ = oplus(L, [0, 0, 0, 0.1, 0.2, 0.3, 0], S)
    assert np.allclose(smap(L, T3, X), smap(L, S, X) + [0.1, 0.2, 0.3], rtol=0, atol=1e-14)


def test_inverse_and_product_map_a_point_to_itself(L):
    rng = np.random.default_rng(4)
    for sc in (0.5, 1.0, 2.0):
        S = state(L, s3m.rot(rng.normal(0, 0.5, 3)), rng.normal(0, 1, 3), sc)
        X = rng.normal(0, 1, 3) + [0, 0, 5]
        Si = inverse(L, S)
        assert Si[7] == 1. / S[7] and np.array_equal(Si[:3], -S[:3]) and Si[3] == S[3]
        assert np.allclose(smap(L, Si, smap(L, S, X)), X, rtol=0, atol=1e-14)
        I = np.zeros(8)
        L.s3m_mul(P(S), P(Si), P(I))
        assert np.allclose(smap(L, I, X), X, rtol=0, atol=1e-14)
        assert np.allclose(I, [0, 0, 0, 1, 0, 0, 0, 1], rtol=0, atol=1e-15)
    # the quaternion of a float matrix is not unit and nothing normalises it: S^-1 S is then off by
    # |q|^2 - 1, about a float32 ulp
    S = state(L, s3m.rot([0.3, 0.2, -0.4]), [0.1, 0.2, 0.3], 1.1, normalise=False)
    assert abs(np.linalg.norm(S[:4]) - 1) > 1e-10
    X = np.array([0.5, -0.4, 6.0])
    d = np.abs(smap(L, inverse(L, S), smap(L, S, X)) - X).max()
    assert 1e-12 < d < 5e-6


def analytic_jacobians(L, S, X1, X2):
    """d e12 / du and d e21 / du at u = 0 for the update Sim3(u) * S, u = (omega, upsilon, sigma)."""
    def dproj(K, Q):
        return np.array([[K[0] / Q[2], 0, -K[0] * Q[0] / Q[2] ** 2], [0, K[1] / Q[2], -K[1] * Q[1] / Q[2] ** 2]])

    Pc = smap(L, S, X2)  # d(exp(u) Pc)/du = [-[Pc]x  I  Pc]
    J12 = -dproj(K1, Pc) @ np.hstack([-skew(Pc), np.eye(3), Pc[:, None]])
    Q = smap(L, inverse(L, S), X1)  # (exp(u) S)^-1 X = S^-1 exp(-u) X
    A = Rmat(L, S).T / S[7]
    J21 = dproj(K2, Q) @ A @ np.hstack([-skew(X1), np.eye(3), X1[:, None]])
    return J12, J21


def test_numeric_jacobian_of_both_edges_against_the_analytic_one(L):
    """The model's Jacobian is g2o's numeric one: (e(+1e-9) - e(-1e-9)) / 2e-9 through oplus.  Its
    distance from the analytic Jacobian is rounding noise: an error evaluation carries about 10
    roundings of relative size eps = 2.2e-16 on values up to |u| = the pixel coordinate (<= 640 here),
    twice (two evaluations), divided by 2 delta: 2 * 10 * eps * 640 / 2e-9 = 1.4e-3.  The truncation
    error (delta^2 * f''' / 6) is below 1e-12.  Entries of J are of order 100 to 3000."""
    rng = np.random.default_rng(5)
    bound = 2 * 10 * np.finfo(f64).eps * 640 / (2 * ND)
    worst = 0.0
    for _ in range(20):
        S = state(L, s3m.rot(rng.normal(0, 0.2, 3)), rng.normal(0, 0.5, 3), float(rng.uniform(0.5, 2)))
        X2 = rng.uniform(-1, 1, 3) + [0, 0, 6]
        X1 = smap(L, S, X2) + rng.normal(0, 0.01, 3)
        obs = rng.uniform(0, 300, 2)
        J12, J21 = analytic_jacobians(L, S, X1, X2)
        _, _, N12 = edge(L, S, K1, X2, obs, 1.0, 0)
        _, _, N21 = edge(L, S, K2, X1, obs, 1.0, 1)
        worst = max(worst, np.abs(N12 - J12).max(), np.abs(N21 - J21).max())
        assert np.abs(J12).max() > 50 and np.abs(J21).max() > 50
    print(f"numeric - analytic Jacobian: worst {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound
    assert worst > 1e-9, "the difference noise is part of what the reference computes"


def three_pairs(rng, L):
    S = state(L, s3m.rot(rng.normal(0, 0.1, 3)), rng.normal(0, 0.3, 3), 1.1, normalise=False)
    X2 = rng.uniform(-1, 1, (3, 3)) + [0, 0, 6]
    X1 = np.array([smap(L, S, x) for x in X2])
    o1 = np.array([edge(L, S, K1, X2[i], [0, 0], 1, 0)[0] for i in range(3)]) * -1 + rng.normal(0, 1, (3, 2))
    o2 = np.array([edge(L, S, K2, X1[i], [0, 0], 1, 1)[0] for i in range(3)]) * -1 + rng.normal(0, 1, (3, 2))
    o1[2] += [9, -7]  # one edge on the Huber branch
    w1, w2 = np.array([1.0, 0.6944, 0.4823]), np.array([1.0, 1.44, 2.0736])
    return S, X1, X2, o1, o2, w1, w2


def build(L, S, X1, X2, o1, o2, w1, w2, order=0):
    H, b = np.zeros(49), np.zeros(7)
    n = len(X1)
    a = [np.ascontiguousarray(v, f64) for v in (X1, X2, o1, o2, w1, w2)]
    chi = L.s3m_build(n, *[P(v) for v in a], P(K1), P(K2), float(TH2), P(np.ascontiguousarray(S)), order, P(H), P(b))
    return H.reshape(7, 7), b, chi


def huber(L, e):
    d, rho = np.zeros(2), np.zeros(3)
    L.s3m_huber(float(TH2), float(e), P(d), P(rho))
    return d, rho


def test_huber_delta_is_a_float_and_the_threshold_is_not(L):
    d, rho = huber(L, 4.0)
    assert d[0] == float(f32(np.sqrt(f32(10.0)))) and d[1] == d[0] * d[0]
    # delta * delta = 10.0000002425..., th2 = 10: the kernel and the classification differ
    assert d[0] == 3.1622776985168457 and d[1] != 10.0 and abs(d[1] - 10.0000002425) < 1e-9
    assert list(rho) == [4.0, 1.0, 0.0]
    _, rho = huber(L, 10.0000001)  # above th2, still on the quadratic branch
    assert rho[1] == 1.0
    _, rho = huber(L, 40.0)
    assert np.isclose(rho[0], 2 * np.sqrt(40) * d[0] - d[1], rtol=1e-15) and np.isclose(rho[1], d[0] / np.sqrt(40))


def test_one_levenberg_step_of_three_pairs_against_numpy(L):
    rng = np.random.default_rng(6)
    S, X1, X2, o1, o2, w1, w2 = three_pairs(rng, L)
    H, b, chi = build(L, S, X1, X2, o1, o2, w1, w2)
    Hn, bn, cn = np.zeros((7, 7)), np.zeros(7), 0.0
    on_huber = 0
    for i in range(3):
        for (K, X, o, w, inv) in ((K1, X2[i], o1[i], w1[i], 0), (K2, X1[i], o2[i], w2[i], 1)):
            e, c2, J = edge(L, S, K, X, o, w, inv)
            assert np.isclose(c2, w * e @ e, rtol=1e-15)
            _, rho = huber(L, c2)
            on_huber += rho[1] != 1.0
            Hn += J.T @ J * (w * rho[1])
            bn += J.T @ (-w * e * rho[1])
            cn += rho[0]
    assert on_huber >= 1
    assert np.allclose(H, Hn, rtol=1e-12, atol=1e-9) and np.allclose(b, bn, rtol=1e-12, atol=1e-9)
    assert np.isclose(chi, cn, rtol=1e-14) and np.array_equal(H, H.T)
    lam = 1e-5 * np.abs(np.diag(H)).max()
    x = np.zeros(7)
    assert L.s3m_solve(P(np.ascontiguousarray(H.reshape(49))), P(b), lam, P(x)) == 1
    assert np.allclose(x, np.linalg.solve(H + lam * np.eye(7), b), rtol=1e-8, atol=1e-12)
    # the sum orders agree to rounding
    for order in (1, 2):
        H2, b2, c2 = build(L, S, X1, X2, o1, o2, w1, w2, order)
        assert np.allclose(H2, H, rtol=1e-13, atol=1e-9) and np.isclose(c2, chi, rtol=1e-14)
    # an indefinite system is refused and x is left alone
    x0 = x.copy()
    assert L.s3m_solve(P(np.ascontiguousarray((-H).reshape(49))), P(b), 0.0, P(x)) == 0 and np.array_equal(x, x0)


def walk(L, c):
    """Optimizer.cc:1857-1916 re-walked in Python over the model's pieces."""
    us = c["usable"].astype(bool)
    idx = np.flatnonzero(us)
    a = {k: c[k][us].astype(f64) for k in ("x3dc1", "x3dc2", "obs1", "obs2", "inv_sigma2_1", "sigma2_2")}
    S = np.zeros(8)
    L.s3m_from_float(P(c["sim3_in"]), P(S))
    S0 = S.copy()
    k1, k2 = np.array(c["K1"], f64), np.array(c["K2"], f64)
    th = float(c["th2"])
    active = np.ones(len(idx), bool)
    log = {"iterations": [0, 0], "trials": 0}
    x = np.zeros(7)
    last = {"S": S.copy()}

    def sysat(S):
        s = {k: np.ascontiguousarray(v[active]) for k, v in a.items()}
        H, b = np.zeros(49), np.zeros(7)
        chi = L.s3m_build(int(active.sum()), P(s["x3dc1"]), P(s["x3dc2"]), P(s["obs1"]), P(s["obs2"]),
                          P(s["inv_sigma2_1"]), P(s["sigma2_2"]), P(k1), P(k2), th, P(np.ascontiguousarray(S)), 0, P(H),
                          P(b))
        return H, b, chi

    def optimize(S, its, r):
        lam, ni, bad_steps = 0.0, 2.0, 0
        for it in range(its):
            log["iterations"][r] += 1
            H, b, cur = sysat(S)
            ini = cur
            if it == 0:
                lam, ni, bad_steps = 1e-5 * max(abs(H[8 * j]) for j in range(7)), 2.0, 0
            qmax = 0
            while True:
                backup = S.copy()
                ok = L.s3m_solve(P(H), P(b), lam, P(x))
                S, _ = oplus(L, x, S)
                last["S"] = S.copy()
                tmp = sysat(S)[2]
                if not ok:
                    tmp = np.finfo(f64).max
                rho = (cur - tmp) / (sum(x[j] * (lam * x[j] + b[j]) for j in range(7)) + 1e-3)
                if rho > 0 and np.isfinite(tmp):
                    lam *= max(1. / 3., min(1. - (2 * rho - 1) ** 3, 2. / 3.))
                    ni, cur = 2.0, tmp
                else:
                    lam *= ni
                    ni *= 2
                    S = backup
                qmax += 1
                log["trials"] += 1
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                break
            bad_steps = bad_steps + 1 if (ini - cur) * 1e3 < ini else 0
            if bad_steps >= 3:
                break
        return S

    def chi2s(S):
        out = np.full((2, len(idx)), np.nan)
        for j in np.flatnonzero(active):
            out[0, j] = edge(L, S, k1, a["x3dc2"][j], a["obs1"][j], a["inv_sigma2_1"][j], 0)[1]
            out[1, j] = edge(L, S, k2, a["x3dc1"][j], a["obs2"][j], a["sigma2_2"][j], 1)[1]
        return out

    kept = us.copy()
    S = optimize(S, 5, 0)
    c1 = chi2s(last["S"])  # the error the last computeActiveErrors left: the last trial's, accepted or not
    fail = (c1[0] > th) | (c1[1] > th)
    kept[idx[fail]] = False
    n_bad = int(fail.sum())
    active &= ~fail
    more = 10 if n_bad > 0 else 5
    if len(idx) - n_bad < 10:
        return {"kept": kept, "n_inliers": 0, "sim3_f64": S0, "n_bad": n_bad, "more": 0, **log}
    S = optimize(S, more, 1)
    c2 = chi2s(last["S"])
    fail = active & ((c2[0] > th) | (c2[1] > th))
    kept[idx[fail]] = False
    return {"kept": kept, "n_inliers": int((active & ~fail).sum()), "sim3_f64": S, "n_bad": n_bad, "more": more, **log}


@pytest.mark.parametrize("name", ["outliers_10", "holes_300", "survivors_9", "pairs_64"])
def test_whole_run_rewalked_in_python(L, name):
    c = s3m.host_cases()[name]
    w, m = walk(L, c), c["model"]
    assert np.array_equal(w["kept"].astype(np.uint8), m["kept"]) and w["n_inliers"] == m["n_inliers"]
    assert (w["n_bad"], w["more"]) == (m["info"].n_bad, m["info"].more_iterations)
    assert w["iterations"] == list(m["info"].iterations) and w["trials"] == m["info"].trials
    assert np.array_equal(w["sim3_f64"], m["sim3_f64"]), "the same statements give the same bits"


def exact_case(seed, n, scale=1.3):
    """make_case with the observations replaced by the exact projections under the true Sim3."""
    c = s3m.make_case(seed, n, outliers=0.0, scale=scale)
    t = c["true"]
    R, tt, sc = t[:9].reshape(3, 3), t[9:12], t[12]
    P1 = sc * (c["x3dc2"].astype(f64) @ R.T) + tt
    P2 = ((c["x3dc1"].astype(f64) - tt) @ R) / sc
    c["obs1"] = np.stack([P1[:, 0] / P1[:, 2] * K1[0] + K1[2], P1[:, 1] / P1[:, 2] * K1[1] + K1[3]], 1).astype(f32)
    c["obs2"] = np.stack([P2[:, 0] / P2[:, 2] * K2[0] + K2[2], P2[:, 1] / P2[:, 2] * K2[1] + K2[3]], 1).astype(f32)
    return c


def test_exact_data_converges_without_outliers(L):
    c = exact_case(20, 60)
    m = s3m.run_case(c)
    assert m["kept"].all() and m["n_inliers"] == 60 and m["info"].n_bad == 0 and m["info"].more_iterations == 5
    assert np.abs(m["sim3"].astype(f64) - c["true"]).max() < 5e-5  # the float32 observations' rounding
    assert np.nanmax(m["chi2"]) < 1e-3 and m["info"].chi2 < 1e-2


def test_one_injected_outlier_pair_gives_ten_more_iterations(L):
    c = exact_case(21, 60)
    c["obs1"][7] += f32([30, -20])
    m = s3m.run_case(c)
    assert m["info"].n_bad == 1 and m["info"].more_iterations == 10 and m["n_inliers"] == 59
    assert not m["kept"][7] and m["kept"].sum() == 59
    assert np.abs(m["sim3"].astype(f64) - c["true"]).max() < 5e-5
    assert s3m.run_case(c, variant=3)["info"].more_iterations == 5


def test_ten_against_nine_surviving_pairs(L):
    cs = s3m.host_cases()
    c9, c10 = cs["survivors_9"], cs["survivors_10"]
    m9, m10 = c9["model"], c10["model"]
    assert m10["info"].n_bad == 10 and m10["info"].more_iterations == 10 and m10["n_inliers"] == 10
    assert m10["info"].iterations[1] > 0 and int(m10["kept"].sum()) == 10
    # 9 left: 0, the input Sim3 (after the quaternion conversion), the 11 slots stay cleared
    assert m9["info"].n_bad == 11 and m9["n_inliers"] == 0 and m9["info"].more_iterations == 0
    assert m9["info"].iterations[1] == 0 and int(m9["kept"].sum()) == 9 and not m9["kept"][:11].any()
    S0 = np.zeros(8)
    L.s3m_from_float(P(c9["sim3_in"]), P(S0))
    assert np.array_equal(m9["sim3_f64"], S0) and np.abs(m9["sim3"] - c9["sim3_in"]).max() < 1e-6
    assert np.isnan(m9["chi2"][1]).all(), "no second classification"
    # the mutant that copies the optimised Sim3 out moves it
    assert not np.array_equal(s3m.run_case(c9, variant=4)["sim3_f64"], S0)


def test_a_pair_whose_e21_alone_fails_loses_both_edges(L):
    c = exact_case(22, 40)
    c["obs2"][3] += f32([20, 10])
    m = s3m.run_case(c)
    assert m["chi2"][0, 0, 3] < 1.0 and m["chi2"][0, 1, 3] > float(TH2), "only e21 fails"
    assert not m["kept"][3] and m["info"].n_bad == 1 and m["n_inliers"] == 39
    assert np.isnan(m["chi2"][1, :, 3]).all(), "neither edge of the pair is in the second optimisation"
    # with only the failing edge removed, e12 of the pair would still be evaluated
    m2 = s3m.run_case(c, variant=2)
    assert np.isfinite(m2["chi2"][0, :, 3]).all() and not m2["kept"][3]


def test_e21_is_weighted_with_sigma2_not_its_inverse(L):
    """A level-3 keypoint in KF2, 2.5 pixels off: sigma2 = 1.2^6 = 2.986 makes chi2 = 2.986 * 6.25 = 18.7
    (somewhat less once the estimate has given way to it) > 10 and the pair goes; 1 / sigma2 would make
    it 2.1 and the pair would stay (Optimizer.cc:1842)."""
    c = exact_case(23, 40)
    c["sigma2_2"][:] = 1.0
    c["inv_sigma2_1"][:] = 1.0
    s2 = float(s3m.LEVEL_SIGMA2[3])
    c["sigma2_2"][5] = s3m.LEVEL_SIGMA2[3]
    c["obs2"][5] += f32([2.5, 0])
    m = s3m.run_case(c)
    assert float(TH2) < m["chi2"][0, 1, 5] <= s2 * 6.25 and m["chi2"][0, 1, 5] > 0.6 * s2 * 6.25
    assert not m["kept"][5] and m["info"].n_bad == 1 and m["info"].more_iterations == 10
    m1 = s3m.run_case(c, variant=1)
    assert 0.6 * 6.25 / s2 < m1["chi2"][0, 1, 5] <= 6.25 / s2 * 1.0001
    assert m1["kept"][5] and m1["info"].n_bad == 0 and m1["info"].more_iterations == 5
    # the same 2.5 pixels at level 0 stay under both
    c["sigma2_2"][5] = 1.0
    assert s3m.run_case(c)["kept"][5]


def test_inverse_edge_maps_with_the_inverse(L):
    c = exact_case(24, 40)
    assert s3m.run_case(c)["kept"].all()
    m6 = s3m.run_case(c, variant=6)  # e21 projected with S: nothing fits
    assert m6["info"].n_bad > 20


def test_threshold_case_is_exact_in_every_order(L):
    c = s3m.threshold_case()
    for order in (0, 1, 2):
        m = s3m.run_case(c, sum_order=order)
        assert np.array_equal(m["chi2"][:, 0, :2], np.full((2, 2), 10.0)) and m["kept"].all()
        assert list(m["info"].iterations) == [1, 1] and m["info"].trials == 2
    m5 = s3m.run_case(c, variant=5)
    assert not m5["kept"][:2].any() and m5["info"].n_bad == 2


def test_no_correspondence(L):
    z3, z2, z1 = np.zeros((0, 3), f32), np.zeros((0, 2), f32), np.zeros(0, f32)
    sin = s3m.sim3_13(s3m.rot([0.1, 0.2, 0.3]), [1, 2, 3], 1.5)
    m = s3m.optimize_sim3(z3, z3, z2, z2, z1, z1, None, K1, K2, TH2, sin)
    assert m["n_inliers"] == 0 and m["info"].n_correspondences == 0 and m["info"].trials == 0
    assert m["info"].lambda_ == -1 and np.abs(m["sim3"] - sin).max() < 1e-6
    # every slot unusable is the same thing
    c = s3m.host_cases()["pairs_64"]
    d = dict(c, usable=np.zeros(64, np.uint8))
    m = s3m.run_case(d)
    assert m["n_inliers"] == 0 and not m["kept"].any() and m["info"].n_correspondences == 0


def test_every_listed_gpu_case_is_decisive():
    for name, c in s3m.host_cases().items():
        assert s3m.decisive(c["model"], c["th2"]), name
