"""csrc/orb_g2o_math.h, the header the two GPU optimizers share, compiled for the host
(tests/native/g2o_math_host.cpp -> build/libg2o_math_host.so) against the two CPU models, byte for byte.

The functions under test use only + - * /, sqrt, fabs and comparisons, each correctly rounded on the
host and on the device, and both sides are built -ffp-contract=off: equal bytes is the assertion, no
tolerance.  The models restate the same pieces of g2o / Eigen independently (run-time indices, an
indexed Quaterniond(Matrix3d), no select-based exchanges), so this pins ldlt<N>'s unrolled form and the
branch-per-index quat_from_matrix to them."""
import ctypes
import pathlib

import numpy as np
import pytest

import pose_optimization_model as pom
import sim3_optimization_model as s3m

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32, f64 = np.float32, np.float64
P = lambda a: a.ctypes.data  # noqa: E731
SENTINEL = -777.0
N_FIXED = 7  # the hand-made systems of g2o_ldlt_case
_vp, _i, _d = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


@pytest.fixture(scope="module")
def G():
    L = ctypes.CDLL(str(ROOT / "build" / "libg2o_math_host.so"))
    L.g2o_ldlt_case_count.restype = _i
    L.g2o_ldlt_case.restype = _i
    L.g2o_ldlt_case.argtypes = [_i, _i, _vp, _vp, _vp]
    L.g2o_solve.restype = _i
    L.g2o_solve.argtypes = [_i, _vp, _vp, _d, _vp]
    for name, n in [("g2o_quat_from_matrix", 2), ("g2o_matrix_from_quat", 2), ("g2o_rotate", 3), ("g2o_quat_mul", 3)]:
        getattr(L, name).argtypes = [_vp] * n
    L.g2o_huber.argtypes = [_d, _d, _vp]
    return L


def model_solve(N):
    return (pom.lib().pom_solve, s3m.lib().s3m_solve)[N - 6]


def system(G, N, idx):
    H, b, lam = np.zeros((N, N)), np.zeros(N), np.zeros(1)
    assert G.g2o_ldlt_case(N, idx, P(H), P(b), P(lam)) == 1
    assert H.tobytes() == H.T.copy().tobytes()
    return H, b, float(lam[0])


def both(G, N, H, b, lam):
    """(accepted, x) of the header's ldlt<N> and of the model's solver, x pre-filled with the sentinel."""
    out = []
    for fn in (lambda *a: G.g2o_solve(N, *a), model_solve(N)):
        x = np.full(N, SENTINEL)
        out.append((fn(P(H), P(b), lam, P(x)), x))
    return out


def pivots(A):
    """The exchange made at every step (the index chosen, strictly-greater search) and the pivots, by
    the textbook algorithm in numpy: what a case is, not what its bits are."""
    A, n = A.copy(), len(A)
    tr, piv = [], []
    for k in range(n):
        p = k + int(np.argmax(np.abs(np.diag(A)[k:])))  # argmax: the first of equals
        tr.append(p)
        A[[k, p]] = A[[p, k]]
        A[:, [k, p]] = A[:, [p, k]]
        piv.append(A[k, k])
        if A[k, k] != 0:
            A[k + 1:, k] /= A[k, k]
            A[k + 1:, k + 1:] -= np.outer(A[k + 1:, k], A[k, k + 1:])
            A[k, k + 1:] = 0
    return tr, np.array(piv)


@pytest.mark.parametrize("N", [6, 7])
class TestLdlt:
    def same(self, G, N, idx, accepted):
        H, b, lam = system(G, N, idx)
        (ok_h, x_h), (ok_m, x_m) = both(G, N, H, b, lam)
        assert ok_h == ok_m == (1 if accepted else 0)
        assert x_h.tobytes() == x_m.tobytes()
        return H, b, x_h

    def test_largest_diagonal_last_at_every_step(self, G, N):
        H, b, x = self.same(G, N, 0, True)
        assert pivots(H)[0][:N - 1] == [N - 1] * (N - 1)  # every k but the last exchanges with the last
        assert np.allclose(H @ x, b, rtol=0, atol=1e-12)

    def test_first_of_two_equal_largest_diagonals_wins(self, G, N):
        H, b, x = self.same(G, N, 1, True)
        assert H[1, 1] == H[3, 3] == np.abs(np.diag(H)).max() and pivots(H)[0][0] == 1
        # the other choice gives other bits: the rows differ, so the assertion above can tell
        Hs, bs = H.copy(), b.copy()
        Hs[[1, 3]] = Hs[[3, 1]]
        Hs[:, [1, 3]] = Hs[:, [3, 1]]
        bs[[1, 3]] = bs[[3, 1]]
        xs = both(G, N, Hs, bs, 0.0)[0][1]
        xs[[1, 3]] = xs[[3, 1]]
        assert xs.tobytes() != x.tobytes()

    def test_exact_zero_pivots_after_elimination(self, G, N):
        H, b, x = self.same(G, N, 2, True)
        piv = pivots(H)[1]
        assert (piv[:N - 2] > 0).all() and (piv[N - 2:] == 0).all()
        assert (x[N - 2:] == 0).all() and (x[:N - 2] != 0).all()  # the zero pivots' unknowns are set to 0

    @pytest.mark.parametrize("idx", [3, 4, 6])
    def test_not_positive_is_refused_and_x_untouched(self, G, N, idx):
        H, b, x = self.same(G, N, idx, False)
        piv = pivots(H)[1]
        assert (piv < 0).any() and ((piv < 0).all() if idx == 3 else (piv > 0).any())
        assert (x == SENTINEL).all()

    def test_all_zero_matrix_is_accepted(self, G, N):
        H, b, x = self.same(G, N, 5, True)
        assert not H.any() and b.any() and (x == 0).all()

    def test_random_normal_equations(self, G, N):
        count = G.g2o_ldlt_case_count()
        assert count == N_FIXED + 200
        lams = set()
        for idx in range(N_FIXED, count):
            H, b, lam = system(G, N, idx)
            lams.add(lam)
            (ok_h, x_h), (ok_m, x_m) = both(G, N, H, b, lam)
            assert ok_h == ok_m == 1, idx
            assert x_h.tobytes() == x_m.tobytes(), idx
        assert lams == {0.0, 1e-8, 1.0}
        assert np.allclose((H + lam * np.eye(N)) @ x_h, b, rtol=0, atol=1e-9)


def rot(axis, angle):
    a = np.asarray(axis, f64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def tie(d, off=(0.125, -0.25, 0.5, 0.0625, -0.375, 0.75)):
    """A matrix (no rotation: the function takes any) with diagonal d and six different off-diagonals."""
    return np.array([[d[0], off[0], off[1]], [off[2], d[1], off[3]], [off[4], off[5], d[2]]], f64)


QUAT_CASES = {
    "positive trace": (rot([1, 2, 3], 0.7), None),
    "i = 0": (rot([1, 0.1, 0.2], 3.0), 0),
    "i = 1": (rot([0.1, 1, -0.2], 3.0), 1),
    "i = 2": (rot([-0.2, 0.1, 1], 3.0), 2),
    "m00 == m11 > m22": (tie([-0.25, -0.25, -0.5]), 0),
    "m00 == m22 > m11": (tie([-0.25, -0.5, -0.25]), 0),
    "m11 == m22 > m00": (tie([-0.5, -0.25, -0.25]), 1),
}


@pytest.mark.parametrize("name", list(QUAT_CASES))
def test_quat_from_matrix(G, name):
    """Against Sim3(R, t, s) of the Sim3 model (the raw quaternion) and Converter::toSE3Quat of the pose
    model (the same, normalised: the sign flip, the left-to-right sum of squares and the four divisions
    are redone here in numpy, which rounds each as the models' compiler does)."""
    R, branch = QUAT_CASES[name]
    R32 = np.ascontiguousarray(R, f32)  # the models take float poses and widen them
    m = R32.astype(f64)
    if branch is None:
        assert np.trace(m) > 0
    else:
        assert np.trace(m) <= 0
        i, j, k = branch, (branch + 1) % 3, (branch + 2) % 3
        assert m[i, i] >= m[j, j] and m[i, i] >= m[k, k]
    q = np.full(4, SENTINEL)
    G.g2o_quat_from_matrix(P(m), P(q))
    if branch is not None:  # the branch taken: Eigen's q[i] = 0.5 * sqrt(m_ii - m_jj - m_kk + 1)
        assert q[i] == 0.5 * np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    s8 = np.zeros(8)
    in13 = np.concatenate([R32.ravel(), np.zeros(4, f32)])  # (kept alive across the calls)
    s3m.lib().s3m_from_float(P(in13), P(s8))
    assert q.tobytes() == s8[:4].tobytes()
    p7 = np.zeros(7)
    pom.lib().pom_pose_from_float(P(in13), P(p7))
    qn = -q if q[3] < 0 else q.copy()
    qn = qn / np.sqrt(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3])
    assert qn.tobytes() == p7[:4].tobytes()


def quats():
    rng = np.random.default_rng(20240611)
    qs = [np.array([0, 0, 0, 1.0]), np.array([0.5, -0.5, 0.5, -0.5]), np.array([0.3, -0.1, 0.2, 1.7])]  # one not unit
    return qs + [v / np.linalg.norm(v) for v in rng.standard_normal((20, 4))]


def test_matrix_from_quat(G):
    for q in quats():
        R = np.full(9, SENTINEL)
        G.g2o_matrix_from_quat(P(q), P(R))
        o13, o12 = np.zeros(13), np.zeros(12)
        s8, p7 = np.concatenate([q, np.zeros(3), [1.0]]), np.concatenate([q, np.zeros(3)])
        s3m.lib().s3m_to_13(P(s8), P(o13))
        pom.lib().pom_pose_to_matrix(P(p7), P(o12))
        assert R.tobytes() == o13[:9].tobytes() == o12[:9].tobytes()


def test_rotate_and_quat_mul(G):
    """Against Sim3::operator* of the Sim3 model, (a, -0, 1) * (b, v, 1): its quaternion is a * b and its
    translation 1 * (a * v) + -0, which is a * v to the bit, the sign of a zero included."""
    rng = np.random.default_rng(7)
    Q = quats()
    for a, b in zip(Q, Q[1:] + Q[:1]):
        v = rng.standard_normal(3) * 10
        o3, o4, r8 = np.full(3, SENTINEL), np.full(4, SENTINEL), np.zeros(8)
        G.g2o_rotate(P(a), P(v), P(o3))
        G.g2o_quat_mul(P(a), P(b), P(o4))
        a8, b8 = np.concatenate([a, np.full(3, -0.0), [1.0]]), np.concatenate([b, v, [1.0]])
        s3m.lib().s3m_mul(P(a8), P(b8), P(r8))
        assert o4.tobytes() == r8[:4].tobytes()
        assert o3.tobytes() == r8[4:7].tobytes()


def test_huber(G):
    d2, rho3, rho2 = np.zeros(2), np.zeros(3), np.zeros(2)
    s3m.lib().s3m_huber(s3m.TH2, 0.0, P(d2), P(rho3))
    deltas = [("s3m", float(d2[0])), ("pom", float(f64(f32(np.sqrt(f64(5.991))))))]
    for which, delta in deltas:
        dsqr = delta * delta
        for e in [0.0, 0.5 * dsqr, np.nextafter(dsqr, 0), dsqr, np.nextafter(dsqr, np.inf), 3.0 * dsqr, 1e6]:
            G.g2o_huber(float(e), delta, P(rho2))
            if which == "s3m":
                s3m.lib().s3m_huber(s3m.TH2, float(e), P(d2), P(rho3))
            else:
                pom.lib().pom_huber(float(e), P(rho3))
            assert rho2.tobytes() == rho3[:2].tobytes(), (which, e)
            if e <= dsqr:  # the quadratic side, the boundary included
                assert rho2[0] == e and rho2[1] == 1.0
            elif e >= 3.0 * dsqr:  # (next to the boundary the linear side rounds to the same values)
                assert rho2[0] < e and rho2[1] < 1.0
