"""csrc/orb_cv_math.h, the OpenCV 2.4 small-matrix arithmetic the GPU units share, compiled for the host
(tests/native/cv_math_host.cpp -> build/libcv_math_host.so) and pinned byte for byte.

The header uses only + - * /, sqrt, fabs, comparisons and conversions, each correctly rounded on the
host and on the device, and both sides are built -ffp-contract=off: equal bytes is the assertion, no
tolerance.  gemm3_add, sub3, norm3 and dot3 are compared with oracle/ocv_ops.cpp; the rest with numpy
float32 / float64 scalar expressions written here (every numpy scalar operation rounds once, to its
own type), which share no text with the header: run-time indices, a cyclic cofactor formula.

Each set of inputs is a seeded few hundred random cases plus the cases where a wrong reading shows, and
where the issue is one reading against another (short path or general path, float or double
evaluation, narrowing before or after) the test also asserts that the set tells the two apart."""
import ctypes
import itertools
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32, f64 = np.float32, np.float64
N = 300
_vp, _i, _d, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_float
P = lambda a: a.ctypes.data  # noqa: E731
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def L():
    lib = ctypes.CDLL(str(ROOT / "build" / "libcv_math_host.so"))
    sig = {
        "cvm_gemm3_add": (None, [_vp] * 4), "ocv_gemm3_add": (None, [_vp] * 4),
        "cvm_gemm3_add_strided": (None, [_vp, _i, _vp, _i, _vp, _d, _d, _vp]),
        "cvm_gemm_out": (_f, [_f, _d, _f, _d]),
        "cvm_sub3": (None, [_vp] * 3), "ocv_sub3": (None, [_vp] * 3),
        "cvm_norm3": (_d, [_vp]), "ocv_norm3": (_d, [_vp]),
        "cvm_dot3": (_d, [_vp] * 2), "ocv_dot3": (_d, [_vp] * 2),
        "cvm_scale": (_f, [_f, _d]), "cvm_scale3": (None, [_vp, _d, _vp]),
        "cvm_add_weighted": (_f, [_f, _d, _f, _d]),
        "cvm_camera_centre": (None, [_vp] * 3),
        "cvm_mul3": (None, [_vp] * 3), "cvm_mul3_alpha": (None, [_vp, _vp, _d, _vp]),
        "cvm_gemm3": (None, [_i, _i, _vp, _vp, _d, _vp]),
        "cvm_det3": (_d, [_vp]), "cvm_inv3": (None, [_vp] * 2), "cvm_neg3x3": (None, [_vp] * 2),
        "cvm_hypot_f": (_f, [_f, _f]), "cvm_hypot_d": (_d, [_d, _d]),
    }
    for name, (res, args) in sig.items():
        getattr(lib, name).restype = res
        getattr(lib, name).argtypes = args
    return lib


@pytest.fixture(autouse=True)
def _quiet():
    with np.errstate(all="ignore"):
        yield


def rng(tag):
    return np.random.default_rng([20240607, tag])


def vecs(tag, n, k):
    """n rows of k floats: mixed magnitudes, so that sums round; a few rows of specials at the end."""
    r = rng(tag)
    v = (r.standard_normal((n, k)) * np.exp2(r.integers(-6, 7, (n, k)))).astype(f32)
    v[-1] = 0.0
    v[-2, 0] = INF
    v[-3, k - 1] = NAN
    v[-4] = -0.0
    return v


def bits(x):
    """The bytes of x, every NaN as one canonical NaN: which NaN an operation gives is not the contract."""
    x = np.array(x)
    if x.dtype.kind == "f":
        x[np.isnan(x)] = np.nan
    return x.tobytes()


def out(k):
    return np.full(k, -777.0, f32)


# ---- the restatements ------------------------------------------------------------------------------

def ref_row(a0, a1, a2, b0, b1, b2):
    """gemm's short path: the float row sum, left to right"""
    s = a0 * b0
    s = s + a1 * b1
    return s + a2 * b2


def ref_gemm_out(t, alpha, c, beta):
    return f32(f64(t) * f64(alpha) + f64(c) * f64(beta))


def ref_mul3(a, b):
    a, b = a.reshape(3, 3), b.reshape(3, 3)
    return np.array([ref_row(a[i, 0], a[i, 1], a[i, 2], b[0, j], b[1, j], b[2, j]) for i in range(3) for j in range(3)], f32)


def ref_gemm3(ta, tb, a, b, alpha):
    """the general path: one double accumulator, k ascending, alpha, narrowed once"""
    a, b = a.reshape(3, 3), b.reshape(3, 3)
    a, b = (a.T if ta else a), (b.T if tb else b)
    d = []
    for i in range(3):
        for j in range(3):
            s = f64(0)
            for k in range(3):
                s = s + f64(a[i, k]) * f64(b[k, j])
            d.append(f32(s * f64(alpha)))
    return np.array(d, f32)


def minor(m, i, j):
    """the cofactor C_ij of a 3 x 3 by cyclic indices, every product and the difference in double"""
    r1, r2, c1, c2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return f64(m[r1, c1]) * f64(m[r2, c2]) - f64(m[r1, c2]) * f64(m[r2, c1])


def ref_det3(a):
    m = a.reshape(3, 3)
    # Laplace along row 0, left to right; the middle minor is subtracted (adding the signed cofactor, or
    # negating it, would give the other zero when the minor is 0)
    m01 = f64(m[1, 0]) * f64(m[2, 2]) - f64(m[1, 2]) * f64(m[2, 0])
    return f64(m[0, 0]) * minor(m, 0, 0) - f64(m[0, 1]) * m01 + f64(m[0, 2]) * minor(m, 0, 2)


def ref_inv3(a):
    m = a.reshape(3, 3)
    d = ref_det3(a)
    if d == 0:
        return np.zeros(9, f32)
    d = f64(1) / d
    return np.array([f32(minor(m, j, i) * d) for i in range(3) for j in range(3)], f32)  # the adjugate: C_ji


def ref_hypot(a, b):
    T = type(a)
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * np.sqrt(T(1) + b * b)
    if b > 0:
        a = a / b
        return b * np.sqrt(T(1) + a * a)
    return T(0)


# ---- against oracle/ocv_ops.cpp ----------------------------------------------------------------------

def test_vector_ops_against_ocv_ops(L):
    A, x, t = vecs(1, N, 9), vecs(2, N, 3), vecs(3, N, 3)
    for k in range(N):
        o, r = out(3), out(3)
        L.cvm_gemm3_add(P(A[k]), P(x[k]), P(t[k]), P(o))
        L.ocv_gemm3_add(P(A[k]), P(x[k]), P(t[k]), P(r))
        assert bits(o) == bits(r), ("gemm3_add", k)
        L.cvm_sub3(P(x[k]), P(t[k]), P(o))
        L.ocv_sub3(P(x[k]), P(t[k]), P(r))
        assert bits(o) == bits(r), ("sub3", k)
        assert bits(f64(L.cvm_norm3(P(x[k])))) == bits(f64(L.ocv_norm3(P(x[k])))), ("norm3", k)
        assert bits(f64(L.cvm_dot3(P(x[k]), P(t[k])))) == bits(f64(L.ocv_dot3(P(x[k]), P(t[k])))), ("dot3", k)


def test_gemm3_add_rounds_the_row_sum_to_float_first(L):
    """The set holds rows whose float row sum, widened, differs from the double row sum: a gemm3_add
    that accumulated in double would not pass test_vector_ops_against_ocv_ops."""
    A, x, t = vecs(1, N, 9), vecs(2, N, 3), vecs(3, N, 3)
    told = 0
    for k in range(N - 4):
        o = out(3)
        L.cvm_gemm3_add(P(A[k]), P(x[k]), P(t[k]), P(o))
        wide = [f32(f64(A[k, 3 * i]) * f64(x[k, 0]) + f64(A[k, 3 * i + 1]) * f64(x[k, 1]) + f64(A[k, 3 * i + 2]) * f64(x[k, 2])
                    + f64(t[k, i])) for i in range(3)]
        told += bits(o) != bits(np.array(wide, f32))
    assert told > 0


@pytest.mark.parametrize("stride,tstride", [(3, 1), (4, 4)])
def test_gemm3_add_strided_with_alpha_beta(L, stride, tstride):
    """The strided form with explicit alpha / beta (the solvers' T12 rows; mt12i = O1 - s*R*O2)."""
    A, T, x = vecs(4, N, 2 * stride + 3), vecs(5, N, 2 * tstride + 1), vecs(6, N, 3)
    ab = rng(7).standard_normal((N, 2))
    ab[:3] = [[1.0, 1.0], [-1.0, 0.0], [-0.75, 1.0]]
    for k in range(N):
        o = out(3)
        L.cvm_gemm3_add_strided(P(A[k]), stride, P(T[k]), tstride, P(x[k]), ab[k, 0], ab[k, 1], P(o))
        r = [ref_gemm_out(ref_row(A[k, i * stride], A[k, i * stride + 1], A[k, i * stride + 2], *x[k]), ab[k, 0],
                          T[k, i * tstride], ab[k, 1]) for i in range(3)]
        assert bits(o) == bits(np.array(r, f32)), k
        assert bits(f32(L.cvm_gemm_out(x[k, 0], ab[k, 0], x[k, 1], ab[k, 1]))) == \
            bits(ref_gemm_out(x[k, 0], ab[k, 0], x[k, 1], ab[k, 1]))


# ---- 3-vectors against numpy -------------------------------------------------------------------------

def test_scale_narrows_alpha_before_the_multiply(L):
    x = vecs(8, N, 3)
    alphas = list(rng(9).standard_normal(N - 3)) + [0.1, 1.0 / 3.0, INF]
    told = 0
    for k in range(N):
        al = alphas[k]
        o = out(3)
        L.cvm_scale3(P(x[k]), al, P(o))
        r = np.array([e * f32(al) + f32(0) for e in x[k]], f32)
        assert bits(o) == bits(r), k
        assert bits(f32(L.cvm_scale(x[k, 0], al))) == bits(r[0])
        told += bits(r) != bits(np.array([f32(f64(e) * f64(al)) for e in x[k]], f32))  # the multiply in double
    assert told > 0
    assert f64(f32(0.1)) != f64(0.1)  # an alpha that float does not hold
    # 0 * inf: n == 0 observations in UpdateNormalAndDepth
    assert np.isnan(L.cvm_scale(0.0, f64(1) / f64(0)))
    z, o = np.zeros(3, f32), out(3)
    L.cvm_scale3(P(z), INF, P(o))
    assert np.isnan(o).all()


def test_add_weighted_is_evaluated_in_double(L):
    a, b = vecs(10, N, 1)[:, 0], vecs(11, N, 1)[:, 0]
    ab = rng(12).standard_normal((N, 2))
    ab[:, 1] = np.where(np.arange(N) % 2 == 0, -1.0, ab[:, 1])  # Triangulate's beta
    ab[1::4, 1] = 1.0                                           # UpdateNormalAndDepth's
    told = 0
    for k in range(N):
        got = f32(L.cvm_add_weighted(a[k], ab[k, 0], b[k], ab[k, 1]))
        want = f32(f64(a[k]) * f64(ab[k, 0]) + f64(b[k]) * f64(ab[k, 1]) + f64(0))
        assert bits(got) == bits(want), k
        told += bits(want) != bits(f32(a[k] * f32(ab[k, 0]) + b[k] * f32(ab[k, 1])))  # the float evaluation
    assert told > 0


def test_camera_centre(L):
    R, t = vecs(13, N, 9), vecs(14, N, 3)
    for k in range(N):
        o = out(3)
        L.cvm_camera_centre(P(R[k]), P(t[k]), P(o))
        r = []
        for i in range(3):
            s = f64(0)
            for j in range(3):
                s = s + f64(R[k, 3 * j + i]) * f64(t[k, j])
            r.append(f32(s * f64(-1)))
        assert bits(o) == bits(np.array(r, f32)), k


# ---- 3 x 3 against numpy -------------------------------------------------------------------------------

def test_short_path_and_general_path(L):
    """mul3 is the float row sum, gemm3<false, false> the double accumulator: the set holds products on
    which the two differ, so neither can stand in for the other."""
    A, B = vecs(15, N, 9), vecs(16, N, 9)
    differ = 0
    for k in range(N):
        o, g = out(9), out(9)
        L.cvm_mul3(P(A[k]), P(B[k]), P(o))
        L.cvm_gemm3(0, 0, P(A[k]), P(B[k]), 1.0, P(g))
        short, general = ref_mul3(A[k], B[k]), ref_gemm3(0, 0, A[k], B[k], 1.0)
        assert bits(o) == bits(short), k
        assert bits(g) == bits(general), k
        differ += bits(short) != bits(general)
    assert differ > 0


def test_gemm3_flags_and_alpha(L):
    A, B = vecs(17, N, 9), vecs(18, N, 9)
    for (ta, tb), alpha in itertools.product([(0, 0), (0, 1), (1, 0), (1, 1)], [1.0, -1.0]):
        for k in range(N):
            o = out(9)
            L.cvm_gemm3(ta, tb, P(A[k]), P(B[k]), alpha, P(o))
            assert bits(o) == bits(ref_gemm3(ta, tb, A[k], B[k], alpha)), (ta, tb, alpha, k)
    # the flags are told apart: a transposed operand gives another matrix
    o = [out(9) for _ in range(4)]
    for f in range(4):
        L.cvm_gemm3(f >> 1, f & 1, P(A[0]), P(B[0]), 1.0, P(o[f]))
    assert len({bits(x) for x in o}) == 4


def test_mul3_alpha_and_neg(L):
    A, B = vecs(19, N, 9), vecs(20, N, 9)
    al = rng(21).standard_normal(N)
    al[:2] = [1.0, -1.0]
    for k in range(N):
        o = out(9)
        L.cvm_mul3_alpha(P(A[k]), P(B[k]), al[k], P(o))
        assert bits(o) == bits(np.array([f32(f64(e) * f64(al[k])) for e in ref_mul3(A[k], B[k])], f32)), k
        L.cvm_neg3x3(P(A[k]), P(o))
        assert bits(o) == bits(np.array([f32(0) - e for e in A[k]], f32)), k
    z, o = np.zeros(9, f32), out(9)
    L.cvm_neg3x3(P(z), P(o))
    assert not np.signbit(o).any()  # 0 - 0 is +0, not the sign flip's -0


def inv_cases():
    A = vecs(22, N, 9)
    e = f32(2.0 ** -13)
    fixed = {
        "zero": np.zeros(9, f32),
        "equal rows": np.array([1, 2, 3, 1, 2, 3, 4, 5, 6], f32),
        "rank one": np.array([2, 4, 6, 1, 2, 3, 3, 6, 9], f32),
        # det = (1 + e)(1 - e) - 1 = -2^-26: 1 - 2^-26 rounds to 1 in float
        "float zero": np.array([1 + e, 1, 0, 1, 1 - e, 0, 0, 0, 1], f32),
        "K": np.array([458.654, 0, 367.215, 0, 457.296, 248.375, 0, 0, 1], f32),
    }
    return A, fixed


def test_det3_and_inv3(L):
    A, fixed = inv_cases()
    for k, a in itertools.chain(enumerate(A), fixed.items()):
        a = np.ascontiguousarray(a)
        o = out(9)
        L.cvm_inv3(P(a), P(o))
        assert bits(f64(L.cvm_det3(P(a)))) == bits(ref_det3(a)), k
        assert bits(o) == bits(ref_inv3(a)), k
    for name in ("zero", "equal rows", "rank one"):  # det exactly 0: nine zeros
        o = out(9)
        L.cvm_inv3(P(fixed[name]), P(o))
        assert L.cvm_det3(P(fixed[name])) == 0.0 and bits(o) == bits(np.zeros(9, f32)), name
    # the determinant is taken in double: 0 when evaluated in float, and the matrix is inverted
    m = fixed["float zero"]
    assert m[0] * m[4] - m[1] * m[3] == f32(0) and m[8] == 1
    assert L.cvm_det3(P(m)) == -(2.0 ** -26)
    o = out(9)
    L.cvm_inv3(P(m), P(o))
    assert np.isfinite(o).all() and o[0] != 0 and o[4] != 0


# ---- hypot ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T,name", [(f32, "cvm_hypot_f"), (f64, "cvm_hypot_d")])
def test_cv_hypot(L, T, name):
    fn = getattr(L, name)
    r = rng(23)
    pairs = [(T(a), T(b)) for a, b in r.standard_normal((N, 2)) * np.exp2(r.integers(-20, 21, (N, 2)))]
    pairs += [(T(3), T(-4)), (T(-4), T(3)), (T(2), T(2)), (T(0), T(0)), (T(-0.0), T(0)), (T(0), T(5)), (T(5), T(0)),
              (T(INF), T(1)), (T(1), T(-INF)), (T(NAN), T(1)), (T(1e-30), T(1e-38)), (T(np.finfo(T).max), T(1))]
    assert any(abs(a) > abs(b) for a, b in pairs[:N]) and any(abs(b) > abs(a) for a, b in pairs[:N])
    for a, b in pairs:
        assert bits(T(fn(a, b))) == bits(T(ref_hypot(a, b))), (a, b)
    assert fn(0, 0) == 0 and fn(INF, 1) == INF and fn(1, -INF) == INF and fn(3, -4) == 5


# ---- the sanitizers ------------------------------------------------------------------------------------

def test_sanitized_program(tmp_path):
    """The same source as a stand-alone program under AddressSanitizer and UBSan, every function on heap
    buffers of exactly the sizes it may touch."""
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge

    exe = tmp_path / "cv_math_host_san"
    subprocess.run(ge.CV_MATH_HOST_CMD(exe, ("-DCV_MATH_HOST_MAIN", "-g", "-fsanitize=address,undefined",
                                             "-fno-sanitize-recover=all")), check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "status 0" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
