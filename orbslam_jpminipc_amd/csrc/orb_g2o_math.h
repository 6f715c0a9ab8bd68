// orb_g2o_math.h — the double-precision restatement of g2o and Eigen that the GPU optimizers share
// (orb_optimizer.hip: PoseOptimization; orb_sim3opt.hip: OptimizeSim3, §14;
// orb_localba.hip: LocalBundleAdjustment, §21; orb_essgraph.hip: OptimizeEssentialGraph, §22).
//
// One definition each of the quaternion / rotation helpers, the Huber kernel, Eigen's dense LDLT
// solve, the Levenberg bookkeeping of optimization_algorithm_levenberg.cpp, the workgroup sum and
// the prepare kernels' compaction step.  The units that include it are built -ffp-contract=off;
// every sum here has one written order, and that order is part of the contract.
//
// Functions marked ORB_G2O_FN use only + - * /, sqrt, fabs and comparisons, all correctly rounded
// on the host and on the device: the same source compiled by a plain C++ compiler gives the same
// bits (tests/native/g2o_math_host.cpp pins them against the CPU models).  What calls
// sin / cos / pow or a wave intrinsic is device code only and sits in the __HIPCC__ block below.
#pragma once
#include <cfloat>
#include <cmath>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define ORB_G2O_FN __host__ __device__
#else
#define ORB_G2O_FN
#endif

ORB_G2O_FN static inline __attribute__((always_inline)) void cross3(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// Eigen's Quaternion * Vector3: v + w * 2(q x v) + q x 2(q x v); q is x y z w
ORB_G2O_FN static inline __attribute__((always_inline)) void rotate(const double* q, const double* v, double* o) {
    double uv[3], c[3];
    cross3(q, v, uv);
#pragma unroll
    for (int k = 0; k < 3; ++k) uv[k] += uv[k];
    cross3(q, uv, c);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = v[k] + q[3] * uv[k] + c[k];
}

// Eigen's Quaternion * Quaternion (SE3Quat::operator*, Sim3::operator*)
ORB_G2O_FN static inline __attribute__((always_inline)) void quat_mul(const double* a, const double* b, double* o) {
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

// Eigen's Quaterniond(Matrix3d), m row-major.  Eigen picks i = argmax of the diagonal (the first
// largest: i = 0; if (m11 > m00) i = 1; if (m22 > m_ii) i = 2) and indexes by i, j = (i + 1) % 3,
// k = (j + 1) % 3.  That is written out here as one branch per i, which is the form kept of the two
// this tree had: every index is a constant, so q and m stay in registers on the device, and each
// branch can be read against Eigen's line by line.  For every input without a NaN on the diagonal
// the branch taken and the order of each sum are those of the indexed form.
ORB_G2O_FN static inline void quat_from_matrix(const double* m, double* q) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else if (m[0] >= m[4] && m[0] >= m[8]) {  // i = 0: !(m11 > m00) && !(m22 > m00)
        t = sqrt(m[0] - m[4] - m[8] + 1.0);
        q[0] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[7] - m[5]) * t;
        q[1] = (m[3] + m[1]) * t;
        q[2] = (m[6] + m[2]) * t;
    } else if (m[4] > m[0] && m[4] >= m[8]) {  // i = 1
        t = sqrt(m[4] - m[8] - m[0] + 1.0);
        q[1] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[2] - m[6]) * t;
        q[2] = (m[7] + m[5]) * t;
        q[0] = (m[1] + m[3]) * t;
    } else {  // i = 2
        t = sqrt(m[8] - m[0] - m[4] + 1.0);
        q[2] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3] - m[1]) * t;
        q[0] = (m[2] + m[6]) * t;
        q[1] = (m[5] + m[7]) * t;
    }
}

// Eigen's toRotationMatrix, row-major
ORB_G2O_FN static inline void matrix_from_quat(const double* q, double* R) {
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
}

// O = hat(omega) and O2 = O * O, row-major; each entry of O2 a three-term row sum, left to right
ORB_G2O_FN static inline __attribute__((always_inline)) void hat_sq(const double* om, double* O, double* O2) {
    O[0] = 0, O[1] = -om[2], O[2] = om[1];
    O[3] = om[2], O[4] = 0, O[5] = -om[0];
    O[6] = -om[1], O[7] = om[0], O[8] = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = O[3 * i] * O[j];
            s += O[3 * i + 1] * O[3 + j];
            s += O[3 * i + 2] * O[6 + j];
            O2[3 * i + j] = s;
        }
}

// RobustKernelHuber::robustify: rho[0], rho[1]
ORB_G2O_FN static inline __attribute__((always_inline)) void huber(double e, double delta, double dsqr, double* rho0,
                                                                   double* rho1) {
    if (e <= dsqr) {
        *rho0 = e, *rho1 = 1.;
    } else {
        const double sqrte = sqrt(e);
        *rho0 = 2 * sqrte * delta - dsqr;
        *rho1 = delta / sqrte;
    }
}

ORB_G2O_FN static inline __attribute__((always_inline)) void cswap(bool c, double& a, double& b) {
    const double ta = a, tb = b;
    a = c ? tb : ta;
    b = c ? ta : tb;
}

// Eigen::LDLT of the N x N A (full symmetric storage, overwritten) and the solve of A x = b
// (linear_solver_dense.h:104-112; Eigen is not in the reference tree: this follows Eigen 3's
// documented algorithm).  Diagonal pivoting on the largest |a_ii|, the first of equals; the sign is
// tracked over the pivots; false, x untouched, when the matrix is not positive (LDLT::isPositive).
// Every loop is unrolled and every index is a compile-time constant: the pivot exchanges are
// selects, so on the device A stays in registers.
template <int N>
ORB_G2O_FN static inline bool ldlt(double* A, const double* b, double* x) {
    int tr[N];
    int sign = 0;  // 0 zero, 1 positive semi-definite, -1 negative semi-definite, 2 indefinite
#pragma unroll
    for (int k = 0; k < N; ++k) {
        int p = k;
        double big = fabs(A[(N + 1) * k]);
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const double v = fabs(A[(N + 1) * i]);
            const bool g = v > big;
            big = g ? v : big;
            p = g ? i : p;
        }
        tr[k] = p;
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            const bool sw = p == i;
#pragma unroll
            for (int j = 0; j < N; ++j) cswap(sw, A[N * k + j], A[N * i + j]);
#pragma unroll
            for (int j = 0; j < N; ++j) cswap(sw, A[N * j + k], A[N * j + i]);
        }
        double temp[N];
#pragma unroll
        for (int j = 0; j < k; ++j) temp[j] = A[(N + 1) * j] * A[N * k + j];
#pragma unroll
        for (int j = 0; j < k; ++j) A[(N + 1) * k] -= A[N * k + j] * temp[j];
#pragma unroll
        for (int i = k + 1; i < N; ++i) {
            double s = A[N * i + k];
#pragma unroll
            for (int j = 0; j < k; ++j) s -= A[N * i + j] * temp[j];
            A[N * i + k] = s;
        }
        const double akk = A[(N + 1) * k];
        if (fabs(akk) > 0) {
#pragma unroll
            for (int i = k + 1; i < N; ++i) A[N * i + k] /= akk;
        }
        if (sign == 1) {
            if (akk < 0) sign = 2;
        } else if (sign == -1) {
            if (akk > 0) sign = 2;
        } else if (sign == 0) {
            if (akk > 0) sign = 1;
            else if (akk < 0) sign = -1;
        }
    }
    if (!(sign == 1 || sign == 0)) return false;
    double y[N];
#pragma unroll
    for (int k = 0; k < N; ++k) y[k] = b[k];
#pragma unroll
    for (int k = 0; k < N; ++k) {
#pragma unroll
        for (int i = k + 1; i < N; ++i) cswap(tr[k] == i, y[k], y[i]);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int j = 0; j < i; ++j) y[i] -= A[N * i + j] * y[j];
    }
    const double tol = 1.0 / DBL_MAX;
#pragma unroll
    for (int i = 0; i < N; ++i) y[i] = fabs(A[(N + 1) * i]) > tol ? y[i] / A[(N + 1) * i] : 0.0;
#pragma unroll
    for (int i = N - 1; i >= 0; --i) {
#pragma unroll
        for (int j = i + 1; j < N; ++j) y[i] -= A[N * j + i] * y[j];
    }
#pragma unroll
    for (int k = N - 1; k >= 0; --k) {
#pragma unroll
        for (int i = k + 1; i < N; ++i) cswap(tr[k] == i, y[k], y[i]);
    }
#pragma unroll
    for (int k = 0; k < N; ++k) x[k] = y[k];
    return true;
}

// ---- Levenberg bookkeeping (optimization_algorithm_levenberg.cpp:61-189) ----------------------
// The solve kernels keep H as the reduced upper triangle, row-major: N (N + 1) / 2 values `tri`.

// computeLambdaInit: 1e-5 * max |h_jj|
template <int N>
ORB_G2O_FN static inline double lm_lambda_init(const double* tri) {
    double mx = 0.;
#pragma unroll
    for (int j = 0, c = 0; j < N; c += N - j, ++j) {  // std::max(fabs(h_jj), maxDiagonal)
        const double v = fabs(tri[c]);
        mx = v < mx ? mx : v;
    }
    return 1e-5 * mx;
}

// A = H + lambda I, full symmetric storage, as the dense solver is handed it
template <int N>
ORB_G2O_FN static inline void lm_damped(const double* tri, double lambda, double* A) {
    int c = 0;
#pragma unroll
    for (int j = 0; j < N; ++j)
#pragma unroll
        for (int k = j; k < N; ++k) A[N * j + k] = A[N * k + j] = tri[c++];
#pragma unroll
    for (int j = 0; j < N; ++j) A[(N + 1) * j] += lambda;
}

// computeScale: what the decrease of chi2 is divided by to give the gain ratio rho
template <int N>
ORB_G2O_FN static inline double lm_scale(const double* x, double lambda, const double* b) {
    double scale = 0.;
#pragma unroll
    for (int j = 0; j < N; ++j) scale += x[j] * (lambda * x[j] + b[j]);
    scale += 1e-3;
    return scale;
}

// After the trials of one iteration: Terminate (the trial limit, or no change at all), then
// three iterations in a row that gained less than a thousandth of chi2
ORB_G2O_FN static inline bool lm_stop(int qmax, double rho, double ini, double cur, int& bad_steps) {
    if (qmax == 10 || rho == 0) return true;
    if ((ini - cur) * 1e3 < ini) ++bad_steps;
    else bad_steps = 0;
    return bad_steps >= 3;
}

// ---- g2o::Sim3 (types/sim3/sim3.h:41-292) ---------------------------------------------------------
// The state of a VertexSim3Expmap (OptimizeSim3, §14; OptimizeEssentialGraph, §22): a quaternion
// that is never normalised, a translation and a scale.  As eight doubles it is q (x y z w), t, s.
struct Sim3 {
    double q[4];  // x y z w
    double t[3];
    double s;
};

ORB_G2O_FN static inline __attribute__((always_inline)) void sim3_map(const Sim3& S, const double* X,
                                                                      double* o) {  // s * (r * xyz) + t
    double r[3];
    rotate(S.q, X, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = S.s * r[k] + S.t[k];
}

ORB_G2O_FN static inline Sim3 sim3_inverse(const Sim3& S) {  // sim3.h:233-236
    Sim3 I;
    I.q[0] = -S.q[0], I.q[1] = -S.q[1], I.q[2] = -S.q[2], I.q[3] = S.q[3];
    const double f = -1. / S.s;
    const double v[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
    rotate(I.q, v, I.t);
    I.s = 1. / S.s;
    return I;
}

ORB_G2O_FN static inline Sim3 sim3_mul(const Sim3& A, const Sim3& B) {  // Sim3::operator* (sim3.h:266-272)
    Sim3 r;
    quat_mul(A.q, B.q, r.q);
    double rt[3];
    rotate(A.q, B.t, rt);
#pragma unroll
    for (int k = 0; k < 3; ++k) r.t[k] = A.s * rt[k] + A.t[k];
    r.s = A.s * B.s;
    return r;
}

// Sim3(Matrix3d R, t, 1.0) of a keyframe's Tcw = [Rcw row-major | tcw] (Optimizer.cc:1515-1517): the
// floats widened, the quaternion of the widened R, not normalised
ORB_G2O_FN static inline Sim3 sim3_from_pose(const float* Tcw) {
    Sim3 S;
    double R[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = (double)Tcw[k];
    quat_from_matrix(R, S.q);
#pragma unroll
    for (int k = 0; k < 3; ++k) S.t[k] = (double)Tcw[9 + k];
    S.s = 1.0;
    return S;
}

// [R | t * (1 / s)] of a Sim3, twelve doubles (Optimizer.cc:1676-1682; LoopClosing.cc:498-506)
ORB_G2O_FN static inline void sim3_to_pose(const Sim3& S, double* M) {
    matrix_from_quat(S.q, M);
    const double is = 1. / S.s;
#pragma unroll
    for (int k = 0; k < 3; ++k) M[9 + k] = S.t[k] * is;
}

// x = W^-1 t as Eigen's Matrix3d::lu().solve(): PartialPivLU, the pivot of a column the largest
// |entry| on or below the diagonal (the first of equals), rows exchanged, then the unit-lower and the
// upper substitution.  Eigen is not in the reference tree, so the order inside it is not pinned
// ("unpinned").  The exchanges are selects: no index depends on the data.
ORB_G2O_FN static inline void lu3_solve(const double* W, const double* t, double* x) {
    double a00 = W[0], a01 = W[1], a02 = W[2], a10 = W[3], a11 = W[4], a12 = W[5], a20 = W[6], a21 = W[7], a22 = W[8];
    double b0 = t[0], b1 = t[1], b2 = t[2];
    {  // column 0
        const double m1 = fabs(a00) < fabs(a10) ? fabs(a10) : fabs(a00);
        const bool p2 = fabs(a20) > m1;
        const bool p1 = !p2 && fabs(a10) > fabs(a00);
        cswap(p1, a00, a10), cswap(p1, a01, a11), cswap(p1, a02, a12), cswap(p1, b0, b1);
        cswap(p2, a00, a20), cswap(p2, a01, a21), cswap(p2, a02, a22), cswap(p2, b0, b2);
    }
    a10 /= a00, a20 /= a00;
    a11 -= a10 * a01, a12 -= a10 * a02;
    a21 -= a20 * a01, a22 -= a20 * a02;
    {  // column 1
        const bool p2 = fabs(a21) > fabs(a11);
        cswap(p2, a10, a20), cswap(p2, a11, a21), cswap(p2, a12, a22), cswap(p2, b1, b2);
    }
    a21 /= a11;
    a22 -= a21 * a12;
    b1 -= a10 * b0;
    b2 -= a20 * b0;
    b2 -= a21 * b1;
    x[2] = b2 / a22;
    x[1] = (b1 - a12 * x[2]) / a11;
    x[0] = ((b0 - a01 * x[1]) - a02 * x[2]) / a00;
}

// Functions marked ORB_G2O_LIBM_FN are one source for the host and the device too, but call log /
// acos / sin / cos: the two libraries round those differently, so their bits are not pinned across
// the two, only their values (tests/native/essential_graph_host.cpp).
#define ORB_G2O_LIBM_FN ORB_G2O_FN

// Which of log()'s four branches an evaluation took, and how far it sat from the two tests
// (|sigma| against eps, d against 1 - eps): what the scene generators' margins are read from.
struct Sim3LogTrace {
    double sigma, d;
    int branch;  // bit 0: |sigma| >= eps, bit 1: d <= 1 - eps
};

// Sim3::log() (sim3.h:148-230): (omega, upsilon, sigma)
ORB_G2O_LIBM_FN static inline void sim3_log(const Sim3& S, double* res, Sim3LogTrace* trace = nullptr) {
    const double sigma = log(S.s);
    double R[9];
    matrix_from_quat(S.q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};  // deltaR (se3_ops.hpp:40-47)
    const double eps = 0.00001;
    double omega[3], A, B, C;
    const bool near = d > 1 - eps;
    if (fabs(sigma) < eps) {
        C = 1;
        if (near) {
#pragma unroll
            for (int k = 0; k < 3; ++k) omega[k] = 0.5 * dR[k];
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d);
            const double theta2 = theta * theta;
            const double f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
            for (int k = 0; k < 3; ++k) omega[k] = f * dR[k];
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (near) {
            const double sigma2 = sigma * sigma;
#pragma unroll
            for (int k = 0; k < 3; ++k) omega[k] = 0.5 * dR[k];
            A = ((sigma - 1) * S.s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            const double f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
            for (int k = 0; k < 3; ++k) omega[k] = f * dR[k];
            const double theta2 = theta * theta;
            const double a = S.s * sin(theta);
            const double b = S.s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    if (trace) trace->sigma = sigma, trace->d = d, trace->branch = (fabs(sigma) < eps ? 0 : 1) | (near ? 0 : 2);
    // W = A * Omega + B * Omega * Omega + C * I: (B * Omega) * Omega, each entry a row sum left to right
    const double O[9] = {0, -omega[2], omega[1], omega[2], 0, -omega[0], -omega[1], omega[0], 0};
    double W[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = (B * O[3 * i]) * O[j];
            s += (B * O[3 * i + 1]) * O[3 + j];
            s += (B * O[3 * i + 2]) * O[6 + j];
            W[3 * i + j] = (A * O[3 * i + j] + s) + C * (i == j ? 1.0 : 0.0);
        }
    lu3_solve(W, S.t, res + 3);
#pragma unroll
    for (int k = 0; k < 3; ++k) res[k] = omega[k];
    res[6] = sigma;
}

#ifdef __HIPCC__

// One trial's verdict: accepted (true) scales lambda by 1 - (2 rho - 1)^3 clamped to [1/3, 2/3] and
// resets ni; rejected multiplies lambda by ni and doubles ni (the caller restores its backup).
__device__ static inline bool lm_accept(double rho, double chi2_trial, double& lambda, double& ni) {
    if (rho > 0 && isfinite(chi2_trial)) {
        double alpha = 1. - pow(2 * rho - 1, 3.0);
        alpha = 2. / 3. < alpha ? 2. / 3. : alpha;           // std::min(alpha, upper)
        const double f = 1. / 3. < alpha ? alpha : 1. / 3.;  // std::max(lower, alpha)
        lambda *= f;
        ni = 2;
        return true;
    }
    lambda *= ni;
    ni *= 2;
    return false;
}

// The rotation of exp(omega) from hat_sq's O, O2 and theta = |omega| (se3quat.h:237-249,
// sim3.h:118-128): I + O + O2 below 1e-5, Rodrigues' formula above
__device__ static inline void rodrigues(const double* O, const double* O2, double theta, double* R) {
    if (theta < 0.00001) {
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + O[k]) + O2[k];
    } else {
        const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta);
#pragma unroll
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + a * O[k]) + b * O2[k];
    }
}

// The SE3 state of a VertexSE3Expmap: SE3Quat as quaternion plus translation (PoseOptimization,
// LocalBundleAdjustment)
struct Pose {
    double q[4];  // x y z w
    double t[3];
};

__device__ __forceinline__ void normalize_rotation(Pose& p) {  // se3quat.h:280-285
    if (p.q[3] < 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) p.q[k] *= -1;
    }
    const double n = sqrt(p.q[0] * p.q[0] + p.q[1] * p.q[1] + p.q[2] * p.q[2] + p.q[3] * p.q[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) p.q[k] /= n;
}

// VertexSE3Expmap::oplusImpl: exp(x) * T with x = (omega, upsilon)
__device__ Pose exp_update(const double* x, const Pose& T) {
    const double* om = x;
    const double* up = x + 3;
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    double O[9], O2[9], R[9], V[9];
    hat_sq(om, O, O2);
    rodrigues(O, O2, theta, R);
    if (theta < 0.00001) {  // se3quat.h:237-243
#pragma unroll
        for (int k = 0; k < 9; ++k) V[k] = R[k];
    } else {
        const double b = (1 - cos(theta)) / (theta * theta), c = (theta - sin(theta)) / pow(theta, 3.0);
#pragma unroll
        for (int k = 0; k < 9; ++k) V[k] = ((k % 4 == 0 ? 1.0 : 0.0) + b * O[k]) + c * O2[k];
    }
    Pose e;
    quat_from_matrix(R, e.q);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double s = V[3 * i] * up[0];
        s += V[3 * i + 1] * up[1];
        s += V[3 * i + 2] * up[2];
        e.t[i] = s;
    }
    normalize_rotation(e);
    // SE3Quat::operator* (se3quat.h:104-110): t += r * T.t; r *= T.r; normalizeRotation
    Pose r = e;
    double rt[3];
    rotate(e.q, T.t, rt);
#pragma unroll
    for (int k = 0; k < 3; ++k) r.t[k] += rt[k];
    quat_mul(e.q, T.q, r.q);
    normalize_rotation(r);
    return r;
}

// Sim3(update) (sim3.h:70-142); update = (omega, upsilon, sigma)
__device__ static inline Sim3 sim3_exp(const double* u) {
    const double* om = u;
    const double* up = u + 3;
    const double sigma = u[6];
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    Sim3 E;
    E.s = exp(sigma);
    double O[9], O2[9], R[9];
    hat_sq(om, O, O2);
    const double eps = 0.00001;
    double A, B, C;
    const bool small_theta = theta < eps;
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (E.s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * E.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * E.s) / (sigma2 * sigma);
        } else {
            const double a = E.s * sin(theta);
            const double b = E.s * cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    rodrigues(O, O2, theta, R);
    quat_from_matrix(R, E.q);
#pragma unroll
    for (int i = 0; i < 3; ++i) {  // t = (A * Omega + B * Omega2 + C * I) * upsilon
        double W[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) W[j] = (A * O[3 * i + j] + B * O2[3 * i + j]) + C * (i == j ? 1.0 : 0.0);
        double s = W[0] * up[0];
        s += W[1] * up[1];
        s += W[2] * up[2];
        E.t[i] = s;
    }
    return E;
}

// VertexSim3Expmap::oplusImpl: Sim3(update) * T
__device__ static inline Sim3 sim3_oplus(const double* u, const Sim3& T) { return sim3_mul(sim3_exp(u), T); }

constexpr int G2O_WAVES = 4;  // both optimizers run 256-thread workgroups

// Sum of v[0..W) over the workgroup, in a fixed order (an xor butterfly across the wave, lane 0 of
// each wave to its LDS row, the waves in order); every thread gets the same bits.
template <int W, int NACC>
__device__ __forceinline__ void block_sum(double* v, double (*s_red)[NACC]) {
    static_assert(W <= NACC, "the LDS row holds W values");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < W; ++k) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[k] += __shfl_xor(v[k], m);
    }
    __syncthreads();  // the readers of the last reduction are done
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < W; ++k) s_red[wave][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < W; ++k) {
        double s = s_red[0][k];
#pragma unroll
        for (int w = 1; w < G2O_WAVES; ++w) s += s_red[w][k];
        v[k] = s;
    }
}

// One step of an index-ordered compaction over the workgroup: ballot + popcount prefix in the wave,
// the wave totals through s_wtot[G2O_WAVES].  Returns the thread's output slot (-1 where !ok) and
// advances `base`, which every thread keeps, by the step's total.  Every thread of the workgroup
// calls it; it may be called again at once.
__device__ __forceinline__ int compact_slot(bool ok, int* s_wtot, int& base) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long bal = __ballot(ok);
    if (lane == 0) s_wtot[wave] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
#pragma unroll
    for (int w = 0; w < G2O_WAVES; ++w) {
        const int t = s_wtot[w];
        if (w < wave) off += t;
        tot += t;
    }
    base += tot;
    __syncthreads();  // s_wtot may be written again
    return ok ? off + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
}

#endif  // __HIPCC__
