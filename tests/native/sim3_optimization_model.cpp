// sim3_optimization_model.cpp — CPU model of Optimizer::OptimizeSim3 (reference
// src/Optimizer.cc:1721-1917) with the parts of g2o it runs, restated in double.
// The GPU tests and scripts/sim3_optimization_timing.py compare orb_optimize_sim3* with it;
// tests/test_sim3_optimization_model.py proves it on cases worked by hand.
//
//   state           g2o::Sim3 (sim3.h:41-292): quaternion r (never normalised), t, s;
//                   Sim3(Matrix3d, t, s) (64-67), map (144-146), inverse (233-236), operator* (266-272)
//   update          VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): Sim3(update) * estimate,
//                   the 7-vector constructor with its four branches (sim3.h:70-142), update = (omega,
//                   upsilon, sigma)
//   edges           EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ::computeError
//                   (types_seven_dof_expmap.h:138-145, 160-167), cam_map1 / cam_map2 (74-88)
//   Jacobian        neither edge defines linearizeOplus: BaseBinaryEdge's numeric one
//                   (base_binary_edge.hpp:131-205), central differences at 1e-9 through oplus
//   quadratic form  base_binary_edge.hpp:91-113 with RobustKernelHuber (robust_kernel_impl.cpp:78-91)
//   Levenberg       optimization_algorithm_levenberg.cpp:61-189, as in pose_optimization_model.cpp
//   dense solver    LinearSolverDense (linear_solver_dense.h:104-112): Eigen::LDLT, refused when not
//                   positive.  Eigen is not part of the reference tree; ldlt below follows Eigen 3's
//                   documented algorithm and is unpinned, as are Quaterniond(Matrix3d), quaternion *
//                   vector and the quaternion product.
//   schedule        Optimizer.cc:1857-1916
//
// Edge sums run in edge order as g2o adds them, e12_0, e21_0, e12_1, ... (sum_order 0); orders 1
// (pairwise tree) and 2 (reversed) measure how far a result depends on the order.  `variant` builds
// the mutants of scripts/gen_sim3_optimization_golden.py: 1 e21 weighted with 1/sigma2, 2 only the
// failing edge of a pair removed, 3 more_iterations always 5, 4 the return-0 path copies the
// optimised Sim3 out, 5 >= for >, 6 e21 projected with S instead of its inverse.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

namespace {

struct Sim3 {
    double q[4];  // x y z w
    double t[3];
    double s;
};

void cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// Eigen's Quaternion * Vector3
void rotate(const double* q, const double* v, double* o) {
    double uv[3], c[3];
    cross(q, v, uv);
    for (int k = 0; k < 3; ++k) uv[k] += uv[k];
    cross(q, uv, c);
    for (int k = 0; k < 3; ++k) o[k] = v[k] + q[3] * uv[k] + c[k];
}

// Eigen's Quaternion * Quaternion
void quat_mul(const double* a, const double* b, double* o) {
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}

// Eigen's Quaterniond(Matrix3d), m row-major
void quat_from_matrix(const double* m, double* q) {
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t;
        q[1] = (m[2] - m[6]) * t;
        q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
}

// Eigen's toRotationMatrix, row-major
void matrix_from_quat(const double* q, double* R) {
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
    R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
    R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
}

Sim3 sim3_from_float(const float* in13) {  // Sim3(Matrix3d R, t, s): the quaternion is not normalised
    double R[9];
    for (int k = 0; k < 9; ++k) R[k] = (double)in13[k];
    Sim3 S;
    quat_from_matrix(R, S.q);
    for (int k = 0; k < 3; ++k) S.t[k] = (double)in13[9 + k];
    S.s = (double)in13[12];
    return S;
}

void sim3_to_13(const Sim3& S, double* o13) {
    matrix_from_quat(S.q, o13);
    for (int k = 0; k < 3; ++k) o13[9 + k] = S.t[k];
    o13[12] = S.s;
}

void sim3_map(const Sim3& S, const double* X, double* o) {  // s * (r * xyz) + t
    double r[3];
    rotate(S.q, X, r);
    for (int k = 0; k < 3; ++k) o[k] = S.s * r[k] + S.t[k];
}

Sim3 sim3_inverse(const Sim3& S) {  // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    Sim3 I;
    I.q[0] = -S.q[0], I.q[1] = -S.q[1], I.q[2] = -S.q[2], I.q[3] = S.q[3];
    const double f = -1. / S.s;
    const double v[3] = {f * S.t[0], f * S.t[1], f * S.t[2]};
    rotate(I.q, v, I.t);
    I.s = 1. / S.s;
    return I;
}

Sim3 sim3_mul(const Sim3& A, const Sim3& B) {
    Sim3 R;
    quat_mul(A.q, B.q, R.q);
    double rt[3];
    rotate(A.q, B.t, rt);
    for (int k = 0; k < 3; ++k) R.t[k] = A.s * rt[k] + A.t[k];
    R.s = A.s * B.s;
    return R;
}

// Sim3(const Vector7d& update), update = (omega, upsilon, sigma); *branch: 0..3 = (|sigma| < eps ? 0 : 2)
// + (theta < eps ? 0 : 1)
Sim3 sim3_exp(const double* u, int* branch = nullptr) {
    const double* om = u;
    const double* up = u + 3;
    const double sigma = u[6];
    const double theta = std::sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    Sim3 S;
    S.s = std::exp(sigma);
    double O2[9], R[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = O[3 * i] * O[j];
            s += O[3 * i + 1] * O[3 + j];
            s += O[3 * i + 2] * O[6 + j];
            O2[3 * i + j] = s;
        }
    const double eps = 0.00001;
    double A, B, C;
    const bool small_theta = theta < eps;
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (small_theta) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - std::cos(theta)) / (theta2);
            B = (theta - std::sin(theta)) / (theta2 * theta);
        }
        if (branch) *branch = small_theta ? 0 : 1;
    } else {
        C = (S.s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * S.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double a = S.s * std::sin(theta);
            const double b = S.s * std::cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
        if (branch) *branch = small_theta ? 2 : 3;
    }
    if (small_theta) {
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + O[k]) + O2[k];
    } else {
        const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta);
        for (int k = 0; k < 9; ++k) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + a * O[k]) + b * O2[k];
    }
    quat_from_matrix(R, S.q);
    for (int i = 0; i < 3; ++i) {  // t = (A * Omega + B * Omega2 + C * I) * upsilon
        double W[3];
        for (int j = 0; j < 3; ++j) W[j] = (A * O[3 * i + j] + B * O2[3 * i + j]) + C * (i == j ? 1.0 : 0.0);
        double s = W[0] * up[0];
        s += W[1] * up[1];
        s += W[2] * up[2];
        S.t[i] = s;
    }
    return S;
}

Sim3 oplus(const double* u, const Sim3& S, int* branch = nullptr) { return sim3_mul(sim3_exp(u, branch), S); }

struct Cam {
    double fx, fy, cx, cy;
};

// obs - cam_map(project(M.map(X))): M is the estimate for e12 and its inverse for e21
void edge_error(const Sim3& M, const Cam& c, const double* X, const double* obs, double* e) {
    double P[3];
    sim3_map(M, X, P);
    e[0] = obs[0] - ((P[0] / P[2]) * c.fx + c.cx);
    e[1] = obs[1] - ((P[1] / P[2]) * c.fy + c.cy);
}

double edge_chi2(const double* e, double s) { return e[0] * (s * e[0]) + e[1] * (s * e[1]); }

constexpr double ND_DELTA = 1e-9;

// The estimates of the numeric Jacobian: index 0 the estimate itself, 1 + 2d / 2 + 2d its oplus with
// +delta / -delta along dimension d; inv: the inverse of each (what e21 maps with).
struct States {
    Sim3 fwd[15], inv[15];
};

void make_states(const Sim3& S, States& st) {
    st.fwd[0] = S;
    for (int d = 0; d < 7; ++d) {
        double u[7] = {0, 0, 0, 0, 0, 0, 0};
        u[d] = ND_DELTA;
        st.fwd[1 + 2 * d] = oplus(u, S);
        u[d] = -ND_DELTA;
        st.fwd[2 + 2 * d] = oplus(u, S);
    }
    for (int k = 0; k < 15; ++k) st.inv[k] = sim3_inverse(st.fwd[k]);
}

// BaseBinaryEdge::linearizeOplus: J 2 x 7 row-major, column d = (1 / (2 delta)) * (e(+) - e(-))
void edge_jacobian(const Sim3* M15, const Cam& c, const double* X, const double* obs, double* J) {
    const double scalar = 1.0 / (2 * ND_DELTA);
    for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        edge_error(M15[1 + 2 * d], c, X, obs, ep);
        edge_error(M15[2 + 2 * d], c, X, obs, em);
        J[d] = scalar * (ep[0] - em[0]);
        J[7 + d] = scalar * (ep[1] - em[1]);
    }
}

struct Huber {
    double delta, dsqr;
    void robustify(double e, double* rho) const {
        if (e <= dsqr) {
            rho[0] = e, rho[1] = 1., rho[2] = 0.;
        } else {
            const double sqrte = std::sqrt(e);
            rho[0] = 2 * sqrte * delta - dsqr;
            rho[1] = delta / sqrte;
            rho[2] = -0.5 * rho[1] / e;
        }
    }
};

Huber make_huber(float th2) {
    const float deltaHuber = std::sqrt(th2);  // Optimizer.cc:1770, a float
    Huber h;
    h.delta = (double)deltaHuber;
    h.dsqr = h.delta * h.delta;
    return h;
}

// Sum of rows [lo, hi) of `w` doubles in the given order.
void sum_rows(const std::vector<double>& v, int w, int lo, int hi, int order, double* out) {
    for (int k = 0; k < w; ++k) out[k] = 0;
    if (order == 1) {
        if (hi - lo <= 0) return;
        if (hi - lo == 1) {
            for (int k = 0; k < w; ++k) out[k] = v[(size_t)lo * w + k];
            return;
        }
        std::vector<double> a(w), b(w);
        const int mid = lo + (hi - lo + 1) / 2;
        sum_rows(v, w, lo, mid, 1, a.data());
        sum_rows(v, w, mid, hi, 1, b.data());
        for (int k = 0; k < w; ++k) out[k] = a[k] + b[k];
    } else if (order == 2) {
        for (int i = hi - 1; i >= lo; --i)
            for (int k = 0; k < w; ++k) out[k] += v[(size_t)i * w + k];
    } else {
        for (int i = lo; i < hi; ++i)
            for (int k = 0; k < w; ++k) out[k] += v[(size_t)i * w + k];
    }
}

// Eigen::LDLT of the N x N A (full symmetric storage, overwritten) and the solve of A x = b.
// false: not positive (LDLT::isPositive), x untouched.
template <int N>
bool ldlt(double* A, const double* b, double* x) {
    int tr[N];
    int sign = 0;  // 0 zero, 1 positive semi-definite, -1 negative semi-definite, 2 indefinite
    for (int k = 0; k < N; ++k) {
        int p = k;
        double big = std::fabs(A[(N + 1) * k]);
        for (int i = k + 1; i < N; ++i)
            if (std::fabs(A[(N + 1) * i]) > big) big = std::fabs(A[(N + 1) * i]), p = i;
        tr[k] = p;
        if (p != k) {
            for (int j = 0; j < N; ++j) std::swap(A[N * k + j], A[N * p + j]);
            for (int j = 0; j < N; ++j) std::swap(A[N * j + k], A[N * j + p]);
        }
        double temp[N];
        for (int j = 0; j < k; ++j) temp[j] = A[(N + 1) * j] * A[N * k + j];
        for (int j = 0; j < k; ++j) A[(N + 1) * k] -= A[N * k + j] * temp[j];
        for (int i = k + 1; i < N; ++i) {
            double s = A[N * i + k];
            for (int j = 0; j < k; ++j) s -= A[N * i + j] * temp[j];
            A[N * i + k] = s;
        }
        const double akk = A[(N + 1) * k];
        if (std::fabs(akk) > 0)
            for (int i = k + 1; i < N; ++i) A[N * i + k] /= akk;
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
    for (int k = 0; k < N; ++k) y[k] = b[k];
    for (int k = 0; k < N; ++k) std::swap(y[k], y[tr[k]]);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < i; ++j) y[i] -= A[N * i + j] * y[j];
    const double tol = 1.0 / DBL_MAX;
    for (int i = 0; i < N; ++i) y[i] = std::fabs(A[(N + 1) * i]) > tol ? y[i] / A[(N + 1) * i] : 0.0;
    for (int i = N - 1; i >= 0; --i)
        for (int j = i + 1; j < N; ++j) y[i] -= A[N * j + i] * y[j];
    for (int k = N - 1; k >= 0; --k) std::swap(y[k], y[tr[k]]);
    for (int k = 0; k < N; ++k) x[k] = y[k];
    return true;
}

constexpr int ROW = 35;  // 28 of H (upper triangle), 7 of b

struct Problem {
    int n = 0;  // pairs
    std::vector<double> X1, X2, obs1, obs2, w1, w2;  // w1 / w2: the information of e12 / e21
    std::vector<int> idx;
    Cam cam1, cam2;
    Huber rk;
    int order = 0, variant = 0;
    std::vector<uint8_t> off12, off21;  // the edge was removed from the optimisation
    std::vector<double> chi12, chi21;   // the edges' chi2 of their last computeError
    std::vector<double> rows;

    int n_active() const {
        int m = 0;
        for (int i = 0; i < n; ++i) m += (off12[i] ? 0 : 1) + (off21[i] ? 0 : 1);
        return m;
    }
    const Sim3& m21(const Sim3* fwd, const Sim3* inv, int k) const { return variant == 6 ? fwd[k] : inv[k]; }

    // computeActiveErrors + activeRobustChi2
    double evaluate(const Sim3& S) {
        const Sim3 Si = sim3_inverse(S);
        rows.assign((size_t)2 * n, 0.0);
        int m = 0;
        for (int i = 0; i < n; ++i) {
            double e[2], rho[3];
            if (!off12[i]) {
                edge_error(S, cam1, &X2[3 * i], &obs1[2 * i], e);
                chi12[i] = edge_chi2(e, w1[i]);
                rk.robustify(chi12[i], rho);
                rows[m++] = rho[0];
            }
            if (!off21[i]) {
                edge_error(variant == 6 ? S : Si, cam2, &X1[3 * i], &obs2[2 * i], e);
                chi21[i] = edge_chi2(e, w2[i]);
                rk.robustify(chi21[i], rho);
                rows[m++] = rho[0];
            }
        }
        double out;
        sum_rows(rows, 1, 0, m, order, &out);
        return out;
    }

    void edge_row(const Sim3* M15, const Cam& c, const double* X, const double* obs, double w, double* row) const {
        double e[2], rho[3], J[14];
        edge_error(M15[0], c, X, obs, e);
        edge_jacobian(M15, c, X, obs, J);
        rk.robustify(edge_chi2(e, w), rho);
        const double wo = w * rho[1];  // weightedOmega = rho[1] * omega
        const double r0 = (-(w * e[0])) * rho[1], r1 = (-(w * e[1])) * rho[1];
        int k = 0;
        for (int j = 0; j < 7; ++j)
            for (int l = j; l < 7; ++l) row[k++] = (J[j] * wo) * J[l] + (J[7 + j] * wo) * J[7 + l];
        for (int j = 0; j < 7; ++j) row[28 + j] = J[j] * r0 + J[7 + j] * r1;
    }

    // buildSystem: H (7 x 7 full) and b
    void build(const Sim3& S, double* H, double* b) {
        States st;
        make_states(S, st);
        rows.assign((size_t)2 * n * ROW, 0.0);
        int m = 0;
        for (int i = 0; i < n; ++i) {
            if (!off12[i]) edge_row(st.fwd, cam1, &X2[3 * i], &obs1[2 * i], w1[i], &rows[(size_t)(m++) * ROW]);
            if (!off21[i])
                edge_row(variant == 6 ? st.fwd : st.inv, cam2, &X1[3 * i], &obs2[2 * i], w2[i],
                         &rows[(size_t)(m++) * ROW]);
        }
        double sum[ROW];
        sum_rows(rows, ROW, 0, m, order, sum);
        int k = 0;
        for (int j = 0; j < 7; ++j)
            for (int l = j; l < 7; ++l) H[7 * j + l] = H[7 * l + j] = sum[k++];
        for (int j = 0; j < 7; ++j) b[j] = sum[28 + j];
    }
};

int g_branches = 0;  // bit k: an accepted update of the last run took branch k of Sim3(update)

struct Info {
    int32_t n_correspondences, n_bad, more_iterations, iterations[2], trials;
    double lambda, chi2;
};

// SparseOptimizer::optimize(its) with OptimizationAlgorithmLevenberg over the active edges
// (x: the solver's solution vector, which a refused solve leaves as it was)
void optimize(Problem& P, Sim3& S, int its, int round, Info& info, double& lambda, double* x) {
    if (P.n_active() == 0) return;
    double ni = 2.;
    int bad_steps = 0;
    for (int it = 0; it < its; ++it) {
        ++info.iterations[round];
        double cur = P.evaluate(S);
        double temp = cur;
        const double ini = cur;
        double H[49], b[7];
        P.build(S, H, b);
        info.chi2 = cur;
        if (it == 0) {  // computeLambdaInit
            double mx = 0.;
            for (int j = 0; j < 7; ++j) mx = std::max(std::fabs(H[8 * j]), mx);
            lambda = 1e-5 * mx;
            ni = 2.;
            bad_steps = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const Sim3 backup = S;
            double A[49];
            std::memcpy(A, H, sizeof A);
            for (int j = 0; j < 7; ++j) A[8 * j] += lambda;
            const bool ok2 = ldlt<7>(A, b, x);
            int branch = 0;
            S = oplus(x, S, &branch);
            temp = P.evaluate(S);
            if (!ok2) temp = DBL_MAX;
            rho = cur - temp;
            double scale = 0.;
            for (int j = 0; j < 7; ++j) scale += x[j] * (lambda * x[j] + b[j]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && std::isfinite(temp)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                const double f = std::max(1. / 3., alpha);
                lambda *= f;
                ni = 2;
                cur = temp;
                g_branches |= 1 << branch;
            } else {
                lambda *= ni;
                ni *= 2;
                S = backup;
            }
            ++qmax;
            ++info.trials;
        } while (rho < 0 && qmax < 10);
        info.chi2 = cur;
        if (qmax == 10 || rho == 0) break;
        if ((ini - cur) * 1e3 < ini) ++bad_steps;
        else bad_steps = 0;
        if (bad_steps >= 3) break;
    }
}

Problem make_problem(int n, const float* x3dc1, const float* x3dc2, const float* obs1, const float* obs2,
                     const float* inv_sigma2_1, const float* sigma2_2, const uint8_t* usable, const float* K1,
                     const float* K2, float th2, int sum_order, int variant) {
    Problem P;
    P.order = sum_order, P.variant = variant;
    P.cam1 = {(double)K1[0], (double)K1[1], (double)K1[2], (double)K1[3]};
    P.cam2 = {(double)K2[0], (double)K2[1], (double)K2[2], (double)K2[3]};
    P.rk = make_huber(th2);
    for (int i = 0; i < n; ++i) {
        if (usable && !usable[i]) continue;
        for (int k = 0; k < 3; ++k) P.X1.push_back((double)x3dc1[3 * i + k]), P.X2.push_back((double)x3dc2[3 * i + k]);
        for (int k = 0; k < 2; ++k) P.obs1.push_back((double)obs1[2 * i + k]), P.obs2.push_back((double)obs2[2 * i + k]);
        P.w1.push_back((double)inv_sigma2_1[i]);
        // Optimizer.cc:1842: GetSigma2, not its inverse
        P.w2.push_back(variant == 1 ? (double)(1.0f / sigma2_2[i]) : (double)sigma2_2[i]);
        P.idx.push_back(i);
    }
    P.n = (int)P.idx.size();
    P.off12.assign(P.n, 0), P.off21.assign(P.n, 0);
    P.chi12.assign(P.n, 0.0), P.chi21.assign(P.n, 0.0);
    return P;
}

}  // namespace

extern "C" {

// The whole routine.  kept (n): the slot is still matched afterwards.  sim3_out_f64: qx qy qz qw t s;
// sim3_out: R row-major, t, s as floats.  chi2_rounds (2 x 2 x n: classification, e12 / e21, slot;
// NaN where there is no edge or the classification did not run).  Returns 0.
int s3m_optimize_sim3(int n, const float* x3dc1, const float* x3dc2, const float* obs1, const float* obs2,
                      const float* inv_sigma2_1, const float* sigma2_2, const uint8_t* usable, const float* K1,
                      const float* K2, float th2, const float* sim3_in, int sum_order, int variant, uint8_t* kept,
                      double* sim3_out_f64, float* sim3_out, int32_t* n_inliers, void* info_out, double* chi2_rounds) {
    Problem P = make_problem(n, x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, sigma2_2, usable, K1, K2, th2, sum_order, variant);
    const int m = P.n;
    g_branches = 0;
    for (int i = 0; i < n; ++i) kept[i] = 0;
    for (int i = 0; i < m; ++i) kept[P.idx[i]] = 1;
    if (chi2_rounds)
        for (size_t k = 0; k < (size_t)4 * n; ++k) chi2_rounds[k] = NAN;
    const Sim3 S0 = sim3_from_float(sim3_in);
    Sim3 S = S0;
    Info info{};
    info.n_correspondences = m;
    double lambda = -1.;
    double x[7] = {0, 0, 0, 0, 0, 0, 0};
    const double th = (double)th2;
    auto fails = [&](double c) { return variant == 5 ? c >= th : c > th; };
    int result = 0;
    bool copy_out = false;
    if (m > 0) {
        optimize(P, S, 5, 0, info, lambda, x);
        int nBad = 0;
        for (int i = 0; i < m; ++i) {
            if (chi2_rounds) chi2_rounds[P.idx[i]] = P.chi12[i], chi2_rounds[(size_t)n + P.idx[i]] = P.chi21[i];
            const bool f12 = fails(P.chi12[i]), f21 = fails(P.chi21[i]);
            if (f12 || f21) {
                kept[P.idx[i]] = 0;
                if (variant == 2) P.off12[i] = f12, P.off21[i] = f21;
                else P.off12[i] = P.off21[i] = 1;
                ++nBad;
            }
        }
        info.n_bad = nBad;
        const int more = (nBad > 0 && variant != 3) ? 10 : 5;
        if (m - nBad >= 10) {
            info.more_iterations = more;
            optimize(P, S, more, 1, info, lambda, x);
            int nIn = 0;
            for (int i = 0; i < m; ++i) {
                if (P.off12[i] || P.off21[i]) continue;
                if (chi2_rounds)
                    chi2_rounds[(size_t)2 * n + P.idx[i]] = P.chi12[i], chi2_rounds[(size_t)3 * n + P.idx[i]] = P.chi21[i];
                if (fails(P.chi12[i]) || fails(P.chi21[i])) kept[P.idx[i]] = 0;
                else ++nIn;
            }
            result = nIn;
            copy_out = true;
        } else if (variant == 4) {
            copy_out = true;
        }
    }
    info.lambda = lambda;
    const Sim3& O = copy_out ? S : S0;
    if (sim3_out_f64) {
        for (int k = 0; k < 4; ++k) sim3_out_f64[k] = O.q[k];
        for (int k = 0; k < 3; ++k) sim3_out_f64[4 + k] = O.t[k];
        sim3_out_f64[7] = O.s;
    }
    if (sim3_out) {
        double M[13];
        sim3_to_13(O, M);
        for (int k = 0; k < 13; ++k) sim3_out[k] = (float)M[k];
    }
    if (n_inliers) *n_inliers = result;
    if (info_out) std::memcpy(info_out, &info, sizeof info);
    return 0;
}

int s3m_last_branches() { return g_branches; }

// ---- the pieces, for the hand-worked checks (sim3 as 8 doubles: qx qy qz qw t s) ----

void s3m_from_float(const float* in13, double* s8) {
    const Sim3 S = sim3_from_float(in13);
    std::memcpy(s8, &S, sizeof S);
}
void s3m_to_13(const double* s8, double* o13) {
    Sim3 S;
    std::memcpy(&S, s8, sizeof S);
    sim3_to_13(S, o13);
}
// Sim3(update); returns the branch taken (0..3)
int s3m_exp(const double* u7, double* s8) {
    int br = 0;
    const Sim3 S = sim3_exp(u7, &br);
    std::memcpy(s8, &S, sizeof S);
    return br;
}
// Sim3(update) * S; returns the branch
int s3m_oplus(const double* u7, const double* s8, double* out8) {
    Sim3 S;
    std::memcpy(&S, s8, sizeof S);
    int br = 0;
    const Sim3 R = oplus(u7, S, &br);
    std::memcpy(out8, &R, sizeof R);
    return br;
}
void s3m_map(const double* s8, const double* X, double* out3) {
    Sim3 S;
    std::memcpy(&S, s8, sizeof S);
    sim3_map(S, X, out3);
}
void s3m_inverse(const double* s8, double* out8) {
    Sim3 S;
    std::memcpy(&S, s8, sizeof S);
    const Sim3 I = sim3_inverse(S);
    std::memcpy(out8, &I, sizeof I);
}
void s3m_mul(const double* a8, const double* b8, double* out8) {
    Sim3 A, B;
    std::memcpy(&A, a8, sizeof A);
    std::memcpy(&B, b8, sizeof B);
    const Sim3 R = sim3_mul(A, B);
    std::memcpy(out8, &R, sizeof R);
}
// One edge at S: inverse = 0 e12 (maps with S), 1 e21 (maps with S^-1).  e (2), chi2 = w e'e and the
// numeric Jacobian J (2 x 7).
void s3m_edge(const double* s8, const double* K4, const double* X, const double* obs, double w, int inverse, double* e,
              double* chi2, double* J) {
    Sim3 S;
    std::memcpy(&S, s8, sizeof S);
    States st;
    make_states(S, st);
    const Cam c{K4[0], K4[1], K4[2], K4[3]};
    const Sim3* M = inverse ? st.inv : st.fwd;
    edge_error(M[0], c, X, obs, e);
    *chi2 = edge_chi2(e, w);
    edge_jacobian(M, c, X, obs, J);
}
// H (49), b (7) and the robust chi2 over n pairs, all active; w1 / w2 the edges' information
double s3m_build(int n, const double* X1, const double* X2, const double* obs1, const double* obs2, const double* w1,
                 const double* w2, const double* K1, const double* K2, float th2, const double* s8, int sum_order,
                 double* H, double* b) {
    Problem P;
    P.n = n, P.order = sum_order;
    P.X1.assign(X1, X1 + 3 * n), P.X2.assign(X2, X2 + 3 * n);
    P.obs1.assign(obs1, obs1 + 2 * n), P.obs2.assign(obs2, obs2 + 2 * n);
    P.w1.assign(w1, w1 + n), P.w2.assign(w2, w2 + n);
    P.off12.assign(n, 0), P.off21.assign(n, 0), P.chi12.assign(n, 0.0), P.chi21.assign(n, 0.0);
    P.cam1 = {K1[0], K1[1], K1[2], K1[3]}, P.cam2 = {K2[0], K2[1], K2[2], K2[3]};
    P.rk = make_huber(th2);
    Sim3 S;
    std::memcpy(&S, s8, sizeof S);
    P.build(S, H, b);
    return P.evaluate(S);
}
// (H + lambda I) x = b; 1 solved, 0 refused
int s3m_solve(const double* H, const double* b, double lambda, double* x) {
    double A[49];
    std::memcpy(A, H, sizeof A);
    for (int j = 0; j < 7; ++j) A[8 * j] += lambda;
    return ldlt<7>(A, b, x) ? 1 : 0;
}
// delta, delta * delta and rho (3) of the Huber kernel for th2
void s3m_huber(float th2, double e, double* delta2, double* rho3) {
    const Huber h = make_huber(th2);
    delta2[0] = h.delta, delta2[1] = h.dsqr;
    h.robustify(e, rho3);
}

}  // extern "C"

#ifdef SIM3_MODEL_MAIN
// Stand-alone run for the sanitizers: a synthetic problem through every sum order and variant.
int main() {
    const int n = 300;
    std::vector<float> x1(3 * n), x2(3 * n), o1(2 * n), o2(2 * n), is1(n), s2(n);
    std::vector<uint8_t> usable(n), kept(n);
    const float K[4] = {320.f, 318.5f, 159.5f, 119.25f};
    uint32_t r = 12345u;
    auto rnd = [&]() { r = r * 1664525u + 1013904223u; return (float)(r >> 8) / 16777216.0f; };
    for (int i = 0; i < n; ++i) {
        const float z = 4 + 8 * rnd(), u = 319 * rnd(), v = 239 * rnd();
        x1[3 * i] = (u - K[2]) / K[0] * z, x1[3 * i + 1] = (v - K[3]) / K[1] * z, x1[3 * i + 2] = z;
        // the true S12 is a translation (0.3, -0.2, 0.1) and a scale 1.1: X2 = (X1 - t) / s
        x2[3 * i] = (x1[3 * i] - 0.3f) / 1.1f, x2[3 * i + 1] = (x1[3 * i + 1] + 0.2f) / 1.1f;
        x2[3 * i + 2] = (z - 0.1f) / 1.1f;
        const bool bad = i % 7 == 0;
        o1[2 * i] = u + rnd() - 0.5f + (bad ? 30.f : 0.f), o1[2 * i + 1] = v + rnd() - 0.5f;
        o2[2 * i] = x2[3 * i] / x2[3 * i + 2] * K[0] + K[2] + rnd() - 0.5f;
        o2[2 * i + 1] = x2[3 * i + 1] / x2[3 * i + 2] * K[1] + K[3] + rnd() - 0.5f;
        is1[i] = 1.0f, s2[i] = 1.0f;
        usable[i] = i % 5 != 0;
    }
    const float in13[13] = {1, 0, 0, 0, 1, 0, 0, 0, 1, 0.32f, -0.18f, 0.12f, 1.08f};
    std::vector<double> chi(4 * n);
    for (int order = 0; order < 3; ++order)
        for (int variant = 0; variant <= 6; ++variant) {
            double o64[8];
            float o32[13];
            int32_t nin = 0;
            Info info;
            s3m_optimize_sim3(n, x1.data(), x2.data(), o1.data(), o2.data(), is1.data(), s2.data(), usable.data(), K, K,
                              10.f, in13, order, variant, kept.data(), o64, o32, &nin, &info, chi.data());
            std::printf("order %d variant %d: inliers %d bad %d more %d trials %d s %.17g\n", order, variant, nin,
                        info.n_bad, info.more_iterations, info.trials, o64[7]);
        }
    s3m_optimize_sim3(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, K, K, 10.f, in13, 0, 0, kept.data(),
                      nullptr, nullptr, nullptr, nullptr, nullptr);
    return 0;
}
#endif
