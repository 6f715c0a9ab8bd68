// pose_optimization_model.cpp — CPU model of Optimizer::PoseOptimization(Frame*) (reference
// src/Optimizer.cc:154-285) with the parts of g2o it runs, restated in double.  The
// GPU tests and scripts/pose_optimization_timing.py compare orb_pose_optimization* with it;
// tests/test_pose_optimization_model.py proves it on cases worked by hand.
//
//   pose in / out   Converter::toSE3Quat (Converter.cc:38-48), SE3Quat(R, t) + normalizeRotation
//                   (se3quat.h:58-59, 280-285), to_homogeneous_matrix (270-278)
//   edge            EdgeSE3ProjectXYZ::computeError / cam_project / linearizeOplus
//                   (types_six_dof_expmap.h:172-177, .cpp:384-428)
//   quadratic form  BaseBinaryEdge::constructQuadraticForm, robust branch (base_binary_edge.hpp:91-113),
//                   RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91)
//   Levenberg       OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-189),
//                   SparseOptimizer::optimize (sparse_optimizer.cpp:354-419)
//   update          VertexSE3Expmap::oplusImpl (types_six_dof_expmap.h:104-107), SE3Quat::exp and
//                   operator* (se3quat.h:104-110, 223-257)
//   dense solver    LinearSolverDense (linear_solver_dense.h:104-112): Eigen::LDLT, refused when not
//                   positive.  Eigen is not part of the reference tree; ldlt6 below follows Eigen 3's
//                   documented algorithm (diagonal pivoting, sign tracking) and is unpinned.
//
// Edge sums run in edge order as g2o adds them (sum_order 0); orders 1 (pairwise tree) and 2
// (reversed) measure how far a result depends on the order.  `variant` builds the mutants of
// scripts/gen_pose_optimization_golden.py: 1 Huber weight dropped, 2 level-1 edges left in the
// optimisation, 3 outlier edges not re-evaluated before classification, 4 >= for >, 5 lambda not
// re-initialised per round.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Pose {
    double q[4];  // x y z w
    double t[3];
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

void normalize_rotation(Pose& p) {  // se3quat.h:280-285
    if (p.q[3] < 0)
        for (int k = 0; k < 4; ++k) p.q[k] *= -1;
    const double n = std::sqrt(p.q[0] * p.q[0] + p.q[1] * p.q[1] + p.q[2] * p.q[2] + p.q[3] * p.q[3]);
    for (int k = 0; k < 4; ++k) p.q[k] /= n;
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

Pose pose_from_float(const float* p12) {  // Converter::toSE3Quat
    double R[9];
    for (int k = 0; k < 9; ++k) R[k] = (double)p12[k];
    Pose p;
    quat_from_matrix(R, p.q);
    for (int k = 0; k < 3; ++k) p.t[k] = (double)p12[9 + k];
    normalize_rotation(p);
    return p;
}

void pose_to_matrix(const Pose& p, double* o12) {
    matrix_from_quat(p.q, o12);
    for (int k = 0; k < 3; ++k) o12[9 + k] = p.t[k];
}

// exp(x) * T (oplusImpl); x = (omega, upsilon)
Pose exp_update(const double* x, const Pose& T) {
    const double* om = x;
    const double* up = x + 3;
    const double theta = std::sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double O2[9], R[9], V[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = O[3 * i] * O[j];
            s += O[3 * i + 1] * O[3 + j];
            s += O[3 * i + 2] * O[6 + j];
            O2[3 * i + j] = s;
        }
    if (theta < 0.00001) {
        for (int k = 0; k < 9; ++k) V[k] = R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + O[k]) + O2[k];
    } else {
        const double a = std::sin(theta) / theta, b = (1 - std::cos(theta)) / (theta * theta),
                     c = (theta - std::sin(theta)) / std::pow(theta, 3);
        for (int k = 0; k < 9; ++k) {
            const double I = k % 4 == 0 ? 1.0 : 0.0;
            R[k] = (I + a * O[k]) + b * O2[k];
            V[k] = (I + b * O[k]) + c * O2[k];
        }
    }
    Pose e;
    quat_from_matrix(R, e.q);
    for (int i = 0; i < 3; ++i) {
        double s = V[3 * i] * up[0];
        s += V[3 * i + 1] * up[1];
        s += V[3 * i + 2] * up[2];
        e.t[i] = s;
    }
    normalize_rotation(e);
    // SE3Quat::operator*: t += r * T.t; r *= T.r; normalizeRotation
    Pose r = e;
    double rt[3];
    rotate(e.q, T.t, rt);
    for (int k = 0; k < 3; ++k) r.t[k] += rt[k];
    const double *a = e.q, *b = T.q;
    r.q[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    r.q[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    r.q[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    r.q[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    normalize_rotation(r);
    return r;
}

struct Cam {
    double fx, fy, cx, cy;
};

// computeError; Xc: the mapped point (for the Jacobian)
void edge_error(const Pose& T, const Cam& c, const double* X, const double* obs, double* e, double* Xc) {
    double r[3];
    rotate(T.q, X, r);
    for (int k = 0; k < 3; ++k) Xc[k] = r[k] + T.t[k];
    e[0] = obs[0] - ((Xc[0] / Xc[2]) * c.fx + c.cx);
    e[1] = obs[1] - ((Xc[1] / Xc[2]) * c.fy + c.cy);
}

double edge_chi2(const double* e, double s) { return e[0] * (s * e[0]) + e[1] * (s * e[1]); }

void edge_jacobian(const Cam& c, const double* Xc, double* J) {  // _jacobianOplusXj, 2 x 6 row-major
    const double x = Xc[0], y = Xc[1], z = Xc[2], z_2 = z * z;
    J[0] = x * y / z_2 * c.fx;
    J[1] = -(1 + (x * x / z_2)) * c.fx;
    J[2] = y / z * c.fx;
    J[3] = -1. / z * c.fx;
    J[4] = 0;
    J[5] = x / z_2 * c.fx;
    J[6] = (1 + y * y / z_2) * c.fy;
    J[7] = -x * y / z_2 * c.fy;
    J[8] = -x / z * c.fy;
    J[9] = 0;
    J[10] = -1. / z * c.fy;
    J[11] = y / z_2 * c.fy;
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

// Sum of `n` rows of `w` doubles in the given order.
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

// Eigen::LDLT of the 6 x 6 A (full symmetric storage, overwritten) and the solve of A x = b.
// false: not positive (LDLT::isPositive), x untouched.
bool ldlt6(double* A, const double* b, double* x) {
    int tr[6];
    int sign = 0;  // 0 zero, 1 positive semi-definite, -1 negative semi-definite, 2 indefinite
    for (int k = 0; k < 6; ++k) {
        int p = k;
        double big = std::fabs(A[7 * k]);
        for (int i = k + 1; i < 6; ++i)
            if (std::fabs(A[7 * i]) > big) big = std::fabs(A[7 * i]), p = i;
        tr[k] = p;
        if (p != k) {
            for (int j = 0; j < 6; ++j) std::swap(A[6 * k + j], A[6 * p + j]);
            for (int j = 0; j < 6; ++j) std::swap(A[6 * j + k], A[6 * j + p]);
        }
        // columns < k of the rows hold L, the diagonal holds D
        double temp[6];
        for (int j = 0; j < k; ++j) temp[j] = A[7 * j] * A[6 * k + j];
        for (int j = 0; j < k; ++j) A[7 * k] -= A[6 * k + j] * temp[j];
        for (int i = k + 1; i < 6; ++i) {
            double s = A[6 * i + k];
            for (int j = 0; j < k; ++j) s -= A[6 * i + j] * temp[j];
            A[6 * i + k] = s;
        }
        const double akk = A[7 * k];
        if (std::fabs(akk) > 0)
            for (int i = k + 1; i < 6; ++i) A[6 * i + k] /= akk;
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
    double y[6];
    for (int k = 0; k < 6; ++k) y[k] = b[k];
    for (int k = 0; k < 6; ++k) std::swap(y[k], y[tr[k]]);
    for (int i = 0; i < 6; ++i)
        for (int j = 0; j < i; ++j) y[i] -= A[6 * i + j] * y[j];
    const double tol = 1.0 / DBL_MAX;
    for (int i = 0; i < 6; ++i) y[i] = std::fabs(A[7 * i]) > tol ? y[i] / A[7 * i] : 0.0;
    for (int i = 5; i >= 0; --i)
        for (int j = i + 1; j < 6; ++j) y[i] -= A[6 * j + i] * y[j];
    for (int k = 5; k >= 0; --k) std::swap(y[k], y[tr[k]]);
    for (int k = 0; k < 6; ++k) x[k] = y[k];
    return true;
}

struct Problem {
    int n = 0;  // edges
    std::vector<double> X, obs, s;
    std::vector<int> idx;
    Cam cam;
    Huber rk;
    int order = 0, variant = 0;
    std::vector<uint8_t> level;  // 1: left out of the optimisation
    std::vector<double> chi2;    // the edges' chi2 of their last computeError
    std::vector<double> rows;    // scratch of the sums

    bool active(int i) const { return variant == 2 || !level[i]; }

    // computeActiveErrors + activeRobustChi2
    double evaluate(const Pose& T) {
        rows.assign((size_t)n, 0.0);
        int m = 0;
        for (int i = 0; i < n; ++i) {
            if (!active(i)) continue;
            double e[2], Xc[3], rho[3];
            edge_error(T, cam, &X[3 * i], &obs[2 * i], e, Xc);
            chi2[i] = edge_chi2(e, s[i]);
            rk.robustify(chi2[i], rho);
            rows[m++] = variant == 1 ? chi2[i] : rho[0];
        }
        double out;
        sum_rows(rows, 1, 0, m, order, &out);
        return out;
    }

    // buildSystem: H (6 x 6 full) and b
    void build(const Pose& T, double* H, double* b) {
        rows.assign((size_t)n * 27, 0.0);
        int m = 0;
        for (int i = 0; i < n; ++i) {
            if (!active(i)) continue;
            double e[2], Xc[3], rho[3], J[12];
            edge_error(T, cam, &X[3 * i], &obs[2 * i], e, Xc);
            edge_jacobian(cam, Xc, J);
            rk.robustify(edge_chi2(e, s[i]), rho);
            if (variant == 1) rho[1] = 1.;
            const double w = s[i] * rho[1];  // weightedOmega = rho[1] * omega
            const double r0 = (-(s[i] * e[0])) * rho[1], r1 = (-(s[i] * e[1])) * rho[1];
            double* row = &rows[(size_t)m * 27];
            int c = 0;
            for (int j = 0; j < 6; ++j)
                for (int k = j; k < 6; ++k) row[c++] = (J[j] * w) * J[k] + (J[6 + j] * w) * J[6 + k];
            for (int j = 0; j < 6; ++j) row[21 + j] = J[j] * r0 + J[6 + j] * r1;
            ++m;
        }
        double sum[27];
        sum_rows(rows, 27, 0, m, order, sum);
        int c = 0;
        for (int j = 0; j < 6; ++j)
            for (int k = j; k < 6; ++k) H[6 * j + k] = H[6 * k + j] = sum[c++];
        for (int j = 0; j < 6; ++j) b[j] = sum[21 + j];
    }
};

struct Info {
    int32_t n_initial, n_bad, rounds, iterations[4], trials;
    double lambda, chi2;
};

}  // namespace

extern "C" {

// The whole routine.  chi2_rounds (4 x n, NaN where there is no edge or the round did not run):
// every edge's chi2 as each of the four classifications read it.  Returns 0.
int pom_pose_optimization(int n, const float* p3d, const float* obs, const float* inv_sigma2, const uint8_t* has_mp,
                          float fx, float fy, float cx, float cy, const float* pose_in, int sum_order, int variant,
                          float* pose_out, double* pose_out_f64, uint8_t* outlier, int32_t* n_inliers, void* info_out,
                          double* chi2_rounds) {
    Problem P;
    P.order = sum_order, P.variant = variant;
    P.cam = {(double)fx, (double)fy, (double)cx, (double)cy};
    const float delta = std::sqrt(5.991);  // Optimizer.cc:189
    P.rk.delta = (double)delta;
    P.rk.dsqr = P.rk.delta * P.rk.delta;
    for (int i = 0; i < n; ++i) {
        outlier[i] = 0;
        if (has_mp && !has_mp[i]) continue;
        for (int k = 0; k < 3; ++k) P.X.push_back((double)p3d[3 * i + k]);
        for (int k = 0; k < 2; ++k) P.obs.push_back((double)obs[2 * i + k]);
        P.s.push_back((double)inv_sigma2[i]);
        P.idx.push_back(i);
    }
    const int m = P.n = (int)P.idx.size();
    P.level.assign(m, 0);
    P.chi2.assign(m, 0.0);
    if (chi2_rounds)
        for (size_t k = 0; k < (size_t)4 * n; ++k) chi2_rounds[k] = NAN;
    Pose T = pose_from_float(pose_in);
    const float th[4] = {9.210f, 7.378f, 5.991f, 5.991f};
    const int its[4] = {10, 10, 7, 5};
    Info info{};
    info.n_initial = m;
    double lambda = -1., ni = 2.;
    double x[6] = {0, 0, 0, 0, 0, 0};
    int nBad = 0;
    for (int r = 0; r < 4; ++r) {
        int n_active = 0;
        for (int i = 0; i < m; ++i) n_active += P.active(i) ? 1 : 0;
        int bad_steps = 0;
        for (int it = 0; n_active > 0 && it < its[r]; ++it) {  // SparseOptimizer::optimize
            ++info.iterations[r];
            double cur = P.evaluate(T);
            double temp = cur;
            const double ini = cur;
            double H[36], b[6];
            P.build(T, H, b);
            info.chi2 = cur;
            if (it == 0 && !(variant == 5 && r > 0)) {
                double mx = 0.;
                for (int j = 0; j < 6; ++j) mx = std::max(std::fabs(H[7 * j]), mx);
                lambda = 1e-5 * mx;
                ni = 2.;
            }
            if (it == 0) bad_steps = 0;
            double rho = 0;
            int qmax = 0;
            do {
                const Pose backup = T;
                double A[36];
                std::memcpy(A, H, sizeof A);
                for (int j = 0; j < 6; ++j) A[7 * j] += lambda;
                const bool ok2 = ldlt6(A, b, x);
                T = exp_update(x, T);
                temp = P.evaluate(T);
                if (!ok2) temp = DBL_MAX;
                rho = cur - temp;
                double scale = 0.;
                for (int j = 0; j < 6; ++j) scale += x[j] * (lambda * x[j] + b[j]);
                scale += 1e-3;
                rho /= scale;
                if (rho > 0 && std::isfinite(temp)) {
                    double alpha = 1. - std::pow((2 * rho - 1), 3);
                    alpha = std::min(alpha, 2. / 3.);
                    const double f = std::max(1. / 3., alpha);
                    lambda *= f;
                    ni = 2;
                    cur = temp;
                } else {
                    lambda *= ni;
                    ni *= 2;
                    T = backup;
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
        nBad = 0;
        for (int i = 0; i < m; ++i) {
            if (outlier[P.idx[i]] && variant != 3) {
                double e[2], Xc[3];
                edge_error(T, P.cam, &P.X[3 * i], &P.obs[2 * i], e, Xc);
                P.chi2[i] = edge_chi2(e, P.s[i]);
            }
            const double c = P.chi2[i];
            if (chi2_rounds) chi2_rounds[(size_t)r * n + P.idx[i]] = c;
            const double t = (double)th[r];
            if (variant == 4 ? c >= t : c > t) {
                outlier[P.idx[i]] = 1, P.level[i] = 1, ++nBad;
            } else if (c <= t) {
                outlier[P.idx[i]] = 0, P.level[i] = 0;
            }
        }
        info.rounds = r + 1;
        if (m < 10) break;
    }
    info.n_bad = nBad;
    info.lambda = lambda;
    double M[12];
    pose_to_matrix(T, M);
    for (int k = 0; k < 12; ++k) {
        if (pose_out_f64) pose_out_f64[k] = M[k];
        if (pose_out) pose_out[k] = (float)M[k];
    }
    if (n_inliers) *n_inliers = m - nBad;
    if (info_out) std::memcpy(info_out, &info, sizeof info);
    return 0;
}

// ---- the pieces, for the hand-worked checks ----

// pose7: quaternion x y z w, then t
void pom_pose_from_float(const float* p12, double* pose7) {
    const Pose p = pose_from_float(p12);
    std::memcpy(pose7, &p, sizeof p);
}
void pom_pose_to_matrix(const double* pose7, double* o12) {
    Pose p;
    std::memcpy(&p, pose7, sizeof p);
    pose_to_matrix(p, o12);
}
void pom_exp_update(const double* x6, const double* pose7, double* out7) {
    Pose p;
    std::memcpy(&p, pose7, sizeof p);
    const Pose r = exp_update(x6, p);
    std::memcpy(out7, &r, sizeof r);
}
// error (2), chi2 and the pose Jacobian (2 x 6) of one edge
void pom_edge(const double* pose7, const double* K4, const double* X, const double* obs, double inv_sigma2, double* e,
              double* chi2, double* J) {
    Pose p;
    std::memcpy(&p, pose7, sizeof p);
    const Cam c{K4[0], K4[1], K4[2], K4[3]};
    double Xc[3];
    edge_error(p, c, X, obs, e, Xc);
    *chi2 = edge_chi2(e, inv_sigma2);
    edge_jacobian(c, Xc, J);
}
// H (36), b (6) and the robust chi2 over n edges, all active
double pom_build(int n, const double* X, const double* obs, const double* inv_sigma2, const double* K4,
                 const double* pose7, int sum_order, double* H, double* b) {
    Problem P;
    P.n = n, P.order = sum_order;
    P.X.assign(X, X + 3 * n), P.obs.assign(obs, obs + 2 * n), P.s.assign(inv_sigma2, inv_sigma2 + n);
    P.level.assign(n, 0), P.chi2.assign(n, 0.0);
    P.cam = {K4[0], K4[1], K4[2], K4[3]};
    P.rk.delta = (double)(float)std::sqrt(5.991), P.rk.dsqr = P.rk.delta * P.rk.delta;
    Pose p;
    std::memcpy(&p, pose7, sizeof p);
    P.build(p, H, b);
    return P.evaluate(p);
}
// (H + lambda I) x = b; 1 solved, 0 refused
int pom_solve(const double* H, const double* b, double lambda, double* x) {
    double A[36];
    std::memcpy(A, H, sizeof A);
    for (int j = 0; j < 6; ++j) A[7 * j] += lambda;
    return ldlt6(A, b, x) ? 1 : 0;
}
void pom_huber(double e, double* rho3) {
    Huber h;
    h.delta = (double)(float)std::sqrt(5.991), h.dsqr = h.delta * h.delta;
    h.robustify(e, rho3);
}

}  // extern "C"
