// local_ba_model.cpp — CPU model of Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:287-536)
// with the parts of g2o it runs, restated in double.  The GPU tests and
// scripts/local_ba_timing.py compare orb_local_bundle_adjustment* with it;
// tests/test_local_ba_model.py proves it on cases worked by hand.
//
//   graph           Optimizer.cc:356-447: keyframe vertices (local first, then fixed), marginalised point
//                   vertices, one EdgeSE3ProjectXYZ per observation in a keyframe that is not bad
//   pose in / out   Converter::toSE3Quat, SE3Quat(R, t) + normalizeRotation, to_homogeneous_matrix
//   edge            EdgeSE3ProjectXYZ::computeError / linearizeOplus with both Jacobians
//                   (types_six_dof_expmap.h:172-183, .cpp:384-428)
//   quadratic form  BaseBinaryEdge::constructQuadraticForm, robust branch (base_binary_edge.hpp:91-113)
//   block solver    BlockSolver::buildSystem / setLambda / solve with the Schur complement
//                   (block_solver.hpp:354-486, 502-589).  The reference hands the reduced system to
//                   CHOLMOD; here it is a dense unpivoted L L' that refuses on a pivot that is not
//                   positive and finite.  Eigen's 3 x 3 inverse() is written as cofactors over the
//                   determinant.  Both are unpinned.
//   Levenberg       optimization_algorithm_levenberg.cpp:61-189 over poses and points
//   two rounds      Optimizer.cc:449-515 with MapPoint::EraseObservation's count (MapPoint.cc:71-91)
//
// Edge sums run in edge order (sum_order 0); orders 1 (pairwise tree) and 2 (reversed, the Schur
// sums over the points reversed too) measure how far a result depends on the order.  `variant`
// builds the mutants of scripts/gen_local_ba_golden.py: 1 Huber weight dropped, 2 edges of a point that
// went bad in round 1 removed from round 2, 3 isDepthPositive dropped, 4 lambda not added to Hll,
// 5 >= for >, 6 lambda not re-initialised in round 2.
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

// exp(x) * T (VertexSE3Expmap::oplusImpl); x = (omega, upsilon)
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

// computeError; Xc: the mapped point
void edge_error(const Pose& T, const Cam& c, const double* X, const double* obs, double* e, double* Xc) {
    double r[3];
    rotate(T.q, X, r);
    for (int k = 0; k < 3; ++k) Xc[k] = r[k] + T.t[k];
    e[0] = obs[0] - ((Xc[0] / Xc[2]) * c.fx + c.cx);
    e[1] = obs[1] - ((Xc[1] / Xc[2]) * c.fy + c.cy);
}

double edge_chi2(const double* e, double s) { return e[0] * (s * e[0]) + e[1] * (s * e[1]); }

// _jacobianOplusXi (A, 2 x 3: -1/z * tmp * R, the terms with tmp's two zeros left out) and
// _jacobianOplusXj (B, 2 x 6), row-major
void edge_jacobians(const Pose& T, const Cam& c, const double* Xc, double* A, double* B) {
    const double x = Xc[0], y = Xc[1], z = Xc[2], z_2 = z * z;
    double R[9];
    matrix_from_quat(T.q, R);
    const double m = -1. / z;
    const double m00 = m * c.fx, m02 = m * (-x / z * c.fx), m11 = m * c.fy, m12 = m * (-y / z * c.fy);
    for (int j = 0; j < 3; ++j) {
        A[j] = m00 * R[j] + m02 * R[6 + j];
        A[3 + j] = m11 * R[3 + j] + m12 * R[6 + j];
    }
    B[0] = x * y / z_2 * c.fx;
    B[1] = -(1 + (x * x / z_2)) * c.fx;
    B[2] = y / z * c.fx;
    B[3] = -1. / z * c.fx;
    B[4] = 0;
    B[5] = x / z_2 * c.fx;
    B[6] = (1 + y * y / z_2) * c.fy;
    B[7] = -x * y / z_2 * c.fy;
    B[8] = -x / z * c.fy;
    B[9] = 0;
    B[10] = -1. / z * c.fy;
    B[11] = y / z_2 * c.fy;
}

struct Huber {
    double delta, dsqr;
    void robustify(double e, double* rho) const {
        if (e <= dsqr) {
            rho[0] = e, rho[1] = 1.;
        } else {
            const double sqrte = std::sqrt(e);
            rho[0] = 2 * sqrte * delta - dsqr;
            rho[1] = delta / sqrte;
        }
    }
};

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

// Matrix3d::inverse(): cofactors over the determinant (unpinned)
void inverse3(const double* m, double* o) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    const double id = 1. / det;
    o[0] = c00 * id, o[3] = c01 * id, o[6] = c02 * id;
    o[1] = (m[2] * m[7] - m[1] * m[8]) * id;
    o[4] = (m[0] * m[8] - m[2] * m[6]) * id;
    o[7] = (m[1] * m[6] - m[0] * m[7]) * id;
    o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// Dense unpivoted L L' of the lower triangle of the n x n S (row-major, overwritten by L) and the solve
// of S x = b.  false: a pivot that is not positive and finite.
bool cholesky_solve(std::vector<double>& S, int n, const double* b, double* x) {
    for (int j = 0; j < n; ++j)
        for (int i = j; i < n; ++i) {
            double s = S[(size_t)i * n + j];
            for (int k = 0; k < j; ++k) s -= S[(size_t)i * n + k] * S[(size_t)j * n + k];
            if (i == j) {
                if (!(s > 0) || !std::isfinite(s)) return false;
                S[(size_t)j * n + j] = std::sqrt(s);
            } else {
                S[(size_t)i * n + j] = s / S[(size_t)j * n + j];
            }
        }
    std::vector<double> y(n);
    for (int i = 0; i < n; ++i) {
        double s = b[i];
        for (int j = 0; j < i; ++j) s -= S[(size_t)i * n + j] * y[j];
        y[i] = s / S[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = y[i];
        for (int k = n - 1; k > i; --k) s -= S[(size_t)k * n + i] * x[k];
        x[i] = s / S[(size_t)i * n + i];
    }
    return true;
}

// MapPoint::EraseObservation's count over one classification (Optimizer.cc:453-470, 497-515): the edges
// in order; an edge whose point is bad is skipped, else erased when chi2 > 5.991 or the depth is not
// positive; the point goes bad when its count reaches 2.
void erase_walk(int n_edge, const int32_t* edge_pt, int32_t* nobs, const double* chi2, const double* depth,
                uint8_t* erased, uint8_t* bad, int round, int variant) {
    for (int e = 0; e < n_edge; ++e) {
        if (erased[e]) continue;  // vpEdges[i] == NULL
        const int p = edge_pt[e];
        if (bad[p]) continue;
        const bool over = variant == 5 ? chi2[e] >= 5.991 : chi2[e] > 5.991;
        const bool behind = variant == 3 ? false : !(depth[e] > 0.0);
        if (over || behind) {
            erased[e] = (uint8_t)round;
            if (--nobs[p] <= 2) bad[p] = (uint8_t)round;
        }
    }
}

struct Round {
    int32_t iterations, trials, active_edges, active_points, active_keyframes, refused;
    double lambda, chi2_before, chi2_after;
};
struct Info {
    int32_t status, n_free_kf;
    Round round[2];
};

struct Graph {
    int n_kf = 0, n_pt = 0, n_edge = 0;
    std::vector<Pose> kf;
    std::vector<Cam> cam;
    std::vector<uint8_t> fixed;
    std::vector<double> X, obs, s;
    std::vector<int32_t> ept, ekf, nobs;
    std::vector<int> e0;  // n_pt + 1: the edges of point p are [e0[p], e0[p + 1])
    std::vector<uint8_t> erased, bad, in_opt;
    std::vector<double> chi2, depth;
    Huber rk;
    int order = 0, variant = 0;
    // the system of the last build()
    std::vector<double> Hpp, bp, Hll, bl, Hpl;  // n_kf x 36, n_kf x 6, n_pt x 9, n_pt x 3, n_edge x 18 (6 x 3)
    std::vector<uint8_t> kf_act, pt_act;        // free and with an active edge / with an active edge
    std::vector<double> xp, xl;                 // n_kf x 6, n_pt x 3

    void activate() {  // initializeOptimization()
        kf_act.assign(n_kf, 0), pt_act.assign(n_pt, 0);
        for (int e = 0; e < n_edge; ++e) {
            if (!in_opt[e]) continue;
            pt_act[ept[e]] = 1;
            if (!fixed[ekf[e]]) kf_act[ekf[e]] = 1;
        }
    }

    // computeActiveErrors + activeRobustChi2
    double evaluate() {
        std::vector<double> rows;
        for (int e = 0; e < n_edge; ++e) {
            if (!in_opt[e]) continue;
            double err[2], Xc[3], rho[2];
            edge_error(kf[ekf[e]], cam[ekf[e]], &X[3 * ept[e]], &obs[2 * e], err, Xc);
            chi2[e] = edge_chi2(err, s[e]);
            rk.robustify(chi2[e], rho);
            rows.push_back(variant == 1 ? chi2[e] : rho[0]);
        }
        double out;
        sum_rows(rows, 1, 0, (int)rows.size(), order, &out);
        return out;
    }

    // buildSystem at the current estimates
    void build() {
        Hpp.assign((size_t)n_kf * 36, 0.), bp.assign((size_t)n_kf * 6, 0.);
        Hll.assign((size_t)n_pt * 9, 0.), bl.assign((size_t)n_pt * 3, 0.), Hpl.assign((size_t)n_edge * 18, 0.);
        std::vector<std::vector<double>> rk_(n_kf), rp(n_pt);
        for (int e = 0; e < n_edge; ++e) {
            if (!in_opt[e]) continue;
            const int p = ept[e], i = ekf[e];
            double err[2], Xc[3], rho[2], A[6], B[12];
            edge_error(kf[i], cam[i], &X[3 * p], &obs[2 * e], err, Xc);
            edge_jacobians(kf[i], cam[i], Xc, A, B);
            rk.robustify(edge_chi2(err, s[e]), rho);
            if (variant == 1) rho[1] = 1.;
            const double w = s[e] * rho[1];  // weightedOmega = rho[1] * omega
            const double r0 = (-(s[e] * err[0])) * rho[1], r1 = (-(s[e] * err[1])) * rho[1];
            for (int j = 0; j < 3; ++j)
                for (int k = j; k < 3; ++k) rp[p].push_back((A[j] * w) * A[k] + (A[3 + j] * w) * A[3 + k]);
            for (int j = 0; j < 3; ++j) rp[p].push_back(A[j] * r0 + A[3 + j] * r1);
            if (fixed[i]) continue;
            for (int j = 0; j < 6; ++j)
                for (int k = j; k < 6; ++k) rk_[i].push_back((B[j] * w) * B[k] + (B[6 + j] * w) * B[6 + k]);
            for (int j = 0; j < 6; ++j) rk_[i].push_back(B[j] * r0 + B[6 + j] * r1);
            for (int j = 0; j < 6; ++j)
                for (int k = 0; k < 3; ++k) Hpl[(size_t)e * 18 + 3 * j + k] = (B[j] * w) * A[k] + (B[6 + j] * w) * A[3 + k];
        }
        for (int p = 0; p < n_pt; ++p) {
            double sum[9];
            sum_rows(rp[p], 9, 0, (int)rp[p].size() / 9, order, sum);
            int c = 0;
            for (int j = 0; j < 3; ++j)
                for (int k = j; k < 3; ++k) Hll[(size_t)p * 9 + 3 * j + k] = Hll[(size_t)p * 9 + 3 * k + j] = sum[c++];
            for (int j = 0; j < 3; ++j) bl[(size_t)p * 3 + j] = sum[6 + j];
        }
        for (int i = 0; i < n_kf; ++i) {
            double sum[27];
            sum_rows(rk_[i], 27, 0, (int)rk_[i].size() / 27, order, sum);
            int c = 0;
            for (int j = 0; j < 6; ++j)
                for (int k = j; k < 6; ++k) Hpp[(size_t)i * 36 + 6 * j + k] = Hpp[(size_t)i * 36 + 6 * k + j] = sum[c++];
            for (int j = 0; j < 6; ++j) bp[(size_t)i * 6 + j] = sum[21 + j];
        }
    }

    double max_diagonal() const {  // computeLambdaInit over poses and points
        double mx = 0.;
        for (int i = 0; i < n_kf; ++i)
            if (kf_act[i])
                for (int j = 0; j < 6; ++j) mx = std::max(std::fabs(Hpp[(size_t)i * 36 + 7 * j]), mx);
        for (int p = 0; p < n_pt; ++p)
            if (pt_act[p])
                for (int j = 0; j < 3; ++j) mx = std::max(std::fabs(Hll[(size_t)p * 9 + 4 * j]), mx);
        return mx;
    }

    // BlockSolver::solve with lambda on both diagonals: xp, xl; false (both untouched): refused
    bool solve(double lambda) {
        std::vector<int> ci(n_kf, -1);
        int na = 0;
        for (int i = 0; i < n_kf; ++i)
            if (kf_act[i]) ci[i] = na++;
        const int N = 6 * na;
        std::vector<double> S((size_t)N * N, 0.), coef(N, 0.), bs(N), Dinv((size_t)n_pt * 9), db((size_t)n_pt * 3);
        for (int i = 0; i < n_kf; ++i) {
            if (ci[i] < 0) continue;
            for (int r = 0; r < 6; ++r)
                for (int c = 0; c < 6; ++c)
                    S[(size_t)(6 * ci[i] + r) * N + 6 * ci[i] + c] = Hpp[(size_t)i * 36 + 6 * r + c] + (r == c ? lambda : 0.);
        }
        for (int pp = 0; pp < n_pt; ++pp) {
            const int p = order == 2 ? n_pt - 1 - pp : pp;
            if (!pt_act[p]) continue;
            double D[9];
            for (int k = 0; k < 9; ++k) D[k] = Hll[(size_t)p * 9 + k] + (k % 4 == 0 && variant != 4 ? lambda : 0.);
            double* Di = &Dinv[(size_t)p * 9];
            inverse3(D, Di);
            double* d = &db[(size_t)p * 3];
            for (int j = 0; j < 3; ++j)
                d[j] = Di[3 * j] * bl[(size_t)p * 3] + Di[3 * j + 1] * bl[(size_t)p * 3 + 1] + Di[3 * j + 2] * bl[(size_t)p * 3 + 2];
            for (int a = e0[p]; a < e0[p + 1]; ++a) {
                if (!in_opt[a] || ci[ekf[a]] < 0) continue;
                const int i1 = ci[ekf[a]];
                const double* Ba = &Hpl[(size_t)a * 18];
                double BD[18];
                for (int r = 0; r < 6; ++r)
                    for (int l = 0; l < 3; ++l)
                        BD[3 * r + l] = Ba[3 * r] * Di[l] + Ba[3 * r + 1] * Di[3 + l] + Ba[3 * r + 2] * Di[6 + l];
                for (int r = 0; r < 6; ++r) coef[6 * i1 + r] += Ba[3 * r] * d[0] + Ba[3 * r + 1] * d[1] + Ba[3 * r + 2] * d[2];
                for (int b = e0[p]; b < e0[p + 1]; ++b) {
                    if (!in_opt[b] || ci[ekf[b]] < i1) continue;
                    const int i2 = ci[ekf[b]];
                    const double* Bb = &Hpl[(size_t)b * 18];
                    for (int r = 0; r < 6; ++r)
                        for (int c = 0; c < 6; ++c)
                            S[(size_t)(6 * i1 + r) * N + 6 * i2 + c] -=
                                BD[3 * r] * Bb[3 * c] + BD[3 * r + 1] * Bb[3 * c + 1] + BD[3 * r + 2] * Bb[3 * c + 2];
                }
            }
        }
        for (int i = 0; i < n_kf; ++i)
            if (ci[i] >= 0)
                for (int r = 0; r < 6; ++r) bs[6 * ci[i] + r] = bp[(size_t)i * 6 + r] - coef[6 * ci[i] + r];
        // the solver reads the upper triangle: mirror it into the lower one for L L'
        for (int r = 0; r < N; ++r)
            for (int c = r + 1; c < N; ++c) S[(size_t)c * N + r] = S[(size_t)r * N + c];
        std::vector<double> x(N);
        if (!cholesky_solve(S, N, bs.data(), x.data())) return false;
        for (int i = 0; i < n_kf; ++i)
            if (ci[i] >= 0)
                for (int r = 0; r < 6; ++r) xp[(size_t)i * 6 + r] = x[6 * ci[i] + r];
        for (int p = 0; p < n_pt; ++p) {
            if (!pt_act[p]) continue;
            double cl[3] = {bl[(size_t)p * 3], bl[(size_t)p * 3 + 1], bl[(size_t)p * 3 + 2]};
            for (int a = e0[p]; a < e0[p + 1]; ++a) {
                if (!in_opt[a] || ci[ekf[a]] < 0) continue;
                const double* Ba = &Hpl[(size_t)a * 18];
                const double* xi = &xp[(size_t)ekf[a] * 6];
                for (int k = 0; k < 3; ++k) {
                    double t = Ba[k] * -xi[0];
                    for (int r = 1; r < 6; ++r) t += Ba[3 * r + k] * -xi[r];
                    cl[k] += t;
                }
            }
            const double* Di = &Dinv[(size_t)p * 9];
            for (int j = 0; j < 3; ++j) xl[(size_t)p * 3 + j] = Di[3 * j] * cl[0] + Di[3 * j + 1] * cl[1] + Di[3 * j + 2] * cl[2];
        }
        return true;
    }

    double scale(double lambda) const {  // computeScale, poses then points
        std::vector<double> rows;
        for (int i = 0; i < n_kf; ++i)
            if (kf_act[i])
                for (int j = 0; j < 6; ++j) rows.push_back(xp[(size_t)i * 6 + j] * (lambda * xp[(size_t)i * 6 + j] + bp[(size_t)i * 6 + j]));
        for (int p = 0; p < n_pt; ++p)
            if (pt_act[p])
                for (int j = 0; j < 3; ++j) rows.push_back(xl[(size_t)p * 3 + j] * (lambda * xl[(size_t)p * 3 + j] + bl[(size_t)p * 3 + j]));
        double out;
        sum_rows(rows, 1, 0, (int)rows.size(), order, &out);
        return out;
    }

    void update() {
        for (int i = 0; i < n_kf; ++i)
            if (kf_act[i]) kf[i] = exp_update(&xp[(size_t)i * 6], kf[i]);
        for (int p = 0; p < n_pt; ++p)
            if (pt_act[p])
                for (int k = 0; k < 3; ++k) X[3 * p + k] += xl[(size_t)p * 3 + k];
    }

    void depths() {  // isDepthPositive's z at the current estimates
        for (int e = 0; e < n_edge; ++e) {
            double r[3];
            rotate(kf[ekf[e]].q, &X[3 * ept[e]], r);
            depth[e] = r[2] + kf[ekf[e]].t[2];
        }
    }
};

int load(Graph& G, int n_kf, const float* kf_pose, const float* kf_K, const uint8_t* kf_fixed, int n_pt,
         const float* pt_pos, const int32_t* pt_nobs, int n_edge, const int32_t* edge_pt, const int32_t* edge_kf,
         const float* edge_obs, const float* edge_inv_sigma2) {
    G.n_kf = n_kf, G.n_pt = n_pt, G.n_edge = n_edge;
    for (int i = 0; i < n_kf; ++i) {
        G.kf.push_back(pose_from_float(kf_pose + 12 * i));
        G.cam.push_back({(double)kf_K[4 * i], (double)kf_K[4 * i + 1], (double)kf_K[4 * i + 2], (double)kf_K[4 * i + 3]});
        G.fixed.push_back(kf_fixed[i] ? 1 : 0);
    }
    for (int k = 0; k < 3 * n_pt; ++k) G.X.push_back((double)pt_pos[k]);
    G.nobs.assign(pt_nobs, pt_nobs + n_pt);
    G.e0.assign(n_pt + 1, 0);
    for (int e = 0; e < n_edge; ++e) {
        const int p = edge_pt[e], i = edge_kf[e];
        if (p < 0 || p >= n_pt || i < 0 || i >= n_kf) return -22;
        if (e && p < edge_pt[e - 1]) return -22;
        for (int a = e - 1; a >= 0 && edge_pt[a] == p; --a)
            if (edge_kf[a] == i) return -22;
        ++G.e0[p + 1];
        G.ept.push_back(p), G.ekf.push_back(i);
        G.obs.push_back((double)edge_obs[2 * e]), G.obs.push_back((double)edge_obs[2 * e + 1]);
        G.s.push_back((double)edge_inv_sigma2[e]);
    }
    for (int p = 0; p < n_pt; ++p) {
        if (G.e0[p + 1] > pt_nobs[p]) return -22;
        G.e0[p + 1] += G.e0[p];
    }
    G.erased.assign(n_edge, 0), G.bad.assign(n_pt, 0), G.in_opt.assign(n_edge, 1);
    G.chi2.assign(n_edge, 0.), G.depth.assign(n_edge, 0.);
    G.xp.assign((size_t)n_kf * 6, 0.), G.xl.assign((size_t)n_pt * 3, 0.);
    G.rk.delta = (double)(float)std::sqrt(5.991);  // Optimizer.cc:397
    G.rk.dsqr = G.rk.delta * G.rk.delta;
    return 0;
}

}  // namespace

extern "C" {

int lbm_max_free_kf() { return 64; }

// The whole routine.  chi2_rounds / depth_rounds (2 x n_edge, NaN where the edge was not in that round's
// optimisation): every edge's chi2 and depth as the two classifications read them; kf_pose_round1
// (n_kf x 12, may be NULL): the poses after the first optimize().  Returns the status.
int lbm_local_bundle_adjustment(int n_kf, const float* kf_pose, const float* kf_K, const uint8_t* kf_fixed, int n_pt,
                                const float* pt_pos, const int32_t* pt_nobs, int n_edge, const int32_t* edge_pt,
                                const int32_t* edge_kf, const float* edge_obs, const float* edge_inv_sigma2,
                                int sum_order, int variant, float* kf_pose_out, double* kf_pose_out_f64,
                                float* pt_pos_out, double* pt_pos_out_f64, uint8_t* edge_erased, uint8_t* pt_bad,
                                void* info_out, double* chi2_rounds, double* depth_rounds, double* kf_pose_round1) {
    Graph G;
    G.order = sum_order, G.variant = variant;
    Info info{};
    int n_free = 0;
    for (int i = 0; i < n_kf; ++i) n_free += kf_fixed[i] ? 0 : 1;
    if (n_free == 0 || n_free > lbm_max_free_kf()) return -95;
    if (int r = load(G, n_kf, kf_pose, kf_K, kf_fixed, n_pt, pt_pos, pt_nobs, n_edge, edge_pt, edge_kf, edge_obs,
                     edge_inv_sigma2))
        return r;
    info.n_free_kf = n_free;
    if (chi2_rounds)
        for (size_t k = 0; k < (size_t)2 * n_edge; ++k) chi2_rounds[k] = depth_rounds[k] = NAN;
    double lambda = -1., ni = 2.;
    const int its[2] = {5, 10};
    for (int r = 0; r < 2; ++r) {
        Round& I = info.round[r];
        for (int e = 0; e < n_edge; ++e) G.in_opt[e] = !G.erased[e] && !(variant == 2 && G.bad[G.ept[e]]);
        G.activate();
        for (int e = 0; e < n_edge; ++e) I.active_edges += G.in_opt[e];
        for (int p = 0; p < n_pt; ++p) I.active_points += G.pt_act[p];
        for (int i = 0; i < n_kf; ++i) I.active_keyframes += G.kf_act[i];
        std::fill(G.xp.begin(), G.xp.end(), 0.), std::fill(G.xl.begin(), G.xl.end(), 0.);
        int bad_steps = 0;
        for (int it = 0; I.active_edges > 0 && it < its[r]; ++it) {  // SparseOptimizer::optimize
            ++I.iterations;
            double cur = G.evaluate();
            const double ini = cur;
            G.build();
            if (it == 0) I.chi2_before = cur;
            if (it == 0 && !(variant == 6 && r > 0)) {
                lambda = 1e-5 * G.max_diagonal();
                ni = 2.;
            }
            if (it == 0) bad_steps = 0;
            double rho = 0;
            int qmax = 0;
            do {
                const std::vector<Pose> kf_backup = G.kf;
                const std::vector<double> X_backup = G.X;
                const bool ok2 = G.solve(lambda);
                if (!ok2) ++I.refused;
                G.update();
                double temp = G.evaluate();
                if (!ok2) temp = DBL_MAX;
                rho = cur - temp;
                double scale = G.scale(lambda);
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
                    G.kf = kf_backup, G.X = X_backup;
                }
                ++qmax;
                ++I.trials;
            } while (rho < 0 && qmax < 10);
            I.chi2_after = cur;
            if (qmax == 10 || rho == 0) break;
            if ((ini - cur) * 1e3 < ini) ++bad_steps;
            else bad_steps = 0;
            if (bad_steps >= 3) break;
        }
        I.lambda = lambda;
        if (r == 0 && kf_pose_round1)
            for (int i = 0; i < n_kf; ++i) pose_to_matrix(G.kf[i], kf_pose_round1 + 12 * i);
        G.depths();
        if (chi2_rounds)
            for (int e = 0; e < n_edge; ++e)
                if (G.in_opt[e]) chi2_rounds[(size_t)r * n_edge + e] = G.chi2[e], depth_rounds[(size_t)r * n_edge + e] = G.depth[e];
        erase_walk(n_edge, G.ept.data(), G.nobs.data(), G.chi2.data(), G.depth.data(), G.erased.data(), G.bad.data(),
                   r + 1, variant);
    }
    for (int i = 0; i < n_kf; ++i) {
        double M[12];
        pose_to_matrix(G.kf[i], M);
        for (int k = 0; k < 12; ++k) {
            if (kf_pose_out_f64) kf_pose_out_f64[12 * i + k] = M[k];
            if (kf_pose_out) kf_pose_out[12 * i + k] = (float)M[k];
        }
    }
    for (int k = 0; k < 3 * n_pt; ++k) {
        if (pt_pos_out_f64) pt_pos_out_f64[k] = G.X[k];
        if (pt_pos_out) pt_pos_out[k] = (float)G.X[k];
    }
    if (edge_erased) std::memcpy(edge_erased, G.erased.data(), n_edge);
    if (pt_bad) std::memcpy(pt_bad, G.bad.data(), n_pt);
    if (info_out) std::memcpy(info_out, &info, sizeof info);
    return 0;
}

// ---- the pieces, for the hand-worked checks ----

// pose7: quaternion x y z w, then t
void lbm_pose_from_float(const float* p12, double* pose7) {
    const Pose p = pose_from_float(p12);
    std::memcpy(pose7, &p, sizeof p);
}
void lbm_pose_to_matrix(const double* pose7, double* o12) {
    Pose p;
    std::memcpy(&p, pose7, sizeof p);
    pose_to_matrix(p, o12);
}
void lbm_exp_update(const double* x6, const double* pose7, double* out7) {
    Pose p;
    std::memcpy(&p, pose7, sizeof p);
    const Pose r = exp_update(x6, p);
    std::memcpy(out7, &r, sizeof r);
}
// error (2), chi2, the point Jacobian A (2 x 3) and the pose Jacobian B (2 x 6) of one edge
void lbm_edge(const double* pose7, const double* K4, const double* X, const double* obs, double inv_sigma2, double* e,
              double* chi2, double* A, double* B) {
    Pose p;
    std::memcpy(&p, pose7, sizeof p);
    const Cam c{K4[0], K4[1], K4[2], K4[3]};
    double Xc[3];
    edge_error(p, c, X, obs, e, Xc);
    *chi2 = edge_chi2(e, inv_sigma2);
    edge_jacobians(p, c, Xc, A, B);
}
// The system at the input estimates, every edge active, and one damped step: Hpp (n_kf x 36), bp (n_kf x 6),
// Hll (n_pt x 9), bl (n_pt x 3), Hpl (n_edge x 18, 6 x 3 each), xp (n_kf x 6), xl (n_pt x 3).
// Returns the status, or 1 when the solve was refused.
int lbm_step(int n_kf, const float* kf_pose, const float* kf_K, const uint8_t* kf_fixed, int n_pt, const float* pt_pos,
             const int32_t* pt_nobs, int n_edge, const int32_t* edge_pt, const int32_t* edge_kf, const float* edge_obs,
             const float* edge_inv_sigma2, double lambda, int sum_order, double* Hpp, double* bp, double* Hll, double* bl,
             double* Hpl, double* xp, double* xl) {
    Graph G;
    G.order = sum_order;
    if (int r = load(G, n_kf, kf_pose, kf_K, kf_fixed, n_pt, pt_pos, pt_nobs, n_edge, edge_pt, edge_kf, edge_obs,
                     edge_inv_sigma2))
        return r;
    G.activate();
    G.evaluate();
    G.build();
    const bool ok = G.solve(lambda);
    std::memcpy(Hpp, G.Hpp.data(), G.Hpp.size() * 8), std::memcpy(bp, G.bp.data(), G.bp.size() * 8);
    std::memcpy(Hll, G.Hll.data(), G.Hll.size() * 8), std::memcpy(bl, G.bl.data(), G.bl.size() * 8);
    std::memcpy(Hpl, G.Hpl.data(), G.Hpl.size() * 8);
    std::memcpy(xp, G.xp.data(), G.xp.size() * 8), std::memcpy(xl, G.xl.data(), G.xl.size() * 8);
    return ok ? 0 : 1;
}
void lbm_erase_walk(int n_edge, const int32_t* edge_pt, int32_t* nobs, const double* chi2, const double* depth,
                    uint8_t* erased, uint8_t* bad, int round) {
    erase_walk(n_edge, edge_pt, nobs, chi2, depth, erased, bad, round, 0);
}
// (S + 0) x = b by the dense L L' on a copy of the n x n S; 1 solved, 0 refused
int lbm_cholesky_solve(int n, const double* S, const double* b, double* x) {
    std::vector<double> A(S, S + (size_t)n * n);
    return cholesky_solve(A, n, b, x) ? 1 : 0;
}

}  // extern "C"
