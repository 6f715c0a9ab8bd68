// essential_graph_model.cpp — the CPU model of Optimizer::OptimizeEssentialGraph that the
// essential-graph tests and scripts/essential_graph_timing.py compare the kernels against.
//
// Written from g2o's sources as read (types/sim3/sim3.h, types_seven_dof_expmap.h, base_binary_edge.hpp,
// block_solver.hpp, optimization_algorithm_levenberg.cpp, sparse_optimizer.cpp) and Optimizer.cc:1470-1719,
// statement for statement: matrices are 3 x 3 arrays, the edge sums run sequentially in edge order, and
// the system is solved by a dense unpivoted column-loop L L' on the compacted matrix (solver 0) or by
// the same column loop restricted to the profile (solver 1: the terms left out are exact zeros).  It
// shares with csrc/orb_essgraph.hip only csrc/orb_g2o_math.h, and of that only the quaternion
// helpers (quat_from_matrix, matrix_from_quat, rotate, quat_mul) that tests/test_g2o_math_host.py
// pins: the Sim3 exponential, logarithm, product, inverse and the 3 x 3 LU are written again here.
//
//   sum_order  0 sequential, 1 pairwise, 2 reversed: how the sums over edges (chi2, a vertex's block and b,
//              an off-diagonal block) and computeScale's sum are taken
//   variant    0 the model; 1..7 the mutants of DESIGN.md §22
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <vector>

#include "../../include/orb_abi.h"
#include "../../orbslam_jpminipc_amd/csrc/orb_g2o_math.h"

namespace {

enum { V_NONE = 0, V_KIND_IGNORED, V_MEAS_SWAPPED, V_LAMBDA_DIAG, V_FIXED_BLOCK, V_T_NOT_DIVIDED, V_LOG_SWAPPED, V_SECOND_VSCW };

struct S3 {
    double q[4], t[3], s;
};

struct Margins {
    double sigma;       // min over evaluations of ||sigma| - eps| / eps
    double d;           // min of |(1 - d) - eps| / eps
    double trial;       // min over trials of |chi2 - trial chi2| / chi2
    double min_chi2;    // the smallest chi2 that a trial compared
    int64_t branch[4];  // evaluations per branch of log(): bit 0 |sigma| >= eps, bit 1 d <= 1 - eps
};

struct Ctx {
    int variant = 0, sum_order = 0;
    Margins* m = nullptr;
};

S3 load(const double* p) {
    S3 S;
    for (int k = 0; k < 4; ++k) S.q[k] = p[k];
    for (int k = 0; k < 3; ++k) S.t[k] = p[4 + k];
    S.s = p[7];
    return S;
}
void store(const S3& S, double* p) {
    for (int k = 0; k < 4; ++k) p[k] = S.q[k];
    for (int k = 0; k < 3; ++k) p[4 + k] = S.t[k];
    p[7] = S.s;
}

S3 from_pose(const float* T) {  // Sim3(Matrix3d R, t, 1.0): r(Quaterniond(R))
    double R[9];
    for (int k = 0; k < 9; ++k) R[k] = (double)T[k];
    S3 S;
    quat_from_matrix(R, S.q);
    for (int k = 0; k < 3; ++k) S.t[k] = (double)T[9 + k];
    S.s = 1.0;
    return S;
}

void map3(const S3& S, const double* X, double* o) {  // s * (r * xyz) + t
    double r[3];
    rotate(S.q, X, r);
    for (int k = 0; k < 3; ++k) o[k] = S.s * r[k] + S.t[k];
}

S3 inverse(const S3& S) {  // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
    S3 I;
    I.q[0] = -S.q[0], I.q[1] = -S.q[1], I.q[2] = -S.q[2], I.q[3] = S.q[3];
    const double f = -1. / S.s;
    double v[3];
    for (int k = 0; k < 3; ++k) v[k] = f * S.t[k];
    rotate(I.q, v, I.t);
    I.s = 1. / S.s;
    return I;
}

S3 mul(const S3& A, const S3& B) {  // ret.r = r * other.r; ret.t = s * (r * other.t) + t; ret.s = s * other.s
    S3 r;
    quat_mul(A.q, B.q, r.q);
    double rt[3];
    rotate(A.q, B.t, rt);
    for (int k = 0; k < 3; ++k) r.t[k] = A.s * rt[k] + A.t[k];
    r.s = A.s * B.s;
    return r;
}

void skew(const double* v, double M[3][3]) {
    M[0][0] = 0, M[0][1] = -v[2], M[0][2] = v[1];
    M[1][0] = v[2], M[1][1] = 0, M[1][2] = -v[0];
    M[2][0] = -v[1], M[2][1] = v[0], M[2][2] = 0;
}
void matmul(const double A[3][3], const double B[3][3], double C[3][3]) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = A[i][0] * B[0][j];
            s += A[i][1] * B[1][j];
            s += A[i][2] * B[2][j];
            C[i][j] = s;
        }
}

S3 exp7(const double* update) {  // Sim3(const Vector7d& update), sim3.h:70-142
    double omega[3], upsilon[3];
    for (int i = 0; i < 3; i++) omega[i] = update[i];
    for (int i = 0; i < 3; i++) upsilon[i] = update[i + 3];
    const double sigma = update[6];
    const double theta = std::sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
    double Omega[3][3], Omega2[3][3], R[3][3];
    skew(omega, Omega);
    S3 E;
    E.s = std::exp(sigma);
    matmul(Omega, Omega, Omega2);
    const double eps = 0.00001;
    double A, B, C;
    double ca = 1, cb = 1;  // R = I + ca * Omega + cb * Omega2
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - std::cos(theta)) / (theta2);
            B = (theta - std::sin(theta)) / (theta2 * theta);
            ca = std::sin(theta) / theta, cb = (1 - std::cos(theta)) / (theta * theta);
        }
    } else {
        C = (E.s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * E.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * E.s) / (sigma2 * sigma);
        } else {
            ca = std::sin(theta) / theta, cb = (1 - std::cos(theta)) / (theta * theta);
            const double a = E.s * std::sin(theta);
            const double b = E.s * std::cos(theta);
            const double theta2 = theta * theta;
            const double sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const bool small = theta < eps;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double I = i == j ? 1.0 : 0.0;
            R[i][j] = small ? (I + Omega[i][j]) + Omega2[i][j] : (I + ca * Omega[i][j]) + cb * Omega2[i][j];
        }
    double Rm[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Rm[3 * i + j] = R[i][j];
    quat_from_matrix(Rm, E.q);
    for (int i = 0; i < 3; ++i) {  // W = A * Omega + B * Omega2 + C * I; t = W * upsilon
        double W[3];
        for (int j = 0; j < 3; ++j) W[j] = (A * Omega[i][j] + B * Omega2[i][j]) + C * (i == j ? 1.0 : 0.0);
        double s = W[0] * upsilon[0];
        s += W[1] * upsilon[1];
        s += W[2] * upsilon[2];
        E.t[i] = s;
    }
    return E;
}

// Matrix3d::lu().solve(t): partial pivoting by rows, the largest |entry| of the column, the first of equals
void lu_solve(double W[3][3], const double* t, double* x) {
    int perm[3] = {0, 1, 2};
    double b[3] = {t[0], t[1], t[2]};
    for (int k = 0; k < 3; ++k) {
        int p = k;
        double big = std::fabs(W[k][k]);
        for (int i = k + 1; i < 3; ++i)
            if (std::fabs(W[i][k]) > big) big = std::fabs(W[i][k]), p = i;
        if (p != k) {
            for (int j = 0; j < 3; ++j) std::swap(W[k][j], W[p][j]);
            std::swap(b[k], b[p]);
            std::swap(perm[k], perm[p]);
        }
        for (int i = k + 1; i < 3; ++i) {
            W[i][k] /= W[k][k];
            for (int j = k + 1; j < 3; ++j) W[i][j] -= W[i][k] * W[k][j];
        }
    }
    for (int i = 1; i < 3; ++i)
        for (int k = 0; k < i; ++k) b[i] -= W[i][k] * b[k];
    for (int i = 2; i >= 0; --i) {
        double s = b[i];
        for (int k = i + 1; k < 3; ++k) s -= W[i][k] * x[k];
        x[i] = s / W[i][i];
    }
}

void log7(const Ctx& cx, const S3& S, double* res, int* branch_out = nullptr) {  // Sim3::log(), sim3.h:148-230
    const double sigma = std::log(S.s);
    double Rm[9];
    matrix_from_quat(S.q, Rm);
    double R[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i][j] = Rm[3 * i + j];
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};
    double omega[3], Omega[3][3];
    const double eps = 0.00001;
    double A, B, C;
    bool near = d > 1 - eps;
    const int branch = (std::fabs(sigma) < eps ? 0 : 1) | (near ? 0 : 2);
    if (cx.m) {
        cx.m->sigma = std::min(cx.m->sigma, std::fabs(std::fabs(sigma) - eps) / eps);
        cx.m->d = std::min(cx.m->d, std::fabs((1 - d) - eps) / eps);
        ++cx.m->branch[branch];
    }
    if (branch_out) *branch_out = branch;
    if (cx.variant == V_LOG_SWAPPED) near = !near;
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (near) {
            for (int k = 0; k < 3; ++k) omega[k] = 0.5 * dR[k];
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = std::acos(d);
            const double theta2 = theta * theta;
            const double f = theta / (2 * std::sqrt(1 - d * d));
            for (int k = 0; k < 3; ++k) omega[k] = f * dR[k];
            A = (1 - std::cos(theta)) / (theta2);
            B = (theta - std::sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (S.s - 1) / sigma;
        if (near) {
            const double sigma2 = sigma * sigma;
            for (int k = 0; k < 3; ++k) omega[k] = 0.5 * dR[k];
            A = ((sigma - 1) * S.s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = std::acos(d);
            const double f = theta / (2 * std::sqrt(1 - d * d));
            for (int k = 0; k < 3; ++k) omega[k] = f * dR[k];
            const double theta2 = theta * theta;
            const double a = S.s * std::sin(theta);
            const double b = S.s * std::cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    skew(omega, Omega);
    double BO[3][3], BOO[3][3], W[3][3];  // W = A * Omega + B * Omega * Omega + C * I
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) BO[i][j] = B * Omega[i][j];
    matmul(BO, Omega, BOO);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W[i][j] = (A * Omega[i][j] + BOO[i][j]) + C * (i == j ? 1.0 : 0.0);
    double upsilon[3];
    lu_solve(W, S.t, upsilon);
    for (int i = 0; i < 3; i++) res[i] = omega[i];
    for (int i = 0; i < 3; i++) res[i + 3] = upsilon[i];
    res[6] = sigma;
}

void compute_error(const Ctx& cx, const S3& C, const S3& v1, const S3& v2, double* err) {  // EdgeSim3::computeError
    log7(cx, mul(mul(C, v1), inverse(v2)), err);
}

S3 oplus(const double* u, const S3& T) { return mul(exp7(u), T); }

// BaseBinaryEdge::linearizeOplus: J row-major 7 x 7 (error component, column)
void linearize(const Ctx& cx, const S3& C, const S3& vi, const S3& vj, bool i_free, bool j_free, double* Ji, double* Jj) {
    const double delta = 1e-9;
    const double scalar = 1.0 / (2 * delta);
    for (int side = 0; side < 2; ++side) {
        double* J = side ? Jj : Ji;
        for (int k = 0; k < 49; ++k) J[k] = 0.;
        if (!(side ? j_free : i_free)) continue;
        double add[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int d = 0; d < 7; ++d) {
            double e1[7], e2[7];
            add[d] = delta;
            if (side) compute_error(cx, C, vi, oplus(add, vj), e1);
            else compute_error(cx, C, oplus(add, vi), vj, e1);
            add[d] = -delta;
            if (side) compute_error(cx, C, vi, oplus(add, vj), e2);
            else compute_error(cx, C, oplus(add, vi), vj, e2);
            add[d] = 0.0;
            for (int k = 0; k < 7; ++k) J[7 * k + d] = scalar * (e1[k] - e2[k]);
        }
    }
}

double sum_ordered(std::vector<double>& v, int order) {
    const size_t n = v.size();
    if (n == 0) return 0.;
    if (order == 2) std::reverse(v.begin(), v.end());
    if (order == 1) {
        size_t m = n;
        while (m > 1) {
            const size_t h = (m + 1) / 2;
            for (size_t k = 0; k + h < m; ++k) v[k] += v[k + h];
            m = h;
        }
        return v[0];
    }
    double s = 0.;
    for (size_t k = 0; k < n; ++k) s += v[k];
    return s;
}

struct Graph {
    int n_kf, n_edge;
    const int32_t *ei, *ej;
    std::vector<S3> S0, est, meas;
    std::vector<int> slot, slot_kf, first;  // first: f(i) per free block row
    int n_active = 0, n_free = 0;
};

double active_chi2(const Ctx& cx, const Graph& g) {
    std::vector<double> c(g.n_edge);
    for (int e = 0; e < g.n_edge; ++e) {
        double err[7];
        compute_error(cx, g.meas[e], g.est[g.ei[e]], g.est[g.ej[e]], err);
        double s = err[0] * err[0];
        for (int k = 1; k < 7; ++k) s += err[k] * err[k];
        c[e] = s;
    }
    return sum_ordered(c, cx.sum_order);
}

// the dense column loop on the N x N lower triangle `L` (row-major, full storage); false on a pivot that
// is not positive and finite
bool cholesky_dense(std::vector<double>& L, int N) {
    for (int j = 0; j < N; ++j) {
        double d = L[(size_t)j * N + j];
        for (int k = 0; k < j; ++k) d -= L[(size_t)j * N + k] * L[(size_t)j * N + k];
        if (!(d > 0) || !std::isfinite(d)) return false;
        const double sq = std::sqrt(d);
        L[(size_t)j * N + j] = sq;
        for (int i = j + 1; i < N; ++i) {
            double s = L[(size_t)i * N + j];
            for (int k = 0; k < j; ++k) s -= L[(size_t)i * N + k] * L[(size_t)j * N + k];
            L[(size_t)i * N + j] = s / sq;
        }
    }
    return true;
}

// the same loop over rows that start at first[i]
struct Profile {
    std::vector<int> first;      // per scalar row
    std::vector<size_t> off;     // row i holds columns first[i] .. i at off[i]
    std::vector<double> v;
    double& at(int i, int k) { return v[off[i] + (size_t)(k - first[i])]; }
};

bool cholesky_profile(Profile& P, int N) {
    for (int i = 0; i < N; ++i) {
        for (int j = P.first[i]; j <= i; ++j) {
            double s = P.at(i, j);
            for (int k = std::max(P.first[i], P.first[j]); k < j; ++k) s -= P.at(i, k) * P.at(j, k);
            if (j < i) {
                P.at(i, j) = s / P.at(j, j);
            } else {
                if (!(s > 0) || !std::isfinite(s)) return false;
                P.at(i, i) = std::sqrt(s);
            }
        }
    }
    return true;
}

}  // namespace

extern "C" {

void eg_model_exp(const double* u, double* sim3) { store(exp7(u), sim3); }

int eg_model_log(const double* sim3, double* out, int variant) {
    Ctx cx;
    cx.variant = variant;
    int br = 0;
    log7(cx, load(sim3), out, &br);
    return br;
}

void eg_model_from_pose(const float* Tcw, double* sim3) { store(from_pose(Tcw), sim3); }

void eg_model_to_pose(const double* sim3, double* M) {
    const S3 S = load(sim3);
    matrix_from_quat(S.q, M);
    const double is = 1. / S.s;
    for (int k = 0; k < 3; ++k) M[9 + k] = S.t[k] * is;  // eigt *= (1. / s)
}

void eg_model_mul(const double* a, const double* b, double* o) { store(mul(load(a), load(b)), o); }
void eg_model_inverse(const double* a, double* o) { store(inverse(load(a)), o); }

void eg_model_edge(const double* C, const double* vi, const double* vj, double* err, double* Ji, double* Jj) {
    Ctx cx;
    compute_error(cx, load(C), load(vi), load(vj), err);
    linearize(cx, load(C), load(vi), load(vj), true, true, Ji, Jj);
}

// to[pair]^-1.map(from[pair].map(P)); pair -1: two identity Sim3s
void eg_model_correct_points(int n_pt, const float* pos, const int32_t* pair, const double* from, const double* to,
                             float* out, double* out64) {
    for (int p = 0; p < n_pt; ++p) {
        const double P[3] = {(double)pos[3 * p], (double)pos[3 * p + 1], (double)pos[3 * p + 2]};
        S3 F, T;
        if (pair[p] >= 0) {
            F = load(from + (size_t)pair[p] * 8), T = inverse(load(to + (size_t)pair[p] * 8));
        } else {
            const double id[8] = {0, 0, 0, 1, 0, 0, 0, 1};
            F = load(id), T = load(id);
        }
        double M[3], Q[3];
        map3(F, P, M);
        map3(T, M, Q);
        for (int k = 0; k < 3; ++k) {
            if (out64) out64[3 * p + k] = Q[k];
            if (out) out[3 * p + k] = (float)Q[k];
        }
    }
}

// The whole call, as orb_optimize_essential_graph takes it.  solver: 0 dense, 1 profile.  margins (may be
// NULL): struct Margins.  The refusals return the ABI's codes.
int eg_model_run(int n_kf, const float* kf_pose, const double* kf_corrected, const uint8_t* kf_has_corrected,
                 const double* kf_noncorrected, const uint8_t* kf_has_noncorrected, const uint8_t* kf_fixed, int n_edge,
                 const int32_t* edge_i, const int32_t* edge_j, const uint8_t* edge_kind, int n_pt, const float* pt_pos,
                 const int32_t* pt_ref, const uint8_t* pt_skip, int n_iterations, int sum_order, int variant, int solver,
                 double* kf_sim3_out, float* kf_pose_out, double* kf_pose_out_f64, float* pt_pos_out,
                 double* pt_pos_out_f64, orb_essential_graph_info_t* info, void* margins) {
    Ctx cx;
    cx.variant = variant, cx.sum_order = sum_order;
    Margins M{HUGE_VAL, HUGE_VAL, HUGE_VAL, HUGE_VAL, {0, 0, 0, 0}};
    cx.m = &M;
    for (int e = 0; e < n_edge; ++e) {
        if (edge_i[e] < 0 || edge_i[e] >= n_kf || edge_j[e] < 0 || edge_j[e] >= n_kf) return ORB_EINVAL;
        if (edge_i[e] == edge_j[e] || edge_kind[e] > 1) return ORB_EINVAL;
    }
    auto bad_sim3 = [](const double* v) {
        for (int k = 0; k < 8; ++k)
            if (!std::isfinite(v[k])) return true;
        return !(v[7] > 0);
    };
    for (int i = 0; i < n_kf; ++i) {
        for (int k = 0; k < 12; ++k)
            if (!std::isfinite(kf_pose[12 * i + k])) return ORB_EINVAL;
        if (kf_has_corrected && kf_has_corrected[i] && bad_sim3(kf_corrected + 8 * (size_t)i)) return ORB_EINVAL;
        if (kf_has_noncorrected && kf_has_noncorrected[i] && bad_sim3(kf_noncorrected + 8 * (size_t)i)) return ORB_EINVAL;
    }
    Graph g;
    g.n_kf = n_kf, g.n_edge = n_edge, g.ei = edge_i, g.ej = edge_j;
    // SET KEYFRAME VERTICES
    g.S0.resize(n_kf), g.meas.resize(n_edge);
    for (int i = 0; i < n_kf; ++i)
        g.S0[i] = kf_has_corrected && kf_has_corrected[i] ? load(kf_corrected + 8 * (size_t)i) : from_pose(kf_pose + 12 * (size_t)i);
    g.est = g.S0;
    auto nonc = [&](int i) {
        return kf_has_noncorrected && kf_has_noncorrected[i] ? load(kf_noncorrected + 8 * (size_t)i) : g.S0[i];
    };
    // SET LOOP EDGES / SET NORMAL EDGES
    for (int e = 0; e < n_edge; ++e) {
        const int i = edge_i[e], j = edge_j[e];
        const bool normal = edge_kind[e] == 1 && variant != V_KIND_IGNORED;
        const S3 Siw = normal ? nonc(i) : g.S0[i];
        const S3 Sjw = normal && variant != V_SECOND_VSCW ? nonc(j) : g.S0[j];
        const S3 Swi = inverse(Siw);
        g.meas[e] = variant == V_MEAS_SWAPPED ? mul(Swi, Sjw) : mul(Sjw, Swi);
    }
    // initializeOptimization(): the vertices that an edge touches
    std::vector<uint8_t> active(n_kf, 0);
    for (int e = 0; e < n_edge; ++e) active[edge_i[e]] = active[edge_j[e]] = 1;
    g.slot.assign(n_kf, -1);
    for (int i = 0; i < n_kf; ++i) {
        if (!active[i]) continue;
        ++g.n_active;
        if (!kf_fixed[i] || variant == V_FIXED_BLOCK) g.slot[i] = g.n_free++, g.slot_kf.push_back(i);
    }
    if (n_edge) {
        bool any_fixed = false;
        for (int i = 0; i < n_kf; ++i) any_fixed = any_fixed || (active[i] && kf_fixed[i]);
        if (!any_fixed) return ORB_EINVAL;
    }
    const int nf = g.n_free, N = 7 * nf;
    g.first.resize(nf);
    for (int i = 0; i < nf; ++i) g.first[i] = i;
    for (int e = 0; e < n_edge; ++e) {
        const int si = g.slot[edge_i[e]], sj = g.slot[edge_j[e]];
        if (si >= 0 && sj >= 0) g.first[std::max(si, sj)] = std::min(g.first[std::max(si, sj)], std::min(si, sj));
    }
    int64_t profile = 0;
    for (int i = 0; i < nf; ++i) profile += (int64_t)49 * (i - g.first[i] + 1) * 8;
    if ((uint64_t)profile > ORB_EG_MAX_PROFILE_BYTES) return ORB_ENOTSUP;
    orb_essential_graph_info_t I;
    std::memset(&I, 0, sizeof I);
    I.status = ORB_OK, I.n_active = g.n_active, I.n_free = nf, I.n_edges = n_edge, I.profile_bytes = profile, I.lambda = -1.;

    // optimize(n_iterations)
    double lambda = -1., ni = 2.;
    int bad_steps = 0;
    std::vector<double> x(N, 0.), b(N, 0.);
    std::vector<double> Ji((size_t)n_edge * 49), Jj((size_t)n_edge * 49), err((size_t)n_edge * 7);
    bool stop = !(N && n_edge);
    for (int it = 0; it < n_iterations && !stop; ++it) {
        ++I.iterations;
        // computeActiveErrors; activeRobustChi2
        double cur = active_chi2(cx, g);
        const double ini = cur;
        // buildSystem: linearizeOplus + constructQuadraticForm per edge, in edge order
        for (int e = 0; e < n_edge; ++e) {
            const int i = edge_i[e], j = edge_j[e];
            compute_error(cx, g.meas[e], g.est[i], g.est[j], &err[(size_t)e * 7]);
            linearize(cx, g.meas[e], g.est[i], g.est[j], g.slot[i] >= 0, g.slot[j] >= 0, &Ji[(size_t)e * 49], &Jj[(size_t)e * 49]);
        }
        // the contributions of each target, in edge order: the diagonal blocks with b behind them, the lower blocks
        std::vector<std::vector<int>> vlist(nf);
        std::map<std::pair<int, int>, std::vector<int>> plist;
        for (int e = 0; e < n_edge; ++e) {
            const int si = g.slot[edge_i[e]], sj = g.slot[edge_j[e]];
            if (si >= 0) vlist[si].push_back(e);
            if (sj >= 0) vlist[sj].push_back(e);
            if (si >= 0 && sj >= 0) plist[{std::max(si, sj), std::min(si, sj)}].push_back(e);
        }
        std::vector<double> hd((size_t)nf * 49);
        std::vector<double> terms;
        for (int sl = 0; sl < nf; ++sl) {
            const int kf = g.slot_kf[sl];
            for (int ent = 0; ent < 56; ++ent) {
                terms.clear();
                for (int e : vlist[sl]) {
                    const double* J = edge_i[e] == kf ? &Ji[(size_t)e * 49] : &Jj[(size_t)e * 49];
                    double s;
                    if (ent < 49) {  // A.transpose() * omega * A with omega the identity
                        const int r = ent / 7, c = ent % 7;
                        s = J[r] * J[c];
                        for (int k = 1; k < 7; ++k) s += J[7 * k + r] * J[7 * k + c];
                    } else {  // A.transpose() * omega_r, omega_r = -omega * _error
                        const int r = ent - 49;
                        s = J[r] * -err[(size_t)e * 7];
                        for (int k = 1; k < 7; ++k) s += J[7 * k + r] * -err[(size_t)e * 7 + k];
                    }
                    terms.push_back(s);
                }
                const double v = sum_ordered(terms, cx.sum_order);
                if (ent < 49) hd[(size_t)sl * 49 + ent] = v;
                else b[7 * sl + ent - 49] = v;
            }
        }
        if (it == 0) {
            lambda = 1e-16;  // setUserLambdaInit(1e-16)
            if (variant == V_LAMBDA_DIAG) {
                double mx = 0.;
                for (int sl = 0; sl < nf; ++sl)
                    for (int k = 0; k < 7; ++k) mx = std::max(std::fabs(hd[(size_t)sl * 49 + 8 * k]), mx);
                lambda = 1e-5 * mx;
            }
            ni = 2.;
            bad_steps = 0;
            I.chi2_before = cur;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const std::vector<S3> backup = g.est;  // push()
            // Hpp + lambda I, then the solve
            bool ok2;
            std::vector<double> y(b);
            auto block_value = [&](int row, int col, int r, int c) {
                terms.clear();
                for (int e : plist[{row, col}]) {
                    const bool i_is_row = g.slot[edge_i[e]] == row;
                    const double* Jr = i_is_row ? &Ji[(size_t)e * 49] : &Jj[(size_t)e * 49];
                    const double* Jc = i_is_row ? &Jj[(size_t)e * 49] : &Ji[(size_t)e * 49];
                    double s = Jr[r] * Jc[c];
                    for (int k = 1; k < 7; ++k) s += Jr[7 * k + r] * Jc[7 * k + c];
                    terms.push_back(s);
                }
                return sum_ordered(terms, cx.sum_order);
            };
            if (solver == 0) {
                std::vector<double> L((size_t)N * N, 0.);
                for (int sl = 0; sl < nf; ++sl)
                    for (int r = 0; r < 7; ++r)
                        for (int c = 0; c <= r; ++c)
                            L[(size_t)(7 * sl + r) * N + 7 * sl + c] = hd[(size_t)sl * 49 + 7 * r + c] + (r == c ? lambda : 0.);
                for (auto& kv : plist)
                    for (int r = 0; r < 7; ++r)
                        for (int c = 0; c < 7; ++c)
                            L[(size_t)(7 * kv.first.first + r) * N + 7 * kv.first.second + c] =
                                block_value(kv.first.first, kv.first.second, r, c);
                ok2 = cholesky_dense(L, N);
                if (ok2) {
                    for (int i = 0; i < N; ++i) {
                        for (int k = 0; k < i; ++k) y[i] -= L[(size_t)i * N + k] * y[k];
                        y[i] /= L[(size_t)i * N + i];
                    }
                    for (int k = N - 1; k >= 0; --k) {
                        x[k] = y[k] / L[(size_t)k * N + k];
                        for (int i = 0; i < k; ++i) y[i] -= L[(size_t)k * N + i] * x[k];
                    }
                }
            } else {
                Profile P;
                P.first.resize(N), P.off.resize(N);
                size_t tot = 0;
                for (int i = 0; i < N; ++i) P.first[i] = 7 * g.first[i / 7], P.off[i] = tot, tot += (size_t)(i - P.first[i] + 1);
                P.v.assign(tot, 0.);
                for (int sl = 0; sl < nf; ++sl)
                    for (int r = 0; r < 7; ++r)
                        for (int c = 0; c <= r; ++c) P.at(7 * sl + r, 7 * sl + c) = hd[(size_t)sl * 49 + 7 * r + c] + (r == c ? lambda : 0.);
                for (auto& kv : plist)
                    for (int r = 0; r < 7; ++r)
                        for (int c = 0; c < 7; ++c)
                            P.at(7 * kv.first.first + r, 7 * kv.first.second + c) = block_value(kv.first.first, kv.first.second, r, c);
                ok2 = cholesky_profile(P, N);
                if (ok2) {
                    for (int i = 0; i < N; ++i) {
                        for (int k = P.first[i]; k < i; ++k) y[i] -= P.at(i, k) * y[k];
                        y[i] /= P.at(i, i);
                    }
                    for (int k = N - 1; k >= 0; --k) {
                        x[k] = y[k] / P.at(k, k);
                        for (int i = P.first[k]; i < k; ++i) y[i] -= P.at(k, i) * x[k];
                    }
                }
            }
            if (!ok2) ++I.refused;
            // update(x)
            for (int sl = 0; sl < nf; ++sl) g.est[g.slot_kf[sl]] = oplus(&x[7 * sl], g.est[g.slot_kf[sl]]);
            // computeActiveErrors; activeRobustChi2
            double temp = active_chi2(cx, g);
            if (!ok2) temp = DBL_MAX;
            // computeScale
            terms.clear();
            for (int j = 0; j < N; ++j) terms.push_back(x[j] * (lambda * x[j] + b[j]));
            double scale = sum_ordered(terms, cx.sum_order);
            scale += 1e-3;
            rho = (cur - temp) / scale;
            bool accepted = false;
            if (std::isfinite(temp) && cur > 0) M.trial = std::min(M.trial, std::fabs(cur - temp) / cur);
            M.min_chi2 = std::min(M.min_chi2, std::min(cur, temp));
            if (rho > 0 && std::isfinite(temp)) {
                double alpha = 1. - std::pow((2 * rho - 1), 3);
                alpha = std::min(alpha, 2. / 3.);
                const double scaleFactor = std::max(1. / 3., alpha);
                lambda *= scaleFactor;
                ni = 2;
                cur = temp;
                accepted = true;
            } else {
                lambda *= ni;
                ni *= 2;
                g.est = backup;  // pop()
            }
            if (I.trials < ORB_EG_MAX_TRIALS) {
                I.trial_rho[I.trials] = rho, I.trial_chi2[I.trials] = temp, I.trial_accepted[I.trials] = accepted ? 1 : 0;
            }
            ++I.trials;
            ++qmax;
        } while (rho < 0 && qmax < 10);
        I.lambda = lambda, I.chi2_after = cur;
        stop = lm_stop(qmax, rho, ini, cur, bad_steps);
    }
    // SE3 Pose Recovering. Sim3:[sR t;0 1] -> SE3:[R t/s;0 1]
    for (int i = 0; i < n_kf; ++i) {
        if (kf_sim3_out) store(g.est[i], kf_sim3_out + 8 * (size_t)i);
        double P[12];
        matrix_from_quat(g.est[i].q, P);
        const double is = 1. / g.est[i].s;
        for (int k = 0; k < 3; ++k) P[9 + k] = variant == V_T_NOT_DIVIDED ? g.est[i].t[k] : g.est[i].t[k] * is;
        for (int k = 0; k < 12; ++k) {
            if (kf_pose_out_f64) kf_pose_out_f64[12 * (size_t)i + k] = P[k];
            if (kf_pose_out) kf_pose_out[12 * (size_t)i + k] = (float)P[k];
        }
    }
    // Correct points
    for (int p = 0; p < n_pt; ++p) {
        if (pt_skip && pt_skip[p]) continue;
        const int r = pt_ref[p];
        const double id[8] = {0, 0, 0, 1, 0, 0, 0, 1};
        const S3 Srw = r >= 0 ? g.S0[r] : load(id);
        const S3 correctedSwr = r >= 0 ? inverse(g.est[r]) : load(id);
        const double P[3] = {(double)pt_pos[3 * p], (double)pt_pos[3 * p + 1], (double)pt_pos[3 * p + 2]};
        double Mid[3], Q[3];
        map3(Srw, P, Mid);
        map3(correctedSwr, Mid, Q);
        for (int k = 0; k < 3; ++k) {
            if (pt_pos_out_f64) pt_pos_out_f64[3 * (size_t)p + k] = Q[k];
            if (pt_pos_out) pt_pos_out[3 * (size_t)p + k] = (float)Q[k];
        }
    }
    if (info) *info = I;
    if (margins) std::memcpy(margins, &M, sizeof M);
    return ORB_OK;
}

}  // extern "C"
