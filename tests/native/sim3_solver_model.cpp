// CPU model of orb_sim3_compute_hypotheses (and, with tests/native/solvers_model.cpp's CheckInliers,
// of orb_sim3_ransac and its batch form): the minimal sets of Sim3Solver::iterate (reference
// src/Sim3Solver.cc:163-177, with DUtils::Random::RandomInt, Thirdparty/DBoW2/DUtils/Random.cpp:47-50),
// centroid (215-224) and computeT (226-332), restated statement for statement.  Built
// -ffp-contract=off.  The cv::Mat arithmetic follows OpenCV 2.4 as oracle/ocv_ops.h states it (the
// 3-term gemm fast path, norm, dot, subtract) and, for what that header does not cover, as the 2.4
// sources are known (Unpinned): reduce, the MatExpr scale, the GEMM_2_T product, the
// 9-element dot, JacobiImpl_<float> and cvRodrigues2.  No OpenCV 2.4 build is at hand, so parity with
// a real one is unpinned.  Single-threaded; scripts/sim3_solver_timing.py also times it.
//
// `variant` (tests only): bit 0 = the sampler removes by position (the "fixed" sampler); bits 1-2,
// 3-4, 5-6 = the results of atan2, cos and sin moved by one ulp (1 = up, 2 = down).
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

namespace {

constexpr int V_FIXED_SAMPLER = 1;

inline double nudge(double v, int code) {
    if (code == 1) return std::nextafter(v, std::numeric_limits<double>::infinity());
    if (code == 2) return std::nextafter(v, -std::numeric_limits<double>::infinity());
    return v;
}

// DUtils::Random::RandomInt(0, size - 1) on the value r that rand() returned (RAND_MAX = 2^31 - 1)
inline int random_int(int r, int size) {
    const int min = 0, max = size - 1;
    const int d = max - min + 1;
    return int(((double)r / ((double)2147483647 + 1.0)) * d) + min;
}

// cv::reduce(P, C, 1, CV_REDUCE_SUM), one row of 3 floats (reduceC_<float, float, OpAdd<float>>):
// a0 = s[0], a1 = s[1]; the tail adds s[2] to a0; a0 + a1
inline float reduce_sum3(const float* s) {
    float a0 = s[0], a1 = s[1];
    a0 = a0 + s[2];
    a0 = a0 + a1;
    return a0;
}

// m = alpha * m (a MatExpr scale assigned: convertTo(m, CV_32F, alpha), cvtScale_<float, float,
// float>): the scale and the zero shift narrowed to float, then v * scale + shift
inline float cvt_scale(float v, double alpha) {
    const float scale = (float)alpha, shift = (float)0.0;
    return v * scale + shift;
}

// the element of gemm's 3-term fast path (ocv::gemm3_add): t the float row sum
inline float gemm_out(float t, double alpha, float c, double beta) { return (float)((double)t * alpha + (double)c * beta); }

inline float jacobi_hypot(float a, float b) {
    a = std::abs(a);
    b = std::abs(b);
    if (a > b) {
        b /= a;
        return a * std::sqrt(1 + b * b);
    }
    if (b > 0) {
        a /= b;
        return b * std::sqrt(1 + a * a);
    }
    return 0;
}

// JacobiImpl_<float> (modules/core/src/lapack.cpp) for n = 4: A row-major (the upper triangle is
// read and written), W the eigenvalues, V the eigenvectors as rows, sorted descending.
void jacobi4(float* A, float* W, float* V) {
    const int n = 4, astep = 4, vstep = 4;
    const float eps = FLT_EPSILON;
    int i, j, k, m;
    for (i = 0; i < n; i++) {
        for (j = 0; j < n; j++) V[i * vstep + j] = 0.0f;
        V[i * vstep + i] = 1.0f;
    }
    int iters, maxIters = n * n * 30;
    int indR[4], indC[4];
    float mv = 0.0f;
    for (k = 0; k < n; k++) {
        W[k] = A[(astep + 1) * k];
        if (k < n - 1) {
            for (m = k + 1, mv = std::abs(A[astep * k + m]), i = k + 2; i < n; i++) {
                float val = std::abs(A[astep * k + i]);
                if (mv < val) mv = val, m = i;
            }
            indR[k] = m;
        }
        if (k > 0) {
            for (m = 0, mv = std::abs(A[k]), i = 1; i < k; i++) {
                float val = std::abs(A[astep * i + k]);
                if (mv < val) mv = val, m = i;
            }
            indC[k] = m;
        }
    }
    for (iters = 0; iters < maxIters; iters++) {
        // find index (k,l) of pivot p
        for (k = 0, mv = std::abs(A[indR[0]]), i = 1; i < n - 1; i++) {
            float val = std::abs(A[astep * i + indR[i]]);
            if (mv < val) mv = val, k = i;
        }
        int l = indR[k];
        for (i = 1; i < n; i++) {
            float val = std::abs(A[astep * indC[i] + i]);
            if (mv < val) mv = val, k = indC[i], l = i;
        }
        float p = A[astep * k + l];
        if (std::abs(p) <= eps) break;
        float y = (float)((W[l] - W[k]) * 0.5);
        float t = std::abs(y) + jacobi_hypot(p, y);
        float s = jacobi_hypot(p, t);
        float c = t / s;
        s = p / s;
        t = (p / t) * p;
        if (y < 0) s = -s, t = -t;
        A[astep * k + l] = 0;
        W[k] -= t;
        W[l] += t;
        float a0, b0;
#define rotate(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
        for (i = 0; i < k; i++) rotate(A[astep * i + k], A[astep * i + l]);
        for (i = k + 1; i < l; i++) rotate(A[astep * k + i], A[astep * i + l]);
        for (i = l + 1; i < n; i++) rotate(A[astep * k + i], A[astep * l + i]);
        for (i = 0; i < n; i++) rotate(V[vstep * k + i], V[vstep * l + i]);
#undef rotate
        for (j = 0; j < 2; j++) {
            int idx = j == 0 ? k : l;
            if (idx < n - 1) {
                for (m = idx + 1, mv = std::abs(A[astep * idx + m]), i = idx + 2; i < n; i++) {
                    float val = std::abs(A[astep * idx + i]);
                    if (mv < val) mv = val, m = i;
                }
                indR[idx] = m;
            }
            if (idx > 0) {
                for (m = 0, mv = std::abs(A[idx]), i = 1; i < idx; i++) {
                    float val = std::abs(A[astep * i + idx]);
                    if (mv < val) mv = val, m = i;
                }
                indC[idx] = m;
            }
        }
    }
    // sort eigenvalues & eigenvectors (descending)
    for (k = 0; k < n - 1; k++) {
        m = k;
        for (i = k + 1; i < n; i++)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            std::swap(W[m], W[k]);
            for (i = 0; i < n; i++) std::swap(V[vstep * m + i], V[vstep * k + i]);
        }
    }
}

// Sim3Solver::centroid: P 3x3 row-major, a correspondence per column
void centroid(const float* P, float* Pr, float* C) {
    for (int r = 0; r < 3; r++) C[r] = reduce_sum3(P + 3 * r);
    for (int r = 0; r < 3; r++) C[r] = cvt_scale(C[r], 1. / (double)3);  // C = C/P.cols
    for (int i = 0; i < 3; i++)
        for (int r = 0; r < 3; r++) Pr[3 * r + i] = P[3 * r + i] - C[r];
}

// Sim3Solver::computeT.  T12 / T21: rows 0-2 of mT12i / mT21i; sim3: mR12i (9), mt12i (3), ms12i;
// quat: row 0 of evec.
void compute_t(const float* P1, const float* P2, int variant, float* T12, float* T21, float* sim3, float* quat) {
    float Pr1[9], Pr2[9], O1[3], O2[3];
    centroid(P1, Pr1, O1);
    centroid(P2, Pr2, O2);
    // M = Pr2*Pr1.t(): gemm with GEMM_2_T, GEMMSingleMul<float, double>
    float M[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
            for (int k = 0; k < 3; k++) s0 += (double)Pr2[3 * i + k] * (double)Pr1[3 * j + k];
            s0 = (s0 + s1 + s2 + s3) * 1.0;
            M[3 * i + j] = (float)s0;
        }
    double N11, N12, N13, N14, N22, N23, N24, N33, N34, N44;
    N11 = M[0] + M[4] + M[8];
    N12 = M[5] - M[7];
    N13 = M[6] - M[2];
    N14 = M[1] - M[3];
    N22 = M[0] - M[4] - M[8];
    N23 = M[1] + M[3];
    N24 = M[6] + M[2];
    N33 = -M[0] + M[4] - M[8];
    N34 = M[5] + M[7];
    N44 = -M[0] - M[4] + M[8];
    float N[16] = {(float)N11, (float)N12, (float)N13, (float)N14, (float)N12, (float)N22, (float)N23, (float)N24,
                   (float)N13, (float)N23, (float)N33, (float)N34, (float)N14, (float)N24, (float)N34, (float)N44};
    float eval[4], evec[16];
    jacobi4(N, eval, evec);
    if (quat)
        for (int k = 0; k < 4; k++) quat[k] = evec[k];
    float vec[3] = {evec[1], evec[2], evec[3]};
    // norm(vec): sqrt of the double sum of squares
    double nrm = 0;
    for (int k = 0; k < 3; k++) nrm += (double)vec[k] * (double)vec[k];
    nrm = std::sqrt(nrm);
    double ang = nudge(std::atan2(nrm, (double)evec[0]), (variant >> 1) & 3);
    // vec = 2*ang*vec/norm(vec): the expression's scale is (2*ang) * (1./norm)
    const double alpha = (2 * ang) * (1. / nrm);
    for (int k = 0; k < 3; k++) vec[k] = cvt_scale(vec[k], alpha);
    // cvRodrigues2 (double), the result converted to float
    float R[9];
    {
        double rx = vec[0], ry = vec[1], rz = vec[2];
        double theta = std::sqrt(rx * rx + ry * ry + rz * rz);
        if (theta < DBL_EPSILON) {
            for (int k = 0; k < 9; k++) R[k] = k % 4 == 0 ? 1.0f : 0.0f;
        } else {
            const double I[] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            double c = nudge(std::cos(theta), (variant >> 3) & 3);
            double s = nudge(std::sin(theta), (variant >> 5) & 3);
            double c1 = 1. - c;
            double itheta = theta ? 1. / theta : 0.;
            rx *= itheta;
            ry *= itheta;
            rz *= itheta;
            double rrt[] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
            double r_x[] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
            for (int k = 0; k < 9; k++) R[k] = (float)(c * I[k] + c1 * rrt[k] + s * r_x[k]);
        }
    }
    // P3 = mR12i*Pr2: the 3-term fast path, alpha = 1, no C
    float P3[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float t = R[3 * i] * Pr2[j] + R[3 * i + 1] * Pr2[3 + j] + R[3 * i + 2] * Pr2[6 + j];
            P3[3 * i + j] = gemm_out(t, 1.0, 0.0f, 0.0);
        }
    // nom = Pr1.dot(P3): dotProd_<float>, 9 elements, unrolled by 4
    double nom = 0;
    {
        int i = 0;
        for (; i <= 9 - 4; i += 4)
            nom += (double)Pr1[i] * P3[i] + (double)Pr1[i + 1] * P3[i + 1] + (double)Pr1[i + 2] * P3[i + 2] +
                   (double)Pr1[i + 3] * P3[i + 3];
        for (; i < 9; i++) nom += (double)Pr1[i] * P3[i];
    }
    double den = 0;
    for (int i = 0; i < 9; i++) {
        const float aux = P3[i] * P3[i];  // cv::pow(P3, 2, aux_P3)
        den += aux;
    }
    const float ms12i = nom / den;
    // mt12i = O1 - ms12i*mR12i*O2: one gemm, alpha = -ms12i, C = O1, beta = 1
    float t12[3];
    for (int i = 0; i < 3; i++) {
        float t = R[3 * i] * O2[0] + R[3 * i + 1] * O2[1] + R[3 * i + 2] * O2[2];
        t12[i] = gemm_out(t, -(double)ms12i, O1[i], 1.0);
    }
    float sR[9], sRinv[9], tinv[3];
    for (int k = 0; k < 9; k++) sR[k] = cvt_scale(R[k], (double)ms12i);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) sRinv[3 * i + j] = cvt_scale(R[3 * j + i], 1.0 / ms12i);
    for (int i = 0; i < 3; i++) {
        float t = sRinv[3 * i] * t12[0] + sRinv[3 * i + 1] * t12[1] + sRinv[3 * i + 2] * t12[2];
        tinv[i] = gemm_out(t, -1.0, 0.0f, 0.0);
    }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            if (T12) T12[4 * i + j] = sR[3 * i + j];
            if (T21) T21[4 * i + j] = sRinv[3 * i + j];
        }
        if (T12) T12[4 * i + 3] = t12[i];
        if (T21) T21[4 * i + 3] = tinv[i];
    }
    if (sim3) {
        for (int k = 0; k < 9; k++) sim3[k] = R[k];
        for (int k = 0; k < 3; k++) sim3[9 + k] = t12[k];
        sim3[12] = ms12i;
    }
}

}  // namespace

extern "C" {

// The minimal sets of n_hyp iterations over N correspondences: rand31 n_hyp x 3 values of rand(),
// sets n_hyp x 3.  vAvailableIndices is a vector of N entries whose size shrinks (the write at
// [idx] may land one slot past the size: inside the allocation, never read again).
int sim3_solver_model_sets(int N, int n_hyp, const int32_t* rand31, int variant, int32_t* sets) {
    if (N < 3) return -1;
    std::vector<size_t> mvAllIndices(N), vAvailableIndices;
    for (int i = 0; i < N; i++) mvAllIndices[i] = i;
    for (int h = 0; h < n_hyp; h++) {
        vAvailableIndices = mvAllIndices;
        size_t size = vAvailableIndices.size();
        for (short i = 0; i < 3; ++i) {
            int randi = random_int(rand31[3 * h + i], (int)size);
            int idx = vAvailableIndices[randi];
            sets[3 * h + i] = idx;
            if (variant & V_FIXED_SAMPLER)
                vAvailableIndices[randi] = vAvailableIndices[size - 1];
            else
                vAvailableIndices[idx] = vAvailableIndices[size - 1];
            size--;  // pop_back()
        }
    }
    return 0;
}

// (r * d) >> 31 against RandomInt's double expression (tests)
int sim3_solver_model_random_int(int r, int d) { return random_int(r, d); }

// cv::eigen on a symmetric 4x4 CV_32F (tests): W 4, V 16 (rows)
int sim3_solver_model_jacobi(const float* A, float* W, float* V) {
    float a[16];
    for (int k = 0; k < 16; k++) a[k] = A[k];
    jacobi4(a, W, V);
    return 0;
}

// computeT for n_hyp minimal sets (n_hyp x 3 indices into the n correspondences).  Outputs may be
// NULL: T12 / T21 n_hyp x 12, sim3 n_hyp x 13, quat n_hyp x 4.
int sim3_solver_model_compute(int n, const float* x3dc1, const float* x3dc2, int n_hyp, const int32_t* sets,
                              int variant, float* T12, float* T21, float* sim3, float* quat) {
    for (int h = 0; h < n_hyp; h++) {
        float P3Dc1i[9], P3Dc2i[9];
        for (int i = 0; i < 3; i++) {
            const int idx = sets[3 * h + i];
            if (idx < 0 || idx >= n) return -1;
            for (int r = 0; r < 3; r++) {
                P3Dc1i[3 * r + i] = x3dc1[3 * idx + r];
                P3Dc2i[3 * r + i] = x3dc2[3 * idx + r];
            }
        }
        compute_t(P3Dc1i, P3Dc2i, variant, T12 ? T12 + 12 * h : nullptr, T21 ? T21 + 12 * h : nullptr,
                  sim3 ? sim3 + 13 * h : nullptr, quat ? quat + 4 * h : nullptr);
    }
    return 0;
}

}  // extern "C"
