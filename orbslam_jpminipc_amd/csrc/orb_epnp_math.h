// orb_epnp_math.h — EPnP's compute_pose (reference src/PnPsolver.cc:347-922) and the OpenCV 2.4
// routines it calls, in double, for the device and for the host.
//
// One statement of the arithmetic, compiled twice: csrc/orb_solvers.hip instantiates it with the
// work matrix in LDS ([element][lane]) and tests/native/pnp_solver_model.cpp with plain arrays.
// Both translation units are built -ffp-contract=off, so every fused multiply-add is one that is
// written here.
//
// EPnP proper sits in the reference's own translation unit, which its build compiles
// g++ -O3 -march=native: the multiply-adds that g++ fuses there are written out as fma()
// (scripts/contraction_check_pnp.sh prints the disassembly they are read from; DESIGN §17 lists them
// per function).  g++ fuses a product into the addition or subtraction that is its only use, taking
// the products of an expression from left to right; a sum that has already become an fma does not
// absorb its other operand, so a*b + c*d + e*f is fma(e, f, fma(a, b, c*d)).
//
// The OpenCV calls (cvMulTransposed, cvSVD, cvInvert, cvSolve: modules/core/src/lapack.cpp
// JacobiSVDImpl_<double>, its own hypot, SVBkSbImpl_<double>; matmul.cpp MulTransposedR) are OpenCV's
// binary, which a distribution builds without FMA: they are restated as read, uncontracted.  No
// OpenCV 2.4 source or binary is at hand, so parity with a real build is unpinned (§16's policy).
// Every dot product is one accumulator with ascending index.  The only libm call is sqrt.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "orb_cv_math.h"

#if defined(__HIPCC__)
#define EPNP_HD __host__ __device__
#else
#define EPNP_HD
#endif

namespace orb_epnp {

// The branches a call visited (the model exports them; the kernels drop them).
enum : unsigned {
    BR_SVD_SKIP = 1u << 0,      // a Jacobi pair already orthogonal (|p| <= eps*sqrt(a*b))
    BR_SVD_BETA_NEG = 1u << 1,  // beta < 0 in the rotation
    BR_SVD_BETA_POS = 1u << 2,
    BR_SVD_SWAP = 1u << 3,      // the sort exchanged two rows
    BR_SVD_FILL = 1u << 4,      // a row with sd <= DBL_MIN refilled from the RNG
    BR_BKSB_SKIP = 1u << 5,     // a singular value under the back-substitution's threshold
    BR_B_NEG = 1u << 6,         // b[0] < 0 in a find_betas_approx
    BR_B_POS = 1u << 7,
    BR_B1_NEG = 1u << 8,        // b[1] < 0 in approx_2 / approx_3 (betas[0] negated)
    BR_QR_ETA0 = 1u << 9,       // qr_solve's early return
    BR_QR_SIGMA_NEG = 1u << 10, // *ppAkk < 0
    BR_SIGN_FLIP = 1u << 11,    // solve_for_sign negated ccs and pcs
    BR_DET_NEG = 1u << 12,      // estimate_R_and_t's det < 0
    BR_N2 = 1u << 13,           // compute_pose chose the second / third set of betas
    BR_N3 = 1u << 14,
    BR_ALL = (1u << 15) - 1,
};

// Element e of a work array whose elements lie STRIDE doubles apart (64 in LDS, 1 on the host).
template <int STRIDE>
struct Mat {
    double* p;
    EPNP_HD double& operator[](int e) const { return p[(size_t)e * STRIDE]; }
    EPNP_HD Mat at(int off) const { return Mat{p + (size_t)off * STRIDE}; }
};

constexpr int WK_W = 144;       // the singular values, after the 12 x 12
constexpr int WK_DOUBLES = 156;
// the small decompositions work in the rows 0-7 of the 12 x 12, which nothing reads after its SVD
constexpr int WK_SMALL_VT = 30;

EPNP_HD inline double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }

// ---- OpenCV 2.4, as read ---------------------------------------------------------------------------

// (lapack.cpp's own hypot: orb_cv::cv_hypot of csrc/orb_cv_math.h)

// The fill-in `while` has no bound in OpenCV; as in §16 it gives up after this many tries.
constexpr int MAX_FILL_TRIES = 16;
// The fill-in's random vector has 1-norm 1 before every projection is taken off.  When what is left has
// a 1-norm under this, the vector lay in the span of the earlier rows (cv::RNG(0x12345678)'s fifth
// vector of six signs is the negative of its fourth) and the renormalisation would scale rounding
// noise back to order 1: a row that is not orthogonal to the earlier ones.  OpenCV keeps that row;
// here the next random vector is tried instead (the second repair).  A vector that does
// not collapse goes through the same operations as in OpenCV.
constexpr double FILL_COLLAPSE = 1e-8;

// JacobiSVDImpl_<double>(At, astep, W, Vt, vstep, m, n, n1, minval = DBL_MIN, eps = DBL_EPSILON*10).
// At: n1 rows of m, the first n orthogonalised.  OpenCV always passes a Vt here; with vt == false its
// rotations are not carried out (nothing reads it), everything that depends on its presence is.
template <class M>
EPNP_HD inline void jacobi_svd(M At, int astep, M W, M Vt, bool vt, int vstep, int m, int n, int n1, unsigned& br) {
    const double minval = DBL_MIN, eps = DBL_EPSILON * 10;
    int i, j, k, iter;
    const int max_iter = m > 30 ? m : 30;
    double c, s, sd;

    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            double t = At[i * astep + k];
            sd += t * t;
        }
        W[i] = sd;
        if (vt) {
            for (k = 0; k < n; k++) Vt[i * vstep + k] = 0;
            Vt[i * vstep + i] = 1;
        }
    }

#pragma unroll 1
    for (iter = 0; iter < max_iter; iter++) {
        bool changed = false;
#pragma unroll 1
        for (i = 0; i < n - 1; i++)
#pragma unroll 1
            for (j = i + 1; j < n; j++) {
                M Ai = At.at(i * astep), Aj = At.at(j * astep);
                double a = W[i], p = 0, b = W[j];
                for (k = 0; k < m; k++) p += Ai[k] * Aj[k];
                if (fabs(p) <= eps * sqrt(a * b)) {
                    br |= BR_SVD_SKIP;
                    continue;
                }
                p *= 2;
                double beta = a - b, gamma = orb_cv::cv_hypot(p, beta);
                if (beta < 0) {
                    br |= BR_SVD_BETA_NEG;
                    double delta = (gamma - beta) * 0.5;
                    s = sqrt(delta / gamma);
                    c = p / (gamma * s * 2);
                } else {
                    br |= BR_SVD_BETA_POS;
                    c = sqrt((gamma + beta) / (gamma * 2));
                    s = p / (gamma * c * 2);
                }
                a = b = 0;
                for (k = 0; k < m; k++) {
                    double t0 = c * Ai[k] + s * Aj[k];
                    double t1 = -s * Ai[k] + c * Aj[k];
                    Ai[k] = t0;
                    Aj[k] = t1;
                    a += t0 * t0;
                    b += t1 * t1;
                }
                W[i] = a;
                W[j] = b;
                changed = true;
                if (vt) {
                    M Vi = Vt.at(i * vstep), Vj = Vt.at(j * vstep);
                    for (k = 0; k < n; k++) {
                        double t0 = c * Vi[k] + s * Vj[k];
                        double t1 = -s * Vi[k] + c * Vj[k];
                        Vi[k] = t0;
                        Vj[k] = t1;
                    }
                }
            }
        if (!changed) break;
    }

    for (i = 0; i < n; i++) {
        for (k = 0, sd = 0; k < m; k++) {
            double t = At[i * astep + k];
            sd += t * t;
        }
        W[i] = sqrt(sd);
    }

    for (i = 0; i < n - 1; i++) {
        j = i;
        for (k = i + 1; k < n; k++)
            if (W[j] < W[k]) j = k;
        if (i != j) {
            br |= BR_SVD_SWAP;
            double t = W[i];
            W[i] = W[j];
            W[j] = t;
            for (k = 0; k < m; k++) {
                t = At[i * astep + k];
                At[i * astep + k] = At[j * astep + k];
                At[j * astep + k] = t;
            }
            if (vt)
                for (k = 0; k < n; k++) {
                    t = Vt[i * vstep + k];
                    Vt[i * vstep + k] = Vt[j * vstep + k];
                    Vt[j * vstep + k] = t;
                }
        }
    }

    uint64_t rng = 0x12345678;  // cv::RNG
    for (i = 0; i < n1; i++) {
        sd = i < n ? (double)W[i] : 0;
        int tries = 0;
        while (sd <= minval && tries++ < MAX_FILL_TRIES) {
            // a zero singular value: a random vector, its projections on the earlier rows taken off
            // twice, normalised
            br |= BR_SVD_FILL;
            bool collapsed = false;
            const double val0 = (double)(1. / m);
            for (k = 0; k < m; k++) {
                rng = (uint64_t)(unsigned)rng * 4164903690U + (unsigned)(rng >> 32);
                double val = ((unsigned)rng & 256) != 0 ? val0 : -val0;
                At[i * astep + k] = val;
            }
            for (iter = 0; iter < 2; iter++)
                for (j = 0; j < i; j++) {
                    sd = 0;
                    for (k = 0; k < m; k++) sd += At[i * astep + k] * At[j * astep + k];
                    double asum = 0;
                    for (k = 0; k < m; k++) {
                        double t = At[i * astep + k] - sd * At[j * astep + k];
                        At[i * astep + k] = t;
                        asum += fabs(t);
                    }
                    if (asum < FILL_COLLAPSE) collapsed = true;
                    asum = asum ? 1 / asum : 0;
                    for (k = 0; k < m; k++) At[i * astep + k] *= asum;
                }
            sd = 0;
            for (k = 0; k < m; k++) {
                double t = At[i * astep + k];
                sd += t * t;
            }
            sd = sqrt(sd);
            if (collapsed && tries < MAX_FILL_TRIES) sd = 0;  // another vector; the last try is kept as it is
        }
        s = 1 / sd;
        for (k = 0; k < m; k++) At[i * astep + k] *= s;
    }
}

// The threshold of SVBkSbImpl_<double>: eps = DBL_EPSILON*2 times the sum of the singular values.
template <class M>
EPNP_HD inline double bksb_threshold(M W, int nm) {
    double threshold = 0;
    for (int i = 0; i < nm; i++) threshold += W[i];
    threshold *= DBL_EPSILON * 2;
    return threshold;
}

// cvSVD(A, W, Ut, 0, MODIFY_A | U_T) of a square n x n already in wk as At = transpose(A) (rows of n):
// m == n takes _SVDcompute's transposing path, temp_u is the work matrix and U_T hands it back
// untransposed: row i of `ut` is the i-th left singular vector.  vt is not asked for.
template <class M>
EPNP_HD inline void svd_ut(M wk, int n, unsigned& br) {
    jacobi_svd(wk, n, wk.at(WK_W), wk, false, n, n, n, n, br);
}

// ---- PnPsolver.cc ------------------------------------------------------------------------------------

// P supplies the correspondences: size(), pw(i, j), u(i, j), and with P::STORED the arrays
// alpha(i, c) and pc(i, j); without, both are recomputed where they are read (same expressions, same
// bits: a value depends on its own correspondence only).
template <class M, class P>
struct Epnp {
    M wk;  // WK_DOUBLES
    P pt;
    double fu, fv, uc, vc;
    double cws[4][3], ccs[4][3], ci[9];
    unsigned br;
};

template <class E>
EPNP_HD inline void alphas_of(const E& e, int i, double* a) {
    const double d0 = e.pt.pw(i, 0) - e.cws[0][0], d1 = e.pt.pw(i, 1) - e.cws[0][1], d2 = e.pt.pw(i, 2) - e.cws[0][2];
#pragma unroll
    for (int j = 0; j < 3; j++) a[1 + j] = fma_(e.ci[3 * j + 2], d2, fma_(e.ci[3 * j], d0, e.ci[3 * j + 1] * d1));
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

template <class E>
EPNP_HD inline void get_alphas(E& e, int i, double* a) {
    if constexpr (decltype(e.pt)::STORED) {
#pragma unroll
        for (int c = 0; c < 4; c++) a[c] = e.pt.alpha(i, c);
    } else
        alphas_of(e, i, a);
}

// compute_pcs' expression for one correspondence
template <class E>
EPNP_HD inline void pc_of(const E& e, const double* a, double* pc) {
#pragma unroll
    for (int j = 0; j < 3; j++)
        pc[j] = fma_(a[3], e.ccs[3][j], fma_(a[2], e.ccs[2][j], fma_(a[0], e.ccs[0][j], a[1] * e.ccs[1][j])));
}

template <class E>
EPNP_HD inline void get_pc(E& e, int i, double* pc) {
    if constexpr (decltype(e.pt)::STORED) {
#pragma unroll
        for (int j = 0; j < 3; j++) pc[j] = e.pt.pc(i, j);
    } else {
        // (after solve_for_sign negated ccs this is the negated value exactly)
        double a[4];
        alphas_of(e, i, a);
        pc_of(e, a, pc);
    }
}

EPNP_HD inline double dot3(const double* v1, const double* v2) {
    return fma_(v1[2], v2[2], fma_(v1[0], v2[0], v1[1] * v2[1]));
}

EPNP_HD inline double dist2(const double* p1, const double* p2) {
    const double d0 = p1[0] - p2[0], d1 = p1[1] - p2[1], d2 = p1[2] - p2[2];
    return fma_(d2, d2, fma_(d0, d0, d1 * d1));
}

template <class E>
EPNP_HD inline void choose_control_points(E& e) {
    const int n = e.pt.size();
    e.cws[0][0] = e.cws[0][1] = e.cws[0][2] = 0;
    for (int i = 0; i < n; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) e.cws[0][j] += e.pt.pw(i, j);
#pragma unroll
    for (int j = 0; j < 3; j++) e.cws[0][j] /= n;

    // cvMulTransposed(PW0, PW0tPW0, 1): MulTransposedR, dst(i, j >= i) = sum over the rows k of
    // src(k, i)*src(k, j), times scale = 1, then completeSymm.  (The six chains advance together;
    // each is its own accumulator with ascending k.)
    double s[6] = {0, 0, 0, 0, 0, 0};
    for (int k = 0; k < n; k++) {
        const double p0 = e.pt.pw(k, 0) - e.cws[0][0], p1 = e.pt.pw(k, 1) - e.cws[0][1], p2 = e.pt.pw(k, 2) - e.cws[0][2];
        s[0] += p0 * p0;
        s[1] += p0 * p1;
        s[2] += p0 * p2;
        s[3] += p1 * p1;
        s[4] += p1 * p2;
        s[5] += p2 * p2;
    }
    const double a[9] = {s[0] * 1.0, s[1] * 1.0, s[2] * 1.0, s[1] * 1.0, s[3] * 1.0,
                         s[4] * 1.0, s[2] * 1.0, s[4] * 1.0, s[5] * 1.0};
    // cvSVD(&PW0tPW0, &DC, &UCt, 0, MODIFY_A | U_T)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) e.wk[i * 3 + k] = a[k * 3 + i];
    svd_ut(e.wk, 3, e.br);
#pragma unroll
    for (int i = 1; i < 4; i++) {
        const double k = sqrt(e.wk[WK_W + i - 1] / n);
#pragma unroll
        for (int j = 0; j < 3; j++) e.cws[i][j] = fma_(k, e.wk[3 * (i - 1) + j], e.cws[0][j]);
    }
}

template <class E>
EPNP_HD inline void compute_barycentric_coordinates(E& e) {
    double cc[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = e.cws[j][i] - e.cws[0][i];

    // cvInvert(&CC, &CC_inv, CV_SVD): SVD::compute (u and vt, m == n: the transposing path) and
    // SVD::backSubst without a right-hand side (nb = m: buffer[j] = u(j, i)/w[i], then MatrAXPY)
    auto At = e.wk, Vt = e.wk.at(9), W = e.wk.at(WK_W);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) At[i * 3 + k] = cc[k * 3 + i];
    jacobi_svd(At, 3, W, Vt, true, 3, 3, 3, 3, e.br);
#pragma unroll
    for (int k = 0; k < 9; k++) e.ci[k] = 0;
    const double threshold = bksb_threshold(W, 3);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) {
            e.br |= BR_BKSB_SKIP;
            continue;
        }
        wi = 1 / wi;
        double buffer[3];
#pragma unroll
        for (int j = 0; j < 3; j++) buffer[j] = At[i * 3 + j] * wi;  // u(j, i) = temp_u(i, j)
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double sv = Vt[i * 3 + r];
#pragma unroll
            for (int j = 0; j < 3; j++) e.ci[r * 3 + j] = e.ci[r * 3 + j] + sv * buffer[j];
        }
    }
    if constexpr (decltype(e.pt)::STORED) {
        const int n = e.pt.size();
        for (int i = 0; i < n; i++) {
            double a[4];
            alphas_of(e, i, a);
#pragma unroll
            for (int c = 0; c < 4; c++) e.pt.alpha(i, c) = a[c];
        }
    }
}

// fill_M for every correspondence, cvMulTransposed(M, MtM, 1) and cvSVD(&MtM, &D, &Ut, 0, MODIFY_A |
// U_T): wk = ut.  MtM(i, j >= i) is the sum over M's rows k = 0 .. 2n-1 of M(k, i)*M(k, j), structural
// zeros included; the 78 chains advance together, each its own accumulator in wk with ascending k.
template <class E>
EPNP_HD inline void mtm_svd(E& e) {
    const int n = e.pt.size();
    for (int k = 0; k < 144; k++) e.wk[k] = 0;
    for (int p = 0; p < n; p++) {
        double as[4], M1[12], M2[12];
        get_alphas(e, p, as);
        const double u = e.pt.u(p, 0), v = e.pt.u(p, 1);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            M1[3 * i] = as[i] * e.fu;
            M1[3 * i + 1] = 0.0;
            M1[3 * i + 2] = as[i] * (e.uc - u);
            M2[3 * i] = 0.0;
            M2[3 * i + 1] = as[i] * e.fv;
            M2[3 * i + 2] = as[i] * (e.vc - v);
        }
#pragma unroll
        for (int i = 0; i < 12; i++)
#pragma unroll
            for (int j = i; j < 12; j++) {
                double s = e.wk[i * 12 + j];
                s += M1[i] * M1[j];
                s += M2[i] * M2[j];
                e.wk[i * 12 + j] = s;
            }
    }
    // tdst[j] = s0*scale, completeSymm; At = transpose(MtM)
    for (int i = 0; i < 12; i++)
        for (int j = i; j < 12; j++) {
            const double s = e.wk[i * 12 + j] * 1.0;
            e.wk[i * 12 + j] = s;
            e.wk[j * 12 + i] = s;
        }
    svd_ut(e.wk, 12, e.br);
}

template <class E>
EPNP_HD inline void compute_L_6x10(const E& e, double* l_6x10) {
    double dv[4][6][3];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const auto v = e.wk.at(12 * (11 - i));
        int a = 0, b = 1;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            dv[i][j][0] = v[3 * a] - v[3 * b];
            dv[i][j][1] = v[3 * a + 1] - v[3 * b + 1];
            dv[i][j][2] = v[3 * a + 2] - v[3 * b + 2];
            b++;
            if (b > 3) {
                a++;
                b = a + 1;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double* row = l_6x10 + 10 * i;
        row[0] = dot3(dv[0][i], dv[0][i]);
        row[1] = 2.0 * dot3(dv[0][i], dv[1][i]);
        row[2] = dot3(dv[1][i], dv[1][i]);
        row[3] = 2.0 * dot3(dv[0][i], dv[2][i]);
        row[4] = 2.0 * dot3(dv[1][i], dv[2][i]);
        row[5] = dot3(dv[2][i], dv[2][i]);
        row[6] = 2.0 * dot3(dv[0][i], dv[3][i]);
        row[7] = 2.0 * dot3(dv[1][i], dv[3][i]);
        row[8] = 2.0 * dot3(dv[2][i], dv[3][i]);
        row[9] = dot3(dv[3][i], dv[3][i]);
    }
}

template <class E>
EPNP_HD inline void compute_rho(const E& e, double* rho) {
    rho[0] = dist2(e.cws[0], e.cws[1]);
    rho[1] = dist2(e.cws[0], e.cws[2]);
    rho[2] = dist2(e.cws[0], e.cws[3]);
    rho[3] = dist2(e.cws[1], e.cws[2]);
    rho[4] = dist2(e.cws[1], e.cws[3]);
    rho[5] = dist2(e.cws[2], e.cws[3]);
}

// cvSolve(&L_6xK, Rho, &B, CV_SVD) with L_6xK's columns c0.. of L_6x10: a = transpose(src) (K rows of
// 6), JacobiSVD(a, w, v, m = 6, n = K) with n1 = n, then SVBkSb with u = a (uT), v (vT), nb = 1:
// s = (sum over j of u(i, j)*b[j]) / w[i], x[j] += s*v(i, j), singular values under the threshold skipped.
template <int K, class E>
EPNP_HD inline void solve_svd(E& e, const double* l_6x10, int c0, int c1, int c2, int c3, int c4, const double* rho,
                              double* x) {
    const int cols[5] = {c0, c1, c2, c3, c4};
    auto At = e.wk, Vt = e.wk.at(WK_SMALL_VT), W = e.wk.at(WK_W);
#pragma unroll
    for (int c = 0; c < K; c++)
#pragma unroll
        for (int r = 0; r < 6; r++) At[c * 6 + r] = l_6x10[10 * r + cols[c]];
    jacobi_svd(At, 6, W, Vt, true, K, 6, K, K, e.br);
#pragma unroll
    for (int j = 0; j < K; j++) x[j] = 0;
    const double threshold = bksb_threshold(W, K);
#pragma unroll
    for (int i = 0; i < K; i++) {
        double wi = W[i];
        if (fabs(wi) <= threshold) {
            e.br |= BR_BKSB_SKIP;
            continue;
        }
        wi = 1 / wi;
        double s = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) s += At[i * 6 + j] * rho[j];
        s *= wi;
#pragma unroll
        for (int j = 0; j < K; j++) x[j] = x[j] + s * Vt[i * K + j];
    }
}

template <class E>
EPNP_HD inline void find_betas_approx_1(E& e, const double* l, const double* rho, double* betas) {
    double b4[4];
    solve_svd<4>(e, l, 0, 1, 3, 6, 0, rho, b4);
    if (b4[0] < 0) {
        e.br |= BR_B_NEG;
        betas[0] = sqrt(-b4[0]);
        betas[1] = -b4[1] / betas[0];
        betas[2] = -b4[2] / betas[0];
        betas[3] = -b4[3] / betas[0];
    } else {
        e.br |= BR_B_POS;
        betas[0] = sqrt(b4[0]);
        betas[1] = b4[1] / betas[0];
        betas[2] = b4[2] / betas[0];
        betas[3] = b4[3] / betas[0];
    }
}

template <class E>
EPNP_HD inline void find_betas_approx_2(E& e, const double* l, const double* rho, double* betas) {
    double b3[3];
    solve_svd<3>(e, l, 0, 1, 2, 0, 0, rho, b3);
    if (b3[0] < 0) {
        e.br |= BR_B_NEG;
        betas[0] = sqrt(-b3[0]);
        betas[1] = (b3[2] < 0) ? sqrt(-b3[2]) : 0.0;
    } else {
        e.br |= BR_B_POS;
        betas[0] = sqrt(b3[0]);
        betas[1] = (b3[2] > 0) ? sqrt(b3[2]) : 0.0;
    }
    if (b3[1] < 0) {
        e.br |= BR_B1_NEG;
        betas[0] = -betas[0];
    }
    betas[2] = 0.0;
    betas[3] = 0.0;
}

template <class E>
EPNP_HD inline void find_betas_approx_3(E& e, const double* l, const double* rho, double* betas) {
    double b5[5];
    solve_svd<5>(e, l, 0, 1, 2, 3, 4, rho, b5);
    if (b5[0] < 0) {
        e.br |= BR_B_NEG;
        betas[0] = sqrt(-b5[0]);
        betas[1] = (b5[2] < 0) ? sqrt(-b5[2]) : 0.0;
    } else {
        e.br |= BR_B_POS;
        betas[0] = sqrt(b5[0]);
        betas[1] = (b5[2] > 0) ? sqrt(b5[2]) : 0.0;
    }
    if (b5[1] < 0) {
        e.br |= BR_B1_NEG;
        betas[0] = -betas[0];
    }
    betas[2] = b5[3] / betas[0];
    betas[3] = 0.0;
}

EPNP_HD inline void compute_A_and_b_gauss_newton(const double* l_6x10, const double* rho, const double* betas,
                                                 double* A, double* b) {
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const double* rowL = l_6x10 + i * 10;
        double* rowA = A + i * 4;
        const double b0 = betas[0], b1 = betas[1], b2 = betas[2], b3 = betas[3];
        rowA[0] = fma_(rowL[6], b3, fma_(rowL[3], b2, fma_(2 * rowL[0], b0, rowL[1] * b1)));
        rowA[1] = fma_(rowL[7], b3, fma_(rowL[4], b2, fma_(rowL[1], b0, 2 * rowL[2] * b1)));
        rowA[2] = fma_(rowL[8], b3, fma_(2 * rowL[5], b2, fma_(rowL[3], b0, rowL[4] * b1)));
        rowA[3] = fma_(2 * rowL[9], b3, fma_(rowL[8], b2, fma_(rowL[6], b0, rowL[7] * b1)));
        double s = fma_(rowL[0] * b0, b0, rowL[1] * b0 * b1);
        s = fma_(rowL[2] * b1, b1, s);
        s = fma_(rowL[3] * b0, b2, s);
        s = fma_(rowL[4] * b1, b2, s);
        s = fma_(rowL[5] * b2, b2, s);
        s = fma_(rowL[6] * b0, b3, s);
        s = fma_(rowL[7] * b1, b3, s);
        s = fma_(rowL[8] * b2, b3, s);
        s = fma_(rowL[9] * b3, b3, s);
        b[i] = rho[i] - s;
    }
}

// qr_solve on the 6 x 4 of gauss_newton (its statics A1 / A2 are scratch).  Returns at once, X
// untouched, when a column's largest magnitude is 0.
EPNP_HD inline void qr_solve(double* pA, double* pb, double* pX, unsigned& br) {
    const int nr = 6, nc = 4;
    double A1[6], A2[6];
#pragma unroll
    for (int k = 0; k < nc; k++) {
        // (ppAkk = pA + k*(nc + 1); the scan starts one row early, as the reference's does)
        double eta = fabs(pA[k * nc + k]);
        for (int i = k + 1; i < nr; i++) {
            double elt = fabs(pA[(i - 1) * nc + k]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) {
            br |= BR_QR_ETA0;
            A1[k] = A2[k] = 0.0;
            return;
        } else {
            double sum = 0.0, inv_eta = 1. / eta;
            for (int i = k; i < nr; i++) {
                pA[i * nc + k] *= inv_eta;
                sum = fma_(pA[i * nc + k], pA[i * nc + k], sum);
            }
            double sigma = sqrt(sum);
            if (pA[k * nc + k] < 0) {
                br |= BR_QR_SIGMA_NEG;
                sigma = -sigma;
            }
            pA[k * nc + k] += sigma;
            A1[k] = sigma * pA[k * nc + k];
            A2[k] = -eta * sigma;
            for (int j = k + 1; j < nc; j++) {
                double sum = 0;
                for (int i = k; i < nr; i++) sum = fma_(pA[i * nc + k], pA[i * nc + j], sum);
                double tau = sum / A1[k];
                for (int i = k; i < nr; i++) pA[i * nc + j] = fma_(-tau, pA[i * nc + k], pA[i * nc + j]);
            }
        }
    }
    // b <- Qt b
#pragma unroll
    for (int j = 0; j < nc; j++) {
        double tau = 0;
        for (int i = j; i < nr; i++) tau = fma_(pA[i * nc + j], pb[i], tau);
        tau /= A1[j];
        for (int i = j; i < nr; i++) pb[i] = fma_(-tau, pA[i * nc + j], pb[i]);
    }
    // X = R-1 b
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
#pragma unroll
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
        for (int j = i + 1; j < nc; j++) sum = fma_(pA[i * nc + j], pX[j], sum);
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

// The reference's x[4] is uninitialised and is read as it is when qr_solve returns early on its
// first call; here it starts as zeros (the first repair).
EPNP_HD inline void gauss_newton(const double* l_6x10, const double* rho, double* betas, unsigned& br) {
    double a[6 * 4], b[6], x[4] = {0, 0, 0, 0};
#pragma unroll 1
    for (int k = 0; k < 5; k++) {
        compute_A_and_b_gauss_newton(l_6x10, rho, betas, a, b);
        qr_solve(a, b, x, br);
#pragma unroll
        for (int i = 0; i < 4; i++) betas[i] += x[i];
    }
}

// compute_ccs, compute_pcs, solve_for_sign, estimate_R_and_t, reprojection_error
template <class E>
EPNP_HD inline double compute_R_and_t(E& e, const double* betas, double* R, double* t) {
    const int n = e.pt.size();
#pragma unroll
    for (int i = 0; i < 4; i++) e.ccs[i][0] = e.ccs[i][1] = e.ccs[i][2] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const auto v = e.wk.at(12 * (11 - i));
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int k = 0; k < 3; k++) e.ccs[j][k] = fma_(betas[i], v[3 * j + k], e.ccs[j][k]);
    }
    if constexpr (decltype(e.pt)::STORED)
        for (int i = 0; i < n; i++) {
            double a[4], pc[3];
            get_alphas(e, i, a);
            pc_of(e, a, pc);
#pragma unroll
            for (int j = 0; j < 3; j++) e.pt.pc(i, j) = pc[j];
        }
    // solve_for_sign
    {
        double pc[3];
        get_pc(e, 0, pc);
        if (pc[2] < 0.0) {
            e.br |= BR_SIGN_FLIP;
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) e.ccs[i][j] = -e.ccs[i][j];
            if constexpr (decltype(e.pt)::STORED)
                for (int i = 0; i < n; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) e.pt.pc(i, j) = -e.pt.pc(i, j);
        }
    }
    // estimate_R_and_t
    double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0};
    for (int i = 0; i < n; i++) {
        double pc[3];
        get_pc(e, i, pc);
#pragma unroll
        for (int j = 0; j < 3; j++) {
            pc0[j] += pc[j];
            pw0[j] += e.pt.pw(i, j);
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        pc0[j] /= n;
        pw0[j] /= n;
    }
    double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; i++) {
        double pc[3];
        get_pc(e, i, pc);
        const double w0 = e.pt.pw(i, 0) - pw0[0], w1 = e.pt.pw(i, 1) - pw0[1], w2 = e.pt.pw(i, 2) - pw0[2];
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double d = pc[j] - pc0[j];
            abt[3 * j] = fma_(d, w0, abt[3 * j]);
            abt[3 * j + 1] = fma_(d, w1, abt[3 * j + 1]);
            abt[3 * j + 2] = fma_(d, w2, abt[3 * j + 2]);
        }
    }
    // cvSVD(&ABt, &ABt_D, &ABt_U, &ABt_V, MODIFY_A): u = transpose(temp_u), v = transpose(vt)
    auto At = e.wk, Vt = e.wk.at(9), W = e.wk.at(WK_W);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) At[i * 3 + k] = abt[k * 3 + i];
    jacobi_svd(At, 3, W, Vt, true, 3, 3, 3, 3, e.br);
    double Rm[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double ui[3] = {At[i], At[3 + i], At[6 + i]}, vj[3] = {Vt[j], Vt[3 + j], Vt[6 + j]};
            Rm[i][j] = dot3(ui, vj);
        }
    double det = fma_(Rm[0][0] * Rm[1][1], Rm[2][2], Rm[0][1] * Rm[1][2] * Rm[2][0]);
    det = fma_(Rm[0][2] * Rm[1][0], Rm[2][1], det);
    det = fma_(-(Rm[0][2] * Rm[1][1]), Rm[2][0], det);
    det = fma_(-(Rm[0][1] * Rm[1][0]), Rm[2][2], det);
    det = fma_(-(Rm[0][0] * Rm[1][2]), Rm[2][1], det);
    if (det < 0) {
        e.br |= BR_DET_NEG;
        Rm[2][0] = -Rm[2][0];
        Rm[2][1] = -Rm[2][1];
        Rm[2][2] = -Rm[2][2];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {
        t[i] = pc0[i] - dot3(Rm[i], pw0);
#pragma unroll
        for (int j = 0; j < 3; j++) R[3 * i + j] = Rm[i][j];
    }
    // reprojection_error
    double sum2 = 0.0;
    for (int i = 0; i < n; i++) {
        const double pw[3] = {e.pt.pw(i, 0), e.pt.pw(i, 1), e.pt.pw(i, 2)};
        const double Xc = dot3(Rm[0], pw) + t[0];
        const double Yc = dot3(Rm[1], pw) + t[1];
        const double inv_Zc = 1.0 / (dot3(Rm[2], pw) + t[2]);
        const double ue = fma_(e.fu * Xc, inv_Zc, e.uc);
        const double ve = fma_(e.fv * Yc, inv_Zc, e.vc);
        const double du = e.pt.u(i, 0) - ue, dv = e.pt.u(i, 1) - ve;
        sum2 += sqrt(fma_(du, du, dv * dv));
    }
    return sum2 / n;
}

// compute_pose (PnPsolver.cc:449-497): R 9 doubles row-major, t 3; returns the reprojection error.
template <class E>
EPNP_HD inline double compute_pose(E& e, double* R, double* t) {
    choose_control_points(e);
    compute_barycentric_coordinates(e);
    mtm_svd(e);

    double l_6x10[6 * 10], rho[6];
    compute_L_6x10(e, l_6x10);
    compute_rho(e, rho);

    double Betas[4], rep, Rk[9], tk[3];
    int N = 1;

    find_betas_approx_1(e, l_6x10, rho, Betas);
    gauss_newton(l_6x10, rho, Betas, e.br);
    double best = compute_R_and_t(e, Betas, R, t);

    find_betas_approx_2(e, l_6x10, rho, Betas);
    gauss_newton(l_6x10, rho, Betas, e.br);
    rep = compute_R_and_t(e, Betas, Rk, tk);
    if (rep < best) {  // rep_errors[2] < rep_errors[1]
        N = 2;
        best = rep;
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = Rk[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = tk[k];
    }

    find_betas_approx_3(e, l_6x10, rho, Betas);
    gauss_newton(l_6x10, rho, Betas, e.br);
    rep = compute_R_and_t(e, Betas, Rk, tk);
    if (rep < best) {  // rep_errors[3] < rep_errors[N]
        N = 3;
        best = rep;
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = Rk[k];
#pragma unroll
        for (int k = 0; k < 3; k++) t[k] = tk[k];
    }
    if (N == 2) e.br |= BR_N2;
    if (N == 3) e.br |= BR_N3;
    return best;
}

// ---- the minimal sets ----------------------------------------------------------------------------------

// DUtils::Random::RandomInt(0, size - 1) on rand()'s value r: int(((double)r / 2^31) * size), which
// for 0 <= r < 2^31 and size <= 8192 is (r * size) >> 31
EPNP_HD inline int random_int(int r, int size) { return (int)(((long long)r * (long long)size) >> 31); }

// K draws from vAvailableIndices, which starts as the identity of size n >= K: randi on the list of
// size n - i, idx = list[randi], then list[idx] = back(), pop_back() with idx the VALUE drawn, not
// its position (PnPsolver.cc:171-172, Sim3Solver.cc:175-176), so a set may hold a correspondence
// twice.  At most K entries differ from the identity: they are kept as (position, value) pairs, the
// later one winning; a position at or past the end is written as the reference writes it (into the
// vector's spare capacity) and never read.  Negative draws are clamped to 0.
template <int K>
EPNP_HD inline void minimal_set(const int32_t* r, int n, int* idx) {
    int pos[K], val[K];
#pragma unroll
    for (int i = 0; i < K; i++) {
        const int size = n - i;
        const int randi = random_int(r[i] > 0 ? r[i] : 0, size);
        int v = randi, back = size - 1;
#pragma unroll
        for (int q = 0; q < i; q++) {
            if (pos[q] == randi) v = val[q];
            if (pos[q] == size - 1) back = val[q];
        }
        idx[i] = v;
        pos[i] = v;
        val[i] = back;
    }
}

}  // namespace orb_epnp
